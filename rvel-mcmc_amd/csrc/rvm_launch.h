// rvm_launch.h -- the host-side launchers every translation unit of librvmcmc.so shares: each is defined in the
// .hip file of its kernels and called from rvm_abi.hip / rvm_plan.hip.  Declarer and definer include this
// header, so a definition that drifts from it is a new overload and the link fails on the declared one.
#pragma once
#include <hip/hip_runtime.h>

#include "rvm_internal.h"

namespace rvm {
// The dynamic LDS a kernel may request on the current device: all the CU has left beside the kernel's static
// LDS, with the attribute admitting it set once per device and kernel; 0 when that could not be done.
// rvm_plan_create calls it for the plan's kernels (prepare_logl, prepare_refine), so a launch never changes
// function attributes -- launches stay capturable -- and a plan that would not fit is refused there.
template <auto Kernel>
static size_t lds_budget() {
    static size_t budget[64] = {};
    static bool known[64] = {};
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) {
        (void)hipGetLastError();
        return 0;
    }
    if (!known[dev]) {
        const void* f = reinterpret_cast<const void*>(Kernel);
        hipFuncAttributes fa{};
        size_t b = 0;
        if (hipFuncGetAttributes(&fa, f) == hipSuccess && fa.sharedSizeBytes < (size_t)RVM_LDS_PER_CU) {
            const size_t lim = (size_t)RVM_LDS_PER_CU - fa.sharedSizeBytes;
            if (hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lim) == hipSuccess) b = lim;
        }
        (void)hipGetLastError();
        budget[dev] = b;
        known[dev] = true;
    }
    return budget[dev];
}

hipError_t launch_logl(const DevPlan& P, int W, const double* params, double hill_factor, unsigned long long* slots,
                       double* logl, int32_t* status, double* rv_out, const StretchArgs& sa, hipStream_t stream,
                       int* dry_blocks);
hipError_t launch_refine(const DevPlan& P, int W, const double* params, double hill_factor, double* logl,
                         int32_t* status, double* rv_out, const StretchArgs& sa, int eager, int hedge,
                         hipStream_t stream);
int hedge_groups(const DevPlan& P, int W, int logl_blocks);
hipError_t launch_hedge(const DevPlan& P, int W, double hill_factor, const StretchArgs& sa, int ngrp,
                        hipStream_t stream);
hipError_t launch_eager(const DevPlan& P, int W, const double* params, double hill_factor, hipStream_t stream);
hipError_t launch_gen_bump(const DevPlan& P, hipStream_t stream);
hipError_t prepare_logl(const DevPlan& P);
hipError_t prepare_refine(const DevPlan& P);
hipError_t launch_stretch_propose(int P, int n0, int64_t s0b, const double* x, int n1, const double* c, double a,
                                  uint64_t seed, uint64_t it, uint32_t half, const double* draws, double* q,
                                  double* z, hipStream_t st);
hipError_t launch_stretch_accept(int P, int n0, int64_t s0b, double* x, double* lnp, const double* q,
                                 const double* lnp_new, const double* z, uint64_t seed, uint64_t it, uint32_t half,
                                 const double* draws, int32_t* acc, hipStream_t st);
hipError_t launch_mh_propose(int P, int n, int64_t b, const double* x, const double* scales, double step,
                             uint64_t seed, uint64_t it, const double* draws, double* q, hipStream_t st);
hipError_t launch_mh_accept(int P, int n, int64_t b, double* x, double* lnp, const double* q, const double* lnp_new,
                            uint64_t seed, uint64_t it, const double* draws, int32_t* acc, hipStream_t st);
hipError_t launch_stretch_iteration_end(const IterEndArgs& g, hipStream_t st);
hipError_t launch_pt_stretch_propose(int P, int T, int Wh, const double* x, const double* c, double a, uint64_t seed,
                                     uint64_t it, uint32_t half, const double* draws, double* q, double* z,
                                     hipStream_t st);
hipError_t launch_pt_stretch_accept(int P, int T, int Wh, const double* betas, double* x, double* lnp,
                                    const double* q, const double* lnp_new, const double* z, uint64_t seed,
                                    uint64_t it, uint32_t half, const double* draws, int32_t* acc, hipStream_t st);
hipError_t launch_pt_swap(int P, int T, int Wh, const double* betas, double* x0, double* x1, double* lnp0,
                          double* lnp1, uint64_t seed, uint64_t it, const double* draws, int32_t* swapped,
                          hipStream_t st);
hipError_t launch_pt_ladder_update(const PtLadderArgs& g, hipStream_t st);
hipError_t launch_chain_record(int P, int n, const double* src, int64_t src_ld, int64_t c0, int64_t cs, double* dst,
                               int64_t dst_ld, int64_t d0, const double* lsrc, double* ldst, hipStream_t st);
hipError_t launch_chain_moments(const double* x, int P, int W, int64_t t0, int64_t t1, double* mean, double* m2,
                                hipStream_t st);
size_t chain_autocov_workspace_doubles(int P, int W, int n_lags);
hipError_t launch_chain_autocov(const double* x, const double* mean, int P, int W, int64_t t0, int64_t t1, int lag0,
                                int n_lags, double* acov, double* part, hipStream_t st);
size_t rows_quantiles_workspace_bytes(int n_rows, int n_q);
hipError_t launch_rows_quantiles(const double* x, int n_rows, int64_t row_stride, int64_t n_outer,
                                 int64_t outer_stride, int64_t n_inner, const SelQ& Q, double* out,
                                 int64_t* n_valid, void* workspace, hipStream_t st);
size_t chain_cov_workspace_doubles(int P, int W);
hipError_t launch_chain_cov(const double* x, int P, int W, int64_t t0, int64_t t1, const double* center, double* cov,
                            double* part, hipStream_t st);
hipError_t launch_chain_draw(const double* x, int P, int W, int64_t t0, int64_t t1, int S, uint64_t seed,
                             uint64_t draw_id, const double* draws, double* xo, int64_t* idx, hipStream_t st);
int64_t gls_chunk_freqs(int N);
size_t gls_workspace_bytes(int N, int F, int S);
hipError_t launch_gls_basis(const double* tau, int N, int64_t ld, double f0, double df, int64_t k0, int F,
                            double* cos_out, double* sin_out, double* freq_out, hipStream_t st);
hipError_t launch_gls_power(const double* tau, const double* w, int N, const double* data, const double* model,
                            int64_t model_ld, int S, double f0, double df, int64_t k0, int F, int float_mean,
                            double* power, int64_t power_ld, double* freq_out, double* ws, hipStream_t st);
hipError_t launch_stability_init(int NP, int inclined, int n, const double* params, double hill_factor, double* xv,
                                 double* ext, int32_t* status, int64_t* steps, hipStream_t st);
hipError_t launch_stability_advance(int NP, int inclined, int n, const double* params, double hill_factor, double h,
                                    int sample_every, int n_blocks, double r_max, double* xv, double* ext,
                                    int32_t* status, int64_t* steps, int64_t* n_alive, hipStream_t st);
hipError_t launch_fd_params(int P, int n, const double* x, double rel, const double* fl, double* out, hipStream_t st);
hipError_t launch_smala_derive(int P, int C, int E, const double* x, double rel, const double* fl,
                               const double* lp_st, const int32_t* st_st, const double* rv, const double* w,
                               double npoints, double alpha, double eps, const SmalaCache& out, int sides,
                               hipStream_t st);
hipError_t launch_smala_center_accept(int P, int C, int64_t begin, double* x, const SmalaCache& cur, const double* xs,
                                      const SmalaCache& prop, const double* lpc, const int32_t* stc, double eps,
                                      uint64_t seed, uint64_t it, const double* draws, int32_t* accepted,
                                      int32_t* failures, hipStream_t st);
hipError_t launch_smala_metric(int P, int C, const double* x, const double* lp, const int32_t* status,
                               const double* grad, const double* hess, double alpha, double eps, const SmalaCache& out,
                               hipStream_t st);
hipError_t launch_smala_propose(int P, int C, int64_t begin, const double* x, const SmalaCache& cur, double eps,
                                uint64_t seed, uint64_t it, const double* draws, double* xs, hipStream_t st);
hipError_t launch_smala_accept(int P, int C, int64_t begin, double* x, const SmalaCache& cur, const double* xs,
                               const SmalaCache& prop, double eps, uint64_t seed, uint64_t it, const double* draws,
                               int32_t* accepted, int32_t* failures, hipStream_t st);
hipError_t launch_smala_derive_accept(int P, int C, int E, const double* xs, double rel, const double* fl,
                                      const double* lp_st, const int32_t* st_st, const double* rv, const double* w,
                                      double npoints, double alpha, double eps, const SmalaCache& prop,
                                      int64_t begin, double* x, const SmalaCache& cur, uint64_t seed, uint64_t it,
                                      const double* draws, int32_t* accepted, int32_t* failures, hipStream_t st);
hipError_t launch_smala_metric_accept(int P, int C, const double* xs, const double* lp, const int32_t* status,
                                      const double* grad, const double* hess, double alpha, double eps,
                                      const SmalaCache& prop, int64_t begin, double* x, const SmalaCache& cur,
                                      uint64_t seed, uint64_t it, const double* draws, int32_t* accepted,
                                      int32_t* failures, hipStream_t st);
hipError_t launch_derivs(const DevPlan& P, int C, const double* params, int n_dirs, const int32_t* dir_rows,
                         double hill_factor, double* ws, int32_t* wst, double* logl, double* grad, double* hess,
                         int32_t* status, hipStream_t stream);
}  // namespace rvm
