// rvm_abi.hip -- the extern "C" surface of librvmcmc.so (declared in include/rvmcmc.h).
//
// The per-step entry points: argument checks on the host, then kernels enqueued on the caller's
// stream.  The plan they run on is built once per observation set in rvm_plan.hip.
#include <cmath>
#include <string>

#include "rvm_launch.h"
#include "rvm_plan.h"

// One likelihood evaluation as every entry point runs it: the likelihood kernel, then (adaptive
// plans) the refinement kernel for the walkers it handed on, stream-ordered.  Everything it enqueues
// is complete when the caller's stream is (the header's conventions): an eager or hedged launch forks
// the plan's side stream from the caller's and joins it back after the refinement kernel, which by then
// has stopped every eager or hedge block it did not wait for (rvm_refine.hip).  No host-side state changes
// per launch -- the launch generation lives on the device -- so a captured hipGraph replays it.
static hipError_t run_logl(const rvm_plan* plan, int W, const double* params, double hill_factor, double* logl,
                           int32_t* status, double* rv_out, const rvm::StretchArgs& sa, hipStream_t st) {
    const bool tm = plan->tn < plan->tcap;
    // eager halving passes (rvm_refine.hip): plain launches of 32..512 walkers, no RV curve wanted
    const bool mapped = sa.c != nullptr || sa.mh_scale != nullptr || sa.fd_x != nullptr;
    const int eager = plan->side != nullptr && !mapped && rv_out == nullptr && params != nullptr &&
                      W >= rvm::RVM_EAGER_MIN && W <= plan->dev.eager_max;
    hipError_t e = hipSuccess;
    // hedged pass 2 (rvm_refine_impl.h hedge_kernel): fused stretch launches (half-steps, speculative
    // iterations) whose likelihood grid leaves at least two CUs idle -- halving pass 2 of the slots with
    // the quickest pericentre passages on the side stream, two CUs per group of them
    int hgrp = 0;
    if (plan->side != nullptr && plan->dev.hedge_groups > 0 && sa.c != nullptr && rv_out == nullptr && !eager) {
        int nblk = 0;
        if (rvm::launch_logl(plan->dev, W, params, hill_factor, plan->slots, logl, status, rv_out, sa, st, &nblk) ==
            hipSuccess)
            hgrp = rvm::hedge_groups(plan->dev, W, nblk);
    }
    if (eager || hgrp > 0) {
        e = hipEventRecord(plan->ev_fork, st);
        if (e == hipSuccess) e = hipStreamWaitEvent(plan->side, plan->ev_fork, 0);
        if (e == hipSuccess)
            e = eager ? rvm::launch_eager(plan->dev, W, params, hill_factor, plan->side)
                      : rvm::launch_hedge(plan->dev, W, hill_factor, sa, hgrp, plan->side);
        if (e != hipSuccess) {
            // (join whatever was enqueued on the side stream before reporting)
            if (hipEventRecord(plan->ev_join, plan->side) == hipSuccess) (void)hipStreamWaitEvent(st, plan->ev_join, 0);
            return e;
        }
    }
    if (tm) (void)hipEventRecord(plan->tev[3 * plan->tn], st);
    e = rvm::launch_logl(plan->dev, W, params, hill_factor, plan->slots, logl, status, rv_out, sa, st, nullptr);
    if (tm) (void)hipEventRecord(plan->tev[3 * plan->tn + 1], st);
    // (the refinement kernel runs even after a failed likelihood launch: it resets the work lists)
    const hipError_t er =
        rvm::launch_refine(plan->dev, W, params, hill_factor, logl, status, rv_out, sa, eager, 2 * hgrp, st);
    if (e == hipSuccess) e = er;
    if (tm) (void)hipEventRecord(plan->tev[3 * plan->tn + 2], st);
    if (tm) plan->tn++;
    if (eager || hgrp > 0) {
        hipError_t ej = hipEventRecord(plan->ev_join, plan->side);
        if (ej == hipSuccess) ej = hipStreamWaitEvent(st, plan->ev_join, 0);
        if (ej == hipSuccess) ej = rvm::launch_gen_bump(plan->dev, st);
        if (e == hipSuccess) e = ej;
    }
    return e;
}

static thread_local std::string g_err;

int rvm::fail(int code, const std::string& msg) {
    g_err = msg;
    return code;
}

int rvm::hip_fail(hipError_t e, const char* where) {
    return fail(-3, std::string(where) + ": " + hipGetErrorString(e));
}

using rvm::Entry;

// ---- the rules more than one entry point checks: the refusal's text, or null ----
static const char* bad_hill(double hill_factor) { return hill_factor >= 0.0 ? nullptr : "hill_factor must be >= 0"; }
static const char* bad_scale(double a) { return a > 1.0 ? nullptr : "stretch scale a must be > 1"; }
static const char* bad_window(int64_t t0, int64_t t1) {  // the steps [t0, t1) of a recorded chain
    return t0 < 0 ? "t0 must be >= 0" : t1 <= t0 ? "t1 must be > t0" : nullptr;
}
// this rank's n_loc walkers of half 0 from s0_begin and of half 1 from s1_begin (global indices)
static const char* bad_halves(int32_t n_loc, int32_t n_half, int64_t s0_begin, int64_t s1_begin) {
    if (s0_begin < 0 || s0_begin + n_loc > n_half || s1_begin < n_half || s1_begin + n_loc > 2 * (int64_t)n_half)
        return "walker ranges outside the halves";
    return nullptr;
}

// parameter rows of the plan's launches (rvm_param_map::n_rows; rvm_logl_derivs' dir_rows index them)
static int plan_rows(const rvm_plan* plan) { return (plan->dev.inclined ? 7 : 5) * plan->dev.n_planets; }

// The map's row count against the plan's, then the map into sa->src / sa->base.  Returns 0 or the refusal.
static int fill_map(const Entry& at, const rvm_plan* plan, const rvm_param_map* map, int32_t n_params,
                    rvm::StretchArgs* sa) {
    const int rows = plan_rows(plan);
    if (map->n_rows != rows) return at.bad("map rows do not match the plan");
    for (int r = 0; r < RVM_MAX_PARAM_ROWS; r++) {
        const int k = r < rows ? map->src[r] : -1;
        if (k >= n_params) return at.bad("map source index out of range");
        sa->src[r] = k < 0 ? -1 : k;
        sa->base[r] = r < rows ? map->base[r] : 0.0;
    }
    return 0;
}

// the fields the fused sampler launches share: the n walkers of x (lnp, accepted) from global index
// s0_begin, and for the stretch move the n1 walkers of c they are proposed against (MH: none, zeros)
static void fill_stretch(rvm::StretchArgs* sa, int32_t n_params, int32_t n, int64_t s0_begin, double* x, double* x_aos,
                         double* lnp, int32_t n1, const double* c, double a, uint64_t seed, uint64_t iteration,
                         uint32_t half, int32_t* accepted) {
    sa->c = c;
    sa->x = x;
    sa->x_aos = x_aos;
    sa->lnp = lnp;
    sa->accepted = accepted;
    sa->s0_begin = s0_begin;
    sa->seed = seed;
    sa->iteration = iteration;
    sa->a = a;
    sa->n1 = n1;
    sa->dim = n_params;
    sa->half = half;
    sa->xstride = n;
}

extern "C" {

const char* rvm_last_error(void) { return g_err.c_str(); }
int rvm_abi_version(void) { return RVM_ABI_VERSION; }

int rvm_logl_batch(const rvm_plan* plan, int32_t n_walkers, const double* params, double hill_factor,
                   double* logl_out, int32_t* status_out, double* rv_out, void* stream) {
    const Entry at{"rvm_logl_batch"};
    if (!plan) return at.null("plan");
    if (n_walkers == 0) return 0;
    if (n_walkers < 0 || n_walkers > plan->max_walkers) return at.bad("n_walkers exceeds the plan's max_walkers");
    if (!params || !logl_out || !status_out) return at.null("buffer");
    if (const char* m = bad_hill(hill_factor)) return at.bad(m);
    rvm::StretchArgs none{};
    return at.done(run_logl(plan, n_walkers, params, hill_factor, logl_out, status_out, rv_out, none, (hipStream_t)stream));
}

int rvm_stretch_half_step(const rvm_plan* plan, const rvm_param_map* map, int32_t n_params, int32_t n_s0,
                          int64_t s0_begin, double* x, double* x_aos, double* lnp, int32_t n_s1, const double* c,
                          double a, uint64_t seed, uint64_t iteration, uint32_t half, double hill_factor,
                          double* lnp_new_out, int32_t* status_out, int32_t* accepted, void* stream) {
    const Entry at{"rvm_stretch_half_step"};
    if (!plan || !map) return at.null("plan or map");
    if (n_s0 == 0) return 0;
    if (n_s0 < 0 || n_s0 > plan->max_walkers) return at.bad("n_s0 exceeds the plan's max_walkers");
    if (n_params < 1 || n_s1 < 1 || !x || !lnp || !c) return at.bad("bad arguments");
    if (const char* m = bad_scale(a)) return at.bad(m);
    if (const char* m = bad_hill(hill_factor)) return at.bad(m);
    rvm::StretchArgs sa{};
    if (const int rc = fill_map(at, plan, map, n_params, &sa)) return rc;
    fill_stretch(&sa, n_params, n_s0, s0_begin, x, x_aos, lnp, n_s1, c, a, seed, iteration, half, accepted);
    return at.done(run_logl(plan, n_s0, nullptr, hill_factor, lnp_new_out, status_out, nullptr, sa, (hipStream_t)stream));
}

int rvm_stretch_iteration_begin(const rvm_plan* plan, const rvm_param_map* map, int32_t n_params, int32_t n_loc,
                                int64_t s0_begin, int64_t s1_begin, double* x0, double* lnp0, const double* x1,
                                const double* lnp1, int32_t n_half, const double* c0, const double* c1, double a,
                                uint64_t seed, uint64_t iteration, double hill_factor, double* lnp_spec,
                                int32_t* status_spec, int32_t* dec, int32_t* accepted0, void* stream) {
    const Entry at{"rvm_stretch_iteration_begin"};
    if (!plan || !map) return at.null("plan or map");
    if (n_loc == 0) return 0;
    if (n_loc < 0 || (int64_t)3 * n_loc > plan->max_walkers) return at.bad("3 n_loc exceeds the plan's max_walkers");
    if (n_params < 1 || n_half < n_loc || !x0 || !lnp0 || !x1 || !c0 || !c1 || !lnp_spec || !status_spec || !dec)
        return at.bad("bad arguments");
    if (const char* m = bad_halves(n_loc, n_half, s0_begin, s1_begin)) return at.bad(m);
    if (const char* m = bad_scale(a)) return at.bad(m);
    if (const char* m = bad_hill(hill_factor)) return at.bad(m);
    rvm::StretchArgs sa{};
    if (const int rc = fill_map(at, plan, map, n_params, &sa)) return rc;
    // (no walker-major mirror of x0: c0 must stay as it was until rvm_stretch_iteration_end)
    fill_stretch(&sa, n_params, n_loc, s0_begin, x0, nullptr, lnp0, n_half, c1, a, seed, iteration, 0, accepted0);
    sa.n_spec = n_loc;
    sa.c0 = c0;
    sa.x1 = x1;
    sa.s1_begin = s1_begin;
    sa.dec = dec;
    sa.lnp1 = lnp1;
    return at.done(run_logl(plan, 3 * n_loc, nullptr, hill_factor, lnp_spec, status_spec, nullptr, sa, (hipStream_t)stream));
}

int rvm_stretch_iteration_end(int32_t n_params, int32_t n_loc, int64_t s0_begin, int64_t s1_begin, const double* x0,
                              double* x0_aos, const int32_t* dec, const int32_t* dec_all, double* x1, double* x1_aos,
                              double* lnp1, int32_t n_half, const double* c0, const double* c1,
                              const double* lnp_spec, const int32_t* status_spec, double a, uint64_t seed,
                              uint64_t iteration, int32_t* accepted1, double* lnp_new_out, int32_t* status_new_out,
                              void* stream) {
    const Entry at{"rvm_stretch_iteration_end"};
    if (n_loc == 0) return 0;
    if (n_params < 1 || n_loc < 0 || n_half < n_loc || !x0 || !dec || !dec_all || !x1 || !lnp1 || !c0 || !c1 ||
        !lnp_spec || !status_spec)
        return at.bad("bad arguments");
    if (const char* m = bad_halves(n_loc, n_half, s0_begin, s1_begin)) return at.bad(m);
    if (const char* m = bad_scale(a)) return at.bad(m);
    rvm::IterEndArgs g{};
    g.dim = n_params;
    g.n = n_loc;
    g.n_half = n_half;
    g.s0_begin = s0_begin;
    g.s1_begin = s1_begin;
    g.x0 = x0;
    g.x0_aos = x0_aos;
    g.dec_local = dec;
    g.dec_all = dec_all;
    g.x1 = x1;
    g.x1_aos = x1_aos;
    g.lnp1 = lnp1;
    g.c0 = c0;
    g.c1 = c1;
    g.lnp_spec = lnp_spec;
    g.st_spec = status_spec;
    g.a = a;
    g.seed = seed;
    g.iteration = iteration;
    g.accepted1 = accepted1;
    g.lnp_new_out = lnp_new_out;
    g.status_new_out = status_new_out;
    return at.done(rvm::launch_stretch_iteration_end(g, (hipStream_t)stream));
}

int rvm_stretch_propose(int32_t n_params, int32_t n_s0, int64_t s0_begin, const double* x, int32_t n_s1,
                        const double* c, double a, uint64_t seed, uint64_t iteration, uint32_t half,
                        const double* draws, double* q_out, double* z_out, void* stream) {
    const Entry at{"rvm_stretch_propose"};
    if (n_s0 == 0) return 0;
    if (n_params < 1 || n_s0 < 0 || n_s1 < 1 || !x || !c || !q_out || !z_out) return at.bad("bad arguments");
    if (const char* m = bad_scale(a)) return at.bad(m);
    return at.done(rvm::launch_stretch_propose(n_params, n_s0, s0_begin, x, n_s1, c, a, seed, iteration, half, draws,
                                               q_out, z_out, (hipStream_t)stream));
}

int rvm_stretch_accept(int32_t n_params, int32_t n_s0, int64_t s0_begin, double* x, double* lnp, const double* q,
                       const double* lnp_new, const double* z, uint64_t seed, uint64_t iteration, uint32_t half,
                       const double* draws, int32_t* accepted, void* stream) {
    const Entry at{"rvm_stretch_accept"};
    if (n_s0 == 0) return 0;
    if (n_params < 1 || n_s0 < 0 || !x || !lnp || !q || !lnp_new || !z) return at.bad("bad arguments");
    return at.done(rvm::launch_stretch_accept(n_params, n_s0, s0_begin, x, lnp, q, lnp_new, z, seed, iteration, half,
                                              draws, accepted, (hipStream_t)stream));
}

// the scalar arguments the three parallel-tempering entry points share (null on success); `cols` =
// columns per temperature the launch indexes with int32 (n_half, or 2 n_half for the exchange)
static const char* pt_bad_shape(int32_t n_params, int32_t n_temps, int32_t n_half, int64_t cols) {
    if (n_params < 1) return "n_params must be >= 1";
    if (n_temps < 1) return "n_temps must be >= 1";
    if (n_half < 1) return "n_half must be >= 1";
    if ((int64_t)n_temps * cols > (int64_t)INT32_MAX) return "n_temps * n_half overflows int32";
    return nullptr;
}

int rvm_pt_stretch_propose(int32_t n_params, int32_t n_temps, int32_t n_half, const double* x, const double* c,
                           double a, uint64_t seed, uint64_t iteration, uint32_t half, const double* draws,
                           double* q_out, double* z_out, void* stream) {
    const Entry at{"rvm_pt_stretch_propose"};
    if (const char* m = pt_bad_shape(n_params, n_temps, n_half, n_half)) return at.bad(m);
    if (half > 1u) return at.bad("half must be 0 or 1");
    if (const char* m = bad_scale(a)) return at.bad(m);
    if (!x || !c || !q_out || !z_out) return at.null("x, c, q_out or z_out");
    return at.done(rvm::launch_pt_stretch_propose(n_params, n_temps, n_half, x, c, a, seed, iteration, half, draws,
                                                  q_out, z_out, (hipStream_t)stream));
}

int rvm_pt_stretch_accept(int32_t n_params, int32_t n_temps, int32_t n_half, const double* betas, double* x,
                          double* lnp, const double* q, const double* lnp_new, const double* z, uint64_t seed,
                          uint64_t iteration, uint32_t half, const double* draws, int32_t* accepted, void* stream) {
    const Entry at{"rvm_pt_stretch_accept"};
    if (const char* m = pt_bad_shape(n_params, n_temps, n_half, n_half)) return at.bad(m);
    if (half > 1u) return at.bad("half must be 0 or 1");
    if (!betas) return at.null("betas");
    if (!x || !lnp || !q || !lnp_new || !z) return at.null("x, lnp, q, lnp_new or z");
    return at.done(rvm::launch_pt_stretch_accept(n_params, n_temps, n_half, betas, x, lnp, q, lnp_new, z, seed,
                                                 iteration, half, draws, accepted, (hipStream_t)stream));
}

int rvm_pt_swap(int32_t n_params, int32_t n_temps, int32_t n_half, const double* betas, double* x0, double* x1,
                double* lnp0, double* lnp1, uint64_t seed, uint64_t iteration, const double* draws,
                int32_t* swapped, void* stream) {
    const Entry at{"rvm_pt_swap"};
    if (const char* m = pt_bad_shape(n_params, n_temps, n_half, 2 * (int64_t)n_half)) return at.bad(m);
    if (n_temps == 1) return 0;  // one temperature has no neighbour: nothing to launch
    if (!betas) return at.null("betas");
    if (!x0 || !x1 || !lnp0 || !lnp1 || !swapped) return at.null("x0, x1, lnp0, lnp1 or swapped");
    return at.done(rvm::launch_pt_swap(n_params, n_temps, n_half, betas, x0, x1, lnp0, lnp1, seed, iteration, draws,
                                       swapped, (hipStream_t)stream));
}

int rvm_pt_ladder_update(int32_t n_temps, int32_t n_half, const int32_t* swapped, const double* lnp0,
                         const double* lnp1, double kappa, double* betas, int64_t* swap_totals_prev,
                         double* ratios_out, int64_t* n_refused, double* lnp_moments, void* workspace,
                         void* stream) {
    const Entry at{"rvm_pt_ladder_update"};
    if (const char* m = pt_bad_shape(1, n_temps, n_half, 2 * (int64_t)n_half)) return at.bad(m);
    if (!std::isfinite(kappa) || kappa < 0.0) return at.bad("kappa must be finite and >= 0");
    if (n_temps == 1) return 0;  // one temperature has no ladder: nothing to launch
    if (!swapped) return at.null("swapped");
    if (!lnp0 || !lnp1) return at.null("lnp0 or lnp1");
    if (!betas) return at.null("betas");
    if (!swap_totals_prev) return at.null("swap_totals_prev");
    if (!ratios_out) return at.null("ratios_out");
    if (!n_refused) return at.null("n_refused");
    if (!workspace) return at.null("workspace");
    rvm::PtLadderArgs g;
    g.T = n_temps;
    g.Wh = n_half;
    g.swapped = swapped;
    g.lnp0 = lnp0;
    g.lnp1 = lnp1;
    g.kappa = kappa;
    g.betas = betas;
    g.totals_prev = swap_totals_prev;
    g.ratios = ratios_out;
    g.n_refused = n_refused;
    g.moments = lnp_moments;
    g.ws_totals = (int64_t*)workspace;
    g.ws_moments = (double*)workspace + (n_temps - 1);
    return at.done(rvm::launch_pt_ladder_update(g, (hipStream_t)stream));
}

// ---- the recorded chain (rvm_chain.hip) ----
// (a kernel grid's y and z extents hold 65535 blocks: the parameter rows, the blocks of 256 walkers)
static const char* chain_bad_shape(int32_t n_params, int32_t n_cols) {
    if (n_params < 1 || n_params > 65534) return "n_params must be 1 .. 65534";
    if (n_cols < 1 || n_cols > 65535 * 256) return "n_cols must be 1 .. 16776960";
    return nullptr;
}

int rvm_chain_record(int32_t n_params, int32_t n_cols, const double* src, int64_t src_ld, int64_t src_col0,
                     int64_t col_stride, double* dst, int64_t dst_ld, int64_t dst_col0, const double* lnp_src,
                     double* lnp_dst, void* stream) {
    const Entry at{"rvm_chain_record"};
    if (const char* m = chain_bad_shape(n_params, n_cols)) return at.bad(m);
    if (!src) return at.null("src");
    if (!dst) return at.null("dst");
    if (col_stride < 1) return at.bad("col_stride must be >= 1");
    if (src_col0 < 0) return at.bad("src_col0 must be >= 0");
    if (dst_col0 < 0) return at.bad("dst_col0 must be >= 0");
    if (col_stride > (INT64_MAX - src_col0) / n_cols || src_ld < src_col0 + (int64_t)(n_cols - 1) * col_stride + 1)
        return at.bad("src_ld is smaller than the last gathered column + 1");
    if (dst_col0 > INT64_MAX - n_cols || dst_ld < dst_col0 + n_cols)
        return at.bad("dst_ld is smaller than dst_col0 + n_cols");
    if ((lnp_src == nullptr) != (lnp_dst == nullptr))
        return at.bad("lnp_src and lnp_dst go together (both or neither)");
    return at.done(rvm::launch_chain_record(n_params, n_cols, src, src_ld, src_col0, col_stride, dst, dst_ld, dst_col0,
                                            lnp_src, lnp_dst, (hipStream_t)stream));
}

int rvm_chain_moments(const double* chain, int32_t n_params, int32_t n_cols, int64_t t0, int64_t t1, double* mean_out,
                      double* m2_out, void* stream) {
    const Entry at{"rvm_chain_moments"};
    if (const char* m = chain_bad_shape(n_params, n_cols)) return at.bad(m);
    if (!chain) return at.null("chain");
    if (const char* m = bad_window(t0, t1)) return at.bad(m);
    if (!mean_out) return at.null("mean_out");
    if (!m2_out) return at.null("m2_out");
    return at.done(rvm::launch_chain_moments(chain, n_params, n_cols, t0, t1, mean_out, m2_out, (hipStream_t)stream));
}

size_t rvm_chain_autocov_workspace_bytes(int32_t n_params, int32_t n_cols, int32_t n_lags) {
    if (chain_bad_shape(n_params, n_cols) || n_lags < 1 || n_lags > (1 << 30) || (int64_t)n_params * n_lags > INT32_MAX)
        return 0;
    return sizeof(double) * rvm::chain_autocov_workspace_doubles(n_params, n_cols, n_lags);
}

int rvm_chain_autocov(const double* chain, const double* mean, int32_t n_params, int32_t n_cols, int64_t t0, int64_t t1,
                      int32_t lag0, int32_t n_lags, double* acov_out, void* workspace, void* stream) {
    const Entry at{"rvm_chain_autocov"};
    if (const char* m = chain_bad_shape(n_params, n_cols)) return at.bad(m);
    if (!chain) return at.null("chain");
    if (!mean) return at.null("mean");
    if (const char* m = bad_window(t0, t1)) return at.bad(m);
    if (lag0 < 0) return at.bad("lag0 must be >= 0");
    if (n_lags < 1 || n_lags > (1 << 30)) return at.bad("n_lags must be 1 .. 2^30");
    if ((int64_t)lag0 + n_lags > t1 - t0) return at.bad("lag0 + n_lags - 1 must be at most t1 - t0 - 1");
    if ((int64_t)n_params * n_lags > INT32_MAX) return at.bad("n_params * n_lags beyond int32");
    if (!acov_out) return at.null("acov_out");
    if (!workspace) return at.null("workspace");
    return at.done(rvm::launch_chain_autocov(chain, mean, n_params, n_cols, t0, t1, lag0, n_lags, acov_out,
                                             (double*)workspace, (hipStream_t)stream));
}

// ---- posterior summaries (rvm_summary.hip) ----
// (a grid's y extent: the rows; 32-bit counters: a row's elements)
static bool quantiles_bad_shape(int32_t n_rows, int32_t n_q) {
    return n_rows < 1 || n_rows > 65535 || n_q < 1 || n_q > RVM_MAX_QUANTILES;
}

size_t rvm_rows_quantiles_workspace_bytes(int32_t n_rows, int32_t n_q) {
    if (quantiles_bad_shape(n_rows, n_q)) return 0;
    return rvm::rows_quantiles_workspace_bytes(n_rows, n_q);
}

int rvm_rows_quantiles(const double* x, int32_t n_rows, int64_t row_stride, int64_t n_outer, int64_t outer_stride,
                       int64_t n_inner, const double* q, int32_t n_q, double* out, int64_t* n_valid_out,
                       void* workspace, void* stream) {
    const Entry at{"rvm_rows_quantiles"};
    if (!x) return at.null("x");
    if (n_rows < 1 || n_rows > 65535) return at.bad("n_rows must be 1 .. 65535");
    if (row_stride < 0) return at.bad("row_stride must be >= 0");
    if (n_outer < 1) return at.bad("n_outer must be >= 1");
    if (outer_stride < 0) return at.bad("outer_stride must be >= 0");
    if (n_inner < 1) return at.bad("n_inner must be >= 1");
    if (n_outer > (int64_t)UINT32_MAX / n_inner)
        return at.bad("n_outer * n_inner beyond the 2^32 - 1 elements a row's counters hold");
    if (!q) return at.null("q");
    if (n_q < 1 || n_q > RVM_MAX_QUANTILES) return at.bad("n_q must be 1 .. 16");
    rvm::SelQ Q{};
    Q.n_q = n_q;
    for (int j = 0; j < n_q; j++) {
        if (!(q[j] >= 0.0 && q[j] <= 1.0)) return at.bad("every q must lie in [0, 1]");
        Q.q[j] = q[j];
    }
    if (!out) return at.null("out");
    if (!workspace) return at.null("workspace");
    if ((uintptr_t)workspace % 8 != 0) return at.bad("workspace must be 8-byte aligned");
    return at.done(rvm::launch_rows_quantiles(x, n_rows, row_stride, n_outer, outer_stride, n_inner, Q, out, n_valid_out,
                                              workspace, (hipStream_t)stream));
}

static const char* cov_bad_shape(int32_t n_params, int32_t n_cols) {
    // (the grid: n_params^2 blocks in x, groups of 64 walkers in z)
    if (n_params < 1 || n_params > 16384) return "n_params must be 1 .. 16384";
    if (n_cols < 1 || n_cols > 65535 * 64) return "n_cols must be 1 .. 4194240";
    return nullptr;
}

size_t rvm_chain_cov_workspace_bytes(int32_t n_params, int32_t n_cols) {
    if (cov_bad_shape(n_params, n_cols)) return 0;
    return sizeof(double) * rvm::chain_cov_workspace_doubles(n_params, n_cols);
}

int rvm_chain_cov(const double* chain, int32_t n_params, int32_t n_cols, int64_t t0, int64_t t1, const double* center,
                  double* cov_out, void* workspace, void* stream) {
    const Entry at{"rvm_chain_cov"};
    if (const char* m = cov_bad_shape(n_params, n_cols)) return at.bad(m);
    if (!chain) return at.null("chain");
    if (const char* m = bad_window(t0, t1)) return at.bad(m);
    if (!center) return at.null("center");
    if (!cov_out) return at.null("cov_out");
    if (!workspace) return at.null("workspace");
    return at.done(rvm::launch_chain_cov(chain, n_params, n_cols, t0, t1, center, cov_out, (double*)workspace,
                                         (hipStream_t)stream));
}

int rvm_chain_draw(const double* chain, int32_t n_params, int32_t n_cols, int64_t t0, int64_t t1, int32_t n_samples,
                   uint64_t seed, uint64_t draw_id, const double* draws, double* x_out, int64_t* idx_out,
                   void* stream) {
    const Entry at{"rvm_chain_draw"};
    if (const char* m = chain_bad_shape(n_params, n_cols)) return at.bad(m);
    if (!chain) return at.null("chain");
    if (const char* m = bad_window(t0, t1)) return at.bad(m);
    if (n_samples < 1) return at.bad("n_samples must be >= 1");
    if (!x_out) return at.null("x_out");
    return at.done(rvm::launch_chain_draw(chain, n_params, n_cols, t0, t1, n_samples, seed, draw_id, draws, x_out,
                                          idx_out, (hipStream_t)stream));
}

// ---- periodograms (rvm_gls.hip) ----
// the frequency grid f0 + (k0 + k) df, k < n_freq: the refusal's text, or null
static const char* gls_bad_grid(double f0, double df, int64_t k0, int32_t n_freq) {
    if (n_freq < 1) return "n_freq must be >= 1";
    if (k0 < 0) return "k0 must be >= 0";
    if (k0 > ((int64_t)1 << 53) - n_freq) return "k0 + n_freq must be <= 2^53";
    if (!std::isfinite(f0)) return "f0 must be finite";
    if (!std::isfinite(df)) return "df must be finite";
    return nullptr;
}
static const char* gls_bad_n_obs(int32_t n_obs) {
    return n_obs < 1 || n_obs > 2 * RVM_MAX_EPOCHS_PER_DIRECTION ? "n_obs must be 1 .. 3400" : nullptr;
}

int rvm_gls_basis(const double* tau, int32_t n_obs, double f0, double df, int64_t k0, int32_t n_freq, double* cos_out,
                  double* sin_out, double* freq_out, void* stream) {
    const Entry at{"rvm_gls_basis"};
    if (!tau) return at.null("tau");
    if (const char* m = gls_bad_n_obs(n_obs)) return at.bad(m);
    if (const char* m = gls_bad_grid(f0, df, k0, n_freq)) return at.bad(m);
    if (!cos_out) return at.null("cos_out");
    if (!sin_out) return at.null("sin_out");
    return at.done(rvm::launch_gls_basis(tau, n_obs, n_obs, f0, df, k0, n_freq, cos_out, sin_out, freq_out,
                                         (hipStream_t)stream));
}

size_t rvm_gls_workspace_bytes(int32_t n_obs, int32_t n_freq, int32_t n_series) {
    if (gls_bad_n_obs(n_obs) || n_freq < 1 || n_series < 1) return 0;
    return rvm::gls_workspace_bytes(n_obs, n_freq, n_series);
}

int rvm_gls_power(const double* tau, const double* w, int32_t n_obs, const double* data, const double* model,
                  int64_t model_ld, int32_t n_series, double f0, double df, int64_t k0, int32_t n_freq,
                  int32_t float_mean, double* power_out, int64_t power_ld, double* freq_out, void* workspace,
                  void* stream) {
    const Entry at{"rvm_gls_power"};
    if (!tau) return at.null("tau");
    if (!w) return at.null("w");
    if (const char* m = gls_bad_n_obs(n_obs)) return at.bad(m);
    if (!data) return at.null("data");
    if (n_series < 1) return at.bad("n_series must be >= 1");
    if (model && model_ld < n_series) return at.bad("model_ld must be >= n_series");
    if (const char* m = gls_bad_grid(f0, df, k0, n_freq)) return at.bad(m);
    if (float_mean != 0 && float_mean != 1) return at.bad("float_mean must be 0 or 1");
    if (!power_out) return at.null("power_out");
    if (power_ld < n_series) return at.bad("power_ld must be >= n_series");
    if (!workspace) return at.null("workspace");
    if ((uintptr_t)workspace % 16 != 0) return at.bad("workspace must be 16-byte aligned");
    return at.done(rvm::launch_gls_power(tau, w, n_obs, data, model, model_ld, n_series, f0, df, k0, n_freq,
                                         float_mean, power_out, power_ld, freq_out, (double*)workspace,
                                         (hipStream_t)stream));
}

// ---- dynamical stability (rvm_stability.hip) ----
// the shape both entry points share: the refusal's text, or null
static const char* stability_bad_shape(int32_t n_planets, int32_t inclined, int32_t n) {
    if (n_planets < 1 || n_planets > RVM_MAX_PLANETS) return "n_planets must be 1 .. 4";
    if (inclined != 0 && inclined != 1) return "inclined must be 0 or 1";
    if (n < 1) return "n must be >= 1";
    return nullptr;
}

int rvm_stability_init(int32_t n_planets, int32_t inclined, int32_t n, const double* params, double hill_factor,
                       double* xv, double* ext, int32_t* status, int64_t* steps, void* stream) {
    const Entry at{"rvm_stability_init"};
    if (const char* m = stability_bad_shape(n_planets, inclined, n)) return at.bad(m);
    if (!params) return at.null("params");
    if (const char* m = bad_hill(hill_factor)) return at.bad(m);
    if (!xv) return at.null("xv");
    if (!ext) return at.null("ext");
    if (!status) return at.null("status");
    if (!steps) return at.null("steps");
    return at.done(rvm::launch_stability_init(n_planets, inclined, n, params, hill_factor, xv, ext, status, steps,
                                              (hipStream_t)stream));
}

int rvm_stability_advance(int32_t n_planets, int32_t inclined, int32_t n, const double* params, double hill_factor,
                          double h, int32_t sample_every, int32_t n_blocks, double r_max, double* xv, double* ext,
                          int32_t* status, int64_t* steps, int64_t* n_alive_out, void* stream) {
    const Entry at{"rvm_stability_advance"};
    if (const char* m = stability_bad_shape(n_planets, inclined, n)) return at.bad(m);
    if (!params) return at.null("params");
    if (const char* m = bad_hill(hill_factor)) return at.bad(m);
    if (!(h > 0.0) || !std::isfinite(h)) return at.bad("h must be > 0 and finite");
    if (sample_every < 1) return at.bad("sample_every must be >= 1");
    if (n_blocks < 1) return at.bad("n_blocks must be >= 1");
    if (!xv) return at.null("xv");
    if (!ext) return at.null("ext");
    if (!status) return at.null("status");
    if (!steps) return at.null("steps");
    return at.done(rvm::launch_stability_advance(n_planets, inclined, n, params, hill_factor, h, sample_every,
                                                 n_blocks, r_max, xv, ext, status, steps, n_alive_out,
                                                 (hipStream_t)stream));
}

int rvm_mh_propose(int32_t n_params, int32_t n_chains, int64_t chain_begin, const double* x, const double* scales,
                   double step_size, uint64_t seed, uint64_t iteration, const double* draws, double* q_out,
                   void* stream) {
    const Entry at{"rvm_mh_propose"};
    if (n_chains == 0) return 0;
    if (n_params < 1 || n_chains < 0 || !x || !scales || !q_out) return at.bad("bad arguments");
    return at.done(rvm::launch_mh_propose(n_params, n_chains, chain_begin, x, scales, step_size, seed, iteration, draws,
                                          q_out, (hipStream_t)stream));
}

int rvm_mh_accept(int32_t n_params, int32_t n_chains, int64_t chain_begin, double* x, double* lnp, const double* q,
                  const double* lnp_new, uint64_t seed, uint64_t iteration, const double* draws, int32_t* accepted,
                  void* stream) {
    const Entry at{"rvm_mh_accept"};
    if (n_chains == 0) return 0;
    if (n_params < 1 || n_chains < 0 || !x || !lnp || !q || !lnp_new) return at.bad("bad arguments");
    return at.done(rvm::launch_mh_accept(n_params, n_chains, chain_begin, x, lnp, q, lnp_new, seed, iteration, draws,
                                         accepted, (hipStream_t)stream));
}

int rvm_mh_step(const rvm_plan* plan, const rvm_param_map* map, int32_t n_params, int32_t n_chains,
                int64_t chain_begin, double* x, double* lnp, const double* scales, double step_size, uint64_t seed,
                uint64_t iteration, double hill_factor, double* lnp_new_out, int32_t* status_out, int32_t* accepted,
                void* stream) {
    const Entry at{"rvm_mh_step"};
    if (!plan || !map) return at.null("plan or map");
    if (n_chains == 0) return 0;
    if (n_chains < 0 || n_chains > plan->max_walkers) return at.bad("n_chains exceeds the plan's max_walkers");
    if (n_params < 1 || !x || !lnp || !scales) return at.bad("bad arguments");
    if (const char* m = bad_hill(hill_factor)) return at.bad(m);
    rvm::StretchArgs sa{};
    if (const int rc = fill_map(at, plan, map, n_params, &sa)) return rc;
    fill_stretch(&sa, n_params, n_chains, chain_begin, x, nullptr, lnp, 0, nullptr, 0.0, seed, iteration, 0, accepted);
    sa.mh_scale = scales;
    sa.mh_step = step_size;
    return at.done(run_logl(plan, n_chains, nullptr, hill_factor, lnp_new_out, status_out, nullptr, sa, (hipStream_t)stream));
}

static bool smala_cache_ok(const rvm_smala_cache* c) {
    return c && c->lp && c->grad && c->mu && c->L && c->G && c->logdet && c->ok;
}

static rvm::SmalaCache smala_cache(const rvm_smala_cache* c) {
    return rvm::SmalaCache{c->lp, c->grad, c->mu, c->L, c->G, c->logdet, c->ok};
}

// n_params free parameters of n_chains chains (every SMALA kernel; refused under "bad arguments")
static bool smala_bad_shape(int32_t n_params, int32_t n_chains) {
    return n_params < 1 || n_params > RVM_SMALA_MAX_PARAMS || n_chains < 0;
}

// the stencil a derive reads and its scalars (rvm_smala_derive's; refused under "bad arguments")
static bool smala_bad_stencil(int32_t n_obs, const double* floor_, const double* lp_stencil,
                              const int32_t* status_stencil, const double* rv_stencil, const double* inv_sigma2,
                              double rel_step, double npoints_norm, double alpha) {
    return n_obs < 0 || !floor_ || !lp_stencil || !status_stencil || (n_obs > 0 && (!rv_stencil || !inv_sigma2)) ||
           !(rel_step > 0.0) || !(npoints_norm != 0.0) || !(alpha > 0.0);
}

int rvm_smala_stencil_logl(const rvm_plan* plan, const rvm_param_map* map, int32_t n_params, int32_t n_chains,
                           const double* x, double rel_step, const double* floor_, double hill_factor,
                           double* logl_out, int32_t* status_out, double* rv_out, void* stream) {
    const Entry at{"rvm_smala_stencil_logl"};
    if (!plan || !map) return at.null("plan or map");
    if (n_chains == 0) return 0;
    const int64_t W = (int64_t)(2 * n_params + 1) * n_chains;
    if (n_params < 1 || n_chains < 0 || !x || !floor_ || !logl_out || !status_out || !(rel_step > 0.0))
        return at.bad("bad arguments");
    if (W > plan->max_walkers) return at.bad("(2 n_params + 1) n_chains exceeds max_walkers");
    if (const char* m = bad_hill(hill_factor)) return at.bad(m);
    rvm::StretchArgs sa{};
    if (const int rc = fill_map(at, plan, map, n_params, &sa)) return rc;
    sa.dim = n_params;
    sa.fd_x = x;
    sa.fd_floor = floor_;
    sa.fd_rel = rel_step;
    sa.fd_n = n_chains;
    return at.done(run_logl(plan, (int)W, nullptr, hill_factor, logl_out, status_out, rv_out, sa, (hipStream_t)stream));
}

int rvm_fd_params(int32_t n_params, int32_t n_chains, const double* x, double rel_step, const double* floor_,
                  double* out, void* stream) {
    const Entry at{"rvm_fd_params"};
    if (n_chains == 0) return 0;
    if (n_params < 1 || n_chains < 0 || !x || !floor_ || !out || !(rel_step > 0.0)) return at.bad("bad arguments");
    return at.done(rvm::launch_fd_params(n_params, n_chains, x, rel_step, floor_, out, (hipStream_t)stream));
}

size_t rvm_logl_derivs_workspace_bytes(int32_t n_chains, int32_t n_dirs) {
    if (n_chains < 0 || n_dirs < 0) return 0;
    const size_t items = (size_t)n_chains * (size_t)(n_dirs * (n_dirs + 1) / 2);
    return items * 2 * (4 * sizeof(double) + sizeof(int32_t));
}

int rvm_logl_derivs(const rvm_plan* plan, int32_t n_chains, const double* params, int32_t n_dirs,
                    const int32_t* dir_rows, double hill_factor, double* logl_out, double* grad_out, double* hess_out,
                    int32_t* status_out, void* workspace, void* stream) {
    const Entry at{"rvm_logl_derivs"};
    if (!plan) return at.null("plan");
    if (n_chains == 0) return 0;
    const int rows = plan_rows(plan);
    if (n_chains < 0 || n_dirs < 1 || n_dirs > rows || !dir_rows || !params || !grad_out || !hess_out || !workspace)
        return at.bad("bad arguments");
    const size_t items = (size_t)n_chains * (size_t)(n_dirs * (n_dirs + 1) / 2);
    if (items > (size_t)(1 << 30)) return at.bad("too many chains x parameter pairs");
    if (const char* m = bad_hill(hill_factor)) return at.bad(m);
    for (int k = 0; k < n_dirs; k++) {
        if (dir_rows[k] < 0 || dir_rows[k] >= rows) return at.bad("dir_rows entry out of range");
        for (int q = 0; q < k; q++)
            if (dir_rows[q] == dir_rows[k]) return at.bad("dir_rows entries must be distinct");
    }
    double* ws = reinterpret_cast<double*>(workspace);
    int32_t* wst = reinterpret_cast<int32_t*>(ws + 2 * 4 * items);
    return at.done(rvm::launch_derivs(plan->dev, n_chains, params, n_dirs, dir_rows, hill_factor, ws, wst, logl_out,
                                      grad_out, hess_out, status_out, (hipStream_t)stream));
}

static int smala_derive(const Entry& at, int sides, int32_t n_params, int32_t n_chains, int32_t n_obs, const double* x,
                        double rel_step, const double* floor_, const double* lp_stencil,
                        const int32_t* status_stencil, const double* rv_stencil, const double* inv_sigma2,
                        double npoints_norm, double alpha, double eps, const rvm_smala_cache* out, void* stream) {
    if (n_chains == 0) return 0;
    if (smala_bad_shape(n_params, n_chains) || !x || !smala_cache_ok(out) ||
        smala_bad_stencil(n_obs, floor_, lp_stencil, status_stencil, rv_stencil, inv_sigma2, rel_step, npoints_norm,
                          alpha))
        return at.bad("bad arguments");
    return at.done(rvm::launch_smala_derive(n_params, n_chains, n_obs, x, rel_step, floor_, lp_stencil, status_stencil,
                                            rv_stencil, inv_sigma2, npoints_norm, alpha, eps, smala_cache(out), sides,
                                            (hipStream_t)stream));
}

int rvm_smala_derive(int32_t n_params, int32_t n_chains, int32_t n_obs, const double* x, double rel_step,
                     const double* floor_, const double* lp_stencil, const int32_t* status_stencil,
                     const double* rv_stencil, const double* inv_sigma2, double npoints_norm, double alpha,
                     double eps, const rvm_smala_cache* out, void* stream) {
    return smala_derive({"rvm_smala_derive"}, 0, n_params, n_chains, n_obs, x, rel_step, floor_, lp_stencil,
                        status_stencil, rv_stencil, inv_sigma2, npoints_norm, alpha, eps, out, stream);
}

int rvm_smala_derive_sides(int32_t n_params, int32_t n_chains, int32_t n_obs, const double* x, double rel_step,
                           const double* floor_, const double* lp_stencil, const int32_t* status_stencil,
                           const double* rv_stencil, const double* inv_sigma2, double npoints_norm, double alpha,
                           double eps, const rvm_smala_cache* out, void* stream) {
    return smala_derive({"rvm_smala_derive_sides"}, 1, n_params, n_chains, n_obs, x, rel_step, floor_, lp_stencil,
                        status_stencil, rv_stencil, inv_sigma2, npoints_norm, alpha, eps, out, stream);
}

int rvm_smala_center_accept(int32_t n_params, int32_t n_chains, int64_t chain_begin, double* x, const double* x_prop,
                            const double* lp_center, const int32_t* status_center, const rvm_smala_cache* cur,
                            const rvm_smala_cache* prop, double eps, uint64_t seed, uint64_t iteration,
                            const double* draws, int32_t* accepted, int32_t* failures, void* stream) {
    const Entry at{"rvm_smala_center_accept"};
    if (n_chains == 0) return 0;
    if (smala_bad_shape(n_params, n_chains) || !x || !x_prop || !lp_center || !status_center || !smala_cache_ok(cur) ||
        !smala_cache_ok(prop))
        return at.bad("bad arguments");
    return at.done(rvm::launch_smala_center_accept(n_params, n_chains, chain_begin, x, smala_cache(cur), x_prop,
                                                   smala_cache(prop), lp_center, status_center, eps, seed, iteration,
                                                   draws, accepted, failures, (hipStream_t)stream));
}

int rvm_smala_metric(int32_t n_params, int32_t n_chains, const double* x, const double* lp, const int32_t* status,
                     const double* grad, const double* hess, double alpha, double eps, const rvm_smala_cache* out,
                     void* stream) {
    const Entry at{"rvm_smala_metric"};
    if (n_chains == 0) return 0;
    if (smala_bad_shape(n_params, n_chains) || !x || !lp || !status || !grad || !hess || !smala_cache_ok(out) ||
        !(alpha > 0.0))
        return at.bad("bad arguments");
    return at.done(rvm::launch_smala_metric(n_params, n_chains, x, lp, status, grad, hess, alpha, eps, smala_cache(out),
                                            (hipStream_t)stream));
}

int rvm_smala_derive_accept(int32_t n_params, int32_t n_chains, int64_t chain_begin, int32_t n_obs, double* x,
                            const double* x_prop, double rel_step, const double* floor_, const double* lp_stencil,
                            const int32_t* status_stencil, const double* rv_stencil, const double* inv_sigma2,
                            double npoints_norm, double alpha, double eps, const rvm_smala_cache* cur,
                            const rvm_smala_cache* prop, uint64_t seed, uint64_t iteration, const double* draws,
                            int32_t* accepted, int32_t* failures, void* stream) {
    const Entry at{"rvm_smala_derive_accept"};
    if (n_chains == 0) return 0;
    if (smala_bad_shape(n_params, n_chains) || !x || !x_prop || !smala_cache_ok(cur) || !smala_cache_ok(prop) ||
        smala_bad_stencil(n_obs, floor_, lp_stencil, status_stencil, rv_stencil, inv_sigma2, rel_step, npoints_norm,
                          alpha))
        return at.bad("bad arguments");
    return at.done(rvm::launch_smala_derive_accept(n_params, n_chains, n_obs, x_prop, rel_step, floor_, lp_stencil,
                                                   status_stencil, rv_stencil, inv_sigma2, npoints_norm, alpha, eps,
                                                   smala_cache(prop), chain_begin, x, smala_cache(cur), seed,
                                                   iteration, draws, accepted, failures, (hipStream_t)stream));
}

int rvm_smala_metric_accept(int32_t n_params, int32_t n_chains, int64_t chain_begin, double* x, const double* x_prop,
                            const double* lp, const int32_t* status, const double* grad, const double* hess,
                            double alpha, double eps, const rvm_smala_cache* cur, const rvm_smala_cache* prop,
                            uint64_t seed, uint64_t iteration, const double* draws, int32_t* accepted,
                            int32_t* failures, void* stream) {
    const Entry at{"rvm_smala_metric_accept"};
    if (n_chains == 0) return 0;
    if (smala_bad_shape(n_params, n_chains) || !x || !x_prop || !lp || !status || !grad || !hess ||
        !smala_cache_ok(cur) || !smala_cache_ok(prop) || !(alpha > 0.0))
        return at.bad("bad arguments");
    return at.done(rvm::launch_smala_metric_accept(n_params, n_chains, x_prop, lp, status, grad, hess, alpha, eps,
                                                   smala_cache(prop), chain_begin, x, smala_cache(cur), seed,
                                                   iteration, draws, accepted, failures, (hipStream_t)stream));
}

int rvm_smala_propose(int32_t n_params, int32_t n_chains, int64_t chain_begin, const double* x,
                      const rvm_smala_cache* cur, double eps, uint64_t seed, uint64_t iteration,
                      const double* draws, double* x_prop, void* stream) {
    const Entry at{"rvm_smala_propose"};
    if (n_chains == 0) return 0;
    if (smala_bad_shape(n_params, n_chains) || !x || !x_prop || !smala_cache_ok(cur)) return at.bad("bad arguments");
    return at.done(rvm::launch_smala_propose(n_params, n_chains, chain_begin, x, smala_cache(cur), eps, seed, iteration,
                                             draws, x_prop, (hipStream_t)stream));
}

int rvm_smala_accept(int32_t n_params, int32_t n_chains, int64_t chain_begin, double* x, const rvm_smala_cache* cur,
                     const double* x_prop, const rvm_smala_cache* prop, double eps, uint64_t seed,
                     uint64_t iteration, const double* draws, int32_t* accepted, int32_t* failures, void* stream) {
    const Entry at{"rvm_smala_accept"};
    if (n_chains == 0) return 0;
    if (smala_bad_shape(n_params, n_chains) || !x || !x_prop || !smala_cache_ok(cur) || !smala_cache_ok(prop))
        return at.bad("bad arguments");
    return at.done(rvm::launch_smala_accept(n_params, n_chains, chain_begin, x, smala_cache(cur), x_prop,
                                            smala_cache(prop), eps, seed, iteration, draws, accepted, failures,
                                            (hipStream_t)stream));
}

}  // extern "C"
