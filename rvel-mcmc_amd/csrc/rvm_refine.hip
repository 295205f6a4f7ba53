// rvm_refine.hip -- dispatch of the refinement and eager kernels (rvm_refine_impl.h; instantiated per
// planet count in rvm_refine_np<N>.hip) and the launch-generation bump.
#include "rvm_launch.h"
#include "rvm_refine_impl.h"

namespace rvm {

// After an eager or hedged launch (run_logl, once the side stream has joined): the next launch generation
// (the refinement kernel advances it itself when no eager or hedge blocks share its generation)
__global__ void gen_bump_kernel(unsigned long long* gen_dev) {
    if (threadIdx.x == 0) __hip_atomic_fetch_add(gen_dev, 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

hipError_t launch_gen_bump(const DevPlan& P, hipStream_t stream) {
    gen_bump_kernel<<<dim3(1), dim3(64), 0, stream>>>(P.gen_dev);
    return hipGetLastError();
}

// the five entry points of a planet count's translation unit (rvm_refine_np<N>.hip), by plan
struct RefineOps {
    decltype(&launch_refine_np1) refine;
    decltype(&launch_eager_np1) eager;
    decltype(&hedge_groups_np1) groups;
    decltype(&launch_hedge_np1) hedge;
    decltype(&prepare_refine_np1) prepare;
};
static const RefineOps* refine_ops(const DevPlan& P) {
#define RVM_OPS(N) {launch_refine_np##N, launch_eager_np##N, hedge_groups_np##N, launch_hedge_np##N, prepare_refine_np##N}
    static const RefineOps ops[4] = {RVM_OPS(1), RVM_OPS(2), RVM_OPS(3), RVM_OPS(4)};
#undef RVM_OPS
    return P.n_planets >= 1 && P.n_planets <= 4 ? &ops[P.n_planets - 1] : nullptr;
}

hipError_t launch_eager(const DevPlan& P, int W, const double* params, double hill_factor, hipStream_t stream) {
    const RefineOps* o = refine_ops(P);
    return o ? o->eager(P, W, params, hill_factor, stream) : hipErrorInvalidValue;
}

// groups a hedged pass 2 of this fused stretch launch may take (rvm_refine_impl.h hedge_kernel; 0: none)
int hedge_groups(const DevPlan& P, int W, int logl_blocks) {
    const RefineOps* o = refine_ops(P);
    return o ? o->groups(P, W, logl_blocks) : 0;
}

hipError_t launch_hedge(const DevPlan& P, int W, double hill_factor, const StretchArgs& sa, int ngrp,
                        hipStream_t stream) {
    const RefineOps* o = refine_ops(P);
    return o ? o->hedge(P, W, hill_factor, sa, ngrp, stream) : hipErrorInvalidValue;
}

hipError_t launch_refine(const DevPlan& P, int W, const double* params, double hill_factor, double* logl,
                         int32_t* status, double* rv_out, const StretchArgs& sa, int eager, int hedge,
                         hipStream_t stream) {
    if (P.rmax <= 0 || P.rq_n == nullptr) return hipSuccess;
    const RefineOps* o = refine_ops(P);
    return o ? o->refine(P, W, params, hill_factor, logl, status, rv_out, sa, eager, hedge, stream) : hipErrorInvalidValue;
}

// rvm_plan_create: set the refinement kernel's LDS attribute for the plan's instantiation and check
// that the plan's schedule fits it (hipErrorInvalidConfiguration otherwise)
hipError_t prepare_refine(const DevPlan& P) {
    if (P.rmax <= 0 || P.rq_n == nullptr) return hipSuccess;
    const RefineOps* o = refine_ops(P);
    return o ? o->prepare(P) : hipErrorInvalidValue;
}

}  // namespace rvm
