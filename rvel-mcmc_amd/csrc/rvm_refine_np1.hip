// rvm_refine_np1.hip -- the refinement and eager kernels for 1-planet plans (rvm_refine_impl.h);
// one translation unit per planet count so that the build compiles them in parallel
#include "rvm_refine_impl.h"

namespace rvm {

hipError_t launch_refine_np1(const DevPlan& P, int W, const double* params, double hill_factor, double* logl,
                              int32_t* status, double* rv_out, const StretchArgs& sa, int eager, int hedge,
                              hipStream_t stream) {
    return P.inclined ? launch_refine_t<1, true>(P, W, params, hill_factor, logl, status, rv_out, sa, eager, hedge, stream)
                      : launch_refine_t<1, false>(P, W, params, hill_factor, logl, status, rv_out, sa, eager, hedge, stream);
}

hipError_t launch_eager_np1(const DevPlan& P, int W, const double* params, double hill_factor, hipStream_t stream) {
    return P.inclined ? launch_eager_t<1, true>(P, W, params, hill_factor, stream)
                      : launch_eager_t<1, false>(P, W, params, hill_factor, stream);
}

int hedge_groups_np1(const DevPlan& P, int W, int logl_blocks) {
    return P.inclined ? hedge_groups_t<1, true>(P, W, logl_blocks) : hedge_groups_t<1, false>(P, W, logl_blocks);
}

hipError_t launch_hedge_np1(const DevPlan& P, int W, double hill_factor, const StretchArgs& sa, int ngrp,
                             hipStream_t stream) {
    return P.inclined ? launch_hedge_t<1, true>(P, W, hill_factor, sa, ngrp, stream)
                      : launch_hedge_t<1, false>(P, W, hill_factor, sa, ngrp, stream);
}

hipError_t prepare_refine_np1(const DevPlan& P) {
    return P.inclined ? prepare_refine_t<1, true>(P) : prepare_refine_t<1, false>(P);
}

}  // namespace rvm
