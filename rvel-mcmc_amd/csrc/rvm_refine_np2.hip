// rvm_refine_np2.hip -- the refinement, eager and hedge kernels for 2-planet plans (rvm_refine_impl.h);
// one translation unit per planet count so that the build compiles them in parallel
#include "rvm_refine_impl.h"

RVM_REFINE_NP_DEFINE(2)

// (timing build: the 2-planet refinement kernel's per-wave records, scripts/probe/refine_prof.py)
#ifdef RVM_PROFILE
extern "C" int rvm_rprof_copy(void* host, size_t bytes) {
    const size_t n = bytes < sizeof(rvm::rvm_rprof) ? bytes : sizeof(rvm::rvm_rprof);
    return (int)hipMemcpyFromSymbol(host, HIP_SYMBOL(rvm::rvm_rprof), n, 0, hipMemcpyDeviceToHost);
}
extern "C" int rvm_rprof_clear(void) {
    static unsigned long long zero[RVM_RPROF_MAX_WAVES * RVM_RPROF_SLOTS];
    return (int)hipMemcpyToSymbol(HIP_SYMBOL(rvm::rvm_rprof), zero, sizeof(zero), 0, hipMemcpyHostToDevice);
}
#endif
