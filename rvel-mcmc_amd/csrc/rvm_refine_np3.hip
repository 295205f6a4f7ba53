// rvm_refine_np3.hip -- the refinement, eager and hedge kernels for 3-planet plans (rvm_refine_impl.h);
// one translation unit per planet count so that the build compiles them in parallel
#include "rvm_refine_impl.h"

RVM_REFINE_NP_DEFINE(3)
