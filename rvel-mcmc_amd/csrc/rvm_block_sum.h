// rvm_block_sum.h -- the fixed-order sum over a block of 256 threads that include/rvmcmc.h promises bit for bit
// (rvm_chain_autocov step 2, rvm_chain_cov, rvm_pt_ladder_update's moments) and the tests restate
// (tests/chain_ref.py, summary_ref.py, pt_adapt_ref._block_sum).
#pragma once
#include <hip/hip_runtime.h>

namespace rvm {

constexpr int BLOCK_SUM_THREADS = 256;

// block_tree_sum: ROWS sums side by side over the block's 256 LDS slots s[r][0 .. 255].  On entry thread tid has
// stored its own term in s[r][tid] for every r (an absent term as +0) and no barrier has run yet; then
//     barrier ; for h = 128, 64, ..., 1:  if tid < h: s[r][tid] = s[r][tid] + s[r][tid + h], r ascending ; barrier
// and on return s[r][0] is row r's sum, visible to every thread of the block.  Every thread of the block calls it
// (the barriers are the block's).  The body is additions only -- nothing a compiler may contract into a fused
// multiply-add -- so the translation units' different contraction settings (-ffp-contract=off for rvm_gls.hip,
// per-function pragmas elsewhere) cannot reach it: the same bits wherever it is instantiated.
template <typename T, int ROWS>
__device__ __forceinline__ void block_tree_sum(T (&s)[ROWS][BLOCK_SUM_THREADS], int tid) {
    __syncthreads();
    for (int h = BLOCK_SUM_THREADS / 2; h > 0; h >>= 1) {
        if (tid < h) {
#pragma unroll
            for (int r = 0; r < ROWS; r++) s[r][tid] = s[r][tid] + s[r][tid + h];
        }
        __syncthreads();
    }
}

}  // namespace rvm
