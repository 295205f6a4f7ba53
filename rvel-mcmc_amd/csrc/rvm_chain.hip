// rvm_chain.hip -- the recorded chain on the device: recording a sampler's positions into a step slot,
// per-column moments, and the walker-averaged autocovariance that the integrated autocorrelation time
// is read from (rvmcmc/chain.py; driver.integrated_time is the host restatement).
//
// A chain is [n_steps][P][W] float64: one recorded step is the SoA block [P][W] every sampler holds.
// All three entry points are stream-ordered launches without allocation, synchronisation or
// floating-point atomics; every sum has one fixed order (include/rvmcmc.h), so the same inputs give
// the same bits from run to run.
#include <hip/hip_runtime.h>
#include <math.h>

#include "rvm_block_sum.h"
#include "rvm_internal.h"
#include "rvm_launch.h"

namespace rvm {

// ---- record -----------------------------------------------------------------------------------------
// Row r < P: dst[r][d0 + j] = src[r][c0 + j cs]; row P (when launched): the log-probabilities, the same
// gather.  One thread per (row, j); the stores are coalesced, the loads strided by cs.
__global__ void __launch_bounds__(256) chain_record_kernel(int P, int n, const double* __restrict__ src, size_t src_ld,
                                                           size_t c0, size_t cs, double* __restrict__ dst,
                                                           size_t dst_ld, size_t d0,
                                                           const double* __restrict__ lsrc,
                                                           double* __restrict__ ldst) {
    const unsigned uj = blockIdx.x * blockDim.x + threadIdx.x;
    if (uj >= (unsigned)n) return;
    const size_t j = uj, row = blockIdx.y;
    if (row < (size_t)P)
        dst[row * dst_ld + d0 + j] = src[row * src_ld + c0 + j * cs];
    else
        ldst[d0 + j] = lsrc[c0 + j * cs];
}

// ---- moments ----------------------------------------------------------------------------------------
// One thread carries column c = p W + w through the steps [t0, t1), twice: the sum left to right and
// one division, then the squared deviations left to right (no contraction: d * d is rounded before it
// is added, as a plain IEEE restatement does).  Consecutive threads read consecutive addresses.
__global__ void __launch_bounds__(256) chain_moments_kernel(const double* __restrict__ x, size_t PW, long long t0,
                                                            long long t1, double* __restrict__ mean,
                                                            double* __restrict__ m2) {
#pragma clang fp contract(off)
    const size_t c = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= PW) return;
    double s = 0.0;
    for (long long t = t0; t < t1; t++) s = s + x[(size_t)t * PW + c];
    const double mu = s / (double)(t1 - t0);
    double q = 0.0;
    for (long long t = t0; t < t1; t++) {
        const double d = x[(size_t)t * PW + c] - mu;
        q = q + d * d;
    }
    mean[c] = mu;
    m2[c] = q;
}

// ---- autocovariance ---------------------------------------------------------------------------------
// Block (lag tile, walker block, parameter): 256 threads = 256 walkers of parameter p, each with the 16
// lags k0 .. k0 + 15 of its tile (k0 = lag0 + 16 tile) as 16 accumulators.  A thread walks t upwards
// once and keeps y[t + k0 .. t + k0 + 15] in a ring of 16 registers, so a step costs two loads -- y[t]
// and the ring's new entry y[t + k0 + 16] -- for its 16 fused multiply-adds
//     acc[i] = fma(y[t], y[t + k0 + i], acc[i]),   y = x - mean[p][w] formed at use.
// The loop is unrolled 16 times so that every ring index is a compile-time constant (no register
// moves, no runtime-indexed array).  The tails need no branches: y reads as 0 at every step >= t1 (and
// in the threads past the last walker), and a product with such a y adds an exact +0 -- that covers
// t + k running past t1 - 1, the tile's lags past lag0 + n_lags - 1 (computed, never stored past the
// padded workspace row) and W not a multiple of 256.
// Then the block's 256 walkers by block_tree_sum, the 16 lags side by side, one partial per lag to
// part[p][16 tile + i][walker block]; chain_autocov_finish_kernel adds the walker blocks in index
// order and divides by W.
constexpr int CH_TILE = 16;
constexpr int CH_BLOCK = BLOCK_SUM_THREADS;

__global__ void __launch_bounds__(CH_BLOCK) chain_autocov_kernel(const double* __restrict__ x,
                                                                 const double* __restrict__ mean, int P, int W,
                                                                 long long t0, long long t1, int lag0,
                                                                 double* __restrict__ part) {
    __shared__ double s[CH_TILE][CH_BLOCK];
    const int tid = (int)threadIdx.x;
    const int w = (int)blockIdx.y * CH_BLOCK + tid, p = (int)blockIdx.z;
    const long long k0 = (long long)lag0 + CH_TILE * (long long)blockIdx.x;  // (<= t1 - t0 - 1: rvm_abi.hip)
    const bool live = w < W;
    const size_t stride = (size_t)P * W;
    const double* col = x + (size_t)p * W + (live ? w : 0);
    const double mu = live ? mean[(size_t)p * W + w] : 0.0;
    auto y = [&](long long t) -> double { return (live && t < t1) ? col[(size_t)t * stride] - mu : 0.0; };

    double acc[CH_TILE], r[CH_TILE];
#pragma unroll
    for (int i = 0; i < CH_TILE; i++) {
        acc[i] = 0.0;
        r[i] = y(t0 + k0 + i);
    }
    // at sub-step tt of a chunk starting at t: r[(tt + i) & 15] = y[t + tt + k0 + i]
    for (long long t = t0; t < t1 - k0; t += CH_TILE) {
#pragma unroll
        for (int tt = 0; tt < CH_TILE; tt++) {
            const double yt = y(t + tt);
#pragma unroll
            for (int i = 0; i < CH_TILE; i++) acc[i] = fma(yt, r[(tt + i) & (CH_TILE - 1)], acc[i]);
            r[tt] = y(t + tt + k0 + CH_TILE);
        }
    }
#pragma unroll
    for (int i = 0; i < CH_TILE; i++) s[i][tid] = acc[i];
    block_tree_sum(s, tid);
    if (tid < CH_TILE) {
        const size_t lpad = (size_t)CH_TILE * gridDim.x;
        part[((size_t)p * lpad + (size_t)CH_TILE * blockIdx.x + tid) * gridDim.y + blockIdx.y] = s[tid][0];
    }
}

// acov[p][j] = (part[p][j][0] + part[p][j][1] + ... left to right) / W, one thread per (p, j)
__global__ void __launch_bounds__(256) chain_autocov_finish_kernel(const double* __restrict__ part, int P, int n_lags,
                                                                   int lpad, int nwb, int W,
                                                                   double* __restrict__ acov) {
    const unsigned ui = blockIdx.x * blockDim.x + threadIdx.x;
    if (ui >= (unsigned)P * (unsigned)n_lags) return;
    const int p = (int)(ui / (unsigned)n_lags), j = (int)(ui - (unsigned)p * (unsigned)n_lags);
    const double* q = part + ((size_t)p * lpad + j) * nwb;
    double a = q[0];
    for (int b = 1; b < nwb; b++) a = a + q[b];
    acov[(size_t)p * n_lags + j] = a / (double)W;
}

hipError_t launch_chain_record(int P, int n, const double* src, int64_t src_ld, int64_t c0, int64_t cs, double* dst,
                               int64_t dst_ld, int64_t d0, const double* lsrc, double* ldst, hipStream_t st) {
    const dim3 grid(blocks_of(n, 256), (unsigned)(P + (lsrc ? 1 : 0)));
    chain_record_kernel<<<grid, 256, 0, st>>>(P, n, src, (size_t)src_ld, (size_t)c0, (size_t)cs, dst, (size_t)dst_ld,
                                              (size_t)d0, lsrc, ldst);
    return hipGetLastError();
}

hipError_t launch_chain_moments(const double* x, int P, int W, int64_t t0, int64_t t1, double* mean, double* m2,
                                hipStream_t st) {
    const size_t PW = (size_t)P * W;
    chain_moments_kernel<<<dim3(blocks_of(PW, 256)), 256, 0, st>>>(x, PW, t0, t1, mean, m2);
    return hipGetLastError();
}

// workspace doubles: [P][16 tiles][walker blocks]
size_t chain_autocov_workspace_doubles(int P, int W, int n_lags) {
    return (size_t)P * CH_TILE * (size_t)blocks_of(n_lags, CH_TILE) * (size_t)blocks_of(W, CH_BLOCK);
}

hipError_t launch_chain_autocov(const double* x, const double* mean, int P, int W, int64_t t0, int64_t t1, int lag0,
                                int n_lags, double* acov, double* part, hipStream_t st) {
    const unsigned tiles = blocks_of(n_lags, CH_TILE), nwb = blocks_of(W, CH_BLOCK);
    chain_autocov_kernel<<<dim3(tiles, nwb, (unsigned)P), CH_BLOCK, 0, st>>>(x, mean, P, W, t0, t1, lag0, part);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    chain_autocov_finish_kernel<<<dim3(blocks_of(P * n_lags, 256)), 256, 0, st>>>(
        part, P, n_lags, (int)(CH_TILE * tiles), (int)nwb, W, acov);
    return hipGetLastError();
}

}  // namespace rvm
