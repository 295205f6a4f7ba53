// rvm_summary.hip -- what the recorded chain says about the posterior, read on the device: exact
// quantiles of many long rows of doubles (the parameters of a chain, the epochs of an rv_out matrix),
// the parameters' covariance, and states drawn from the chain (rvmcmc/chain.py summary / draw / predict;
// driver.py:265-333 is the reference's host side).
//
// All entry points are stream-ordered launches without allocation, synchronisation or floating-point
// atomics.  The quantiles count with integer adds (whose sums do not depend on their order) and the
// covariance has one fixed summation order (include/rvmcmc.h), so the same inputs give the same bits
// from run to run.  No block waits on another: every dependency is a launch boundary.
#include <hip/hip_runtime.h>
#include <math.h>

#include "rvm_block_sum.h"
#include "rvm_device.h"
#include "rvm_internal.h"
#include "rvm_launch.h"
#include "rvm_stretch.h"

namespace rvm {

// ---- quantiles: a radix select ------------------------------------------------------------------------
// A row's order statistics are found on the order-preserving key of its values (sel_key), eight bits at a
// time from the top.  A target is one rank wanted of the row -- lo and hi of every quantile, 2 n_q <= 32 of
// them -- and carries the key bits found so far (its prefix) and its rank among the elements that share
// them.  Targets with the same prefix form a group: they need the same histogram.  One pass is
//   select_hist_kernel    several blocks per row: for every element and every group whose prefix the
//                         element's key continues, count the key's next digit in the block's LDS histogram;
//                         then one integer add per non-empty bin and block into the workspace;
//   select_narrow_kernel  one block per row: every target finds the digit whose bin holds its rank,
//                         appends it to its prefix, and the groups are formed anew; the histograms are
//                         cleared for the next pass.
// Pass 0 counts every non-NaN element in one group; its narrowing also learns m, the number of such
// elements, and with it the ranks.  After pass 7 a target's prefix is the whole key of v[rank].
constexpr int SEL_BLOCK = 256;
constexpr int SEL_BINS = 256;                 // 8-bit digits: 8 passes over a 64-bit key
constexpr int SEL_PASSES = 8;
constexpr int SEL_TARGETS = 2 * RVM_MAX_QUANTILES;  // 32: a block's histograms are 32 KiB of LDS
constexpr int SEL_SEG = 2048;                 // elements of a work unit: 256 threads x 8, along i
constexpr int SEL_MAX_BLOCKS = 2048;          // hist blocks of a launch (over all rows), about 8 per CU

struct SelState {  // per row, in the workspace
    uint64_t m;                       // non-NaN elements (pass 0)
    uint32_t n_groups, pad;           // 0: nothing to count (m = 0)
    uint64_t gprefix[SEL_TARGETS];    // a group's key bits above the current digit, the rest 0
    uint32_t tgroup[SEL_TARGETS];     // target -> group
    uint32_t trank[SEL_TARGETS];      // target's rank among the elements of its group
};

// negatives: all bits flipped; the rest: the sign bit flipped.  -0 < +0, -inf first, +inf last.
__device__ __forceinline__ uint64_t sel_key(uint64_t bits) {
    return (bits >> 63) ? ~bits : (bits ^ 0x8000000000000000ull);
}
__device__ __forceinline__ double sel_value(uint64_t key) {
    return __longlong_as_double((long long)((key >> 63) ? (key ^ 0x8000000000000000ull) : ~key));
}

// hist [n_rows][T][256] <- 0 ; every row: one group with the empty prefix
__global__ void __launch_bounds__(SEL_BLOCK) select_init_kernel(int T, SelState* __restrict__ states,
                                                                uint32_t* __restrict__ hist) {
    const size_t row = blockIdx.y;
    hist[(row * T + blockIdx.x) * SEL_BINS + threadIdx.x] = 0u;
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        states[row].m = 0;
        states[row].n_groups = 1;
        states[row].gprefix[0] = 0;
    }
}

// Block (b, row) counts the work units [b upb, (b + 1) upb) of its row: unit u is the segment
// [2048 s, 2048 s + 2048) of the line o, u = o segs + s.  VEC (x 16-byte aligned, both strides even):
// 16-byte loads, a thread takes the pairs (256 k + tid), k < 4, of the segment; otherwise 8-byte loads of
// the elements 256 k + tid, k < 8.  Either way a wave reads consecutive addresses.  An element past the
// line's end reads as NaN, which is never counted.
template <bool VEC>
__global__ void __launch_bounds__(SEL_BLOCK)
    select_hist_kernel(const double* __restrict__ x, size_t row_stride, size_t outer_stride, uint64_t n_inner,
                       uint64_t segs, uint64_t units, uint64_t upb, int T, int shift,
                       const SelState* __restrict__ states, uint32_t* __restrict__ hist) {
    __shared__ uint32_t h[SEL_TARGETS * SEL_BINS];
    __shared__ uint64_t gp[SEL_TARGETS];
    const int tid = (int)threadIdx.x;
    const size_t row = blockIdx.y;
    const SelState* st = states + row;
    const int G = (int)st->n_groups;  // (<= T: select_narrow_kernel)
    const uint64_t u0 = (uint64_t)blockIdx.x * upb;
    if (G == 0 || G > T || u0 >= units) return;
    const uint64_t u1 = u0 + upb < units ? u0 + upb : units;
    for (int i = tid; i < G * SEL_BINS; i += SEL_BLOCK) h[i] = 0u;
    if (tid < G) gp[tid] = st->gprefix[tid];
    __syncthreads();
    const uint64_t himask = shift == 56 ? 0ull : ~0ull << (shift + 8);
    auto count = [&](double v) {
        const uint64_t bits = (uint64_t)__double_as_longlong(v);
        if ((bits & 0x7FFFFFFFFFFFFFFFull) > 0x7FF0000000000000ull) return;  // NaN
        const uint64_t key = sel_key(bits), kp = key & himask;
        const uint32_t d = (uint32_t)(key >> shift) & (SEL_BINS - 1);
        for (int g = 0; g < G; g++)
            if (kp == gp[g]) atomicAdd(&h[g * SEL_BINS + d], 1u);
    };
    const double* xr = x + row * row_stride;
    const double nan = RVM_QNAN;
    for (uint64_t u = u0; u < u1; u++) {
        const uint64_t o = u / segs, s = u - o * segs;
        const double* line = xr + o * outer_stride;
        const uint64_t i0 = s * SEL_SEG;
        if (VEC) {
            double2 v[4];
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const uint64_t i = i0 + 2 * (uint64_t)(k * SEL_BLOCK + tid);
                v[k] = double2{nan, nan};
                if (i + 1 < n_inner)
                    v[k] = *reinterpret_cast<const double2*>(line + i);
                else if (i < n_inner)
                    v[k].x = line[i];
            }
#pragma unroll
            for (int k = 0; k < 4; k++) {
                count(v[k].x);
                count(v[k].y);
            }
        } else {
            double v[8];
#pragma unroll
            for (int k = 0; k < 8; k++) {
                const uint64_t i = i0 + (uint64_t)(k * SEL_BLOCK + tid);
                v[k] = i < n_inner ? line[i] : nan;
            }
#pragma unroll
            for (int k = 0; k < 8; k++) count(v[k]);
        }
    }
    __syncthreads();
    uint32_t* hr = hist + row * (size_t)T * SEL_BINS;
    for (int i = tid; i < G * SEL_BINS; i += SEL_BLOCK) {
        const uint32_t c = h[i];
        if (c) atomicAdd(&hr[i], c);
    }
}

// One block per row.  pass 0: m and the ranks lo = floor(q (m - 1)), hi = min(lo + 1, m - 1) first.
// Every pass: target t < T = 2 n_q walks its group's bins upwards to the one that holds its rank; then
// the groups of the next pass -- a target's group is the number of distinct prefixes among the targets
// before the first one that shares its own.  The last pass writes the quantiles.
__global__ void __launch_bounds__(SEL_BLOCK)
    select_narrow_kernel(int pass, SelQ Q, SelState* __restrict__ states, uint32_t* __restrict__ hist,
                         double* __restrict__ out, int64_t* __restrict__ n_valid) {
#pragma clang fp contract(off)
    __shared__ uint32_t h[SEL_TARGETS * SEL_BINS];
    __shared__ uint64_t npref[SEL_TARGETS];
    __shared__ int first[SEL_TARGETS];
    const int tid = (int)threadIdx.x, T = 2 * Q.n_q, shift = 56 - 8 * pass;
    const size_t row = blockIdx.x;
    SelState* st = states + row;
    const int G = (int)st->n_groups;
    if (G == 0 || G > T) return;  // (m = 0: the NaNs were written in pass 0)
    uint32_t* hr = hist + row * (size_t)T * SEL_BINS;
    for (int i = tid; i < G * SEL_BINS; i += SEL_BLOCK) {
        h[i] = hr[i];
        hr[i] = 0u;
    }
    __syncthreads();
    uint64_t m = st->m;
    if (pass == 0) {
        m = 0;
        for (int b = 0; b < SEL_BINS; b++) m += h[b];
        if (tid == 0) {
            st->m = m;
            if (n_valid) n_valid[row] = (int64_t)m;
            if (m == 0) st->n_groups = 0;
        }
        if (m == 0) {
            if (tid < Q.n_q) out[row * Q.n_q + tid] = RVM_QNAN;
            return;
        }
    }
    uint32_t rank = 0;
    if (tid < T) {
        int grp = 0;
        uint64_t prefix = 0;
        if (pass == 0) {
            const double hq = Q.q[tid >> 1] * (double)(m - 1);
            const uint64_t lo = (uint64_t)floor(hq), hi = lo + 1 < m ? lo + 1 : m - 1;
            rank = (uint32_t)((tid & 1) ? hi : (lo < m ? lo : m - 1));
        } else {
            grp = (int)st->tgroup[tid];
            grp = grp < G ? grp : G - 1;
            rank = st->trank[tid];
            prefix = st->gprefix[grp];
        }
        uint32_t below = 0, digit = SEL_BINS - 1;
        for (int b = 0; b < SEL_BINS; b++) {
            const uint32_t c = h[grp * SEL_BINS + b];
            if (rank - below < c) {
                digit = (uint32_t)b;
                break;
            }
            below += c;
        }
        rank -= below;
        npref[tid] = prefix | ((uint64_t)digit << shift);
    }
    __syncthreads();  // (every read of the row's state is done: it is rewritten below)
    if (tid < T) {
        int f = 0;
        while (npref[f] != npref[tid]) f++;
        first[tid] = f;
    }
    __syncthreads();
    if (tid < T) {
        const int f = first[tid];
        int g = 0;
        for (int k = 0; k < f; k++) g += first[k] == k;
        st->tgroup[tid] = (uint32_t)g;
        st->trank[tid] = rank;
        if (f == tid) st->gprefix[g] = npref[tid];
        if (tid == 0) {
            int n = 0;
            for (int k = 0; k < T; k++) n += first[k] == k;
            st->n_groups = (uint32_t)n;
        }
    }
    if (pass == SEL_PASSES - 1 && tid < Q.n_q) {
        const double vlo = sel_value(npref[2 * tid]), vhi = sel_value(npref[2 * tid + 1]);
        const double hq = Q.q[tid] * (double)(m - 1);
        const double g = hq - floor(hq);
        double r = vlo;
        if (!(g == 0.0 || vhi == vlo)) {
            const double step = g * (vhi - vlo);
            r = vlo + step;
        }
        out[row * Q.n_q + tid] = r;
    }
}

size_t rows_quantiles_workspace_bytes(int n_rows, int n_q) {
    return (size_t)n_rows * (sizeof(SelState) + (size_t)2 * n_q * SEL_BINS * sizeof(uint32_t));
}

hipError_t launch_rows_quantiles(const double* x, int n_rows, int64_t row_stride, int64_t n_outer,
                                 int64_t outer_stride, int64_t n_inner, const SelQ& Q, double* out,
                                 int64_t* n_valid, void* workspace, hipStream_t st) {
    const int T = 2 * Q.n_q;
    SelState* states = (SelState*)workspace;
    uint32_t* hist = (uint32_t*)(states + n_rows);
    const uint64_t segs = ((uint64_t)n_inner + SEL_SEG - 1) / SEL_SEG, units = segs * (uint64_t)n_outer;
    // blocks per row: at most SEL_MAX_BLOCKS over all rows, at least one; then as many as have a unit
    uint64_t bpr = (uint64_t)(SEL_MAX_BLOCKS / n_rows > 1 ? SEL_MAX_BLOCKS / n_rows : 1);
    if (bpr > units) bpr = units;
    const uint64_t upb = (units + bpr - 1) / bpr;
    bpr = (units + upb - 1) / upb;
    const bool vec = ((uintptr_t)x % 16 == 0) && row_stride % 2 == 0 && outer_stride % 2 == 0;
    select_init_kernel<<<dim3((unsigned)T, (unsigned)n_rows), SEL_BLOCK, 0, st>>>(T, states, hist);
    hipError_t e = hipGetLastError();
    for (int pass = 0; pass < SEL_PASSES && e == hipSuccess; pass++) {
        const int shift = 56 - 8 * pass;
        const dim3 grid((unsigned)bpr, (unsigned)n_rows);
        if (vec)
            select_hist_kernel<true><<<grid, SEL_BLOCK, 0, st>>>(x, (size_t)row_stride, (size_t)outer_stride,
                                                                 (uint64_t)n_inner, segs, units, upb, T, shift,
                                                                 states, hist);
        else
            select_hist_kernel<false><<<grid, SEL_BLOCK, 0, st>>>(x, (size_t)row_stride, (size_t)outer_stride,
                                                                  (uint64_t)n_inner, segs, units, upb, T, shift,
                                                                  states, hist);
        e = hipGetLastError();
        if (e != hipSuccess) break;
        select_narrow_kernel<<<dim3((unsigned)n_rows), SEL_BLOCK, 0, st>>>(pass, Q, states, hist, out, n_valid);
        e = hipGetLastError();
    }
    return e;
}

// ---- covariance ---------------------------------------------------------------------------------------
// chain_cov_kernel: block (parameter tile i, parameter tile j <= i, group of 64 walkers) is one wave; a
// thread is one walker with the 2 x 2 products of the parameters 2 i, 2 i + 1 and 2 j, 2 j + 1 as four
// accumulators,
//     acc[a][b] = fma(y_p, y_q, acc[a][b]),  t ascending,  y_p = x[t][p][w] - center[p] formed at use
// (a parameter past the last reads as y = 0), written per walker to sums[p][q][w] for p >= q.  Small tiles
// and one-wave blocks because the walkers and the pairs are all the parallelism there is: a walker's
// steps are one thread's, in order.
// chain_cov_finish_kernel: block (p, q <= p) adds the walkers in rvm_chain_autocov's order -- each block of
// 256 walkers by block_tree_sum (an absent walker is +0), the walker blocks in index order -- divides once and
// writes cov[p][q] and cov[q][p].
constexpr int CV_TILE = 2;
constexpr int CV_WAVE = 64;
constexpr int CV_BLOCK = BLOCK_SUM_THREADS;

__global__ void __launch_bounds__(CV_WAVE) chain_cov_kernel(const double* __restrict__ x,
                                                            const double* __restrict__ center, int P, int W,
                                                            long long t0, long long t1,
                                                            double* __restrict__ sums) {
    const int p0 = CV_TILE * (int)blockIdx.x, q0 = CV_TILE * (int)blockIdx.y;
    const int w = (int)blockIdx.z * CV_WAVE + (int)threadIdx.x;
    if (q0 > p0 || w >= W) return;
    const size_t PW = (size_t)P * W;
    const double* colp[CV_TILE];
    const double* colq[CV_TILE];
    double cp[CV_TILE], cq[CV_TILE];
    bool hp[CV_TILE], hq[CV_TILE];
#pragma unroll
    for (int a = 0; a < CV_TILE; a++) {
        hp[a] = p0 + a < P;
        hq[a] = q0 + a < P;
        colp[a] = x + (hp[a] ? (size_t)(p0 + a) * W + w : 0);
        colq[a] = x + (hq[a] ? (size_t)(q0 + a) * W + w : 0);
        cp[a] = hp[a] ? center[p0 + a] : 0.0;
        cq[a] = hq[a] ? center[q0 + a] : 0.0;
    }
    double acc[CV_TILE][CV_TILE];
#pragma unroll
    for (int a = 0; a < CV_TILE; a++)
#pragma unroll
        for (int b = 0; b < CV_TILE; b++) acc[a][b] = 0.0;
#pragma unroll 8
    for (long long t = t0; t < t1; t++) {
        double yp[CV_TILE], yq[CV_TILE];
#pragma unroll
        for (int a = 0; a < CV_TILE; a++) {
            yp[a] = hp[a] ? colp[a][(size_t)t * PW] - cp[a] : 0.0;
            yq[a] = hq[a] ? colq[a][(size_t)t * PW] - cq[a] : 0.0;
        }
#pragma unroll
        for (int a = 0; a < CV_TILE; a++)
#pragma unroll
            for (int b = 0; b < CV_TILE; b++) acc[a][b] = fma(yp[a], yq[b], acc[a][b]);
    }
#pragma unroll
    for (int a = 0; a < CV_TILE; a++)
#pragma unroll
        for (int b = 0; b < CV_TILE; b++) {
            const int p = p0 + a, q = q0 + b;
            if (p < P && q <= p) sums[((size_t)p * P + q) * W + w] = acc[a][b];
        }
}

__global__ void __launch_bounds__(CV_BLOCK) chain_cov_finish_kernel(const double* __restrict__ sums, int P, int W,
                                                                    long long nW, double* __restrict__ cov) {
    __shared__ double s[1][CV_BLOCK];
    const int p = (int)(blockIdx.x / (unsigned)P), q = (int)(blockIdx.x - (unsigned)p * (unsigned)P);
    if (q > p) return;
    const int tid = (int)threadIdx.x;
    const double* r = sums + ((size_t)p * P + q) * W;
    double total = 0.0;
    for (int w0 = 0; w0 < W; w0 += CV_BLOCK) {
        s[0][tid] = w0 + tid < W ? r[w0 + tid] : 0.0;
        block_tree_sum(s, tid);
        if (tid == 0) total = w0 == 0 ? s[0][0] : total + s[0][0];
        __syncthreads();
    }
    if (tid == 0) {
        const double v = nW > 1 ? total / (double)(nW - 1) : RVM_QNAN;
        cov[(size_t)p * P + q] = v;
        cov[(size_t)q * P + p] = v;
    }
}

// workspace doubles: [P][P][W], a walker's sums (the entries p >= q are used)
size_t chain_cov_workspace_doubles(int P, int W) { return (size_t)P * P * (size_t)W; }

hipError_t launch_chain_cov(const double* x, int P, int W, int64_t t0, int64_t t1, const double* center, double* cov,
                            double* sums, hipStream_t st) {
    const unsigned nt = blocks_of(P, CV_TILE);
    chain_cov_kernel<<<dim3(nt, nt, blocks_of(W, CV_WAVE)), CV_WAVE, 0, st>>>(
        x, center, P, W, t0, t1, sums);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    chain_cov_finish_kernel<<<dim3((unsigned)P * (unsigned)P), CV_BLOCK, 0, st>>>(sums, P, W,
                                                                                  (long long)(t1 - t0) * W, cov);
    return hipGetLastError();
}

// ---- draw ---------------------------------------------------------------------------------------------
// Sample s: step t = t0 + min(floor(u1 n), n - 1) and walker w = min(floor(u2 W), W - 1) -- the device's
// uniform can round to 1.0 -- of (u1, u2) = uniform2(seed, s, draw_id, RNG_CHAIN_DRAW) or draws[0][s], draws[1][s].
__device__ __forceinline__ long long draw_index(double u, long long n) {
#pragma clang fp contract(off)
    const double d = floor(u * (double)n);
    return d >= (double)n ? n - 1 : (d > 0.0 ? (long long)d : 0);
}

__global__ void __launch_bounds__(256) chain_draw_kernel(const double* __restrict__ x, int P, int W, long long t0,
                                                         long long t1, int S, uint64_t seed, uint64_t draw_id,
                                                         const double* __restrict__ draws, double* __restrict__ xo,
                                                         int64_t* __restrict__ idx) {
    const int s = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (s >= S) return;
    double u1, u2;
    if (draws) {
        u1 = draws[s];
        u2 = draws[(size_t)S + s];
    } else {
        uniform2(seed, (uint64_t)s, draw_id, RNG_CHAIN_DRAW, u1, u2);
    }
    const long long t = t0 + draw_index(u1, t1 - t0), w = draw_index(u2, (long long)W);
    const double* src = x + (size_t)t * P * W + w;
    for (int p = 0; p < P; p++) xo[(size_t)p * S + s] = src[(size_t)p * W];
    if (idx) idx[s] = (int64_t)(t * W + w);
}

hipError_t launch_chain_draw(const double* x, int P, int W, int64_t t0, int64_t t1, int S, uint64_t seed,
                             uint64_t draw_id, const double* draws, double* xo, int64_t* idx, hipStream_t st) {
    chain_draw_kernel<<<dim3(blocks_of(S, 256)), 256, 0, st>>>(x, P, W, t0, t1, S, seed, draw_id, draws, xo, idx);
    return hipGetLastError();
}

}  // namespace rvm
