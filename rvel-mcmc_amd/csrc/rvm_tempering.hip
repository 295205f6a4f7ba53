// rvm_tempering.hip -- parallel tempering of the affine-invariant ensemble: n_temps ensembles of W
// walkers at inverse temperatures betas[0] = 1 > betas[1] > ... > 0 (temperature 0 the coldest).
//
//   * the stretch proposal of all temperatures' walkers of one half in ONE launch (each walker's
//     partner comes from the other half of its own temperature), so that one likelihood launch
//     evaluates the n_temps * W / 2 proposals;
//   * the tempered accept, beta_t on both log-probabilities (rvm_stretch.h stretch_accepts_tempered);
//   * the exchange sweep between neighbouring temperatures.
// Each half is SoA [n_params][n_temps * Wh] float64, Wh = W / 2, column i = t * Wh + k; lnp holds the
// UNtempered log-probabilities [n_temps * Wh].  The Philox item of walker k of half h at temperature
// t is g = t * W + h * Wh + k: at n_temps = 1 the global walker index of rvm_samplers.hip's stretch
// kernels, whose results these kernels then reproduce bit for bit.
#include <hip/hip_runtime.h>
#include <math.h>

#include "rvm_block_sum.h"
#include "rvm_device.h"
#include "rvm_internal.h"
#include "rvm_launch.h"
#include "rvm_stretch.h"

// No FMA contraction (as rvm_samplers.hip): bit-identical to a plain IEEE restatement (numpy).
#pragma clang fp contract(off)

namespace rvm {

__global__ void pt_stretch_propose_kernel(int P, int T, int Wh, const double* __restrict__ x,
                                          const double* __restrict__ c, double a, uint64_t seed, uint64_t iteration,
                                          uint32_t half, const double* __restrict__ draws, double* __restrict__ q,
                                          double* __restrict__ zout) {
    const int n = T * Wh;
    const unsigned ui = blockIdx.x * blockDim.x + threadIdx.x;  // (< 2^32: n <= INT32_MAX, rvm_abi.hip)
    if (ui >= (unsigned)n) return;
    const int i = (int)ui;
    const int t = i / Wh, k = i - t * Wh;
    double z;
    int j;
    if (draws)
        stretch_zj(draws[i], draws[(size_t)n + i], a, Wh, z, j);
    else
        stretch_draw(seed, (uint64_t)t * (2u * (uint64_t)Wh) + (uint64_t)half * Wh + k, iteration, half, a, Wh, z, j);
    const size_t cj = (size_t)t * Wh + j;  // the partner: same temperature, other half
    for (int p = 0; p < P; p++) q[(size_t)p * n + i] = stretch_q(c[(size_t)p * n + cj], z, x[(size_t)p * n + i]);
    zout[i] = z;
}

__global__ void pt_stretch_accept_kernel(int P, int T, int Wh, const double* __restrict__ betas,
                                         double* __restrict__ x, double* __restrict__ lnp,
                                         const double* __restrict__ q, const double* __restrict__ lnp_new,
                                         const double* __restrict__ z, uint64_t seed, uint64_t iteration,
                                         uint32_t half, const double* __restrict__ draws,
                                         int32_t* __restrict__ accepted) {
    const int n = T * Wh;
    const unsigned ui = blockIdx.x * blockDim.x + threadIdx.x;  // (< 2^32: n <= INT32_MAX, rvm_abi.hip)
    if (ui >= (unsigned)n) return;
    const int i = (int)ui;
    const int t = i / Wh, k = i - t * Wh;
    const double u3 =
        draws ? draws[i]
              : stretch_u3(seed, (uint64_t)t * (2u * (uint64_t)Wh) + (uint64_t)half * Wh + k, iteration, half);
    if (stretch_accepts_tempered(P, z[i], betas[t], lnp_new[i], lnp[i], u3)) {
        for (int p = 0; p < P; p++) x[(size_t)p * n + i] = q[(size_t)p * n + i];
        lnp[i] = lnp_new[i];
        if (accepted) accepted[i] += 1;
    }
}

// One thread owns walker index w = h * Wh + k of every temperature through the whole sweep (pairs
// T-2 .. 0, hottest first): it alone reads and writes column t * Wh + k of half h, so the sweep
// needs no atomics and is deterministic.  x0 and x1 (lnp0 and lnp1) are distinct buffers, each
// touched by its own half's threads only.
__global__ void pt_swap_kernel(int P, int T, int Wh, const double* __restrict__ betas, double* x0, double* x1,
                               double* lnp0, double* lnp1, uint64_t seed, uint64_t iteration,
                               const double* __restrict__ draws, int32_t* __restrict__ swapped) {
    const int W = 2 * Wh;
    const unsigned uw = blockIdx.x * blockDim.x + threadIdx.x;
    if (uw >= (unsigned)W) return;
    const int w = (int)uw;
    const int h = w / Wh, k = w - h * Wh;
    double* x = h ? x1 : x0;
    double* lnp = h ? lnp1 : lnp0;
    const size_t n = (size_t)T * Wh;
    double l_hot = lnp[(size_t)(T - 1) * Wh + k];
    for (int p = T - 2; p >= 0; p--) {
        const size_t ic = (size_t)p * Wh + k, ih = ic + Wh;  // the pair's colder and hotter column
        const size_t item = (size_t)p * W + w;
        const double l_cold = lnp[ic];
        double u, unused;
        if (draws)
            u = draws[item];
        else
            uniform2(seed, (uint64_t)item, iteration, RNG_PT_SWAP, u, unused);
        if (pt_swaps(betas[p], betas[p + 1], l_cold, l_hot, u)) {
            for (int r = 0; r < P; r++) {
                const double xc = x[(size_t)r * n + ic];
                x[(size_t)r * n + ic] = x[(size_t)r * n + ih];
                x[(size_t)r * n + ih] = xc;
            }
            lnp[ic] = l_hot;
            lnp[ih] = l_cold;
            swapped[item] += 1;
            // (temperature p now holds what came down from p + 1: l_hot stays for the next pair)
        } else {
            l_hot = l_cold;
        }
    }
}

// ---- the ladder's statistics and dynamics (rvm_pt_ladder_update) -----------------------------------
// One block of 256 threads per row.  Rows 0 .. T-2: the int64 total of the cumulative counter row
// swapped[p][0..W) (integer sums do not depend on the order).  Rows T-1 .. 2T-2 (launched only when
// the moments are asked for): sum lnp and sum lnp^2 over temperature t's W walkers in the index
// order j = 0 .. W-1 (half 0's columns t Wh .. t Wh + Wh - 1, then half 1's): thread i adds j = i,
// i + 256, ... in that order, then block_tree_sum over the 256 slots, the two sums side by side -- a
// fixed order, no atomics, the same bits from run to run.
__global__ void __launch_bounds__(BLOCK_SUM_THREADS) pt_ladder_stats_kernel(PtLadderArgs g) {
    __shared__ int64_t sn[1][BLOCK_SUM_THREADS];
    __shared__ double sm[2][BLOCK_SUM_THREADS];  // sum lnp, sum lnp^2
    const int tid = (int)threadIdx.x, row = (int)blockIdx.x;  // (the branches below are block-uniform)
    const int Wh = g.Wh, W = 2 * g.Wh;
    if (row < g.T - 1) {
        const int32_t* r = g.swapped + (size_t)row * W;
        int64_t part = 0;
        for (int w = tid; w < W; w += BLOCK_SUM_THREADS) part += r[w];
        sn[0][tid] = part;
        block_tree_sum(sn, tid);
        if (tid == 0) g.ws_totals[row] = sn[0][0];
        return;
    }
    const int t = row - (g.T - 1);
    if (t >= g.T) return;
    const double* l0 = g.lnp0 + (size_t)t * Wh;
    const double* l1 = g.lnp1 + (size_t)t * Wh;
    double a = 0.0, b = 0.0;
    for (int j = tid; j < W; j += BLOCK_SUM_THREADS) {
        const double v = j < Wh ? l0[j] : l1[j - Wh];
        a = a + v;
        b = b + v * v;
    }
    sm[0][tid] = a;
    sm[1][tid] = b;
    block_tree_sum(sm, tid);
    if (tid == 0) {
        g.ws_moments[2 * t] = sm[0][0];
        g.ws_moments[2 * t + 1] = sm[1][0];
    }
}

// The dynamics of Vousden, Farr & Mandel 2016 with both end temperatures fixed, every expression
// left to right:
//   dS[i] = kappa (A[i] - A[i+1]) ; dT[i] = (1/beta[i+1] - 1/beta[i]) exp(dS[i]) ;
//   acc = 1/beta[0] ; acc = acc + dT[i] ; new[i+1] = 1 / acc                       i = 0 .. T-3
// With store = false only the verdict: ok (every new beta finite, the ladder still strictly
// decreasing down to the fixed beta[T-1]) and driven (some dS != 0).  The second pass repeats the
// same operations on the same inputs (beta[i+1] is read before it is overwritten), so it stores
// exactly what the first one judged, with no scratch array and no bound on T.
__device__ static void pt_ladder_pass(const PtLadderArgs& g, bool store, bool& ok, bool& driven) {
    const int T = g.T;
    ok = true;
    driven = false;
    double tm = 1.0 / g.betas[0];
    double acc = tm, prev = g.betas[0];
    for (int i = 0; i <= T - 3; i++) {
        const double dS = g.kappa * (g.ratios[i] - g.ratios[i + 1]);
        if (dS != 0.0) driven = true;
        const double tn = 1.0 / g.betas[i + 1];
        const double dT = (tn - tm) * exp(dS);
        acc = acc + dT;
        const double nb = 1.0 / acc;
        if (!isfinite(nb) || !(prev > nb)) ok = false;
        if (store) g.betas[i + 1] = nb;
        prev = nb;
        tm = tn;
    }
    if (!(prev > g.betas[T - 1])) ok = false;  // the interior may not pass the fixed hottest temperature
}

// One block, one thread: at T <= 64 the update is serial and tiny.
__global__ void pt_ladder_adapt_kernel(PtLadderArgs g) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    const int T = g.T;
    const double W = (double)(2 * g.Wh);
    for (int p = 0; p < T - 1; p++) {
        const int64_t total = g.ws_totals[p];
        const int64_t count = total - g.totals_prev[p];
        g.totals_prev[p] = total;
        g.ratios[p] = (double)count / W;
    }
    if (g.moments)
        for (int i = 0; i < 2 * T; i++) g.moments[i] = g.moments[i] + g.ws_moments[i];
    if (T < 3) return;  // no interior temperature
    bool ok, driven;
    pt_ladder_pass(g, false, ok, driven);
    // no drive (kappa = 0, or equal ratios): the ladder stays bit for bit (1 / (1 / beta) need not
    // give beta back), and that is no refusal
    if (!driven) return;
    if (!ok) {
        *g.n_refused += 1;
        return;
    }
    pt_ladder_pass(g, true, ok, driven);
}

hipError_t launch_pt_stretch_propose(int P, int T, int Wh, const double* x, const double* c, double a, uint64_t seed,
                                     uint64_t it, uint32_t half, const double* draws, double* q, double* z,
                                     hipStream_t st) {
    pt_stretch_propose_kernel<<<blocks_of(T * Wh, 256), 256, 0, st>>>(P, T, Wh, x, c, a, seed, it, half, draws, q, z);
    return hipGetLastError();
}
hipError_t launch_pt_stretch_accept(int P, int T, int Wh, const double* betas, double* x, double* lnp,
                                    const double* q, const double* lnp_new, const double* z, uint64_t seed,
                                    uint64_t it, uint32_t half, const double* draws, int32_t* acc, hipStream_t st) {
    pt_stretch_accept_kernel<<<blocks_of(T * Wh, 256), 256, 0, st>>>(P, T, Wh, betas, x, lnp, q, lnp_new, z, seed, it,
                                                                     half, draws, acc);
    return hipGetLastError();
}
hipError_t launch_pt_swap(int P, int T, int Wh, const double* betas, double* x0, double* x1, double* lnp0,
                          double* lnp1, uint64_t seed, uint64_t it, const double* draws, int32_t* swapped,
                          hipStream_t st) {
    pt_swap_kernel<<<blocks_of(2 * Wh, 256), 256, 0, st>>>(P, T, Wh, betas, x0, x1, lnp0, lnp1, seed, it, draws,
                                                           swapped);
    return hipGetLastError();
}
hipError_t launch_pt_ladder_update(const PtLadderArgs& g, hipStream_t st) {
    const unsigned rows = (unsigned)(g.T - 1) + (g.moments ? (unsigned)g.T : 0u);
    pt_ladder_stats_kernel<<<dim3(rows), BLOCK_SUM_THREADS, 0, st>>>(g);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    pt_ladder_adapt_kernel<<<dim3(1), 64, 0, st>>>(g);
    return hipGetLastError();
}

}  // namespace rvm
