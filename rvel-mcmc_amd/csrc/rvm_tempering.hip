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

#include "rvm_device.h"
#include "rvm_internal.h"
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

static inline dim3 grid1(int n) { return dim3((unsigned)(((int64_t)n + 255) / 256)); }

hipError_t launch_pt_stretch_propose(int P, int T, int Wh, const double* x, const double* c, double a, uint64_t seed,
                                     uint64_t it, uint32_t half, const double* draws, double* q, double* z,
                                     hipStream_t st) {
    pt_stretch_propose_kernel<<<grid1(T * Wh), 256, 0, st>>>(P, T, Wh, x, c, a, seed, it, half, draws, q, z);
    return hipGetLastError();
}
hipError_t launch_pt_stretch_accept(int P, int T, int Wh, const double* betas, double* x, double* lnp,
                                    const double* q, const double* lnp_new, const double* z, uint64_t seed,
                                    uint64_t it, uint32_t half, const double* draws, int32_t* acc, hipStream_t st) {
    pt_stretch_accept_kernel<<<grid1(T * Wh), 256, 0, st>>>(P, T, Wh, betas, x, lnp, q, lnp_new, z, seed, it, half,
                                                            draws, acc);
    return hipGetLastError();
}
hipError_t launch_pt_swap(int P, int T, int Wh, const double* betas, double* x0, double* x1, double* lnp0,
                          double* lnp1, uint64_t seed, uint64_t it, const double* draws, int32_t* swapped,
                          hipStream_t st) {
    pt_swap_kernel<<<grid1(2 * Wh), 256, 0, st>>>(P, T, Wh, betas, x0, x1, lnp0, lnp1, seed, it, draws, swapped);
    return hipGetLastError();
}

}  // namespace rvm
