// rvm_stability.hip -- dynamical stability of many states at once (rvmcmc/stability.py, rvmcmc/chain.py
// ChainRecorder.stability): the likelihood kernel's Wisdom-Holman map kept alive over 10^4 .. 10^6 orbits, with
// the running extremes of each planet's osculating Jacobi elements.  include/rvmcmc.h states the rule, block by
// block.
//
//   stability_init_kernel     walker_setup at t = 0, its prior and pair test, the elements of the t = 0 state
//   stability_advance_kernel  n_blocks blocks of sample_every steps for every state still OK
//   stability_count_kernel    the states still OK, an integer count in one block
//
// A state's planets run on LanesPerWalker<NP> adjacent lanes, as in the likelihood kernel, and a block of one
// wave holds 64 / L states: a few hundred states spread over the CUs.  The kernel is one dependent chain of
// double operations per wave -- latency-bound by construction; it uses no LDS and no scratch.
//
// Chunk invariance.  A block starts from xv alone: |r|, 1 / |r| and the interaction (kick_prep) are formed anew
// from the positions at every block start, in a launch's first block and in every later one alike, and the lane
// constants come from walker_setup on params, as stability_init formed them.  What a launch carries from block
// to block in registers is therefore exactly what it would load.
//
// Independence.  Every lane of the wave runs every instruction (the DPP exchanges and ballots need them); a
// state that has ended, or a lane past n, computes on and writes nothing.  An ended state's lanes are entered in
// Lane::encm, so the gated drift never takes the wave to the second Halley step or the general solver on their
// account (rvm_device.h lane_encountered), and a live lane's bits never depend on another lane's solve.
#include <hip/hip_runtime.h>
#include <math.h>

#pragma clang fp contract(on)
#include "rvm_launch.h"
#include "rvm_walker.h"

namespace rvm {

constexpr int SC_BLOCK = 256;  // count: one block, its threads stride over the states

// |r| and 1 / |r| of the own coordinate from its position (the header's r2, |r|, ir)
template <bool D3, int NP>
__device__ __forceinline__ void lane_radius(Lane<NP>& s) {
    double r2 = fma(s.ry, s.ry, s.rx * s.rx);
    if constexpr (D3) r2 = fma(s.rz, s.rz, r2);
    s.r = sqrt(r2);
    s.ir = 1.0 / s.r;
}

// osculating a and e^2 of the own coordinate (the header's elements; igm2 = 1 / (GM GM)); lane_radius first
template <bool D3, int NP>
__device__ __forceinline__ void lane_elements(const Lane<NP>& s, const double igm2, double& a, double& e2) {
    double v2 = fma(s.vy, s.vy, s.vx * s.vx);
    if constexpr (D3) v2 = fma(s.vz, s.vz, v2);
    const double beta = fma(s.GM2, s.ir, -v2);
    a = s.GM / beta;
    const double hz = fma(s.rx, s.vy, -(s.ry * s.vx));
    double h2 = hz * hz;
    if constexpr (D3) {
        const double hx = fma(s.ry, s.vz, -(s.rz * s.vy));
        const double hy = fma(s.rz, s.vx, -(s.rx * s.vz));
        h2 = fma(hz, hz, fma(hy, hy, hx * hx));
    }
    const double hb = h2 * beta;
    e2 = fma(-hb, igm2, 1.0);
}

// the wave mask of every lane whose state (its L lanes) has a lane with p set
template <int L>
__device__ __forceinline__ uint64_t state_lanes(uint64_t m) {
    if constexpr (L == 1) {
        return m;
    } else if constexpr (L == 2) {
        const uint64_t t = (m | (m >> 1)) & 0x5555555555555555ull;
        return t | (t << 1);
    } else {
        const uint64_t t = (m | (m >> 1) | (m >> 2) | (m >> 3)) & 0x1111111111111111ull;
        return t | (t << 1) | (t << 2) | (t << 3);
    }
}

// what both kernels begin with: the lane's state index (clamped: lanes past n compute on the last state), its
// parameter rows and walker_setup.  Returns whether the lane writes (a planet's lane of a state below n).
template <int NP, bool D3>
__device__ __forceinline__ bool stability_setup(const int n, const double* __restrict__ params,
                                                const double hill_factor, Lane<NP>& s, int& st0, size_t& col) {
    constexpr int L = LanesPerWalker<NP>::value;
    constexpr int R = (D3 ? 7 : 5) * NP;
    const int lane = (int)threadIdx.x;
    const int pl_idx = lane & (L - 1);
    const int64_t w = (int64_t)blockIdx.x * (64 / L) + lane / L;
    const int wk = w < n ? (int)w : n - 1;
    double rowv[R];
#pragma unroll
    for (int r = 0; r < R; r++) rowv[r] = params[(size_t)r * (size_t)n + (size_t)wk];
    st0 = RVM_STATUS_OK;
    double e2w;
    walker_setup<NP, D3, L>(rowv, pl_idx, hill_factor, s, st0, e2w);
    col = (size_t)wk;
    return w < n && pl_idx < NP;
}

template <int NP, bool D3>
__global__ void __launch_bounds__(64)
    stability_init_kernel(const int n, const double* __restrict__ params, const double hill_factor,
                          double* __restrict__ xv, double* __restrict__ ext, int32_t* __restrict__ status,
                          int64_t* __restrict__ steps) {
    constexpr int L = LanesPerWalker<NP>::value;
    Lane<NP> s;
    int st;
    size_t col;
    const bool writes = stability_setup<NP, D3>(n, params, hill_factor, s, st, col);
    // the pair test before the first step, as the likelihood kernel makes it
    (void)kick_prep<NP, L, D3>(s, 1.875);
    const int base = (int)threadIdx.x & ~(L - 1);
    if (st == RVM_STATUS_OK && ((s.encm >> base) & kick_enc_bits<NP>()) != 0) st = RVM_STATUS_ENCOUNTER;
    lane_radius<D3>(s);
    double a, e2;
    lane_elements<D3>(s, 1.0 / (s.GM * s.GM), a, e2);
    if (!writes) return;
    const bool ok = st == RVM_STATUS_OK;
    const size_t N = (size_t)n, o = (size_t)s.p * N + col;
    const double v[6] = {s.rx, s.ry, D3 ? s.rz : 0.0, s.vx, s.vy, D3 ? s.vz : 0.0};
#pragma unroll
    for (int c = 0; c < 6; c++) xv[(size_t)c * NP * N + o] = ok ? v[c] : RVM_QNAN;
    ext[o] = ok ? a : RVM_QNAN;
    ext[(size_t)NP * N + o] = ok ? a : RVM_QNAN;
    ext[(size_t)2 * NP * N + o] = ok ? e2 : RVM_QNAN;
    if ((threadIdx.x & (L - 1)) == 0) {
        status[col] = st;
        steps[col] = 0;
    }
}

template <int NP, bool D3>
__global__ void __launch_bounds__(64)
    stability_advance_kernel(const int n, const double* __restrict__ params, const double hill_factor, const double h,
                             const int sample_every, const int n_blocks, const double r_max, double* __restrict__ xv,
                             double* __restrict__ ext, int32_t* __restrict__ status, int64_t* __restrict__ steps) {
    constexpr int L = LanesPerWalker<NP>::value;
    Lane<NP> s;
    int st_setup;
    size_t col;
    const bool writes = stability_setup<NP, D3>(n, params, hill_factor, s, st_setup, col);
    int st = status[col];
    const bool entered = st == RVM_STATUS_OK;  // only these states are written
    if (ballot(entered) == 0) return;          // (wave-uniform: every state of the wave had ended)
    const size_t N = (size_t)n, o = (size_t)s.p * N + col;
    double a_min = 0.0, a_max = 0.0, e2_max = 0.0;
    if (entered) {  // (an ended state keeps walker_setup's t = 0 state: finite, and never written)
        s.rx = xv[o];
        s.ry = xv[(size_t)NP * N + o];
        s.vx = xv[(size_t)3 * NP * N + o];
        s.vy = xv[(size_t)4 * NP * N + o];
        if constexpr (D3) {
            s.rz = xv[(size_t)2 * NP * N + o];
            s.vz = xv[(size_t)5 * NP * N + o];
        }
        a_min = ext[o];
        a_max = ext[(size_t)NP * N + o];
        e2_max = ext[(size_t)2 * NP * N + o];
    }
    lane_radius<D3>(s);
    const double igm2 = 1.0 / (s.GM * s.GM);
    // the state as last stored (step 3): what the launch writes at its end
    double gx = s.rx, gy = s.ry, gz = s.rz, gvx = s.vx, gvy = s.vy, gvz = s.vz;
    int done = 0;  // blocks the state has run in this launch
    const int lane = (int)threadIdx.x, base = lane & ~(L - 1);
    for (int b = 0; b < n_blocks; b++) {
        const uint64_t live = ballot(st == RVM_STATUS_OK);
        if (live == 0) break;  // (wave-uniform, outside the convergent code below)
        s.encm |= ~live;       // ended states: their drifts no longer vote (lane_encountered)
        KickPrep<NP> kp = kick_prep<NP, L, D3>(s, 1.875);
        bool unused = false;
        segment_steps<8, true, D3, NP, L, 0, RVM_DRIFT_ACC>(s, kp, h, sample_every, unused);
        lane_radius<D3>(s);
        double a, e2;
        lane_elements<D3>(s, igm2, a, e2);
        const bool alive = ((live >> lane) & 1) != 0;
        const bool enc = ((s.encm >> base) & kick_enc_bits<NP>()) != 0;
        const bool nonf = ((state_lanes<L>(ballot(!(isfinite(s.r) && isfinite(a) && isfinite(e2)))) >> lane) & 1) != 0;
        const bool esc = ((state_lanes<L>(ballot(s.r > r_max && r_max > 0.0)) >> lane) & 1) != 0;
        if (alive) {
            done++;
            if (enc) {
                st = RVM_STATUS_ENCOUNTER;
            } else if (nonf) {
                st = RVM_STATUS_NONFINITE;
            } else {
                a_min = fmin(a_min, a);
                a_max = fmax(a_max, a);
                e2_max = fmax(e2_max, e2);
                gx = s.rx;
                gy = s.ry;
                gz = s.rz;
                gvx = s.vx;
                gvy = s.vy;
                gvz = s.vz;
                if (esc) st = RVM_STATUS_ESCAPE;
            }
        }
    }
    if (!writes || !entered) return;
    xv[o] = gx;
    xv[(size_t)NP * N + o] = gy;
    xv[(size_t)3 * NP * N + o] = gvx;
    xv[(size_t)4 * NP * N + o] = gvy;
    if constexpr (D3) {
        xv[(size_t)2 * NP * N + o] = gz;
        xv[(size_t)5 * NP * N + o] = gvz;
    }
    ext[o] = a_min;
    ext[(size_t)NP * N + o] = a_max;
    ext[(size_t)2 * NP * N + o] = e2_max;
    if ((lane & (L - 1)) == 0) {
        status[col] = st;
        steps[col] += (int64_t)done * (int64_t)sample_every;
    }
}

__global__ void __launch_bounds__(SC_BLOCK)
    stability_count_kernel(const int n, const int32_t* __restrict__ status, int64_t* __restrict__ out) {
    __shared__ int64_t part[SC_BLOCK / 64];
    int64_t c = 0;
    for (int64_t i = threadIdx.x; i < n; i += SC_BLOCK) c += status[i] == RVM_STATUS_OK ? 1 : 0;
    // (an integer sum: any order gives the same count)
    for (int off = 32; off > 0; off >>= 1) c += __shfl_down(c, off);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) {
        int64_t t = 0;
        for (int i = 0; i < SC_BLOCK / 64; i++) t += part[i];
        out[0] = t;
    }
}

template <int NP, bool D3>
static hipError_t launch_init_t(int n, const double* params, double hill_factor, double* xv, double* ext,
                                int32_t* status, int64_t* steps, hipStream_t st) {
    constexpr int WPB = 64 / LanesPerWalker<NP>::value;
    stability_init_kernel<NP, D3><<<dim3(blocks_of((uint64_t)n, WPB)), 64, 0, st>>>(n, params, hill_factor, xv, ext,
                                                                                  status, steps);
    return hipGetLastError();
}

template <int NP, bool D3>
static hipError_t launch_advance_t(int n, const double* params, double hill_factor, double h, int sample_every,
                                   int n_blocks, double r_max, double* xv, double* ext, int32_t* status,
                                   int64_t* steps, hipStream_t st) {
    constexpr int WPB = 64 / LanesPerWalker<NP>::value;
    stability_advance_kernel<NP, D3><<<dim3(blocks_of((uint64_t)n, WPB)), 64, 0, st>>>(
        n, params, hill_factor, h, sample_every, n_blocks, r_max, xv, ext, status, steps);
    return hipGetLastError();
}

// the instantiation of (NP, inclined): CALL(NP, D3) for the pair, hipErrorInvalidValue for any other
#define RVM_STABILITY_DISPATCH(NP, inclined, CALL)   \
    switch (2 * (NP) + ((inclined) ? 1 : 0)) {       \
        case 2: return CALL(1, false);               \
        case 3: return CALL(1, true);                \
        case 4: return CALL(2, false);               \
        case 5: return CALL(2, true);                \
        case 6: return CALL(3, false);               \
        case 7: return CALL(3, true);                \
        case 8: return CALL(4, false);               \
        case 9: return CALL(4, true);                \
    }                                                \
    return hipErrorInvalidValue

hipError_t launch_stability_init(int NP, int inclined, int n, const double* params, double hill_factor, double* xv,
                                 double* ext, int32_t* status, int64_t* steps, hipStream_t st) {
#define CALL(P, D3) launch_init_t<P, D3>(n, params, hill_factor, xv, ext, status, steps, st)
    RVM_STABILITY_DISPATCH(NP, inclined, CALL);
#undef CALL
}

static hipError_t advance_states(int NP, int inclined, int n, const double* params, double hill_factor, double h,
                                 int sample_every, int n_blocks, double r_max, double* xv, double* ext,
                                 int32_t* status, int64_t* steps, hipStream_t st) {
#define CALL(P, D3) \
    launch_advance_t<P, D3>(n, params, hill_factor, h, sample_every, n_blocks, r_max, xv, ext, status, steps, st)
    RVM_STABILITY_DISPATCH(NP, inclined, CALL);
#undef CALL
}

hipError_t launch_stability_advance(int NP, int inclined, int n, const double* params, double hill_factor, double h,
                                    int sample_every, int n_blocks, double r_max, double* xv, double* ext,
                                    int32_t* status, int64_t* steps, int64_t* n_alive, hipStream_t st) {
    hipError_t e = advance_states(NP, inclined, n, params, hill_factor, h, sample_every, n_blocks, r_max, xv, ext,
                                  status, steps, st);
    if (e == hipSuccess && n_alive != nullptr) {
        stability_count_kernel<<<dim3(1), SC_BLOCK, 0, st>>>(n, status, n_alive);
        e = hipGetLastError();
    }
    return e;
}

}  // namespace rvm
