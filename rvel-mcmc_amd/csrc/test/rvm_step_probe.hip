// rvm_step_probe.hip -- test-only library (rvmcmc/librvm_step_probe.so): the device functions under
// the likelihood kernel, one call at a time.  tests/test_gpu_step_units.py holds them to the mpmath
// run of tests/wh_ref.py (tier U0).  Not linked into librvmcmc.so; nothing on the
// product's path loads it.
//
// Every kernel is one wave per block, one item per lane (drift, stumpff, recip) or one walker per
// L adjacent lanes (setup, kick: the likelihood kernel's packing), SoA in and SoA out: array k of
// a buffer of n items starts at k * n.  Lanes past the end compute on the last item, as the
// likelihood kernel's lanes past W do, and write nothing.  Entry points return 0, or -1 for an
// instantiation that does not exist and -2 for a launch error.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

// (as rvm_logl.hip and rvm_refine.hip: a walker's bits are those of the product's kernels)
#pragma clang fp contract(on)
#include "../rvm_walker.h"
using namespace rvm;

namespace {

// ---- drift ----------------------------------------------------------------------------------
// what the gated drift does with a lane (rvm_device.h drift, second_chance, kepler_rare), found
// before the call from the header's own functions
enum Path : int32_t {
    FIRST = 0,          // the first Halley step passes the cheap test
    ZAWARE = 1,         // ACC 1/2/4: accepted by the z-aware form
    TAYLOR = 2,         // ACC 1/2/4: the Taylor second step
    SECOND8 = 3,        // the second Halley step with the 8-term series
    RARE_HALLEY = 4,    // kepler_rare's Halley loop converges
    SAFE_HARD = 5,      // |beta| u^2 > 0.5: the bracketed solver at once
    SAFE_FALLBACK = 6,  // kepler_rare's Halley loop does not converge: the bracketed solver
    NAN_GUESS = 7       // the first step's correction is not finite (then kepler_rare from the guess)
};

template <int NT, int KG, int ACC, bool D3, int NP>
__device__ __forceinline__ int32_t drift_path(const Lane<NP>& s, double dt, const VConsts& vk) {
    // the drift's preamble (rvm_device.h drift)
    const double GM = s.GM, r0 = s.r, ir0 = s.ir;
    double v2 = fma(s.vx, s.vx, s.vy * s.vy);
    double eta = fma(s.rx, s.vx, s.ry * s.vy);
    if constexpr (D3) {
        v2 = fma(s.vz, s.vz, v2);
        eta = fma(s.rz, s.vz, eta);
    }
    const double beta = fma(s.GM2, ir0, -v2);
    const double zeta = fma(-beta, r0, GM);
    const double u = dt * ir0, sg = eta * ir0, g = GM * ir0;
    const double hs = 0.5 * sg;
    const double T3 = fma(hs, sg, (beta - g) * (1.0 / 6.0));
    const double T4 = sg * fma(-0.625 * sg, sg, fma(5.0 / 12.0, g, -0.375 * beta));
    double x;
    if constexpr (KG == 1) {
        const double s2 = sg * sg;
        const double T5 = fma(beta, fma(9.0 / 120.0, beta, fma(-19.0 / 120.0, g, 0.75 * s2)),
                              fma(g, fma(1.0 / 12.0, g, -0.875 * s2), 0.875 * (s2 * s2)));
        x = u * fma(u, fma(u, fma(u, fma(u, T5, T4), T3), -hs), 1.0);
    } else {
        x = u * fma(u, fma(u, fma(u, T4, T3), -hs), 1.0);
    }
    double G0, G1, G2, G3, fp, fpp, Q, z, x3, f0;
    halley<NT>(x, beta, r0, eta, zeta, GM, dt, G0, G1, G2, G3, fp, fpp, Q, z, x3, vk.k2, vk.k3, f0);
    if (!isfinite(Q)) return NAN_GUESS;
    constexpr double B = stumpff_bound<NT>();
    const bool zok = fabs(z) <= B;
    if (zok && halley_ok<NT>(Q, x)) return FIRST;
    if constexpr (ACC == 1 || ACC == 2 || ACC == 4) {
        // (the three bounds below are written inside drift's second_chance, not in a function of
        // the header: they are the only constants this file states again)
        if (zok && fabs((Q * Q) * (Q * z)) <= 7.3e-17 * fabs(x3)) return ZAWARE;
        if (zok && fabs(Q) <= 1e-4 * fabs(x)) {
            const double f3 = fma(zeta, G0, -(beta * eta) * G1);
            const double f4 = -beta * fpp;
            const double d = -Q;
            const double F = fma(d, fma(d, fma(d, fma(d, f4 * (1.0 / 24.0), f3 * (1.0 / 6.0)), 0.5 * fpp), fp), f0);
            const double F1 = fma(d, fma(d, fma(d, f4 * (1.0 / 6.0), 0.5 * f3), fpp), fp);
            const double q2 = F * rcp_nr(F1);
            if (fabs(q2) <= 1e-8 * fabs(x)) return TAYLOR;
        }
    }
    constexpr double B8 = stumpff_bound<8>();
    double xe = x;
    const double X1 = x - Q;
    if (fabs(beta * X1 * X1) <= B8) {
        xe = X1;
        double fu;
        halley<8>(xe, beta, r0, eta, zeta, GM, dt, G0, G1, G2, G3, fp, fpp, Q, z, x3, vk.k2_8, vk.k3_8, fu);
        if (fabs(z) <= B8 && halley_ok<8>(Q, xe)) return SECOND8;
    }
    if (fabs(beta) * (u * u) > 0.5) return SAFE_HARD;
    const double start = xe - Q;
    double X = isfinite(start) && xe != x ? start : x;
    for (int it = 0; it < 8; it++) {  // kepler_rare's loop
        double c0, c1, c2, c3;
        const double zi = beta * X * X;
        stumpff_full(zi, c0, c1, c2, c3);
        const double g1 = X * c1, g2 = X * X * c2, g3 = X * X * X * c3;
        const double ff = r0 * g1 + eta * g2 + GM * g3 - dt;
        const double ffp = r0 * c0 + eta * g1 + GM * g2;
        const double ffpp = eta * c0 + zeta * g1;
        const double dX = ff * ffp / (ffp * ffp - 0.5 * ff * ffpp);
        if (halley_done(dX, zi, X * X * X)) return RARE_HALLEY;
        X = X - dX;
    }
    return SAFE_FALLBACK;
}

// in: rx ry rz vx vy vz GM dt; out: rx ry rz vx vy vz r ir.  enc: the item's walker has met an
// encounter (NP = 2: either item of the pair of lanes).  |r| and 1/|r| enter as walker_setup leaves them.
template <int NT, bool GATED, int ACC, bool D3, int KG, int NP>
__global__ __launch_bounds__(64) void drift_kernel(int n, const double* __restrict__ in, const int32_t* __restrict__ enc,
                                                   double* __restrict__ out, int32_t* __restrict__ bad_out,
                                                   int32_t* __restrict__ path_out) {
    const int i0 = blockIdx.x * 64 + (int)threadIdx.x;
    const bool valid = i0 < n;
    const size_t i = valid ? i0 : n - 1;
    const size_t N = n;
    Lane<NP> s;
    s.rx = in[0 * N + i];
    s.ry = in[1 * N + i];
    s.rz = D3 ? in[2 * N + i] : 0.0;
    s.vx = in[3 * N + i];
    s.vy = in[4 * N + i];
    s.vz = D3 ? in[5 * N + i] : 0.0;
    s.GM = in[6 * N + i];
    s.GM2 = 2.0 * s.GM;
    const double dt = in[7 * N + i];
    s.r = D3 ? sqrt(s.rx * s.rx + s.ry * s.ry + s.rz * s.rz) : sqrt(s.rx * s.rx + s.ry * s.ry);
    s.ir = 1.0 / s.r;
    s.encm = ballot(enc[i] != 0);
    const VConsts vk = vconsts_for<NT>();
    const int32_t path = drift_path<NT, KG, ACC, D3>(s, dt, vk);
    bool bad = false;
    drift<NT, GATED, D3, NP, KG, ACC>(s, dt, bad, vk);
    if (valid) {
        out[0 * N + i] = s.rx;
        out[1 * N + i] = s.ry;
        out[2 * N + i] = D3 ? s.rz : 0.0;
        out[3 * N + i] = s.vx;
        out[4 * N + i] = s.vy;
        out[5 * N + i] = D3 ? s.vz : 0.0;
        out[6 * N + i] = s.r;
        out[7 * N + i] = s.ir;
        bad_out[i] = bad ? 1 : 0;
        path_out[i] = path;
    }
}

typedef void (*drift_fn)(int, const double*, const int32_t*, double*, int32_t*, int32_t*);

// mode: 0 ungated, 1 + ACC gated
template <int NT, bool D3, int KG, int NP>
drift_fn drift_pick(int mode) {
    if constexpr (KG == 0) {
        switch (mode) {
            case 0:
                return drift_kernel<NT, false, 0, D3, KG, NP>;
            case 1:
                return drift_kernel<NT, true, 0, D3, KG, NP>;
            case 4:
                return drift_kernel<NT, true, 3, D3, KG, NP>;
        }
        if constexpr (!D3 && NP == 1) {
            switch (mode) {
                case 2:
                    return drift_kernel<NT, true, 1, D3, KG, NP>;
                case 3:
                    return drift_kernel<NT, true, 2, D3, KG, NP>;
                case 5:
                    return drift_kernel<NT, true, 4, D3, KG, NP>;
            }
        }
    } else {
        switch (mode) {
            case 1:
                return drift_kernel<NT, true, 0, D3, KG, NP>;
            case 4:
                return drift_kernel<NT, true, 3, D3, KG, NP>;
        }
    }
    return nullptr;
}

template <int NT>
drift_fn drift_pick_nt(int mode, int d3, int kg, int np) {
    if (np == 2) return (d3 || kg) ? nullptr : drift_pick<NT, false, 0, 2>(mode);
    if (np != 1) return nullptr;
    if (kg == 1) return d3 ? nullptr : drift_pick<NT, false, 1, 1>(mode);
    if (kg != 0) return nullptr;
    return d3 ? drift_pick<NT, true, 0, 1>(mode) : drift_pick<NT, false, 0, 1>(mode);
}

// ---- stumpff / recip --------------------------------------------------------------------------
// out: for NT = 6, 7, 8 in turn c2, c3 of stumpff23<NT>(z, c2, c3, k2, k3) then of
// stumpff23<NT>(z, c2, c3) (12 arrays), then c0 .. c3 of stumpff_full
template <int NT>
__device__ __forceinline__ void stumpff_both(double z, double* o) {
    const VConsts vk = vconsts_for<NT>();
    stumpff23<NT>(z, o[0], o[1], vk.k2, vk.k3);
    stumpff23<NT>(z, o[2], o[3]);
}

__global__ __launch_bounds__(64) void stumpff_kernel(int n, const double* __restrict__ zin, double* __restrict__ out) {
    const int i0 = blockIdx.x * 64 + (int)threadIdx.x;
    const size_t i = i0 < n ? i0 : n - 1;
    const double z = zin[i];
    double o[16];
    stumpff_both<6>(z, o);
    stumpff_both<7>(z, o + 4);
    stumpff_both<8>(z, o + 8);
    stumpff_full(z, o[12], o[13], o[14], o[15]);
    if (i0 < n) {
#pragma unroll
        for (int k = 0; k < 16; k++) out[(size_t)k * n + i] = o[k];
    }
}

// out: rcp_nr, rsq_nr, rcube_nr of x
__global__ __launch_bounds__(64) void recip_kernel(int n, const double* __restrict__ xin, double* __restrict__ out) {
    const int i0 = blockIdx.x * 64 + (int)threadIdx.x;
    const size_t i = i0 < n ? i0 : n - 1;
    const double x = xin[i];
    const double a = rcp_nr(x), b = rsq_nr(x), c = rcube_nr(x, vconst(1.875));
    if (i0 < n) {
        out[i] = a;
        out[(size_t)n + i] = b;
        out[2 * (size_t)n + i] = c;
    }
}

// ---- setup ------------------------------------------------------------------------------------
// rows: the kernel's parameter matrix [PR * NP][W]; out [12][W * L] per lane: rx ry rz vx vy vz r ir
// GM dmin2 e2w and the walker's status (as a double)
template <int NP, bool D3>
__global__ __launch_bounds__(64) void setup_kernel(int W, const double* __restrict__ rows, double hill_factor,
                                                   double* __restrict__ out) {
    constexpr int L = LanesPerWalker<NP>::value;
    constexpr int R = (D3 ? 7 : 5) * NP;
    const int lane = threadIdx.x & 63;
    const int w = blockIdx.x * (64 / L) + lane / L;
    const bool valid = w < W;
    const int wl = valid ? w : W - 1;
    double rowv[R];
#pragma unroll
    for (int r = 0; r < R; r++) rowv[r] = rows[(size_t)r * W + wl];
    Lane<NP> s;
    int status = RVM_STATUS_OK;
    double e2w;
    walker_setup<NP, D3, L>(rowv, lane % L, hill_factor, s, status, e2w);
    if (valid) {
        const size_t N = (size_t)W * L, i = (size_t)w * L + lane % L;
        const double o[12] = {s.rx, s.ry, s.rz, s.vx, s.vy, s.vz, s.r, s.ir, s.GM, s.dmin2, e2w, (double)status};
#pragma unroll
        for (int k = 0; k < 12; k++) out[k * N + i] = o[k];
    }
}

// ---- kick -------------------------------------------------------------------------------------
// state [6][W * L] per lane: the Jacobi rx ry rz vx vy vz of planet min(lane % L, NP - 1);
// mass [NP][W]; dmin2 [W].  out [16][W * L] per lane: (vx vy vz enc) after kick<NP, L, D3>, after
// kick_generic, after kick_prep + kick_apply (full) and after kick_prep + kick_apply (half), all
// from the same state with the step h, enc the walker's bits of Lane::encm relative to its first
// lane (kick_enc_bits); star [W * L]: star_vx of the input velocities.
template <int NP, bool D3>
__global__ __launch_bounds__(64) void kick_kernel(int W, const double* __restrict__ state, const double* __restrict__ mass,
                                                  const double* __restrict__ dmin2, double h, double* __restrict__ out,
                                                  double* __restrict__ star) {
    constexpr int L = LanesPerWalker<NP>::value;
    const int lane = threadIdx.x & 63;
    const int w = blockIdx.x * (64 / L) + lane / L;
    const bool valid = w < W;
    const int wl = valid ? w : W - 1;
    const size_t N = (size_t)W * L, i = (size_t)wl * L + lane % L;
    Lane<NP> s;
    s.q = lane % L;
    s.p = s.q < NP ? s.q : NP - 1;
    // masses as walker_setup derives them
    double Mi[NP + 1];
    Mi[0] = 1.0;
#pragma unroll
    for (int p = 0; p < NP; p++) {
        s.m[p] = mass[(size_t)p * W + wl];
        Mi[p + 1] = Mi[p] + s.m[p];
    }
#pragma unroll
    for (int p = 0; p <= NP; p++) s.iMi[p] = 1.0 / Mi[p];
#pragma unroll
    for (int p = 0; p < NP; p++) s.mu[p] = s.m[p] / Mi[p + 1];
    s.GM = Mi[1];
#pragma unroll
    for (int p = 1; p < NP; p++)
        if (s.p == p) s.GM = Mi[p + 1];
    s.dmin2 = dmin2[wl];
    s.rx = state[0 * N + i];
    s.ry = state[1 * N + i];
    s.rz = D3 ? state[2 * N + i] : 0.0;
    s.vx = state[3 * N + i];
    s.vy = state[4 * N + i];
    s.vz = D3 ? state[5 * N + i] : 0.0;
    s.r = D3 ? sqrt(s.rx * s.rx + s.ry * s.ry + s.rz * s.rz) : sqrt(s.rx * s.rx + s.ry * s.ry);
    s.ir = 1.0 / s.r;
    s.encm = 0;
    lane_finish(s);
    lane_set_step(s, h);
    const double c1875 = vconst(1.875);
    const int base = lane & ~(L - 1);
    auto bits = [&](const Lane<NP>& t) { return (double)((t.encm >> base) & kick_enc_bits<NP>()); };
    double o[16];
    auto put = [&](int k, const Lane<NP>& t) {
        o[4 * k] = t.vx;
        o[4 * k + 1] = t.vy;
        o[4 * k + 2] = D3 ? t.vz : 0.0;
        o[4 * k + 3] = bits(t);
    };
    const double sv = star_vx<NP, L>(s);
    Lane<NP> a = s;
    kick<NP, L, D3>(a, h, c1875);
    put(0, a);
    Lane<NP> b = s;
    kick_generic<NP, L, D3>(b, h);
    put(1, b);
    Lane<NP> c = s;
    const KickPrep<NP> kc = kick_prep<NP, L, D3>(c, c1875);
    kick_apply<NP, false, D3>(c, kc);
    put(2, c);
    Lane<NP> d = s;
    const KickPrep<NP> kd = kick_prep<NP, L, D3>(d, c1875);
    kick_apply<NP, true, D3>(d, kd);
    put(3, d);
    if (valid) {
#pragma unroll
        for (int k = 0; k < 16; k++) out[k * N + i] = o[k];
        star[i] = sv;
    }
}

int done() { return hipGetLastError() == hipSuccess ? 0 : -2; }

}  // namespace

extern "C" {

// mode: 0 ungated, 1 + ACC gated (ACC 0 .. 4).  nt 6 / 7 / 8; d3 0 / 1; kg 0 / 1; np 1 / 2.
int rvm_probe_drift(int nt, int mode, int d3, int kg, int np, int n, const double* in, const int32_t* enc, double* out,
                    int32_t* bad, int32_t* path, hipStream_t stream) {
    drift_fn f = nt == 6   ? drift_pick_nt<6>(mode, d3, kg, np)
                 : nt == 7 ? drift_pick_nt<7>(mode, d3, kg, np)
                 : nt == 8 ? drift_pick_nt<8>(mode, d3, kg, np)
                           : nullptr;
    if (!f || n <= 0) return -1;
    hipLaunchKernelGGL(f, dim3((n + 63) / 64), dim3(64), 0, stream, n, in, enc, out, bad, path);
    return done();
}

int rvm_probe_stumpff(int n, const double* z, double* out, hipStream_t stream) {
    if (n <= 0) return -1;
    hipLaunchKernelGGL(stumpff_kernel, dim3((n + 63) / 64), dim3(64), 0, stream, n, z, out);
    return done();
}

int rvm_probe_recip(int n, const double* x, double* out, hipStream_t stream) {
    if (n <= 0) return -1;
    hipLaunchKernelGGL(recip_kernel, dim3((n + 63) / 64), dim3(64), 0, stream, n, x, out);
    return done();
}

#define RVM_PROBE_NP_D3(KERNEL, ...)                                                                     \
    do {                                                                                                 \
        const int L = np <= 2 ? np : 4;                                                                  \
        const dim3 grid((W * L + 63) / 64), block(64);                                                   \
        switch (np * 2 + (d3 ? 1 : 0)) {                                                                 \
            case 2: hipLaunchKernelGGL((KERNEL<1, false>), grid, block, 0, stream, __VA_ARGS__); break;  \
            case 3: hipLaunchKernelGGL((KERNEL<1, true>), grid, block, 0, stream, __VA_ARGS__); break;   \
            case 4: hipLaunchKernelGGL((KERNEL<2, false>), grid, block, 0, stream, __VA_ARGS__); break;  \
            case 5: hipLaunchKernelGGL((KERNEL<2, true>), grid, block, 0, stream, __VA_ARGS__); break;   \
            case 6: hipLaunchKernelGGL((KERNEL<3, false>), grid, block, 0, stream, __VA_ARGS__); break;  \
            case 7: hipLaunchKernelGGL((KERNEL<3, true>), grid, block, 0, stream, __VA_ARGS__); break;   \
            case 8: hipLaunchKernelGGL((KERNEL<4, false>), grid, block, 0, stream, __VA_ARGS__); break;  \
            case 9: hipLaunchKernelGGL((KERNEL<4, true>), grid, block, 0, stream, __VA_ARGS__); break;   \
        }                                                                                                \
    } while (0)

int rvm_probe_setup(int np, int d3, int W, const double* rows, double hill_factor, double* out, hipStream_t stream) {
    if (np < 1 || np > 4 || W <= 0) return -1;
    RVM_PROBE_NP_D3(setup_kernel, W, rows, hill_factor, out);
    return done();
}

int rvm_probe_kick(int np, int d3, int W, const double* state, const double* mass, const double* dmin2, double h,
                   double* out, double* star, hipStream_t stream) {
    if (np < 1 || np > 4 || W <= 0) return -1;
    RVM_PROBE_NP_D3(kick_kernel, W, state, mass, dmin2, h, out, star);
    return done();
}

}  // extern "C"
