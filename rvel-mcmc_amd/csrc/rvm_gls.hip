// rvm_gls.hip -- generalised Lomb-Scargle periodograms (Zechmeister & Kuerster 2009: weights, floating mean) of
// many residual series at once: the data's own and those of the posterior's RV curves (rvmcmc/periodogram.py,
// rvmcmc/chain.py residual_periodogram).  Over S series, F frequencies and N epochs the work is a
// [2 F][N] x [N][S] product whose left factor, the weighted and centred cos/sin table, depends on the epochs
// alone; include/rvmcmc.h states the definition, operation by operation.
//
//   gls_basis_kernel    (k, i): c, s = cos, sin of 2 pi f_k tau_i -- once per frequency and epoch, never per series;
//                       rvm_gls_basis and the table of rvm_gls_power are both this kernel
//   gls_prepare_kernel  per frequency: the weighted means C, S, then u = w (c - C), v = w (s - S) written over
//                       the table, and CC, SS, CS
//   gls_centre_kernel   per series: z = y - m and YY
//   gls_product_kernel  per (k, s): YC = sum u z, YS = sum v z and the power
//
// Every sum runs over i ascending in one thread from acc = 0 with one fma per term, so the result does not
// depend on tiles, chunks or the run.  Nothing here contracts a product into a sum except where fma is written:
// every kernel switches contraction off for its body, and the Makefile compiles this file with it off.
// Stream-ordered launches without allocation, synchronisation or atomics.
#include <hip/hip_runtime.h>
#include <math.h>

#include "rvm_internal.h"
#include "rvm_launch.h"

namespace rvm {

constexpr int GB_BLOCK = 256;          // basis: a thread takes two epochs of a frequency per turn
constexpr int GB_MAX_BLOCKS = 1 << 16; // and a launch at most so many blocks (the threads stride over the rest)
constexpr int GP_BLOCK = 64;           // prepare: a thread is a frequency
constexpr int GC_BLOCK = 256;          // centre: a thread is a series
constexpr int GL_BATCH = 8;            // prepare, centre: epochs whose loads a thread has in flight
// product: a block of 256 threads owns GT_F frequencies x GT_S series; thread (tx, ty) = (tid % 16, tid / 16)
// holds the frequencies 4 ty + a, a < 4, against the series 32 j + 2 tx + h, j < 4, h < 2
constexpr int GT_BLOCK = 256;
constexpr int GT_F = 64;
constexpr int GT_S = 128;
constexpr int GT_RF = 4;
constexpr int GT_RS = 8;
constexpr int GT_SLICE = 16;           // epochs staged through LDS at a time
constexpr int GT_UPITCH = GT_F + 2;    // doubles of an epoch's u (v) row in LDS: 528 bytes, 16-byte aligned
constexpr size_t GLS_TABLE_BYTES = (size_t)64 << 20;  // a chunk's u and v tables together, about

// The epochs [i, i + 2) of frequency k per turn, k = e / ceil(N / 2) over the launch's turns e; row k of the
// outputs starts at k ld.  wide: both outputs 16-byte aligned and ld even -- a pair is one 16-byte store.
__global__ void __launch_bounds__(GB_BLOCK)
    gls_basis_kernel(const double* __restrict__ tau, int N, int64_t ld, double f0, double df, int64_t k0, int F,
                     int wide, double* __restrict__ cos_out, double* __restrict__ sin_out,
                     double* __restrict__ freq_out) {
#pragma clang fp contract(off)
    const uint64_t pairs = (uint64_t)(N + 1) / 2, total = (uint64_t)F * pairs;
    const uint64_t stride = (uint64_t)gridDim.x * GB_BLOCK;
    for (uint64_t e = (uint64_t)blockIdx.x * GB_BLOCK + threadIdx.x; e < total; e += stride) {
        const uint64_t k = e / pairs;
        const int i = 2 * (int)(e - k * pairs);
        const double f = fma((double)(k0 + (int64_t)k), df, f0);
        const int cnt = i + 1 < N ? 2 : 1;
        double s[2] = {0.0, 0.0}, c[2] = {0.0, 0.0};
        for (int j = 0; j < cnt; j++) {
            const double x = f * tau[i + j];
            const double r = x - rint(x);  // exact: the phase in cycles, within [-1/2, 1/2]
            sincospi(2.0 * r, &s[j], &c[j]);
        }
        const size_t o = (size_t)k * (size_t)ld + (size_t)i;
        if (wide && cnt == 2) {
            *reinterpret_cast<double2*>(cos_out + o) = double2{c[0], c[1]};
            *reinterpret_cast<double2*>(sin_out + o) = double2{s[0], s[1]};
        } else {
            for (int j = 0; j < cnt; j++) {
                cos_out[o + j] = c[j];
                sin_out[o + j] = s[j];
            }
        }
        if (i == 0 && freq_out) freq_out[k] = f;
    }
}

// One pass of a thread over the epochs 0 .. N - 1, as prepare and centre make it twice each (the mean, then the
// sums): the loads of GL_BATCH epochs are issued together -- load(i) returns what the thread needs of epoch i; a
// batch that runs past the end loads epoch N - 1 again and does not use it -- and then used in order, use(i, e) for
// i ascending.  A thread's chain of fmas is serial; its loads need not be.  The order of the use calls is the
// definition's order of operations.
template <typename Load, typename Use>
__device__ __forceinline__ void gls_epochs(int N, const Load& load, const Use& use) {
    for (int i0 = 0; i0 < N; i0 += GL_BATCH) {
        decltype(load(0)) e[GL_BATCH];
#pragma unroll
        for (int j = 0; j < GL_BATCH; j++) e[j] = load(i0 + j < N ? i0 + j : N - 1);
#pragma unroll
        for (int j = 0; j < GL_BATCH; j++)
            if (i0 + j < N) use(i0 + j, e[j]);
    }
}

// Step 2 of the definition.  Row k of u holds c on entry and u on exit, of v likewise s and v.
__global__ void __launch_bounds__(GP_BLOCK)
    gls_prepare_kernel(const double* __restrict__ w, int N, int64_t ld, int F, int float_mean, double* __restrict__ u,
                       double* __restrict__ v, double* __restrict__ cc_out, double* __restrict__ ss_out,
                       double* __restrict__ cs_out) {
#pragma clang fp contract(off)
    const int k = (int)blockIdx.x * GP_BLOCK + (int)threadIdx.x;
    if (k >= F) return;
    double* cu = u + (size_t)k * (size_t)ld;
    double* sv = v + (size_t)k * (size_t)ld;
    struct Epoch {
        double c, s, w;
    };
    const auto load = [&](int i) { return Epoch{cu[i], sv[i], w[i]}; };
    double C = 0.0, S = 0.0;
    if (float_mean)
        gls_epochs(N, load, [&](int, const Epoch& e) {
            C = fma(e.w, e.c, C);
            S = fma(e.w, e.s, S);
        });
    double CC = 0.0, SS = 0.0, CS = 0.0;
    gls_epochs(N, load, [&](int i, const Epoch& e) {
        const double ct = e.c - C, st = e.s - S;
        const double ui = e.w * ct, vi = e.w * st;
        CC = fma(ui, ct, CC);
        SS = fma(vi, st, SS);
        CS = fma(ui, st, CS);
        cu[i] = ui;
        sv[i] = vi;
    });
    cc_out[k] = CC;
    ss_out[k] = SS;
    cs_out[k] = CS;
}

// Step 3.  z [N][zld], series s in column s (a wave reads and writes consecutive columns).
__global__ void __launch_bounds__(GC_BLOCK)
    gls_centre_kernel(const double* __restrict__ w, const double* __restrict__ data, const double* __restrict__ model,
                      int64_t model_ld, int N, int S, int64_t zld, int float_mean, double* __restrict__ z,
                      double* __restrict__ yy_out) {
#pragma clang fp contract(off)
    const int64_t s = (int64_t)blockIdx.x * GC_BLOCK + threadIdx.x;
    if (s >= S) return;
    const double* col = model ? model + (size_t)s : nullptr;
    struct Epoch {
        double y, w;
    };
    const auto load = [&](int i) {
        return Epoch{col ? data[i] - col[(size_t)i * (size_t)model_ld] : data[i], w[i]};
    };
    double m = 0.0;
    if (float_mean) gls_epochs(N, load, [&](int, const Epoch& e) { m = fma(e.w, e.y, m); });
    double yy = 0.0;
    gls_epochs(N, load, [&](int i, const Epoch& e) {
        const double zi = e.y - m;
        const double wz = e.w * zi;
        z[(size_t)i * (size_t)zld + (size_t)s] = zi;
        yy = fma(wz, zi, yy);
    });
    yy_out[s] = yy;
}

// Step 4.  Per slice of GT_SLICE epochs the block stages u and v of its frequencies, transposed to
// [epoch][frequency], and z of its series, [epoch][series], in LDS (2 x 8.25 + 16 KiB); per epoch a thread
// then reads its four u, four v (two 16-byte reads each, the same addresses across tx: a broadcast) and its
// eight z (four 16-byte reads, consecutive across tx: whole bank rows) for 64 independent fma chains.  Every
// global load is a 16-byte pair: the rows of u, v (ld) and z (zld) are even numbers of doubles from 16-byte
// aligned bases.  An absent frequency or series is staged as 0 and its results are not written.  An epoch
// past N is staged as 0 on both sides and summed like the others: fma(0, 0, acc) is acc bit for bit, since an
// accumulator that starts at +0 is never -0 (a sum is -0 only when both terms are), so the last slice needs
// no loop of its own.
__global__ void __launch_bounds__(GT_BLOCK)
    gls_product_kernel(const double* __restrict__ u, const double* __restrict__ v, int64_t ld,
                       const double* __restrict__ z, int64_t zld, const double* __restrict__ cc_in,
                       const double* __restrict__ ss_in, const double* __restrict__ cs_in,
                       const double* __restrict__ yy_in, int N, int F, int S, double* __restrict__ power,
                       int64_t power_ld) {
#pragma clang fp contract(off)
    __shared__ __attribute__((aligned(16))) double us[GT_SLICE][GT_UPITCH];
    __shared__ __attribute__((aligned(16))) double vs[GT_SLICE][GT_UPITCH];
    __shared__ __attribute__((aligned(16))) double zs[GT_SLICE][GT_S];
    const int tid = (int)threadIdx.x, tx = tid & 15, ty = tid >> 4;
    const int kb = (int)blockIdx.y * GT_F;
    const int64_t sb = (int64_t)blockIdx.x * GT_S;
    double yc[GT_RF][GT_RS], ys[GT_RF][GT_RS];
#pragma unroll
    for (int a = 0; a < GT_RF; a++)
#pragma unroll
        for (int b = 0; b < GT_RS; b++) yc[a][b] = ys[a][b] = 0.0;

    auto step = [&](int ii) {
        double uu[GT_RF], vv[GT_RF];
#pragma unroll
        for (int a = 0; a < GT_RF; a += 2) {
            const double2 p = *reinterpret_cast<const double2*>(&us[ii][GT_RF * ty + a]);
            const double2 q = *reinterpret_cast<const double2*>(&vs[ii][GT_RF * ty + a]);
            uu[a] = p.x, uu[a + 1] = p.y;
            vv[a] = q.x, vv[a + 1] = q.y;
        }
        double zz[GT_RS];
#pragma unroll
        for (int j = 0; j < GT_RS / 2; j++) {
            const double2 p = *reinterpret_cast<const double2*>(&zs[ii][32 * j + 2 * tx]);
            zz[2 * j] = p.x, zz[2 * j + 1] = p.y;
        }
#pragma unroll
        for (int a = 0; a < GT_RF; a++)
#pragma unroll
            for (int b = 0; b < GT_RS; b++) {
                yc[a][b] = fma(uu[a], zz[b], yc[a][b]);
                ys[a][b] = fma(vv[a], zz[b], ys[a][b]);
            }
    };

    for (int i0 = 0; i0 < N; i0 += GT_SLICE) {
        for (int p = tid; p < GT_F * GT_SLICE / 2; p += GT_BLOCK) {
            const int row = p / (GT_SLICE / 2), pi = 2 * (p % (GT_SLICE / 2));
            const int k = kb + row, i = i0 + pi;
            double2 a{0.0, 0.0}, b{0.0, 0.0};
            if (k < F) {
                const size_t o = (size_t)k * (size_t)ld + (size_t)i;
                if (i + 1 < N) {
                    a = *reinterpret_cast<const double2*>(u + o);
                    b = *reinterpret_cast<const double2*>(v + o);
                } else if (i < N) {
                    a.x = u[o];
                    b.x = v[o];
                }
            }
            us[pi][row] = a.x, us[pi + 1][row] = a.y;
            vs[pi][row] = b.x, vs[pi + 1][row] = b.y;
        }
        for (int p = tid; p < GT_SLICE * GT_S / 2; p += GT_BLOCK) {
            const int ii = p / (GT_S / 2), sp = 2 * (p % (GT_S / 2));
            const int i = i0 + ii;
            const int64_t s = sb + sp;
            double2 a{0.0, 0.0};
            if (i < N && s < zld) a = *reinterpret_cast<const double2*>(z + (size_t)i * (size_t)zld + (size_t)s);
            *reinterpret_cast<double2*>(&zs[ii][sp]) = a;
        }
        __syncthreads();
#pragma unroll 4
        for (int ii = 0; ii < GT_SLICE; ii++) step(ii);
        __syncthreads();
    }

#pragma unroll
    for (int a = 0; a < GT_RF; a++) {
        const int k = kb + GT_RF * ty + a;
        if (k >= F) continue;
        const double CC = cc_in[k], SS = ss_in[k], CS = cs_in[k];
        const double ccss = CC * SS, cscs = CS * CS;
        const double D = ccss - cscs;
#pragma unroll
        for (int b = 0; b < GT_RS; b++) {
            const int64_t s = sb + 32 * (b >> 1) + 2 * tx + (b & 1);
            if (s >= S) continue;
            const double YC = yc[a][b], YS = ys[a][b];
            const double t1 = (SS * YC) * YC;
            const double t2 = (CC * YS) * YS;
            const double t3 = (2.0 * (CS * YC)) * YS;
            const double num = (t1 + t2) - t3;
            const double den = yy_in[s] * D;
            power[(size_t)k * (size_t)power_ld + (size_t)s] = num / den;
        }
    }
}

// frequencies of a chunk of rvm_gls_power: a multiple of the product kernel's tile
int64_t gls_chunk_freqs(int N) {
    const int64_t ld = N + (N & 1);
    const int64_t c = (int64_t)(GLS_TABLE_BYTES / (16 * (size_t)ld)) / GT_F * GT_F;
    return c > GT_F ? c : GT_F;
}

// The workspace of rvm_gls_power, in doubles from a 16-byte aligned base (every part an even number of them):
//   u, v [fc][ld]   a chunk's table, fc = min(F, gls_chunk_freqs(N)), ld = N rounded up to even
//   cc, ss, cs [fc] the chunk's per-frequency sums
//   yy [S]          per series
//   z [N][zld]      zld = S rounded up to even
struct GlsLayout {
    int64_t ld, zld, fc;
    size_t u, v, cc, ss, cs, yy, z, total;
};

static GlsLayout gls_layout(int N, int F, int S) {
    GlsLayout L;
    L.ld = N + (N & 1);
    L.zld = (int64_t)S + (S & 1);
    const int64_t chunk = gls_chunk_freqs(N);
    L.fc = F < chunk ? F : chunk;
    const size_t fce = (size_t)L.fc + (size_t)(L.fc & 1);
    L.u = 0;
    L.v = L.u + (size_t)L.fc * (size_t)L.ld;
    L.cc = L.v + (size_t)L.fc * (size_t)L.ld;
    L.ss = L.cc + fce;
    L.cs = L.ss + fce;
    L.yy = L.cs + fce;
    L.z = L.yy + (size_t)L.zld;
    L.total = L.z + (size_t)N * (size_t)L.zld;
    return L;
}

size_t gls_workspace_bytes(int N, int F, int S) { return sizeof(double) * gls_layout(N, F, S).total; }

hipError_t launch_gls_basis(const double* tau, int N, int64_t ld, double f0, double df, int64_t k0, int F,
                            double* cos_out, double* sin_out, double* freq_out, hipStream_t st) {
    const uint64_t turns = (uint64_t)F * (uint64_t)((N + 1) / 2);
    unsigned blocks = blocks_of(turns, GB_BLOCK);
    if (turns > (uint64_t)GB_MAX_BLOCKS * GB_BLOCK) blocks = GB_MAX_BLOCKS;
    const int wide = (uintptr_t)cos_out % 16 == 0 && (uintptr_t)sin_out % 16 == 0 && ld % 2 == 0;
    gls_basis_kernel<<<dim3(blocks), GB_BLOCK, 0, st>>>(tau, N, ld, f0, df, k0, F, wide, cos_out, sin_out, freq_out);
    return hipGetLastError();
}

hipError_t launch_gls_power(const double* tau, const double* w, int N, const double* data, const double* model,
                            int64_t model_ld, int S, double f0, double df, int64_t k0, int F, int float_mean,
                            double* power, int64_t power_ld, double* freq_out, double* ws, hipStream_t st) {
    const GlsLayout L = gls_layout(N, F, S);
    gls_centre_kernel<<<dim3(blocks_of((uint64_t)S, GC_BLOCK)), GC_BLOCK, 0, st>>>(
        w, data, model, model_ld, N, S, L.zld, float_mean, ws + L.z, ws + L.yy);
    hipError_t e = hipGetLastError();
    for (int64_t kc = 0; kc < F && e == hipSuccess; kc += L.fc) {
        const int fc = (int)(F - kc < L.fc ? F - kc : L.fc);
        e = launch_gls_basis(tau, N, L.ld, f0, df, k0 + kc, fc, ws + L.u, ws + L.v, freq_out ? freq_out + kc : nullptr,
                             st);
        if (e != hipSuccess) break;
        gls_prepare_kernel<<<dim3(blocks_of((uint64_t)fc, GP_BLOCK)), GP_BLOCK, 0, st>>>(
            w, N, L.ld, fc, float_mean, ws + L.u, ws + L.v, ws + L.cc, ws + L.ss, ws + L.cs);
        e = hipGetLastError();
        if (e != hipSuccess) break;
        gls_product_kernel<<<dim3(blocks_of((uint64_t)S, GT_S), blocks_of((uint64_t)fc, GT_F)), GT_BLOCK, 0, st>>>(
            ws + L.u, ws + L.v, L.ld, ws + L.z, L.zld, ws + L.cc, ws + L.ss, ws + L.cs, ws + L.yy, N, fc, S,
            power + (size_t)kc * (size_t)power_ld, power_ld);
        e = hipGetLastError();
    }
    return e;
}

}  // namespace rvm
