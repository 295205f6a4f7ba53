// rvm_walker.h -- per-walker pieces shared by the likelihood kernel (rvm_logl.hip: main pass and
// extension) and the refinement kernel (rvm_refine.hip: halving passes): the segment loop, the
// walker's parameters and Wisdom-Holman lane state at t = 0, the sampler's accept inputs, the
// direction-meeting encoding and the walker's final writes.  Both translation units compile with
// `#pragma clang fp contract(on)` before including it, so a walker's bits are the same in both.
#pragma once
#include "rvm_device.h"
#include "rvm_internal.h"
#include "rvm_stretch.h"

// the gated drift's second chance for a lane whose first Halley step fails (rvm_device.h drift ACC)
#ifndef RVM_DRIFT_ACC
#define RVM_DRIFT_ACC 0
#endif

namespace rvm {

// One epoch-to-epoch segment of ns Wisdom-Holman kick-drift-kick steps of size h (ns >= 1,
// wave-uniform): K(h/2) [D(h) K(h)]^(ns-1) D(h) K(h/2).  kp holds the interaction at the current
// positions (rvm_device.h kick_prep): evaluated at the end of the previous segment, it serves this
// segment's opening half kick, and leaves holding the one at the next epoch.  (The step loop is
// unrolled by hand: the compiler will not unroll a runtime trip count around the convergent DPP /
// ballot operations.)
template <int NT, bool GATED, bool D3, int NP, int L, int KG = 0, int ACC = RVM_DRIFT_ACC>
__device__ __forceinline__ void segment_steps(Lane<NP>& s, KickPrep<NP>& kp, double h, int ns, bool& bad) {
    lane_set_step(s, h);
    const VConsts vk = vconsts_for<NT>();  // loop-invariant VGPR constants
    kick_apply<NP, true, D3>(s, kp);
    int j = 0;
    for (; j + 2 <= ns - 1; j += 2) {
        drift<NT, GATED, D3, NP, KG, ACC>(s, h, bad, vk);
        kp = kick_prep<NP, L, D3>(s, vk.c1875);
        kick_apply<NP, false, D3>(s, kp);
        drift<NT, GATED, D3, NP, KG, ACC>(s, h, bad, vk);
        kp = kick_prep<NP, L, D3>(s, vk.c1875);
        kick_apply<NP, false, D3>(s, kp);
    }
    if (j < ns - 1) {
        drift<NT, GATED, D3, NP, KG, ACC>(s, h, bad, vk);
        kp = kick_prep<NP, L, D3>(s, vk.c1875);
        kick_apply<NP, false, D3>(s, kp);
    }
    drift<NT, GATED, D3, NP, KG, ACC>(s, h, bad, vk);
    kp = kick_prep<NP, L, D3>(s, vk.c1875);
    kick_apply<NP, true, D3>(s, kp);
}

// SPEC: run the segment with ungated drifts (rvm_device.h) and vote once at its end; if any lane
// of the wave had a step that needs the general solver, restore the segment's initial state and
// redo it gated.  Used on the fine levels, where such steps are rare.  Returns whether the
// segment was redone (wave-uniform).  Either way every lane ends bit-identical to a gated run.
template <int NT, bool SPEC, bool D3, int NP, int L, int KG = 0, int ACC = RVM_DRIFT_ACC>
__device__ __forceinline__ bool segment(Lane<NP>& s, KickPrep<NP>& kp, double h, int ns, int& redo) {
    bool bad = false;
    if constexpr (SPEC) {
        const double rx = s.rx, ry = s.ry, vx = s.vx, vy = s.vy, r = s.r, ir = s.ir;
        const double rz = s.rz, vz = s.vz;
        const uint64_t encm = s.encm;
        const KickPrep<NP> kp0 = kp;
        segment_steps<NT, false, D3, NP, L, KG, ACC>(s, kp, h, ns, bad);
        if (__builtin_expect(ballot(bad) != 0, 0)) {
#ifdef RVM_PROFILE
            redo++;
#endif
            s.rx = rx;
            s.ry = ry;
            s.vx = vx;
            s.vy = vy;
            s.rz = rz;
            s.vz = vz;
            s.r = r;
            s.ir = ir;
            s.encm = encm;
            kp = kp0;
            segment_steps<NT, true, D3, NP, L, KG, ACC>(s, kp, h, ns, bad);
            return true;
        }
    } else {
        segment_steps<NT, true, D3, NP, L, KG, ACC>(s, kp, h, ns, bad);
    }
    (void)redo;
    return false;
}

// a gated segment with the Stumpff series length of the level (nt: 6, 7 or 8); KG: the Kepler guess
// (rvm_device.h drift: 0 fourth order, 1 fifth)
// (late: the gated drift's late vote, rvm_device.h drift ACC 3 -- the same bits, faster where few
// lanes fail their first Halley step: the refinement passes' fine levels)
template <bool D3, int NP, int L, int KG = 0, int ACC = RVM_DRIFT_ACC>
__device__ __forceinline__ void segment_gated(Lane<NP>& s, KickPrep<NP>& kp, double h, int ns, int nt,
                                              bool late = false) {
    int unused = 0;
    if (late) {
        if (nt <= 6)
            segment<6, false, D3, NP, L, KG, 3>(s, kp, h, ns, unused);
        else if (nt == 7)
            segment<7, false, D3, NP, L, KG, 3>(s, kp, h, ns, unused);
        else
            segment<8, false, D3, NP, L, KG, 3>(s, kp, h, ns, unused);
        return;
    }
    if (nt <= 6)
        segment<6, false, D3, NP, L, KG, ACC>(s, kp, h, ns, unused);
    else if (nt == 7)
        segment<7, false, D3, NP, L, KG, ACC>(s, kp, h, ns, unused);
    else
        segment<8, false, D3, NP, L, KG, ACC>(s, kp, h, ns, unused);
}

// The speculation back-off of a wave (wave-uniform; fresh: {0, 4}): segments left to run gated after a redo, and
// the next back-off -- doubled by each redo up to 64, back to 4 after a clean speculative segment.  A head hands
// it to its tail as one LDS word: as two members there it moved the level-split instantiations' registers
// (3 planets 170 -> 204 VGPRs).
struct SpecState {
    int off, bo;
    __device__ __forceinline__ int pack() const { return off | (bo << 16); }
    __device__ __forceinline__ static SpecState unpack(int w) { return SpecState{w & 0xFFFF, w >> 16}; }
};
// One segment of a level with the Stumpff series length nt; spec (implies nt <= 6): speculate unless a recent
// segment of this wave needed a redo -- walkers whose orbits keep needing the general solver then run gated for
// a while instead of paying for redos; the same bits either way.  (The extension's; the main loop of
// rvm_logl.hip writes the same text out -- a change to one is a change to both.)
template <bool D3, int NP, int L, int KG = 0>
__device__ __forceinline__ void segment_backoff(Lane<NP>& s, KickPrep<NP>& kp, double h, int ns, int nt, bool spec,
                                                SpecState& st, int& redo) {
    if (spec) {
        if (st.off == 0) {
            if (segment<6, true, D3, NP, L, KG>(s, kp, h, ns, redo)) {
                st.off = st.bo;
                st.bo = st.bo < 64 ? 2 * st.bo : 64;
            } else {
                st.bo = 4;
            }
        } else {
            segment<6, false, D3, NP, L, KG>(s, kp, h, ns, redo);
            st.off--;
        }
    } else {
        segment_gated<D3, NP, L, KG>(s, kp, h, ns, nt);
    }
}
// A lane's eight dynamic doubles to and from rows of 64 doubles (o: the lane's entry of row 0): the t = 0 state,
// a head's hand-off to its tail.  encm stays with the caller (zeroed, or handed over as a wave-uniform word).
template <int NP>
__device__ __forceinline__ void lane_save(const Lane<NP>& s, double* o) {
    o[0] = s.rx;
    o[64] = s.ry;
    o[128] = s.vx;
    o[192] = s.vy;
    o[256] = s.rz;
    o[320] = s.vz;
    o[384] = s.r;
    o[448] = s.ir;
}
template <int NP>
__device__ __forceinline__ void lane_load(Lane<NP>& s, const double* in) {
    s.rx = in[0];
    s.ry = in[64];
    s.vx = in[128];
    s.vy = in[192];
    s.rz = in[256];
    s.vz = in[320];
    s.r = in[384];
    s.ir = in[448];
}
// One direction's epoch schedule as staged in LDS: [E] seg_h1 | [E] obs_rv | [E] obs_s2 | [E] (seg_n, obs_idx)
struct SchedView {
    double *len, *rv, *s2;
    int *n, *idx;
    __device__ __forceinline__ SchedView(double* b, int E)
        : len(b), rv(b + E), s2(b + 2 * E), n(reinterpret_cast<int*>(b + 3 * E)), idx(n + E) {}
};
__device__ __forceinline__ void stage_sched(const DirSched& S, const SchedView& v, int i0, int stride) {
    for (int i = i0; i < S.n_epochs; i += stride) {  // (epochs i0, i0 + stride, ... of S into its view)
        v.len[i] = S.seg_h1[i];
        v.rv[i] = S.obs_rv[i];
        v.s2[i] = S.obs_s2[i];
        v.n[i] = S.seg_n[i];
        v.idx[i] = S.obs_idx[i];
    }
}

// kernel parameter row r of walker w: from the SoA input, or (fused sampler step) the row's fixed
// value or the walker's proposal of the free parameter feeding it: MH (sa.mh_scale), or stretch
// (kind 1 / 2: half 1's walker of a speculative iteration against its partner's rejected /
// accepted position, StretchArgs)
__device__ __forceinline__ double walker_param(bool mapped, const double* __restrict__ params, int W, int w,
                                               const StretchArgs& sa, int r, double z, int j, int kind, double zp,
                                               int jp) {
    if (!mapped) return params[(size_t)r * W + w];
    const int k = sa.src[r];
    if (k < 0) return sa.base[r];
    if (sa.fd_x) return fd_point(sa.fd_x, sa.fd_floor, sa.fd_rel, sa.fd_n, k, w);
    if (sa.mh_scale)
        return mh_q(sa.x[(size_t)k * sa.xstride + w], sa.mh_step, sa.mh_scale[k],
                    mh_normal(sa.seed, (uint64_t)(sa.s0_begin + w), sa.iteration, k));
    if (kind == 0) return stretch_q(sa.c[(size_t)j * sa.dim + k], z, sa.x[(size_t)k * sa.xstride + w]);
    double c = sa.c0[(size_t)j * sa.dim + k];
    if (kind == 2) c = stretch_q(sa.c[(size_t)jp * sa.dim + k], zp, c);  // q0(j): bit-identical to slot j's
    return stretch_q(c, z, sa.x1[(size_t)k * sa.n_spec + w]);
}

// a fused launch's walker slot: its kind (0 = half-step / half 0, 1 / 2 = half 1 against its
// partner's rejected / accepted position), walker index within its half, its stretch draws and
// (kind 2) the partner's
__device__ __forceinline__ void stretch_slot(const StretchArgs& sa, int wl, int& kind, int& wk, double& z, int& j,
                                             double& zp, int& jp) {
    const int nsp = sa.n_spec;
    kind = nsp > 0 ? (wl < nsp ? 0 : (wl < 2 * nsp ? 1 : 2)) : 0;
    wk = wl - kind * nsp;
    // (one call for the slot's own draw, each result in a local of its own: two calls writing z, j
    // from both branches were merged into one through a select of their addresses, which put z, j
    // in scratch -- 56 B per lane in the likelihood kernel)
    const uint64_t key = kind == 0 ? (uint64_t)(sa.s0_begin + wk) : (uint64_t)(sa.s1_begin + wk);
    double z0;
    int j0;
    stretch_draw(sa.seed, key, sa.iteration, kind == 0 ? sa.half : 1u, sa.a, sa.n1, z0, j0);
    z = z0;
    j = j0;
    double z1 = 0.0;
    int j1 = 0;
    // the partner's own draws (half 0's keys are its global indices 0 .. n1-1)
    if (kind == 2) stretch_draw(sa.seed, (uint64_t)j0, sa.iteration, 0u, sa.a, sa.n1, z1, j1);
    zp = z1;
    jp = j1;
}

// ---- setup_sim (state.py:36-47): prior, Pal -> heliocentric (own planet) -> Jacobi, Hill exit ----
// rowv: the walker's kernel parameter rows (m, a, h, k, l [, ix, iy] per planet).  Sets the lane's
// state at t = 0 (lane pl_idx of the walker's L lanes), `status` (RVM_STATUS_PRIOR, else
// unchanged) and e2w, the walker's largest e^2 (the eccentricity guard).
template <int NP, bool D3, int L>
__device__ __forceinline__ void walker_setup(const double* rowv, const int pl_idx, const double hill_factor,
                                             Lane<NP>& s, int& status, double& e2w) {
    constexpr int PR = D3 ? 7 : 5;  // parameter rows per planet
    double pa[NP], ph[NP], pk[NP], pl[NP], pix[NP], piy[NP];
#pragma unroll
    for (int p = 0; p < NP; p++) {
        s.m[p] = rowv[PR * p + 0];
        pa[p] = rowv[PR * p + 1];
        ph[p] = rowv[PR * p + 2];
        pk[p] = rowv[PR * p + 3];
        pl[p] = rowv[PR * p + 4];
        pix[p] = D3 ? rowv[PR * p + 5] : 0.0;
        piy[p] = D3 ? rowv[PR * p + 6] : 0.0;
        bool bad = !(pa[p] > 0.02) || !(s.m[p] > 5e-6) || !(ph[p] * ph[p] + pk[p] * pk[p] < 1.0) ||
                   !isfinite(pl[p]);
        if constexpr (D3) bad = bad || !(pix[p] * pix[p] + piy[p] * piy[p] < 4.0);  // state.py:311-313
        if (bad) status = RVM_STATUS_PRIOR;
    }
    e2w = 0.0;
#pragma unroll
    for (int p = 0; p < NP; p++) e2w = fmax(e2w, ph[p] * ph[p] + pk[p] * pk[p]);
    if (status != RVM_STATUS_OK) {  // keep the lane numerically benign; its result is discarded
#pragma unroll
        for (int p = 0; p < NP; p++) {
            s.m[p] = 1e-3;
            pa[p] = 1.0 + p;
            ph[p] = 0.0;
            pk[p] = 0.0;
            pl[p] = 0.0;
            pix[p] = 0.0;
            piy[p] = 0.0;
        }
    }
    s.p = pl_idx < NP ? pl_idx : NP - 1;
    s.q = pl_idx;
    double Mi[NP + 1];
    Mi[0] = 1.0;
    double hill = 0.0;
#pragma unroll
    for (int p = 0; p < NP; p++) {
        Mi[p + 1] = Mi[p] + s.m[p];
        const double rh = pa[p] * cbrt(s.m[p] / 3.0);
        hill = rh > hill ? rh : hill;
    }
#pragma unroll
    for (int p = 0; p <= NP; p++) s.iMi[p] = 1.0 / Mi[p];
#pragma unroll
    for (int p = 0; p < NP; p++) s.mu[p] = s.m[p] / Mi[p + 1];
    s.dmin2 = (hill_factor * hill) * (hill_factor * hill);
    double own_m = s.m[0], own_a = pa[0], own_h = ph[0], own_k = pk[0], own_l = pl[0], own_M = Mi[1];
    double own_ix = pix[0], own_iy = piy[0];
#pragma unroll
    for (int p = 1; p < NP; p++) {
        if (s.p == p) {
            own_m = s.m[p];
            own_a = pa[p];
            own_h = ph[p];
            own_k = pk[p];
            own_l = pl[p];
            own_M = Mi[p + 1];
            own_ix = pix[p];
            own_iy = piy[p];
        }
    }
    s.GM = own_M;
    double X, Y, VX, VY, Z = 0.0, VZ = 0.0;
    pal_to_cart(1.0 + own_m, own_a, own_l, own_k, own_h, X, Y, VX, VY);
    if constexpr (D3) {
        if (own_ix != 0.0 || own_iy != 0.0) pal_incline(own_ix, own_iy, X, Y, Z, VX, VY, VZ);
    }
    {
        // r'_p = x_p - (sum_{q<p} m_q x_q) / M_{p-1}   (heliocentric -> Jacobi)
        double sx = 0.0, sy = 0.0, sz = 0.0, svx = 0.0, svy = 0.0, svz = 0.0;
        double jx = X, jy = Y, jz = Z, jvx = VX, jvy = VY, jvz = VZ;
#pragma unroll
        for (int q = 0; q < NP - 1; q++) {
            const double xq = grp_get<L>(X, q), yq = grp_get<L>(Y, q);
            const double vxq = grp_get<L>(VX, q), vyq = grp_get<L>(VY, q);
            sx += s.m[q] * xq;
            sy += s.m[q] * yq;
            svx += s.m[q] * vxq;
            svy += s.m[q] * vyq;
            if constexpr (D3) {
                sz += s.m[q] * grp_get<L>(Z, q);
                svz += s.m[q] * grp_get<L>(VZ, q);
            }
            if (s.p == q + 1) {
                jx = X - sx * s.iMi[q + 1];
                jy = Y - sy * s.iMi[q + 1];
                jvx = VX - svx * s.iMi[q + 1];
                jvy = VY - svy * s.iMi[q + 1];
                if constexpr (D3) {
                    jz = Z - sz * s.iMi[q + 1];
                    jvz = VZ - svz * s.iMi[q + 1];
                }
            }
        }
        s.rx = jx;
        s.ry = jy;
        s.vx = jvx;
        s.vy = jvy;
        s.rz = D3 ? jz : 0.0;
        s.vz = D3 ? jvz : 0.0;
    }
    s.r = D3 ? sqrt(s.rx * s.rx + s.ry * s.ry + s.rz * s.rz) : sqrt(s.rx * s.rx + s.ry * s.ry);
    s.ir = 1.0 / s.r;
    s.encm = 0;
    lane_finish(s);
}

// global-address-space views for agent-scope atomics (cdna_hip_programming.md §6 Guideline 16)
typedef __attribute__((address_space(1))) unsigned long long gu64;
typedef __attribute__((address_space(1))) int gi32;
// Bounded waits: a cross-workgroup wait gives up after P.spin_ticks of the 100 MHz real-time counter
// WITHOUT PROGRESS (restarted whenever the awaited side advances), counts the give-up in the plan's
// fault counter (rvm_plan_faults) and reports its walkers NONFINITE instead of hanging the GPU.
struct SpinClock {
    unsigned long long last;
    __device__ __forceinline__ void restart() { last = __builtin_amdgcn_s_memrealtime(); }
    __device__ __forceinline__ bool expired(unsigned long long ticks) const {
        return __builtin_amdgcn_s_memrealtime() - last > ticks;
    }
};
// The bounded wait on another wave's progress: polls progress() (an int >= 0, wave-uniform) every s_sleep SLEEP
// until done(progress); the clock restarts whenever the value moves, `ticks` without a move gives up (returns
// true).  The level-split layout's waits on LDS counters; the LDS-coupled layouts' two write the same loop out
// (rvm_logl.hip lc_wait: the call cost the 3-planet paired layout time).  The level-split combiner's polls of
// the HBM-handed values keep their own shape on purpose (a straight-line first test, a bottom-tested loop: the
// compiler then does not wait for every prefetched load in flight).
template <int SLEEP, typename Progress, typename Done>
__device__ __forceinline__ bool wait_progress(SpinClock& clk, unsigned long long ticks, Progress&& progress,
                                              Done&& done) {
    int seen = -1;
    for (;;) {
        const int p = progress();
        if (done(p)) return false;
        if (p != seen) {
            seen = p;
            clk.restart();
        } else if (clk.expired(ticks)) {
            return true;
        }
        __builtin_amdgcn_s_sleep(SLEEP);
    }
}

// A gated segment (segment_gated) that a partner can stop part-way: the work a team B or an eager
// block does speculatively (rvm_refine.hip) is cancelled through a word that reaches `tag`.  Polled
// at the epochs alone, a cancel waited for the rest of the segment -- up to ~100 us on the passes'
// long segments, which kept the refinement launch open after team A had finished every walker
// (scripts/probe/refine_prof.py).  The words (c1 may be null) are loaded every CH steps, each load
// tested after the CH steps that follow it (no wait on the step chain).  Returns false when cancelled:
// the lanes' state is then partial, and the caller discards it.  A segment that runs to its end
// computes exactly segment_gated's bits.
template <int NT, bool D3, int NP, int L, int KG, int CH = 64, int ACC = RVM_DRIFT_ACC>
__device__ __forceinline__ bool segment_steps_c(Lane<NP>& s, KickPrep<NP>& kp, double h, int ns, const gu64* c0,
                                                const gu64* c1, unsigned long long tag) {
    bool bad = false;
    lane_set_step(s, h);
    const VConsts vk = vconsts_for<NT>();
    kick_apply<NP, true, D3>(s, kp);
    // (unconditional loads: a load under a branch is waited for where the branches join; c1 null
    // reads c0 twice)
    const gu64* w1 = c1 ? c1 : c0;
    auto load = [](const gu64* c) { return __hip_atomic_load(c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); };
    // the ns - 1 drift-kick pairs in chunks of CH steps, each chunk's loop the plain segment_steps
    // loop; the words are loaded before a chunk and compared after it.  A compare before the chunk
    // made the wave wait for the load there, a test inside the step loop cost ~60 cycles per step, and
    // chunks of 16 (32) steps still ~17 (~3) -- the agent-scope load outlasting the chunk; 64 steps
    // cost nothing measurable and bound a cancel's latency at ~17 us (scripts/probe/seg_bench.hip,
    // profiles/r05q_seg_bench_cancel_chunks.txt)
    int left = ns - 1;
    while (left >= 2) {
        const unsigned long long a = load(c0), b = load(w1);
        const int c = left < CH ? (left & ~1) : CH;
        for (int j = 0; j < c; j += 2) {
            drift<NT, true, D3, NP, KG, ACC>(s, h, bad, vk);
            kp = kick_prep<NP, L, D3>(s, vk.c1875);
            kick_apply<NP, false, D3>(s, kp);
            drift<NT, true, D3, NP, KG, ACC>(s, h, bad, vk);
            kp = kick_prep<NP, L, D3>(s, vk.c1875);
            kick_apply<NP, false, D3>(s, kp);
        }
        left -= c;
        if (__builtin_amdgcn_readfirstlane((int)((a == tag) | (b == tag)))) return false;
    }
    if (left == 1) {
        drift<NT, true, D3, NP, KG, ACC>(s, h, bad, vk);
        kp = kick_prep<NP, L, D3>(s, vk.c1875);
        kick_apply<NP, false, D3>(s, kp);
    }
    drift<NT, true, D3, NP, KG, ACC>(s, h, bad, vk);
    kp = kick_prep<NP, L, D3>(s, vk.c1875);
    kick_apply<NP, true, D3>(s, kp);
    return true;
}

template <bool D3, int NP, int L, int KG = 0, int ACC = RVM_DRIFT_ACC>
__device__ __forceinline__ bool segment_gated_c(Lane<NP>& s, KickPrep<NP>& kp, double h, int ns, int nt,
                                                const gu64* c0, const gu64* c1, unsigned long long tag,
                                                bool late = false) {
    if (late) {
        if (nt <= 6) return segment_steps_c<6, D3, NP, L, KG, 64, 3>(s, kp, h, ns, c0, c1, tag);
        if (nt == 7) return segment_steps_c<7, D3, NP, L, KG, 64, 3>(s, kp, h, ns, c0, c1, tag);
        return segment_steps_c<8, D3, NP, L, KG, 64, 3>(s, kp, h, ns, c0, c1, tag);
    }
    if (nt <= 6) return segment_steps_c<6, D3, NP, L, KG, 64, ACC>(s, kp, h, ns, c0, c1, tag);
    if (nt == 7) return segment_steps_c<7, D3, NP, L, KG, 64, ACC>(s, kp, h, ns, c0, c1, tag);
    return segment_steps_c<8, D3, NP, L, KG, 64, ACC>(s, kp, h, ns, c0, c1, tag);
}

// ---- the two directions of a walker meet (rvm_logl.hip finish) -------------------------------
// One 64-bit slot per walker (plan workspace, RVM_SLOT_EMPTY between launches).  The direction that
// arrives first leaves its result there, the second takes it with one agent-scope exchange:
//   settled  chi2 >= 0 (sign bit clear, finite)
//   open     -lb (sign bit set, finite; -0.0 for lb = 0): the adaptive resolution's lower bound on
//            the direction's chi2 (rvm_refine.hip, oracle/rvoracle.c walker_cut)
//   status   a negative quiet NaN whose low byte is the status (PRIOR, ENCOUNTER, NONFINITE, ...)
#define RVM_SLOT_EMPTY 0x7FF4DEADBEEF0001ULL  // a NaN pattern no direction result can take
#define RVM_SLOT_STATUS 0xFFF8000000000000ULL
__device__ __forceinline__ unsigned long long slot_status(int st) {
    return RVM_SLOT_STATUS | (unsigned long long)(unsigned)st;
}
__device__ __forceinline__ bool slot_is_status(unsigned long long b) { return (b & 0xFFFFFFFFFFFFFF00ULL) == RVM_SLOT_STATUS; }

// per-direction flag bits of a walker (encflag / enc): 1 encounter, 2 prior, 4 unresolved after
// the last refinement, 8 a hand-off of this launch gave up (the values are not trustworthy)
#define RVM_ENC_UNRESOLVED 4
#define RVM_ENC_FAULT 8

// a direction's status from its flag bits and chi2 (prior > encounter > fault > unresolved;
// a settled direction's non-finite chi2 is NONFINITE)
__device__ __forceinline__ int dir_status(int enc, bool open, double chi2) {
    int st = (enc & 2) ? RVM_STATUS_PRIOR : RVM_STATUS_OK;
    if (st == RVM_STATUS_OK && (enc & 1)) st = RVM_STATUS_ENCOUNTER;
    if (st == RVM_STATUS_OK && (enc & RVM_ENC_FAULT)) st = RVM_STATUS_NONFINITE;
    if (st == RVM_STATUS_OK && (enc & RVM_ENC_UNRESOLVED)) st = RVM_STATUS_UNRESOLVED;
    if (st == RVM_STATUS_OK && !open && !isfinite(chi2)) st = RVM_STATUS_NONFINITE;
    return st;
}

// lower bound on an open direction's chi2 after a stage (oracle/rvoracle.c lb_of): chi2 less the
// change the stage brought (d; +inf if none) or a large multiple of its estimate, 0 if non-finite
__device__ __forceinline__ double open_lb(double chi2, double d, double est_raw) {
    const double b = chi2 - fmin(d, RVM_CUT_EST_FACTOR * est_raw);
    return b > 0.0 ? b : 0.0;  // (NaN -> 0)
}

// ---- the adaptive resolution's rules after the main pass, one statement each (oracle/rvoracle.c) ----
// The Richardson combiner of one epoch for one walker: from the levels' star vx (lv(q), level q's value) the
// extrapolated RV, the RV without the coarsest level, and the epoch's terms of chi2 and of the error estimate
// against the observation ob of variance s2; with want5, s5 = the extension's partial sum over the main pass's
// levels.  Ascending q from 0.0, rv3 from q = 1, each term one expression: the bits rest on it (fp contract).
// The likelihood kernel's combiners and side_pass call this; refine_kernel's epoch loop writes these expressions
// out itself -- its register allocation is pinned by a test and the call moved it (DESIGN.md section 10 item
// 10): a change to one is a change to both.
template <typename Lv>
__device__ __forceinline__ void combine_epoch(const DevPlan& P, const int nl, Lv&& lv, const double ob,
                                              const double s2, double& rvx, double& rv3, double& dc2, double& de2,
                                              const bool want5, double& s5) {
    rvx = 0.0;
    rv3 = 0.0;
    for (int q = 0; q < nl; q++) rvx += P.lw[q] * lv(q);
    for (int q = 1; q < nl; q++) rv3 += P.lw3[q] * lv(q);
    const double r = rvx - ob;
    dc2 = (r * r) / s2;
    de2 = fabs((rvx - rv3) * (r + (rv3 - ob))) / s2;
    if (want5) {
        s5 = 0.0;
        for (int q = 0; q < nl; q++) s5 += P.lw5[q] * lv(q);
    }
}
// The extension's sums at one epoch: r5 = all nl + 1 levels (s5 the main pass's partial sum, vx the extension
// level's value of weight w5), its chi2 term dc5 and the term dd5 of its change against the main pass's RV r.
__device__ __forceinline__ void extension_epoch(const double s5, const double w5, const double vx, const double r,
                                                const double ob, const double s2, double& r5, double& dc5,
                                                double& dd5) {
    r5 = s5 + w5 * vx;
    const double q = r5 - ob;
    dc5 = (q * q) / s2;
    dd5 = fabs((r5 - r) * (q + (r - ob))) / s2;
}
// One level's flag word as it joins the walker's (OR them): on an adaptive plan an encounter that a level other
// than the finest (DevPlan::fin_level) sees moves to RVM_ENC_COARSE.  (Values: references cost scratch.)
#define RVM_ENC_COARSE 0x100
__device__ __forceinline__ int level_flags(const int f, const bool fin, const bool adaptive) {
    return fin || !adaptive ? f : (f & ~1) | ((f & 1) ? RVM_ENC_COARSE : 0);
}
// ... an encounter only the coarser levels saw: the direction refines instead (`cenc`)
__device__ __forceinline__ bool coarse_only_encounter(const int encs) {
    return (encs & RVM_ENC_COARSE) != 0 && (encs & 1) == 0;
}
// A direction stays open after the main pass (dir_main `bad`): no flag, and its estimate above the bound, a
// non-finite chi2 or estimate, the walker past the eccentricity guard (e2), or a coarse-only encounter.
__device__ __forceinline__ bool direction_open(const DevPlan& P, const int enc, const double chi2, const double est,
                                               const double e2, const bool cenc) {
    return enc == 0 && (est / P.npoints > P.rtol_dir || !isfinite(chi2) || !isfinite(est) ||
                        (P.ext_mult > 0 && e2 > P.e2_guard) || cenc);
}
// The extension's verdict on an open direction: 2 its own encounter (xenc) ends the walker ENCOUNTER, 1 a change
// dd within RVM_EXT_ACCEPT rtol_dir npoints settles it (false for a non-finite one) -- either way its chi2 is
// the extension's --, 0 it stays open.  coarse_blocks: a coarse-only encounter keeps the change from settling
// it; cx and lsx pass their cenc, extend_pass passes false -- it has no such test.
__device__ __forceinline__ int extension_verdict(const DevPlan& P, const bool xenc, const double dd,
                                                 const bool coarse_blocks) {
    if (xenc) return 2;
    return !coarse_blocks && dd <= RVM_EXT_ACCEPT * P.rtol_dir * P.npoints ? 1 : 0;
}
// A direction's lower bound on its chi2 after the main pass and the extension (oracle/rvoracle.c dir_extend): 0
// when settled; the extension's (xc5, its change xdd) when it ran and is finite, else the main pass's alone.
__device__ __forceinline__ double direction_lb(const bool need, const double chi2_main, const double est_raw,
                                               const bool xran, const double xc5, const double xdd) {
    if (!need) return 0.0;
    if (xran && isfinite(xc5) && isfinite(xdd)) return open_lb(xc5, xdd, est_raw);
    return open_lb(chi2_main, INFINITY, est_raw);
}
// ... with the cut guard (DevPlan::e2_cut): past it (past_cut = e2 > e2_cut; e2 is never NaN, walker_setup
// forms it with fmax from 0) the extension's bound counts only with cut_guard_k > 0, its change k-fold; a
// coarse-only encounter (cenc) has no bound at all.
__device__ __forceinline__ double guarded_lb(const DevPlan& P, const bool need, const double chi2_main,
                                             const double est_raw, const bool xran, const bool past_cut,
                                             const bool cenc, const double xc5, const double xdd) {
    if (cenc) return 0.0;
    return direction_lb(need, chi2_main, est_raw, xran && (!past_cut || P.cut_guard_k > 0.0), xc5,
                        past_cut ? P.cut_guard_k * xdd : xdd);
}

// The sampler's accept inputs of walker slot wo of a fused launch (the certain-reject test):
// dmode 0 none, 1 emcee stretch, 2 MH; z, u and the current lnp.  Half 1's slots of a speculative
// iteration accept later (rvm_stretch_iteration_end) but their inputs are known (sa.lnp1).
__device__ __forceinline__ void accept_inputs(const StretchArgs& sa, int wo, int& dmode, double& dz, double& du,
                                              double& dl) {
    dmode = 0;
    dz = du = dl = 0.0;
    if (sa.c != nullptr) {
        int k2, wk2, j2, jp2;
        double z2, zp2;
        stretch_slot(sa, wo, k2, wk2, z2, j2, zp2, jp2);
        if (k2 == 0) {
            dmode = 1;
            du = stretch_u3(sa.seed, (uint64_t)(sa.s0_begin + wo), sa.iteration, sa.half);
            dl = sa.lnp[wo];
        } else if (sa.lnp1 != nullptr) {
            dmode = 1;
            du = stretch_u3(sa.seed, (uint64_t)(sa.s1_begin + wk2), sa.iteration, 1u);
            dl = sa.lnp1[wk2];
        }
        dz = z2;
    } else if (sa.mh_scale != nullptr) {
        dmode = 2;
        du = mh_u(sa.seed, (uint64_t)(sa.s0_begin + wo), sa.iteration);
        dl = sa.lnp[wo];
    }
}

__device__ __forceinline__ bool accepts_at(const StretchArgs& sa, int dmode, double dz, double du, double dl,
                                           double lp) {
    return dmode == 1 ? stretch_accepts(sa.dim, dz, lp, dl, du) : mh_accepts(lp, dl, du);
}

// The walker's final writes: logl / status, the fault counters, and (fused sampler launches) the
// accept with the proposal's rows row(r) written back on acceptance.
template <int R, typename Row>
__device__ __forceinline__ void walker_out(const DevPlan& P, const StretchArgs& sa, const int wo, const int stw,
                                           const double lp, double* __restrict__ logl_out,
                                           int32_t* __restrict__ status_out, Row&& row, const double z, const double u3,
                                           const double lnp0) {
    if (logl_out) logl_out[wo] = lp;
    if (status_out) status_out[wo] = stw;
    // (rare: counted for rvm_plan_faults -- never a silent rejection)
    if (stw == RVM_STATUS_NONFINITE || stw == RVM_STATUS_UNRESOLVED)
        __hip_atomic_fetch_add(P.counters + (stw == RVM_STATUS_NONFINITE ? 1 : 2), 1ull, __ATOMIC_RELAXED,
                               __HIP_MEMORY_SCOPE_AGENT);
    const bool mh = sa.mh_scale != nullptr;
    const bool fused = sa.c != nullptr || mh;
    if (fused && (sa.n_spec == 0 || wo < sa.n_spec)) {
        // emcee / MH accept (half 1's slots of a speculative iteration only deliver their logl:
        // rvm_stretch_iteration_end)
        const bool acc = mh ? mh_accepts(lp, lnp0, u3) : stretch_accepts(sa.dim, z, lp, lnp0, u3);
        if (acc) {
#pragma unroll
            for (int r = 0; r < R; r++) {
                if (sa.src[r] >= 0) {
                    const double v = row(r);
                    sa.x[(size_t)sa.src[r] * sa.xstride + wo] = v;
                    if (sa.x_aos) sa.x_aos[(size_t)wo * sa.dim + sa.src[r]] = v;
                }
            }
            sa.lnp[wo] = lp;
            if (sa.accepted) sa.accepted[wo] += 1;
        }
        if (sa.dec) sa.dec[wo] = acc ? 1 : 0;
    }
}

}  // namespace rvm
