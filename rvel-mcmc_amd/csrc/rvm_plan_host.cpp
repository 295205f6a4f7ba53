// rvm_plan_host.cpp -- the host arithmetic of plan creation (rvm_plan_host.h).  No HIP call here.
#include "rvm_plan_host.h"

#include <algorithm>
#include <cmath>
#include <cstdlib>

// the eager first halving pass for small plain launches (rvm_refine.hip), unless RVM_EAGER says otherwise
#ifndef RVM_EAGER_DEFAULT
#define RVM_EAGER_DEFAULT true
#endif
// eager halving passes run beside the likelihood kernel: pass 1 only (pass 2 as well, RVM_EAGER_PASSES=2,
// measured slower: config 4 at 0.90 -> 1.07 ms per step -- the side stream's next launch queues behind
// the longer eager kernel)
#ifndef RVM_EAGER_PASSES_DEFAULT
#define RVM_EAGER_PASSES_DEFAULT 1
#endif

namespace rvm {

static bool starts(const char* s, char c) { return s && s[0] == c; }

PlanKnobs read_plan_knobs() {
    PlanKnobs K;
    K.skip_variants = starts(getenv("RVM_SKIP_VARIANTS"), '0') ? 0 : 1;
    const char* ls = getenv("RVM_LATE_SPO");
    K.late_spo = ls ? atof(ls) : 96.0;
    K.no_level_split = false;
#ifdef RVM_PROFILE
    K.no_level_split = starts(getenv("RVM_NO_LEVEL_SPLIT"), '1');
#endif
    K.n_teams = RVM_TEAMS_DEFAULT;
    if (const char* tp = getenv("RVM_REFINE_TEAMS")) K.n_teams = std::max(1, std::min(atoi(tp), RVM_TEAMS_MAX));
    K.eager_split = starts(getenv("RVM_EAGER_SPLIT"), '0') ? 0 : 1;
    K.no_extension = starts(getenv("RVM_NO_EXTENSION"), '1');
    K.refine_split = !starts(getenv("RVM_REFINE_SPLIT"), '0');
    K.teams_hint = !starts(getenv("RVM_TEAMS_HINT"), '0');
    const char* eg = getenv("RVM_EAGER");
    K.eager = eg ? eg[0] == '1' : RVM_EAGER_DEFAULT;
    const char* ep = getenv("RVM_EAGER_PASSES");
    K.eager_passes = starts(ep, '1') ? 1 : (starts(ep, '2') ? 2 : RVM_EAGER_PASSES_DEFAULT);
    K.hedge_groups = starts(getenv("RVM_HEDGE"), '0') ? 0 : RVM_HEDGE_GROUPS_MAX;
    if (const char* hn = getenv("RVM_HEDGE_GROUPS"))
        K.hedge_groups = std::min(K.hedge_groups, std::max(0, std::min(atoi(hn), (int)RVM_HEDGE_GROUPS_MAX)));
    K.hedge_mark = starts(getenv("RVM_HEDGE_MARK"), '0') ? 0 : 1;
    const char* hwt = getenv("RVM_HEDGE_WAIT");
    K.hedge_wait = starts(hwt, '0') ? 0 : (starts(hwt, '2') ? 2 : 1);
    return K;
}

const char* check_plan_config(const rvm_config* cfg, const double* t, const double* rv, const double* sigma,
                              int32_t n_obs, int32_t max_walkers, int mult[RVM_MAX_LEVELS], int* max_mult) {
    if (cfg->n_planets < 1 || cfg->n_planets > RVM_MAX_PLANETS) return "rvm_plan_create: n_planets out of range";
    if (cfg->n_levels < 1 || cfg->n_levels > RVM_MAX_LEVELS) return "rvm_plan_create: n_levels out of range";
    if (!(cfg->dt > 0.0) || !std::isfinite(cfg->dt)) return "rvm_plan_create: dt must be > 0";
    if (n_obs < 0 || max_walkers < 1) return "rvm_plan_create: bad sizes";
    if (!(cfg->npoints_norm != 0.0)) return "rvm_plan_create: npoints_norm must be nonzero";
    bool harmonic = true;
    for (int k = 0; k < cfg->n_levels; k++) harmonic = harmonic && cfg->level_mult[k] == 0;
    *max_mult = 1;
    for (int k = 0; k < cfg->n_levels; k++) {
        mult[k] = harmonic ? k + 1 : cfg->level_mult[k];
        if (mult[k] < 1 || mult[k] > 64) return "rvm_plan_create: level_mult out of range (1..64)";
        for (int j = 0; j < k; j++)
            if (mult[j] == mult[k]) return "rvm_plan_create: level_mult entries must be distinct";
        *max_mult = std::max(*max_mult, mult[k]);
    }
    if (!(cfg->period_hint >= 0.0) || !std::isfinite(cfg->period_hint))
        return "rvm_plan_create: period_hint must be >= 0";
    if (std::isnan(cfg->resolve_tol) || cfg->resolve_max < 0 || cfg->resolve_max > RVM_RESOLVE_MAX_LIMIT)
        return "rvm_plan_create: resolve_tol must be a number and resolve_max in 0..12";
    for (int i = 0; i < n_obs; i++)
        if (!std::isfinite(t[i]) || !std::isfinite(rv[i]) || !std::isfinite(sigma[i]))
            return "rvm_plan_create: non-finite observation";
    return nullptr;
}

// The epoch count nearest the share `frac` of the direction's steps (0: split at 0), and the steps before it
static void split_point(const HostDir& D, double frac, int32_t* split, int32_t* pre) {
    const double target = frac * (double)D.total_steps;
    long long cum = 0, best_cum = 0;
    int best = 0;
    double best_d = target;
    for (size_t i = 0; i < D.seg_n.size(); i++) {
        cum += D.seg_n[i];
        const double dist = std::fabs((double)cum - target);
        if (dist < best_d) {
            best_d = dist;
            best = (int)i + 1;
            best_cum = cum;
        }
    }
    *split = best;
    *pre = (int32_t)best_cum;
}

const char* build_schedule(const rvm_config* cfg, const int* mult, int max_mult, const double* t, const double* rv,
                           const double* sigma, int32_t n_obs, HostDir dir[2]) {
    const int rmax = cfg->resolve_tol > 0.0 ? cfg->resolve_max : 0;
    // head / tail split points (rvm_logl.hip level-split roles): level 0 at the share f0 of the
    // steps that balances SIMD loads m2 + f0 m0 = m3 + (1 - f0) m0, level 1 at one half
    double f0 = 0.5;
    // (+0.11: the tail's SIMD runs level 3 alone until the head ends, at the lone-wave rate;
    // measured at 6144 slots, scripts/probe/prof_clock.py with RVM_LS_F0: 0.625 -> SIMD 0/1
    // end 6 % after SIMD 2/3, 0.74 -> within 1 %)
    if (cfg->n_levels == 4) f0 = (double)(mult[3] + mult[0] - mult[2]) / (2.0 * mult[0]) + 0.11;
#ifdef RVM_PROFILE
    if (const char* ef = getenv("RVM_LS_F0")) f0 = atof(ef);  // (timing build only: scripts/probe)
#endif
    f0 = std::min(1.0, std::max(0.0, f0));
    for (int dd = 0; dd < 2; dd++) {
        HostDir& D = dir[dd];
        for (int i = 0; i < n_obs; i++)
            if ((dd == 0) == (t[i] >= 0.0)) D.idx.push_back(i);
        std::stable_sort(D.idx.begin(), D.idx.end(), [&](int a, int b) { return std::fabs(t[a]) < std::fabs(t[b]); });
        const double sign = dd == 0 ? 1.0 : -1.0;
        double tprev = 0.0;
        for (int i : D.idx) {
            const double at = std::fabs(t[i]);
            const double len = at - tprev;
            tprev = at;
            int n = len > 0.0 ? (int)std::ceil(len / cfg->dt - 1e-9) : 0;
            if (len > 0.0 && n < 1) n = 1;
            D.seg_n.push_back(n);
            D.seg_len.push_back(n > 0 ? sign * len / n : 0.0);
            D.orv.push_back(rv[i]);
            D.os2.push_back(sigma[i] * sigma[i]);
            D.total_steps += n;
        }
        if ((D.total_steps * (long long)max_mult) << rmax > (1LL << 30))
            return "rvm_plan_create: dt too small for the epoch span";
        if (D.idx.size() > (size_t)RVM_MAX_EPOCHS_PER_DIRECTION)
            return "rvm_plan_create: too many epochs in one direction (the schedule is staged in LDS)";
        split_point(D, f0, &D.split0, &D.pre0);
        split_point(D, 0.5, &D.split1, &D.pre1);
    }
    return nullptr;
}

void lagrange_at_zero(const int* m, int k0, int n, double* w) {
    for (int k = k0; k < n; k++) {
        const double xk = 1.0 / ((double)m[k] * m[k]);
        double wk = 1.0;
        for (int j = k0; j < n; j++) {
            if (j == k) continue;
            const double xj = 1.0 / ((double)m[j] * m[j]);
            wk *= xj / (xj - xk);
        }
        w[k] = wk;
    }
}

void fill_plan_scalars(const rvm_config* cfg, const int* mult, int32_t n_obs, size_t nf, size_t nb, int n_cu,
                       const PlanKnobs& K, DevPlan* Pp) {
    DevPlan& P = *Pp;
    const int nl = cfg->n_levels;
    P.n_planets = cfg->n_planets;
    P.n_levels = nl;
    P.npoints = cfg->npoints_norm;
    P.n_obs = n_obs;
    P.inclined = cfg->inclined ? 1 : 0;
    P.n_cu = n_cu;
    for (int k = 0; k < RVM_MAX_LEVELS; k++) {
        P.mult[k] = k < nl ? mult[k] : 1;
        P.inv_mult[k] = 1.0 / P.mult[k];
        P.lw[k] = P.lw3[k] = 0.0;
        // Stumpff series length (rvm_device.h stumpff_bound): nominal z = (2 pi h / P)^2 on a
        // circular orbit, x2 for the pericentre of e ~ 0.25 orbits; lanes beyond the bound take
        // the general evaluation, so this choice only affects speed.  Levels whose nominal z is
        // small enough that the first Halley step is accepted almost always (fine levels) run
        // their segments speculatively (rvm_logl.hip segment<>)
        P.nt[k] = 8;
        P.spec[k] = 0;
        if (k < nl && cfg->period_hint > 0.0) {
            const double nh = 2.0 * M_PI * cfg->dt / (mult[k] * cfg->period_hint);
            const double zn = 2.0 * nh * nh;
            P.nt[k] = zn <= 0.1 ? 6 : (zn <= 0.3 ? 7 : 8);
            P.spec[k] = zn <= 0.04 ? 1 : 0;
        }
    }
    // Richardson weights for the h^2 expansion: level k steps dt/mult[k]; Lagrange at 0 in x = 1/mult^2.
    // Adaptive resolution: lw3, the weights of levels 1 .. n-1 alone (the estimate drops the coarsest)
    lagrange_at_zero(mult, 0, nl, P.lw);
    lagrange_at_zero(mult, 1, nl, P.lw3);
    P.rtol_dir = cfg->resolve_tol > 0.0 && nl >= 2 ? 0.5 * cfg->resolve_tol : INFINITY;
    P.fin_level = 0;
    for (int k = 1; k < nl; k++)
        if (mult[k] > mult[P.fin_level]) P.fin_level = k;
    P.rmax = P.rtol_dir < INFINITY ? cfg->resolve_max : 0;
    P.cut = 1;
    P.spin_ticks = 200000000ull;  // 2 s of the 100 MHz real-time counter without progress
    P.hedge_wait_ticks = hedge_wait_bound(P.spin_ticks);
    // the LDS-coupled layouts' ring (DevPlan::lc_ring): up to RVM_LC_RING epochs, within
    // RVM_LC_RING_BYTES per group, at least 2 (a level runs at most a ring ahead of its combiner)
    const int emax = (int)std::max<size_t>(std::max(nf, nb), 1);
    const int fit = (int)(RVM_LC_RING_BYTES / ((size_t)(nl + 1) * walkers_per_group(cfg->n_planets) * sizeof(double)));
    P.lc_ring = std::max(2, std::min(std::min(RVM_LC_RING, emax), fit));
    P.skip_variants = K.skip_variants;
    // the halving passes' late vote (DevPlan::late_mult): levels of at least RVM_LATE_SPO steps per period_hint
    P.late_mult = 0;
    if (K.late_spo > 0.0 && cfg->period_hint > 0.0)
        P.late_mult = std::max(1, (int32_t)std::ceil(K.late_spo * cfg->dt / cfg->period_hint - 1e-9));
    // (adaptive plans run at least two teams' worth of exchange words: rq_layout)
    P.n_teams = P.rmax > 0 ? std::max(K.n_teams, 2) : K.n_teams;
    P.eager_split = K.eager_split;
    P.e2_guard = P.e2_cut = INFINITY;
    P.cut_guard_k = 0.0;
    P.ext_mult = 0;
    P.ext_nt = 8;
    P.ext_spec = 0;
    P.inv_ext = 1.0;
    for (int k = 0; k <= RVM_MAX_LEVELS; k++) P.lw5[k] = 0.0;
}

uint32_t hedge_wait_bound(unsigned long long spin_ticks) {
    const unsigned long long q = spin_ticks >> 2;  // (a 32-bit field: 42 s at the most)
    return q < 0xFFFFFFFFull ? (uint32_t)q : 0xFFFFFFFFu;
}

bool plan_wants_extension(const DevPlan& P, const PlanKnobs& K) {
    return P.rmax > 0 && P.n_levels >= 2 && P.n_levels < RVM_MAX_LEVELS && !K.no_extension;
}

// the extension level (rvm_logl.hip extend_pass): max(mult) + 1 steps per base step, its Stumpff
// series as the finest level's (a finer step than the finest level's: speculate where it does)
void fill_plan_extension(DevPlan* Pp) {
    DevPlan& P = *Pp;
    const int nl = P.n_levels, fin = P.fin_level;
    int m5[RVM_MAX_LEVELS + 1];
    for (int k = 0; k < nl; k++) m5[k] = P.mult[k];
    m5[nl] = P.mult[fin] + 1;
    lagrange_at_zero(m5, 0, nl + 1, P.lw5);
    P.ext_mult = m5[nl];
    P.ext_nt = P.nt[fin];
    P.ext_spec = P.spec[fin];
    P.inv_ext = 1.0 / m5[nl];
    // and as plan level slot nl (lw[nl] = 0): the concurrent extension wave of the
    // LDS-coupled layout integrates it like any level (rvm_logl.hip, cx)
    P.mult[nl] = P.ext_mult;
    P.nt[nl] = P.ext_nt;
    P.spec[nl] = P.ext_spec;
    P.inv_mult[nl] = P.inv_ext;
}

bool plan_wants_level_split(const DevPlan& P, int32_t max_walkers, const PlanKnobs& K) {
    const int wpb = walkers_per_group(P.n_planets);
    const int64_t groups = ((int64_t)max_walkers + wpb - 1) / wpb;
    bool inc = P.n_levels == 4 && !K.no_level_split;
    for (int k = 1; inc && k < 4; k++) inc = P.mult[k] > P.mult[k - 1];
    return inc && P.n_cu > 0 && 2 * groups > P.n_cu;
}

LoglLayout choose_logl_layout(const DevPlan& P, int W, bool want_rv, bool fused, bool cx_pairs, size_t budget_lc,
                              size_t budget_ls) {
    const int wpb = walkers_per_group(P.n_planets);
    const int groups = (W + wpb - 1) / wpb;
    const int nl = P.n_levels, n_cu = P.n_cu;
    const int emax = std::max(P.fwd.n_epochs, P.bwd.n_epochs);
    const bool init = P.rmax > 0;
    // the extension level can run beside the main pass: the plan has one, and no model RVs are asked for
    const bool xcon = P.ext_mult > 0 && !want_rv;
    const bool crowded = n_cu > 0 && 2 * groups > n_cu;  // one group per block would not fit one block per CU
    // One walker group per block while the blocks fit one per CU (every wave alone on its SIMD: latency-bound);
    // beyond that two groups with mirrored level order per block, which pairs the heaviest level with the
    // lightest on each SIMD.  Paired one-group blocks (3 planets, planar): where two groups would share a block,
    // a launch of at most one group per CU instead runs one group per block with the extension as its fifth wave
    // (cx), two such blocks per CU (that instantiation is held to 168 VGPRs for it) -- the extension beside the
    // main pass instead of after it, for 4096-walker half-steps.  (A/B knob RVM_CX_PAIRS=0: cx_pairs false)
    const bool pairs = P.n_planets == 3 && !P.inclined && cx_pairs && xcon && crowded && groups <= n_cu &&
                       W >= RVM_CX_MIN_WALKERS;
    LoglLayout Y{};
    Y.G = !pairs && crowded && 2 * nl * 64 <= 512 ? 2 : 1;
    // One group per block: the extension level as an extra wave (cx).  The fifth wave shares SIMD 0 with level 0
    // (4 + 8 steps per base step against level 3's 7 alone), which costs every launch ~60 % (a one-walker launch
    // 0.335 -> 0.538 ms with nothing flagged, scripts/probe/config1_probe.py): worth it only where a launch almost
    // surely holds a flagged walker.  Launches of a few walkers run the extension after the main pass, only when
    // flagged -- the same bits either way.
    Y.cx = Y.G == 1 && xcon && W >= RVM_CX_MIN_WALKERS ? 1 : 0;
    Y.tB = 8;
    Y.grid_x = (unsigned)((groups + Y.G - 1) / Y.G);
    Y.grid_y = 2;
    Y.block = (unsigned)(64 * (nl + Y.cx) * Y.G);
    Y.lds = LoglLds::coupled(emax, wpb, Y.G, (P.inclined ? 7 : 5) * P.n_planets, fused, init, P.lc_ring, nl);
    // Level-split layout (logl_kernel): one round of na type-A and nb type-B blocks, one per CU
    const bool can_split = P.lv_rv != nullptr && W <= P.lv_stride && nl == 4 && n_cu > 0;
    const int units = 2 * groups, na = groups;
    auto split = [&](int tB, int nb, const LoglLds& lds) {
        Y.nA = na;
        Y.nB = nb;
        Y.tB = tB;
        Y.grid_x = (unsigned)(na + nb);
        Y.grid_y = 1;
        Y.block = 8 * 64;
        Y.lds = lds;
    };
    // ... with the extension level: where two groups would share a block (no room for the concurrent extension
    // wave), it carries the extension as a fifth level of the main pass (lsx) -- the ring holds whole directions
    if (can_split && xcon && Y.G == 2 && emax <= RVM_LS_RING) {
        const int nb = (units + 7) / 8;
        const LoglLds lds = LoglLds::level_split(emax, wpb, 4, init);
        if (na + nb <= n_cu && lds.bytes() <= budget_ls) {
            split(8, nb, lds);
            Y.lsx = 1;
        }
    }
    // ... else when it lowers the heaviest SIMD's load: in steps per base step, max(m3, m2 + m0, 2 m1) for one
    // round of <= n_cu blocks, against m3 per round of one-group or max_i(m_i + m_{n-1-i}) of two-group blocks
    if (Y.nA == 0 && can_split) {
        const int32_t* m = P.mult;
        // type-B blocks carry 6 units' level 1 (two of them split head / tail) when the CUs allow, else 8
        const int tB = na + (units + 5) / 6 <= n_cu ? 6 : 8;
        const int nb = (units + tB - 1) / tB;
        const int c_dec = std::max(m[3], std::max(m[2] + m[0], 2 * m[1]));
        const int c_cpl = Y.G == 1 ? m[3] * ((2 * groups + n_cu - 1) / n_cu)
                                   : std::max(m[0] + m[3], m[1] + m[2]) * ((groups + n_cu - 1) / n_cu);
        const LoglLds lds = LoglLds::level_split(emax, wpb, 3, init);
        if (na + nb <= n_cu && c_dec < c_cpl && lds.bytes() <= budget_ls) {
            split(tB, nb, lds);
            // (level 0 split head / tail: the combiner starts with the head's hand-off)
            Y.splitA = emax <= RVM_LS_RING ? 1 : 0;
        }
    }
    Y.smem = Y.lds.bytes();
    Y.fits = Y.nA > 0 || Y.smem <= budget_lc;
    return Y;
}

// the next sub-range of a block: its offset, the block's running size `end` moved past it
static size_t take(size_t& end, size_t bytes) {
    end += bytes;
    return end - bytes;
}
static size_t epochs_max(size_t nf, size_t nb) { return std::max<size_t>(std::max(nf, nb), 1); }

DmemLayout dmem_layout(size_t nf, size_t nb, int32_t max_walkers) {
    DmemLayout L{};
    const size_t n[2] = {nf, nb};
    for (int d = 0; d < 2; d++) {
        L.seg_h1[d] = take(L.bytes, n[d] * sizeof(double));
        L.obs_rv[d] = take(L.bytes, n[d] * sizeof(double));
        L.obs_s2[d] = take(L.bytes, n[d] * sizeof(double));
    }
    L.slots = take(L.bytes, (size_t)max_walkers * sizeof(unsigned long long));
    L.counters = take(L.bytes, RVM_N_COUNTERS * sizeof(unsigned long long));
    for (int d = 0; d < 2; d++) {
        L.seg_n[d] = take(L.bytes, n[d] * sizeof(int32_t));
        L.obs_idx[d] = take(L.bytes, n[d] * sizeof(int32_t));
    }
    L.bytes += 64;
    return L;
}

LvLayout lv_layout(size_t nf, size_t nb, int32_t max_walkers) {
    LvLayout L{};
    L.emax = (int32_t)epochs_max(nf, nb);
    L.rv = take(L.bytes, (size_t)(2 * (int64_t)L.emax * max_walkers) * sizeof(double));
    L.enc = take(L.bytes, (size_t)(2 * (int64_t)max_walkers) * sizeof(int32_t));
    return L;
}

XLayout x_layout(size_t nf, size_t nb, int32_t max_walkers, int n_teams) {
    XLayout L{};
    L.emax = (int32_t)epochs_max(nf, nb);
    const size_t bl = 2 * (size_t)L.emax * (size_t)max_walkers * sizeof(double);  // partial sums
    L.lvx = take(L.bytes, bl);
    L.rvp = take(L.bytes, bl);  // + last RV (per team)
    L.rvp2 = take(L.bytes, ((size_t)n_teams - 1) * bl);
    return L;
}

// (+ the split exchange: flags and double-buffered values per both-direction group of up to 64
// walkers and team; groups of 16 walkers at 3-4 planets; + team A's published state and flag)
RqLayout rq_layout(int32_t max_walkers, int n_teams) {
    RqLayout L{};
    const size_t xg = (size_t)(((int64_t)max_walkers + 15) / 16 + 1), nt = (size_t)std::max(n_teams, 2);
    const size_t u64 = sizeof(unsigned long long);
    L.xgroups = (int32_t)xg;
    L.x = take(L.bytes, xg * nt * 2 * 2 * 64 * u64);
    L.xf = take(L.bytes, xg * nt * 2 * u64);
    L.t = take(L.bytes, xg * (nt - 1) * 16 * 64 * u64);
    L.tf = take(L.bytes, xg * nt * u64);  // (+ the group's done word)
    L.tb = take(L.bytes, xg * u64);       // (right behind rq_tf: team B has arrived, team A's wait gives way)
    L.c = take(L.bytes, 2 * (size_t)max_walkers * sizeof(double));
    // (rounded up to 8 bytes: an odd max_walkers left the 64-bit words after it, gen_dev and depth_w, 4 off)
    L.w = take(L.bytes, (3 * (size_t)max_walkers * sizeof(int32_t) + 7) & ~(size_t)7);
    L.n = take(L.bytes, 64);  // rq_n [4], the launch generation at + 32
    L.gen = L.n + 32;
    L.mark = take(L.bytes, ((size_t)max_walkers * sizeof(int32_t) + 63) & ~(size_t)63);
    L.depth = take(L.bytes, (RVM_DEPTH_WINDOW + 1) * u64);
    return L;
}

HLayout h_layout(int32_t lvx_emax, int32_t max_walkers) {
    HLayout L{};
    const size_t hs = RVM_HEDGE_STRIDE, w = sizeof(double);
    L.hrv = take(L.bytes, 2 * (size_t)lvx_emax * hs * w);
    L.hsum = take(L.bytes, 6 * hs * w);
    L.hslot = take(L.bytes, 2 * hs * w);
    L.htab = take(L.bytes, (size_t)max_walkers * w);
    L.hw = take(L.bytes, RVM_HW_WORDS * w);
    return L;
}

ELayout e_layout(int32_t lvx_emax, int32_t lvx_stride) {
    ELayout L{};
    const size_t plane = (size_t)lvx_emax * lvx_stride;
    L.rve = take(L.bytes, 4 * plane * sizeof(double));
    L.esum = take(L.bytes, 12 * (size_t)lvx_stride * sizeof(double));
    L.eflag = take(L.bytes, (RVM_EFLAG_WORDS * (size_t)((RVM_EAGER_MAX + 15) / 16) + 8) * sizeof(double));
    return L;
}

}  // namespace rvm
