// Host-side sanitizer driver for librvmcmc's C ABI (not part of the library): every entry point's
// argument checks, and rvm_plan_create's host work on valid inputs -- through the ABI up to the first
// HIP call, which fails on a GPU-less host (an error return), and past it by calling the host
// arithmetic of rvm_plan_host.h directly: schedule, weights, scalar fields, knobs, block layouts.
// Built with AddressSanitizer + UBSan on the host side only (`make sanitize-host`), run by
// tests/test_sanitizers.py.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "rvm_plan_host.h"

static int fails = 0;
static void expect(bool ok, const char* what) {
    if (!ok) {
        std::fprintf(stderr, "FAIL %s\n", what);
        fails++;
    }
}

// w_k = prod_{j != k} m_k^2 / (m_k^2 - m_j^2) over levels k0 .. n-1, numerator and denominator exact integers
static double exact_weight(const int* m, int k0, int n, int k) {
    long long num = 1, den = 1;
    for (int j = k0; j < n; j++) {
        if (j == k) continue;
        num *= (long long)m[k] * m[k];
        den *= (long long)m[k] * m[k] - (long long)m[j] * m[j];
    }
    return (double)num / (double)den;
}

static bool close_rel(double a, double b, double rel) { return std::fabs(a - b) <= rel * std::fabs(b); }

static double ulp_of(double x) { return std::nextafter(std::fabs(x), INFINITY) - std::fabs(x); }

struct Range {
    size_t off, bytes;
    bool wide;  // holds double / unsigned long long
};
// a block's sub-ranges: in order, disjoint, inside the block, the 8-byte ones aligned
static void check_block(const std::vector<Range>& r, size_t block_bytes, const char* what) {
    size_t end = 0;
    for (const Range& x : r) {
        expect(x.off >= end, what);
        expect(!x.wide || x.off % 8 == 0, what);
        end = x.off + x.bytes;
    }
    expect(end <= block_bytes, what);
}

static const char* const kKnobNames[] = {
    "RVM_SKIP_VARIANTS", "RVM_LATE_SPO",   "RVM_NO_LEVEL_SPLIT", "RVM_REFINE_TEAMS", "RVM_EAGER_SPLIT",
    "RVM_NO_EXTENSION",  "RVM_REFINE_SPLIT", "RVM_TEAMS_HINT",   "RVM_EAGER",        "RVM_EAGER_PASSES",
    "RVM_HEDGE",         "RVM_HEDGE_GROUPS", "RVM_HEDGE_MARK",   "RVM_HEDGE_WAIT",
    "RVM_LS_F0"};

static rvm::PlanKnobs knobs_with(const char* name, const char* value) {
    setenv(name, value, 1);
    const rvm::PlanKnobs K = rvm::read_plan_knobs();
    unsetenv(name);
    return K;
}

// the host half of plan creation on the driver's config, past the point the ABI call reaches without a GPU
static void check_plan_host(const rvm_config& cfg, const std::vector<double>& t, const std::vector<double>& rv,
                            const std::vector<double>& sg) {
    using namespace rvm;
    const int n_obs = (int)t.size();
    for (const char* name : kKnobNames) unsetenv(name);
    const PlanKnobs K = read_plan_knobs();
    expect(K.skip_variants == 1 && K.late_spo == 96.0 && !K.no_level_split && K.n_teams == RVM_TEAMS_DEFAULT &&
               K.eager_split == 1 && !K.no_extension && K.refine_split && K.teams_hint && K.eager &&
               K.eager_passes == 1 && K.hedge_groups == RVM_HEDGE_GROUPS_MAX && K.hedge_mark == 1 &&
               K.hedge_wait == 1,
           "knob defaults");
    expect(knobs_with("RVM_REFINE_TEAMS", "9").n_teams == RVM_TEAMS_MAX, "RVM_REFINE_TEAMS=9 clamps");
    expect(knobs_with("RVM_HEDGE", "0").hedge_groups == 0, "RVM_HEDGE=0");
    expect(knobs_with("RVM_HEDGE_GROUPS", "3").hedge_groups == 3, "RVM_HEDGE_GROUPS=3");
    expect(knobs_with("RVM_EAGER_PASSES", "2").eager_passes == 2, "RVM_EAGER_PASSES=2");
    expect(knobs_with("RVM_SKIP_VARIANTS", "0").skip_variants == 0, "RVM_SKIP_VARIANTS=0");
    expect(knobs_with("RVM_HEDGE_WAIT", "0").hedge_wait == 0 && knobs_with("RVM_HEDGE_WAIT", "1").hedge_wait == 1 &&
               knobs_with("RVM_HEDGE_WAIT", "2").hedge_wait == 2 && knobs_with("RVM_HEDGE_WAIT", "x").hedge_wait == 1,
           "RVM_HEDGE_WAIT");

    int mult[RVM_MAX_LEVELS] = {}, max_mult = 0;
    expect(check_plan_config(&cfg, t.data(), rv.data(), sg.data(), n_obs, 4096, mult, &max_mult) == nullptr,
           "config ok");
    expect(mult[0] == 4 && mult[1] == 5 && mult[2] == 6 && mult[3] == 7 && max_mult == 7, "explicit ladder");
    {
        rvm_config h = cfg;
        h.n_levels = 3;
        std::memset(h.level_mult, 0, sizeof(h.level_mult));
        int hm[RVM_MAX_LEVELS] = {}, hmax = 0;
        expect(check_plan_config(&h, t.data(), rv.data(), sg.data(), n_obs, 64, hm, &hmax) == nullptr && hm[0] == 1 &&
                   hm[1] == 2 && hm[2] == 3 && hmax == 3,
               "harmonic ladder");
    }

    // schedule
    HostDir dir[2];
    expect(build_schedule(&cfg, mult, max_mult, t.data(), rv.data(), sg.data(), n_obs, dir) == nullptr, "schedule ok");
    std::vector<int> seen(n_obs, 0);
    int n_dup = 0;
    for (int d = 0; d < 2; d++) {
        const HostDir& D = dir[d];
        const size_t n = D.idx.size();
        expect(D.seg_n.size() == n && D.seg_len.size() == n && D.orv.size() == n && D.os2.size() == n,
               "schedule sizes");
        long long sum = 0, pre0 = 0, pre1 = 0;
        double tprev = 0.0;
        for (size_t i = 0; i < n; i++) {
            const int o = D.idx[i];
            expect(o >= 0 && o < n_obs && (d == 0) == (t[o] >= 0.0), "obs_idx direction");
            if (o >= 0 && o < n_obs) seen[o]++;
            const double at = std::fabs(t[o]), len = (d == 0 ? 1.0 : -1.0) * (at - tprev);
            expect(at >= tprev, "|t| non-decreasing");
            if (at == tprev) {
                n_dup += i > 0;
                expect(D.seg_n[i] == 0 && D.seg_len[i] == 0.0, "duplicate epoch: empty segment");
            } else {
                expect(D.seg_n[i] >= 1 && std::fabs(D.seg_len[i]) <= cfg.dt * (1.0 + 1e-9), "segment step <= dt");
                expect(std::fabs(D.seg_n[i] * D.seg_len[i] - len) <= 4.0 * ulp_of(len), "segment steps x step = length");
            }
            tprev = at;
            if ((int)i < D.split0) pre0 += D.seg_n[i];
            if ((int)i < D.split1) pre1 += D.seg_n[i];
            sum += D.seg_n[i];
        }
        expect(sum == D.total_steps, "sum(seg_n) = n_steps");
        expect(D.split0 >= 0 && D.split0 <= (int)n && D.split1 >= 0 && D.split1 <= (int)n, "split range");
        expect(pre0 == D.pre0 && pre1 == D.pre1, "pre = steps before the split");
    }
    expect(std::all_of(seen.begin(), seen.end(), [](int c) { return c == 1; }), "obs_idx is a permutation");
    expect(n_dup == 1, "one duplicate epoch");

    // weights against the exact rational form
    const size_t nf = dir[0].idx.size(), nb = dir[1].idx.size();
    rvm_config ad = cfg;
    ad.resolve_tol = 5e-7;
    ad.resolve_max = 6;
    DevPlan P{};
    fill_plan_scalars(&ad, mult, n_obs, nf, nb, 256, K, &P);
    expect(P.ext_mult == 0 && plan_wants_extension(P, K), "extension wanted, not yet applied");
    fill_plan_extension(&P);
    const int m5[5] = {4, 5, 6, 7, 8};
    for (int k = 0; k < 4; k++) expect(close_rel(P.lw[k], exact_weight(m5, 0, 4, k), 1e-14), "lw");
    for (int k = 1; k < 4; k++) expect(close_rel(P.lw3[k], exact_weight(m5, 1, 4, k), 1e-14), "lw3");
    for (int k = 0; k < 5; k++) expect(close_rel(P.lw5[k], exact_weight(m5, 0, 5, k), 1e-14), "lw5");
    expect(P.lw3[0] == 0.0 && P.lw[4] == 0.0 && P.lw[5] == 0.0 && P.lw5[5] == 0.0, "unused weights are zero");

    // scalars, each from its rule
    expect(P.fin_level == 3, "fin_level");
    expect(P.ext_mult == 8 && P.mult[4] == 8 && P.inv_ext == 0.125 && P.inv_mult[4] == 0.125, "ext_mult");
    expect(P.rmax == 6 && P.rtol_dir == 2.5e-7 && P.cut == 1 && P.n_teams == RVM_TEAMS_DEFAULT, "adaptive scalars");
    // team A's wait for a hedge block ends strictly before team B's wait for team A could
    expect(P.hedge_wait_ticks == hedge_wait_bound(P.spin_ticks) && P.hedge_wait_ticks < (P.spin_ticks << 1),
           "hedge_wait_ticks");
    for (unsigned long long sp : {1ull, 2ull, 3ull, 4ull, 1000ull, 200000000ull, 1ull << 40, 1ull << 62})
        expect(hedge_wait_bound(sp) < sp && hedge_wait_bound(sp) < (sp << 1), "hedge_wait_bound");
    for (int k = 0; k < 4; k++) {
        const double nh = 2.0 * M_PI * cfg.dt / (mult[k] * cfg.period_hint), zn = 2.0 * nh * nh;
        expect(P.nt[k] == (zn <= 0.1 ? 6 : (zn <= 0.3 ? 7 : 8)) && P.spec[k] == (zn <= 0.04 ? 1 : 0), "nt / spec");
        expect(P.inv_mult[k] == 1.0 / mult[k], "inv_mult");
    }
    expect(P.ext_nt == P.nt[3] && P.ext_spec == P.spec[3] && P.nt[4] == P.nt[3] && P.spec[4] == P.spec[3],
           "ext nt / spec");
    expect(P.late_mult == (int)std::ceil(96 * 0.65 / 5.2 - 1e-9) && P.late_mult == 12, "late_mult");
    expect(P.lc_ring >= 2 && P.lc_ring <= RVM_LC_RING, "lc_ring range");
    expect((size_t)(cfg.n_levels + 1) * 32 * 8 * P.lc_ring <= RVM_LC_RING_BYTES, "lc_ring bytes");
    {
        DevPlan Q{};  // the driver's own config: resolve_tol 0, no refinement, no extension
        fill_plan_scalars(&cfg, mult, n_obs, nf, nb, 256, K, &Q);
        expect(Q.rmax == 0 && !plan_wants_extension(Q, K) && Q.ext_mult == 0, "no extension without resolve_tol");
        ad.resolve_max = 0;
        fill_plan_scalars(&ad, mult, n_obs, nf, nb, 256, K, &Q);
        expect(!plan_wants_extension(Q, K) && Q.ext_mult == 0, "no extension with resolve_max 0");
        expect(!plan_wants_extension(P, knobs_with("RVM_NO_EXTENSION", "1")), "RVM_NO_EXTENSION=1");
        fill_plan_scalars(&cfg, mult, n_obs, nf, nb, 256, knobs_with("RVM_LATE_SPO", "0"), &Q);
        expect(Q.late_mult == 0, "RVM_LATE_SPO=0");
    }

    // layouts
    for (int32_t mw : {1, 64, 6144}) {
        const size_t w = (size_t)mw, em = std::max(nf, nb);
        const DmemLayout D = dmem_layout(nf, nb, mw);
        check_block({{D.seg_h1[0], 8 * nf, true}, {D.obs_rv[0], 8 * nf, true}, {D.obs_s2[0], 8 * nf, true},
                     {D.seg_h1[1], 8 * nb, true}, {D.obs_rv[1], 8 * nb, true}, {D.obs_s2[1], 8 * nb, true},
                     {D.slots, 8 * w, true}, {D.counters, 8 * RVM_N_COUNTERS, true}, {D.seg_n[0], 4 * nf, false},
                     {D.obs_idx[0], 4 * nf, false}, {D.seg_n[1], 4 * nb, false}, {D.obs_idx[1], 4 * nb, false}},
                    D.bytes, "dmem layout");
        const LvLayout V = lv_layout(nf, nb, mw);
        expect(V.emax == (int32_t)em, "lv emax");
        check_block({{V.rv, 8 * 2 * em * w, true}, {V.enc, 4 * 2 * w, false}}, V.bytes, "lvmem layout");
        for (int teams : {1, 2, 4}) {
            const size_t nt = (size_t)std::max(teams, 2), xg = (w + 15) / 16 + 1;
            const XLayout X = x_layout(nf, nb, mw, teams);
            check_block({{X.lvx, 16 * em * w, true}, {X.rvp, 16 * em * w, true},
                         {X.rvp2, 16 * em * w * (teams - 1), true}},
                        X.bytes, "xmem layout");
            const RqLayout R = rq_layout(mw, teams);
            expect(R.xgroups == (int32_t)xg, "rq xgroups");
            check_block({{R.x, xg * nt * 256 * 8, true}, {R.xf, xg * nt * 2 * 8, true},
                         {R.t, xg * (nt - 1) * 1024 * 8, true}, {R.tf, xg * nt * 8, true}, {R.tb, xg * 8, true},
                         {R.c, 16 * w, true},
                         {R.w, 12 * w, false}, {R.n, 16, false}, {R.gen, 8, true}, {R.mark, 4 * w, false},
                         {R.depth, 8 * (RVM_DEPTH_WINDOW + 1), true}},
                        R.bytes, "rqmem layout");
            expect(R.tb == R.tf + xg * nt * 8, "rq_tb right behind rq_tf");
            expect(R.gen == R.n + 32 && R.mark == R.n + 64 && R.mark % 64 == R.n % 64, "rq_n | gen_dev | rq_mark");
        }
        const HLayout H = h_layout((int32_t)em, mw);
        const size_t hs = RVM_HEDGE_STRIDE;
        check_block({{H.hrv, 16 * em * hs, true}, {H.hsum, 48 * hs, true}, {H.hslot, 16 * hs, true},
                     {H.htab, 8 * w, true}, {H.hw, 8 * RVM_HW_WORDS, true}},
                    H.bytes, "hmem layout");
        expect(RVM_HW_STATS + 5 <= RVM_HW_MARK && RVM_HW_MARK + 2 * RVM_HEDGE_GROUPS_MAX <= RVM_HW_WAIT &&
                   RVM_HW_WAIT + 3 <= RVM_HW_WORDS,
               "hw words");
        const ELayout E = e_layout((int32_t)em, mw);
        check_block({{E.rve, 32 * em * w, true}, {E.esum, 96 * w, true},
                     {E.eflag, 8 * (RVM_EFLAG_WORDS * (size_t)((RVM_EAGER_MAX + 15) / 16) + 8), true}},
                    E.bytes, "emem layout");
    }
}

int main() {
    expect(rvm_abi_version() == RVM_ABI_VERSION, "abi version");
    rvm_config cfg{};
    cfg.n_planets = 2;
    cfg.dt = 0.65;
    cfg.n_levels = 4;
    cfg.npoints_norm = 100.0;
    const int mult[4] = {4, 5, 6, 7};
    std::memcpy(cfg.level_mult, mult, sizeof(mult));
    cfg.period_hint = 5.2;
    std::vector<double> t, rv, sg;
    for (int i = 0; i < 101; i++) {  // both directions, unsorted, a duplicate epoch
        t.push_back(i % 2 ? -0.6 * i : 0.55 * (100 - i));
        rv.push_back(1e-4 * std::sin(i));
        sg.push_back(1.5e-4);
    }
    t[7] = t[9];
    rvm_plan* plan = nullptr;
    const int rc = rvm_plan_create(&cfg, t.data(), rv.data(), sg.data(), (int)t.size(), 4096, &plan);
    expect(rc == 0 || (rc < 0 && plan == nullptr), "plan_create valid input");
    if (rc == 0) rvm_plan_destroy(plan);
    check_plan_host(cfg, t, rv, sg);
    rvm_config bad = cfg;
    bad.n_levels = 0;
    expect(rvm_plan_create(&bad, t.data(), rv.data(), sg.data(), (int)t.size(), 64, &plan) < 0, "n_levels 0");
    bad = cfg;
    bad.level_mult[1] = 4;
    expect(rvm_plan_create(&bad, t.data(), rv.data(), sg.data(), (int)t.size(), 64, &plan) < 0, "dup multipliers");
    bad = cfg;
    bad.dt = -1.0;
    expect(rvm_plan_create(&bad, t.data(), rv.data(), sg.data(), (int)t.size(), 64, &plan) < 0, "negative dt");
    std::vector<double> tn = t;
    tn[3] = NAN;
    expect(rvm_plan_create(&cfg, tn.data(), rv.data(), sg.data(), (int)t.size(), 64, &plan) < 0, "nan epoch");
    expect(std::strlen(rvm_last_error()) > 0, "last_error");
    expect(rvm_logl_batch(nullptr, 1, nullptr, 1.0, nullptr, nullptr, nullptr, nullptr) < 0, "logl null plan");
    int64_t mk = -1, gu = -1;
    expect(rvm_plan_hedge_marks(nullptr, 0, &mk, &gu, nullptr) < 0 && mk == -1 && gu == -1, "hedge_marks null plan");
    int64_t lh = -1;
    expect(rvm_plan_hedge_waits(nullptr, 0, &mk, &lh, &gu, nullptr) < 0 && mk == -1 && lh == -1 && gu == -1,
           "hedge_waits null plan");
    rvm_param_map pm{};
    expect(rvm_stretch_half_step(nullptr, &pm, 10, 1, 0, nullptr, nullptr, nullptr, 1, nullptr, 2.0, 0, 0, 0, 1.0,
                                 nullptr, nullptr, nullptr, nullptr) < 0,
           "half_step null plan");
    expect(rvm_stretch_propose(0, 1, 0, nullptr, 1, nullptr, 2.0, 0, 0, 0, nullptr, nullptr, nullptr, nullptr) < 0,
           "propose bad");
    // parallel tempering: every refusal comes before any HIP call (the int32 bound in 64-bit arithmetic)
    double d1 = 0.5;
    int32_t i1 = 0;
    expect(rvm_pt_stretch_propose(10, 0, 1, &d1, &d1, 2.0, 0, 0, 0, nullptr, &d1, &d1, nullptr) < 0, "pt n_temps 0");
    expect(rvm_pt_stretch_propose(10, 2, 1, &d1, &d1, 1.0, 0, 0, 0, nullptr, &d1, &d1, nullptr) < 0, "pt a = 1");
    expect(rvm_pt_stretch_propose(10, 1 << 16, 1 << 16, &d1, &d1, 2.0, 0, 0, 0, nullptr, &d1, &d1, nullptr) < 0,
           "pt int32 overflow");
    expect(rvm_pt_stretch_accept(10, 2, 1, nullptr, &d1, &d1, &d1, &d1, &d1, 0, 0, 0, nullptr, &i1, nullptr) < 0,
           "pt null betas");
    expect(rvm_pt_stretch_accept(10, 2, 1, &d1, &d1, &d1, &d1, &d1, &d1, 0, 0, 2, nullptr, &i1, nullptr) < 0,
           "pt half 2");
    expect(rvm_pt_swap(10, 2, 0, &d1, &d1, &d1, &d1, &d1, 0, 0, nullptr, &i1, nullptr) < 0, "pt n_half 0");
    expect(rvm_pt_swap(10, 1 << 15, 1 << 15, &d1, &d1, &d1, &d1, &d1, 0, 0, nullptr, &i1, nullptr) < 0,
           "pt swap int32 overflow");
    expect(rvm_pt_swap(10, 1, 4, nullptr, nullptr, nullptr, nullptr, nullptr, 0, 0, nullptr, nullptr, nullptr) == 0,
           "pt swap of one temperature");
    int64_t l1 = 0;
    expect(rvm_pt_ladder_update(3, 1, &i1, &d1, &d1, -1.0, &d1, &l1, &d1, &l1, nullptr, &d1, nullptr) < 0,
           "pt ladder kappa < 0");
    expect(rvm_pt_ladder_update(3, 1, &i1, &d1, &d1, 0.5, &d1, &l1, &d1, &l1, nullptr, nullptr, nullptr) < 0,
           "pt ladder null workspace");
    expect(rvm_pt_ladder_update(1 << 16, 1 << 15, &i1, &d1, &d1, 0.5, &d1, &l1, &d1, &l1, nullptr, &d1, nullptr) < 0,
           "pt ladder int32 overflow");
    expect(rvm_pt_ladder_update(1, 4, nullptr, nullptr, nullptr, 0.5, nullptr, nullptr, nullptr, nullptr, nullptr,
                                nullptr, nullptr) == 0,
           "pt ladder of one temperature");
    // the stability screen: every refusal before any HIP call
    {
        int64_t s1 = 0;
        expect(rvm_stability_init(0, 0, 4, &d1, 1.0, &d1, &d1, &i1, &s1, nullptr) < 0, "stability n_planets 0");
        expect(rvm_stability_init(2, 0, 0, &d1, 1.0, &d1, &d1, &i1, &s1, nullptr) < 0, "stability n 0");
        expect(rvm_stability_init(2, 0, 4, nullptr, 1.0, &d1, &d1, &i1, &s1, nullptr) < 0, "stability null params");
        expect(rvm_stability_advance(2, 0, 4, &d1, 1.0, 0.0, 4, 1, 0.0, &d1, &d1, &i1, &s1, nullptr, nullptr) < 0,
               "stability h 0");
        expect(rvm_stability_advance(2, 0, 4, &d1, 1.0, NAN, 4, 1, 0.0, &d1, &d1, &i1, &s1, nullptr, nullptr) < 0,
               "stability h nan");
        expect(rvm_stability_advance(2, 1, 4, &d1, 1.0, 0.3, 0, 1, 0.0, &d1, &d1, &i1, &s1, nullptr, nullptr) < 0,
               "stability sample_every 0");
        expect(rvm_stability_advance(2, 1, 4, &d1, 1.0, 0.3, 4, 0, 0.0, &d1, &d1, &i1, &s1, nullptr, nullptr) < 0,
               "stability n_blocks 0");
        expect(rvm_stability_advance(2, 1, 4, &d1, 1.0, 0.3, 4, 1, 0.0, &d1, &d1, nullptr, &s1, nullptr, nullptr) < 0,
               "stability null status");
    }
    // the recorded chain: refusals before any HIP call, the column and lag bounds in 64-bit arithmetic
    expect(rvm_chain_record(2, 4, &d1, 16, 0, INT64_MAX, &d1, 8, 0, nullptr, nullptr, nullptr) < 0,
           "chain record stride overflow");
    expect(rvm_chain_record(2, 4, &d1, 16, 0, 1, &d1, INT64_MAX, INT64_MAX - 1, nullptr, nullptr, nullptr) < 0,
           "chain record dst_col0 overflow");
    expect(rvm_chain_record(2, 4, &d1, 16, 0, 1, &d1, 8, 0, &d1, nullptr, nullptr) < 0, "chain record lone lnp_src");
    expect(rvm_chain_moments(&d1, 2, 4, 5, 5, &d1, &d1, nullptr) < 0, "chain moments empty range");
    expect(rvm_chain_autocov(&d1, &d1, 2, 4, 0, 10, INT32_MAX, 1 << 30, &d1, &d1, nullptr) < 0,
           "chain autocov lag overflow");
    expect(rvm_chain_autocov(&d1, &d1, 65534, 4, 0, INT64_MAX, 0, 1 << 30, &d1, &d1, nullptr) < 0,
           "chain autocov n_params * n_lags");
    expect(rvm_chain_autocov_workspace_bytes(10, 200, 17) == (size_t)8 * 10 * 32, "chain autocov workspace");
    expect(rvm_chain_autocov_workspace_bytes(1, 65535 * 256, 1 << 30) == (size_t)8 * ((size_t)1 << 30) * 65535,
           "chain autocov workspace, largest");
    expect(rvm_chain_autocov_workspace_bytes(65534, 4, 1 << 30) == 0, "chain autocov workspace, refused");
    expect(rvm_mh_accept(0, 1, 0, nullptr, nullptr, nullptr, nullptr, 0, 0, nullptr, nullptr, nullptr) < 0, "mh bad");
    expect(rvm_fd_params(10, 1, nullptr, 1e-6, nullptr, nullptr, nullptr) < 0, "fd bad");
    const int32_t rows[2] = {0, 0};
    expect(rvm_logl_derivs(nullptr, 1, nullptr, 2, rows, 1.0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) < 0,
           "derivs null plan");
    expect(rvm_logl_derivs_workspace_bytes(256, 10) == (size_t)256 * 55 * 2 * 36, "derivs workspace");
    rvm_smala_cache c{};
    expect(rvm_smala_metric(10, 1, nullptr, nullptr, nullptr, nullptr, nullptr, 1.0, 0.5, &c, nullptr) < 0, "metric bad");
    std::printf("host sanitize driver: %d failures\n", fails);
    return fails;
}
