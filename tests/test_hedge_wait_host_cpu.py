"""The host half of team A's wait for a running hedge block (rvm_plan_host.cpp; no GPU): the RVM_HEDGE_WAIT
knob as read_plan_knobs parses it, the wait's safety bound against team B's own (hedge_wait_bound: strictly
below spin_ticks << 1 for every hand-off timeout, the 10 ns one of tests/test_gpu_resolve.py included), and the
layouts grown for it (rq_tb right behind rq_tf, the wait's counters behind the mark words of hw).  rvm_plan_host.cpp is
built with the host compiler and a small driver, as csrc/host_sanitize.cpp does."""
import pytest

from support import host_driver_report

DRIVER = r"""
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "rvm_plan_host.h"
using namespace rvm;
static int knob(const char* v) {
    if (v) setenv("RVM_HEDGE_WAIT", v, 1); else unsetenv("RVM_HEDGE_WAIT");
    return read_plan_knobs().hedge_wait;
}
struct R { size_t off, bytes; };
static bool disjoint(const std::vector<R>& r, size_t total) {
    size_t end = 0;
    for (const R& x : r) {
        if (x.off < end || x.off % 8 != 0) return false;
        end = x.off + x.bytes;
    }
    return end <= total;
}
int main() {
    std::printf("{\"unset\": %d, \"0\": %d, \"1\": %d, \"2\": %d, \"garbage\": %d, \"empty\": %d", knob(nullptr), knob("0"),
                knob("1"), knob("2"), knob("yes"), knob(""));
    // the bound for every small timeout, powers of two and their neighbours up to 2^62, and the default
    int bad = 0;
    auto chk = [&](unsigned long long sp) {
        const unsigned long long b = hedge_wait_bound(sp);
        if (sp >= 4 && b == 0) bad++;
        if (!(b < (sp << 1)) || !(b < sp)) bad++;
    };
    for (unsigned long long sp = 1; sp <= 100000; sp++) chk(sp);
    for (int s = 1; s <= 62; s++)
        for (long long d = -1; d <= 1; d++) chk((1ull << s) + d);
    chk(200000000ull);
    rvm_config cfg{};
    cfg.n_planets = 2; cfg.dt = 0.65; cfg.n_levels = 4; cfg.npoints_norm = 100.0; cfg.period_hint = 5.2;
    cfg.resolve_tol = 5e-7; cfg.resolve_max = 6;
    const int mult[4] = {4, 5, 6, 7};
    for (int k = 0; k < 4; k++) cfg.level_mult[k] = mult[k];
    unsetenv("RVM_HEDGE_WAIT");
    DevPlan P{};
    fill_plan_scalars(&cfg, mult, 101, 51, 50, 256, read_plan_knobs(), &P);
    std::printf(", \"bound_violations\": %d, \"bound_1\": %llu, \"bound_default\": %llu, \"plan_ticks\": %llu, \"plan_spin\": %llu, \"devplan_bytes\": %zu",
                bad, (unsigned long long)hedge_wait_bound(1), (unsigned long long)hedge_wait_bound(200000000ull),
                (unsigned long long)P.hedge_wait_ticks, P.spin_ticks, sizeof(DevPlan));
    int lay = 0;
    for (int32_t mw : {1, 33, 64, 6144, 12288})
        for (int teams : {1, 2, 4}) {
            const size_t w = mw, xg = (w + 15) / 16 + 1, nt = teams < 2 ? 2 : teams;
            const RqLayout L = rq_layout(mw, teams);
            if (!disjoint({{L.x, xg * nt * 256 * 8}, {L.xf, xg * nt * 16}, {L.t, xg * (nt - 1) * 8192}, {L.tf, xg * nt * 8},
                           {L.tb, xg * 8}, {L.c, 16 * w}, {L.w, (12 * w + 7) & ~(size_t)7}, {L.n, 64}, {L.mark, 4 * w},
                           {L.depth, 8 * (RVM_DEPTH_WINDOW + 1)}}, L.bytes) || L.tb != L.tf + xg * nt * 8 || L.gen != L.n + 32 || L.xgroups != (int32_t)xg)
                lay++;
            const HLayout H = h_layout(101, mw);
            const size_t hs = RVM_HEDGE_STRIDE;
            if (!disjoint({{H.hrv, 16 * 101 * hs}, {H.hsum, 48 * hs}, {H.hslot, 16 * hs}, {H.htab, 8 * w},
                           {H.hw, 8 * (size_t)RVM_HW_WORDS}}, H.bytes))
                lay++;
        }
    // hw: cancel, leave count, completion words | statistics (5 used of 6) | marks | the wait's three counters
    const bool hw_ok = RVM_HW_STATS == 2 + 2 * RVM_HEDGE_GROUPS_MAX && RVM_HW_STATS + 5 <= RVM_HW_MARK &&
                       RVM_HW_MARK + 2 * RVM_HEDGE_GROUPS_MAX == RVM_HW_WAIT && RVM_HW_WAIT + 3 == RVM_HW_WORDS;
    std::printf(", \"layout_failures\": %d, \"hw_ok\": %d}\n", lay, hw_ok ? 1 : 0);
    return 0;
}
"""


@pytest.fixture(scope="module")
def report(tmp_path_factory):
    return host_driver_report(tmp_path_factory, "hedge_wait_host", DRIVER)


def test_knob_parses(report):
    assert report["unset"] == 1 and report["1"] == 1
    assert report["0"] == 0
    assert report["2"] == 2
    assert report["garbage"] == 1 and report["empty"] == 1


def test_safety_bound_is_below_team_bs(report):
    assert report["bound_violations"] == 0
    # (rvm_plan_set_handoff_timeout(1e-8) gives spin_ticks 1: the bound is 0, team A's poll ends at once)
    assert report["bound_1"] == 0
    assert report["bound_default"] == 50000000
    assert report["plan_spin"] == 200000000 and report["plan_ticks"] == 50000000


def test_grown_layouts_do_not_overlap(report):
    assert report["layout_failures"] == 0
    assert report["hw_ok"] == 1
