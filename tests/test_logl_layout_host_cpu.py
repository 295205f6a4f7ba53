"""The likelihood launch's layout, on the host (rvm_plan_host.cpp choose_logl_layout, rvm_internal.h LoglLds; no
GPU): over a grid of plans and launch sizes the dynamic-LDS request is LoglLds's total, that total is the sum
the layouts' comments state, every range of it lies inside without overlap, and the choice keeps its
invariants; and the layout of every shape the GPU tests name (tests/test_gpu_logl.py, and the adaptive plans of
tests/test_gpu_resolve_systems.py) is pinned, each value derived from the rule.  rvm_plan_host.cpp is built with the host compiler and a small driver, as
tests/test_hedge_wait_host_cpu.py does.  The same driver reaches rvm_internal.h's blocks_of and RVM_QNAN, which the
sampler and read-out launchers share: the block count at the edges of a block and of int32, the NaN's bits."""
import pytest

from support import host_driver_report

DRIVER = r"""
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "rvm_plan_host.h"
using namespace rvm;
struct R { size_t off, n; };
// the ranges in ascending order, none overlapping, all inside `total` (doubles)
static bool disjoint(std::vector<R> r, size_t total) {
    std::sort(r.begin(), r.end(), [](const R& a, const R& b) { return a.off < b.off || (a.off == b.off && a.n < b.n); });
    size_t end = 0;
    for (const R& x : r) {
        if (x.off < end) return false;
        end = x.off + x.n;
    }
    return end <= total;
}
static double dummy;
static DevPlan plan(int np, int inc, int nl, const int* lad, int em, int rmax, int ext, int ncu, int mw) {
    rvm_config cfg{};
    cfg.n_planets = np; cfg.dt = 0.65; cfg.n_levels = nl; cfg.npoints_norm = 100.0; cfg.period_hint = 5.2;
    cfg.inclined = inc; cfg.resolve_tol = rmax ? 5e-7 : 0.0; cfg.resolve_max = rmax;
    int mult[RVM_MAX_LEVELS] = {};
    for (int k = 0; k < nl; k++) cfg.level_mult[k] = mult[k] = lad[k];
    DevPlan P{};
    const PlanKnobs K = read_plan_knobs();
    fill_plan_scalars(&cfg, mult, em + em / 2, em, em / 2, ncu, K, &P);
    P.fwd.n_epochs = em; P.bwd.n_epochs = em / 2;
    if (ext) fill_plan_extension(&P);
    if (plan_wants_level_split(P, mw, K)) { P.lv_rv = &dummy; P.lv_stride = mw; }  // (rvm_plan.hip alloc_level_split)
    return P;
}
// (the budgets on an MI355X: the CU's LDS less the two instantiation families' static LDS, 3216 and 12936 B)
static const size_t BUD_LC = (size_t)RVM_LDS_PER_CU - 3216, BUD_LS = (size_t)RVM_LDS_PER_CU - 12936;
int main() {
    const int emaxs[6] = {0, 1, 51, 64, 65, 151};
    const int Ws[13] = {1, 63, 64, 65, 2048, 2900, 4096, 4128, 4160, 6000, 6400, 8192, 12288};
    const int lad4[4] = {4, 5, 6, 7}, lad3[3] = {1, 2, 3};
    long long cases = 0, f_smem = 0, f_sum = 0, f_range = 0, f_cu = 0, f_block = 0, f_ring = 0, f_cx = 0, f_split = 0,
              f_grid = 0, n_split = 0, n_lsx = 0, n_cx = 0, n_g2 = 0;
    for (int nl = 3; nl <= 4; nl++)
    for (int np = 1; np <= 4; np++)
    for (int inc = 0; inc < 2; inc++)
    for (int ei = 0; ei < 6; ei++)
    for (int rmax = 0; rmax <= 6; rmax += 6)
    for (int ext = 0; ext < 2; ext++)
    for (int ncu : {64, 256})
    for (int mw : {6000, 12288}) {
        const int em = emaxs[ei];
        const DevPlan P = plan(np, inc, nl, nl == 4 ? lad4 : lad3, em, rmax, ext, ncu, mw);
        const int wpb = walkers_per_group(np), rows = (inc ? 7 : 5) * np;
        for (int fused = 0; fused < 2; fused++)
        for (int rv = 0; rv < 2; rv++)
        for (int wi = 0; wi < 13; wi++) {
            const int W = Ws[wi];
            const LoglLayout Y = choose_logl_layout(P, W, rv != 0, fused != 0, true, BUD_LC, BUD_LS);
            const LoglLds& L = Y.lds;
            cases++;
            n_split += Y.nA > 0; n_lsx += Y.lsx; n_cx += Y.cx; n_g2 += Y.G == 2;
            if (Y.smem != L.bytes() || L.bytes() != 8 * L.total()) f_smem++;
            // the sums as the layouts' comments state them (rvm_internal.h LoglLds), restated here
            const size_t init = rmax > 0 ? RVM_INIT_DOUBLES : 0;
            const size_t ring = (size_t)std::min(em, (int)RVM_LS_RING);
            const size_t want = Y.nA > 0 ? (size_t)8 * em + 2 * (Y.lsx ? 4 : 3) * ring * wpb + 2 * init
                                         : (size_t)4 * em + (fused ? (size_t)(rows + 3) * Y.G * wpb : 0) + Y.G * init +
                                               (size_t)Y.G * P.lc_ring * (nl + 1) * wpb;
            if (L.total() != want) f_sum++;
            std::vector<R> r;
            if (Y.nA > 0) {
                r = {{L.sched_dir(0), (size_t)4 * em}, {L.sched_dir(1), (size_t)4 * em}, {L.ring(), L.ring_size()},
                     {L.init_state(), L.init_size()}};
                if (L.sched_dir(1) + (size_t)4 * em > L.sched_size()) f_range++;
            } else {
                r = {{L.sched_dir(0), L.sched_size()}, {L.staging(), L.staging_size()}, {L.init_state(), L.init_size()},
                     {L.ring(), L.ring_size()}};
                if (L.sched_dir(1) != 0) f_range++;
            }
            if (!disjoint(r, L.total())) f_range++;
            if (Y.nA > 0 && Y.nA + Y.nB > ncu) f_cu++;
            if (Y.block > 512 || Y.block % 64 != 0 || Y.block == 0) f_block++;
            if ((Y.lsx || Y.splitA) && em > RVM_LS_RING) f_ring++;
            if ((Y.lsx || Y.splitA) && Y.nA == 0) f_ring++;
            if (Y.cx && Y.G != 1) f_cx++;
            if (Y.nA > 0 && !(W <= P.lv_stride && nl == 4 && P.lv_rv != nullptr)) f_split++;
            const int groups = (W + wpb - 1) / wpb;
            if (Y.nA > 0 ? !(Y.grid_x == (unsigned)(Y.nA + Y.nB) && Y.grid_y == 1 && Y.block == 512 && Y.nA == groups &&
                             Y.nB * Y.tB >= 2 * groups && (Y.tB == 6 || Y.tB == 8))
                         : !(Y.grid_x * Y.G >= (unsigned)groups && Y.grid_y == 2 &&
                             Y.block == (unsigned)(64 * (nl + Y.cx) * Y.G)))
                f_grid++;
        }
    }
    std::printf("{\"cases\": %lld, \"smem\": %lld, \"sum\": %lld, \"ranges\": %lld, \"cus\": %lld, \"block\": %lld, "
                "\"ring\": %lld, \"cx\": %lld, \"split\": %lld, \"grid\": %lld, \"n_split\": %lld, \"n_lsx\": %lld, "
                "\"n_cx\": %lld, \"n_g2\": %lld, \"pins\": {",
                cases, f_smem, f_sum, f_range, f_cu, f_block, f_ring, f_cx, f_split, f_grid, n_split, n_lsx, n_cx, n_g2);
    // the GPU tests' shapes: fixed-resolution plans (no extension, rmax 0) of levels 4..7 on 256 CUs, 51 / 25 epochs,
    // max_walkers = W, model RVs asked for
    const int pins[7][2] = {{2, 4096}, {2, 4128}, {2, 6000}, {2, 6400}, {2, 8192}, {3, 2900}, {3, 4160}};
    for (int i = 0; i < 7; i++) {
        const DevPlan P = plan(pins[i][0], 0, 4, lad4, 51, 0, 0, 256, pins[i][1]);
        const LoglLayout Y = choose_logl_layout(P, pins[i][1], true, false, true, BUD_LC, BUD_LS);
        std::printf("%s\"%d:%d\": [%d, %d, %d, %d, %d, %d, %d, %u, %u, %u]", i ? ", " : "", pins[i][0], pins[i][1], Y.G, Y.cx,
                    Y.nA, Y.nB, Y.tB, Y.splitA, Y.lsx, Y.grid_x, Y.grid_y, Y.block);
    }
    // the adaptive GPU tests' shapes (tests/test_gpu_resolve_systems.py): plans with the extension and resolve_max 4,
    // otherwise as above; plain launches (not fused) that ask for no model RVs; {planets, inclined, W}
    const int apins[19][3] = {{3, 0, 24}, {3, 0, 256}, {3, 0, 2304}, {3, 0, 3264}, {3, 0, 3265},
                              {4, 0, 24}, {4, 0, 256}, {4, 0, 2304},
                              {2, 1, 24}, {2, 1, 256}, {2, 1, 2304}, {2, 1, 4096}, {2, 1, 4097},
                              {3, 1, 24}, {3, 1, 256}, {3, 1, 2304}, {4, 1, 24}, {4, 1, 256}, {4, 1, 2304}};
    for (int i = 0; i < 19; i++) {
        const DevPlan P = plan(apins[i][0], apins[i][1], 4, lad4, 51, 4, 1, 256, apins[i][2]);
        const LoglLayout Y = choose_logl_layout(P, apins[i][2], false, false, true, BUD_LC, BUD_LS);
        std::printf(", \"%s%d:%d\": [%d, %d, %d, %d, %d, %d, %d, %u, %u, %u]", apins[i][1] ? "i" : "p", apins[i][0],
                    apins[i][2], Y.G, Y.cx, Y.nA, Y.nB, Y.tB, Y.splitA, Y.lsx, Y.grid_x, Y.grid_y, Y.block);
    }
    // the launchers' block count (rvm_internal.h blocks_of) at the edges of a block of 256 and at the largest count
    // the ABI admits, where n + 255 does not fit an int32; and the read-outs' quiet NaN, bit for bit
    std::printf("}, \"blocks_of\": [");
    const long long ns[6] = {0, 1, 255, 256, 257, INT32_MAX};
    for (int i = 0; i < 6; i++) std::printf("%s%u", i ? ", " : "", blocks_of((uint64_t)ns[i], 256));
    std::printf(", %u, %u]", blocks_of((uint64_t)2 * INT32_MAX, 256), blocks_of((uint64_t)INT32_MAX, 2));
    const double qnan = RVM_QNAN;
    unsigned long long bits;
    std::memcpy(&bits, &qnan, sizeof bits);
    std::printf(", \"qnan_bits\": \"%016llx\"}\n", bits);
    return 0;
}
"""


@pytest.fixture(scope="module")
def report(tmp_path_factory):
    return host_driver_report(tmp_path_factory, "logl_layout_host", DRIVER)


def test_request_is_the_lds_layouts_total(report):
    # 2 ladders x 4 planet counts x 2 x 6 epoch counts x 2 x 2 x 2 CU counts x 2 max_walkers, x 2 x 2 x 13 launches
    assert report["cases"] == 2 * 4 * 2 * 6 * 2 * 2 * 2 * 2 * 2 * 2 * 13
    assert report["smem"] == 0
    assert report["sum"] == 0


def test_offset_ranges_lie_inside_without_overlap(report):
    assert report["ranges"] == 0


def test_choice_keeps_its_invariants(report):
    assert report["cus"] == 0      # nA + type-B blocks <= n_cu
    assert report["block"] == 0    # whole waves, at most 512 threads
    assert report["ring"] == 0     # lsx / splitA only with a whole direction in the ring, and only level-split
    assert report["cx"] == 0       # the concurrent extension wave only with one group per block
    assert report["split"] == 0    # level-split only when W <= lv_stride, four levels, the workspace exists
    assert report["grid"] == 0     # the grid covers every group / unit
    # (the grid reaches every layout)
    assert min(report["n_split"], report["n_lsx"], report["n_cx"], report["n_g2"]) > 0


# [G, cx, nA, nB, tB, splitA, lsx, grid_x, grid_y, block] of the shapes tests/test_gpu_logl.py names.  Levels
# m = (4, 5, 6, 7), 256 CUs, no extension (so no cx, no lsx), 51 epochs (<= RVM_LS_RING: splitA when level-split).
# Level-split needs the plan's workspace (2 groups(max_walkers) > 256), na + nb <= 256 with na = groups,
# nb = ceil(2 groups / tB), tB = 6 when groups + ceil(2 groups / 6) <= 256 else 8, and
# c_dec = max(m3, m2 + m0, 2 m1) = 10 below c_cpl = m3 ceil(2 groups / 256) for one-group blocks or
# max(m0 + m3, m1 + m2) ceil(groups / 256) = 11 ceil(groups / 256) for two-group blocks.
PINS = {
    # 2 planets, 32 walkers per group
    # 4096: 128 groups, 2 x 128 = 256 is not > 256: one group per block, no workspace; grid 128 x 2 of 4 waves
    "2:4096": [1, 0, 0, 0, 8, 0, 0, 128, 2, 256],
    # 4128: 129 groups, 258 > 256: two groups per block would be 65 x 2 blocks of 8 waves, c_cpl = 11; tB = 6
    # (129 + 43 = 172 <= 256), nb = 43, 10 < 11: level-split, 129 + 43 blocks
    "2:4128": [2, 0, 129, 43, 6, 1, 0, 172, 1, 512],
    # 6000: 188 groups; tB = 6 (188 + 63 = 251 <= 256), nb = 63: level-split, 251 blocks
    "2:6000": [2, 0, 188, 63, 6, 1, 0, 251, 1, 512],
    # 6400: 200 groups; 200 + 67 = 267 > 256 so tB = 8, nb = 50, 250 <= 256: level-split, 250 blocks
    "2:6400": [2, 0, 200, 50, 8, 1, 0, 250, 1, 512],
    # 8192: 256 groups; tB = 8, nb = 64, 320 > 256: two groups per block, grid 128 x 2 of 8 waves
    "2:8192": [2, 0, 0, 0, 8, 0, 0, 128, 2, 512],
    # 3 planets, 16 walkers per group (no extension: no paired one-group blocks)
    # 2900: 182 groups, 364 > 256; tB = 6 (182 + 61 = 243 <= 256), nb = 61: level-split, 243 blocks
    "3:2900": [2, 0, 182, 61, 6, 1, 0, 243, 1, 512],
    # 4160: 260 groups; tB = 8, nb = 65, 325 > 256: two groups per block, grid 130 x 2 of 8 waves
    "3:4160": [2, 0, 0, 0, 8, 0, 0, 130, 2, 512],
}

# The shapes tests/test_gpu_resolve_systems.py names ("p" planar / "i" inclined, planets : W): adaptive plans
# (resolve_max 4, so the extension level m4 = 8 and the t = 0 state in LDS), max_walkers = W, plain launches
# without model RVs.  The extension runs beside the main pass (xcon) as a fifth wave of one-group blocks (cx) from
# RVM_CX_MIN_WALKERS = 32 walkers on, or as a fifth level of the level-split layout (lsx, type-B blocks of 8
# units) where two groups would share a block.  3 and 4 planets: 16 walkers per group; 2 planets: 32.
PINS.update({
    # 24: 2 groups (i2: 1), below RVM_CX_MIN_WALKERS: no cx, the extension after the main pass; 4 waves
    "p3:24": [1, 0, 0, 0, 8, 0, 0, 2, 2, 256],
    "p4:24": [1, 0, 0, 0, 8, 0, 0, 2, 2, 256],
    "i2:24": [1, 0, 0, 0, 8, 0, 0, 1, 2, 256],
    "i3:24": [1, 0, 0, 0, 8, 0, 0, 2, 2, 256],
    "i4:24": [1, 0, 0, 0, 8, 0, 0, 2, 2, 256],
    # 256: 16 groups (i2: 8), one per block with the extension wave: 5 waves
    "p3:256": [1, 1, 0, 0, 8, 0, 0, 16, 2, 320],
    "p4:256": [1, 1, 0, 0, 8, 0, 0, 16, 2, 320],
    "i2:256": [1, 1, 0, 0, 8, 0, 0, 8, 2, 320],
    "i3:256": [1, 1, 0, 0, 8, 0, 0, 16, 2, 320],
    "i4:256": [1, 1, 0, 0, 8, 0, 0, 16, 2, 320],
    # 2304: 144 groups, 288 > 256: crowded.  4 planets and inclined: two groups would share a block, so lsx with
    # nb = ceil(288 / 8) = 36, 144 + 36 = 180 <= 256 blocks
    "p4:2304": [2, 0, 144, 36, 8, 0, 1, 180, 1, 512],
    "i3:2304": [2, 0, 144, 36, 8, 0, 1, 180, 1, 512],
    "i4:2304": [2, 0, 144, 36, 8, 0, 1, 180, 1, 512],
    # 3 planar planets pair one-group blocks (G = 1, cx) instead -- but the plan has the level-split workspace,
    # and the fixed-resolution rule above then still applies: tB = 6 (144 + 48 = 192 <= 256), c_dec = 10 below
    # c_cpl = m3 ceil(288 / 256) = 14: level-split without the fifth level (the extension after the main pass),
    # 144 + 48 blocks.  (cx is the coupled layout's and unused here.)
    "p3:2304": [1, 1, 144, 48, 6, 1, 0, 192, 1, 512],
    # ... up to 204 groups (3264 walkers: tB = 8, 204 + 51 = 255 <= 256).  From 205 groups on (3265 walkers, the
    # last group with one: 205 + 52 = 257 > 256) the level-split layout does not fit and the paired one-group blocks
    # run: 205 x 2 blocks of 5 waves, two per CU
    "p3:3264": [1, 1, 204, 51, 8, 1, 0, 255, 1, 512],
    "p3:3265": [1, 1, 0, 0, 8, 0, 0, 205, 2, 320],
    # 2 inclined planets, 32 walkers per group: 2304 is 72 groups and 4096 is 128, 256 is not > 256: still cx.
    # 4097: 129 groups, crowded: lsx with nb = ceil(258 / 8) = 33, 129 + 33 = 162 blocks
    "i2:2304": [1, 1, 0, 0, 8, 0, 0, 72, 2, 320],
    "i2:4096": [1, 1, 0, 0, 8, 0, 0, 128, 2, 320],
    "i2:4097": [2, 0, 129, 33, 8, 0, 1, 162, 1, 512],
})


@pytest.mark.parametrize("shape", sorted(PINS))
def test_layout_of_the_gpu_tests_shapes(report, shape):
    assert report["pins"][shape] == PINS[shape]


def test_block_count_and_quiet_nan(report):
    # ceil(n / 256) for n = 0, 1, 255, 256, 257, INT32_MAX (2^23 blocks: n + 255 computed in int32 would wrap),
    # then rvm_stretch_iteration_end's 2 n threads at n = INT32_MAX and rvm_chain_cov's tiles of 2 parameters
    assert report["blocks_of"] == [0, 1, 1, 1, 2, 1 << 23, 1 << 24, 1 << 30]
    assert report["qnan_bits"] == "7ff8000000000000"
