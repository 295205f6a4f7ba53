// rvm_plan_host.h -- the host arithmetic of rvm_plan_create (rvm_plan.hip): config checks, the epoch
// schedule, the DevPlan's scalar fields, the environment knobs and the byte layout of every device
// block.  Plain C++ with no HIP call, so csrc/host_sanitize.cpp runs all of it on a host without a GPU.
#pragma once
#include <cstddef>
#include <vector>

#include "rvm_internal.h"

namespace rvm {

// Every environment variable plan creation reads (read_plan_knobs; parsing differs per knob on purpose).
struct PlanKnobs {
    int32_t skip_variants;   // RVM_SKIP_VARIANTS: 0 refines the variants the partner's decision rules out (A/B)
    double late_spo;         // RVM_LATE_SPO: steps per period_hint from which a level takes the late vote (96; 0: off)
    bool no_level_split;     // RVM_NO_LEVEL_SPLIT=1 forces the LDS-coupled layout (timing build only: scripts/probe)
    int32_t n_teams;         // RVM_REFINE_TEAMS: 0 or 1 runs the passes one after the other, 2 .. RVM_TEAMS_MAX at once
    int32_t eager_split;     // RVM_EAGER_SPLIT: 0 keeps both directions of an eager launch's refinement in one block
    bool no_extension;       // RVM_NO_EXTENSION=1: no extension stage, flagged directions go straight to halving passes
    bool refine_split;       // RVM_REFINE_SPLIT: 0 keeps both directions in one block
    bool teams_hint;         // RVM_TEAMS_HINT: 0 always runs the plan's team count
    bool eager;              // RVM_EAGER: 0 turns the eager pass off, 1 on
    int32_t eager_passes;    // RVM_EAGER_PASSES: 1 or 2
    int32_t hedge_groups;    // RVM_HEDGE=0: no hedged pass 2; RVM_HEDGE_GROUPS caps its groups (0 .. RVM_HEDGE_GROUPS_MAX)
    int32_t hedge_mark;      // RVM_HEDGE_MARK: 0 leaves unneeded hedge blocks to the cancel
    int32_t hedge_wait;      // RVM_HEDGE_WAIT: 0 team A never waits for a hedge block, 1 (default) it does, 2 it always polls
};
PlanKnobs read_plan_knobs();

// Argument checks after the null test, in the order their messages win; resolves the multipliers
// (all-zero level_mult: the harmonic ladder 1, 2, ...).  Returns the message, or nullptr.
const char* check_plan_config(const rvm_config* cfg, const double* t, const double* rv, const double* sigma,
                              int32_t n_obs, int32_t max_walkers, int mult[RVM_MAX_LEVELS], int* max_mult);

// One direction's epochs sorted by |t| (stable), each segment cut into ceil(len / dt) steps
struct HostDir {
    std::vector<int32_t> idx, seg_n;
    std::vector<double> seg_len, orv, os2;  // signed base step (level step = this / mult), RV, sigma^2
    long long total_steps = 0;
    int32_t split0 = 0, pre0 = 0, split1 = 0, pre1 = 0;  // DirSched's head / tail split points
};
// dir[0]: t >= 0, dir[1]: t < 0.  Returns a refusal's message, or nullptr.
const char* build_schedule(const rvm_config* cfg, const int* mult, int max_mult, const double* t, const double* rv,
                           const double* sigma, int32_t n_obs, HostDir dir[2]);

// Lagrange-at-zero weights in x = 1 / m^2 of levels k0 .. n-1 (w[k] written for those k only)
void lagrange_at_zero(const int* m, int k0, int n, double* w);

inline int walkers_per_group(int n_planets) { return n_planets == 1 ? 64 : (n_planets == 2 ? 32 : 16); }

// Every DevPlan field that is no device pointer and no DirSched, for a plan without extension (ext_mult 0)
void fill_plan_scalars(const rvm_config* cfg, const int* mult, int32_t n_obs, size_t nf, size_t nb, int n_cu,
                       const PlanKnobs& K, DevPlan* P);
// DevPlan::hedge_wait_ticks for a plan whose hand-off waits give up after spin_ticks: a quarter of it (42 s at
// the most), so strictly below team B's own bound (spin_ticks << 1) for every spin_ticks >= 1 -- team A never
// out-waits B
uint32_t hedge_wait_bound(unsigned long long spin_ticks);
bool plan_wants_extension(const DevPlan& P, const PlanKnobs& K);
// the extension level's fields (ext_*, lw5, slot n_levels of mult / nt / spec / inv_mult), once its workspace exists
void fill_plan_extension(DevPlan* P);
// the level-split layout's condition (four strictly increasing levels, a largest launch of two-group blocks)
bool plan_wants_level_split(const DevPlan& P, int32_t max_walkers, const PlanKnobs& K);

// The layout one likelihood launch takes (rvm_logl.hip launch_logl_t launches exactly this):
//   LDS-coupled (nA = 0): 2-D grid of blocks of G = 1 or 2 walker groups, one wave per level (G = 2: the second
//     group's levels mirrored), with cx the extension level as a further wave (G = 1 only);
//   level-split (nA > 0; four levels, W <= lv_stride): 1-D grid of 8-wave blocks, nA of type A and nB of type B
//     carrying tB (6 or 8) units each; splitA: level 0 split head / tail, lsx: the extension as a fifth level --
//     both need a whole direction in the ring (emax <= RVM_LS_RING).  smem = lds.bytes(); fits: within budget.
struct LoglLayout {
    int G, cx, nA, nB, tB, splitA, lsx;
    unsigned grid_x, grid_y, block;
    LoglLds lds;
    size_t smem;
    bool fits;
};
// The whole decision, from the plan's scalars (its pointers only tested against null), the launch's (W, model RVs
// asked for, a fused sampler step), the RVM_CX_PAIRS knob and the two instantiations' dynamic-LDS budgets.
LoglLayout choose_logl_layout(const DevPlan& P, int W, bool want_rv, bool fused, bool cx_pairs, size_t budget_lc,
                              size_t budget_ls);

// Byte offsets inside the plan's device blocks, in the order they are laid out; `bytes` the block's size.
struct DmemLayout {  // schedule f64 | slots | counters (u64) | schedule int32, + 64
    size_t seg_h1[2], obs_rv[2], obs_s2[2], slots, counters, seg_n[2], obs_idx[2], bytes;
};
DmemLayout dmem_layout(size_t nf, size_t nb, int32_t max_walkers);
struct LvLayout {  // DevPlan::lv_rv [2][emax][max_walkers] | lv_enc [2][max_walkers]
    size_t rv, enc, bytes;
    int32_t emax;
};
LvLayout lv_layout(size_t nf, size_t nb, int32_t max_walkers);
struct XLayout {  // lvx | rvp | rvp2 [n_teams - 1], each [2][emax][max_walkers] doubles
    size_t lvx, rvp, rvp2, bytes;
    int32_t emax;
};
XLayout x_layout(size_t nf, size_t nb, int32_t max_walkers, int n_teams);
struct RqLayout {  // rq_x | rq_xf | rq_t | rq_tf | rq_tb | rq_c | rq_w | rq_n [4] | gen_dev at + 32 | rq_mark at + 64 | depth_w
    size_t x, xf, t, tf, tb, c, w, n, gen, mark, depth, bytes;
    int32_t xgroups;  // exchange groups; each sized for max(n_teams, 2) teams
};
RqLayout rq_layout(int32_t max_walkers, int n_teams);
struct HLayout {  // hrv [2][emax][stride] | hsum [2][3][stride] | hslot [2][stride] | htab [max_walkers] | hw
    size_t hrv, hsum, hslot, htab, hw, bytes;
};
HLayout h_layout(int32_t lvx_emax, int32_t max_walkers);
struct ELayout {  // passes 1 and 2: rve [2][2][emax][stride] | esum [2][2][3][stride] | eflag [groups][8] (zeroed)
    size_t rve, esum, eflag, bytes;
};
ELayout e_layout(int32_t lvx_emax, int32_t lvx_stride);

}  // namespace rvm
