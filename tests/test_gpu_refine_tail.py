"""Hedge blocks nobody can use stop when the refinement kernel starts (DESIGN.md §4 *blocks nobody can use
stop early*; §10 item 8).

A hedge result is only ever read for a walker slot on the refinement kernel's lists.  At its start the
refinement kernel marks the hedge blocks (group, direction) none of whose slots is listed
(rvm_refine_impl.h hedge_mark_unneeded, hw[RVM_HW_MARK ..]), and those blocks stop at their next epoch instead
of integrating until the launch's final cancel, so the join after the refinement kernel rarely has a block to
wait for.  RVM_HEDGE_MARK=0 at plan creation leaves them running (the former path).  rvm_plan_hedge_marks
counts the marks written and the blocks that stopped on theirs.

Nothing a caller sees may change -- positions, log-probabilities, accept counters and the plan's counters
are those of a plan created with RVM_HEDGE_MARK=0, bit for bit,

  * at the bench chain's steady state (scripts/probe/ens_it2000.npy, seed 2017, 4 speculative iterations:
    the oracle has pass-2 slots in iterations 1, 2 and 3, tests/test_gpu_hedge.py) with the team hint,
    two teams, one team and one block per group -- the pass-2 walker-directions the hedge covers are still
    replayed -- and without the hedge (RVM_HEDGE=0: no marks);
  * with one hedge group only (RVM_HEDGE_GROUPS=1: two hedge blocks, both marked in most launches);
  * on wide-ball walkers (two-pass walkers, deeper ones, encounters, prior rejections) through fused
    half-steps of 48 and 64 walkers per half: every slot hedged, so most groups hold a listed slot and
    stay; at 48 the last hedge group and the last refinement group are partial.  A mark on a group that
    holds a listed slot would cost a replay, never a bit.
And the marks are really there: at the steady state (16 hedge blocks per launch, ~340 listed slots of 6144,
of which a handful rank within the hedge's 256) marks are written in every hedged layout, and with the default
layout blocks stop on them; with the switch off, or without a hedge, none.  A block can only stop on a mark that was written, and no
launch writes more marks than it has hedge blocks.
The hedge statistics depend on timing and are excluded from the equality.
"""
import pytest

from support import assert_same_run as _assert_same, hedge_run

pytestmark = pytest.mark.gpu

OFF = {"RVM_HEDGE_MARK": "0"}
LAYOUTS = {"team_hint": {}, "two_teams": {"RVM_REFINE_TEAMS": "2"}, "one_team": {"RVM_REFINE_TEAMS": "1"},
           "one_block": {"RVM_REFINE_SPLIT": "0"}, "no_hedge": {"RVM_HEDGE": "0"},
           "one_hedge_group": {"RVM_HEDGE_GROUPS": "1"}}

_RUNS = {}


def _run(kind, env, iters):
    """test_gpu_hedge._run with the marks' counters as a sixth entry; computed once per (kind, env)."""
    return hedge_run(_RUNS, kind, env, iters, lambda ens: ens.plan.hedge_marks(reset=True))


@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_steady_state_bit_identical(layout):
    iters = 4
    on = _run("steady", LAYOUTS[layout], iters)
    off = _run("steady", {**LAYOUTS[layout], **OFF}, iters)
    print(f"[hedge mark {layout}] counters {on[3]} hedge on {on[4]} off {off[4]} marks on {on[5]} off {off[5]}")
    assert off[3]["refined"] > 0 and off[3]["truncated"] > 0
    assert on[3]["handoff_timeouts"] == off[3]["handoff_timeouts"] == 0
    _assert_same(on, off)
    assert on[4]["hedged"] == off[4]["hedged"] == {"no_hedge": 0, "one_hedge_group": 4 * 32}.get(layout, 4 * 256)
    # (the marks stop only blocks without a listed slot: what the hedge covers is replayed as before)
    if layout not in ("no_hedge", "one_hedge_group"):
        assert on[4]["replayed"] >= 1, on[4]
    assert off[5] == dict(marked=0, gave_up=0), off[5]
    blocks = {"no_hedge": 0, "one_hedge_group": 2}.get(layout, 16)
    assert 0 <= on[5]["gave_up"] <= on[5]["marked"] <= iters * blocks, on[5]
    if layout != "no_hedge":
        assert on[5]["marked"] > 0, on[5]
    # (whether a marked block is still integrating when its mark comes depends on timing: with teams the marks
    # come ~0.6 ms into hedge blocks that run ~1.1 ms, and 21-22 of 22 marked blocks stopped on them in every
    # run; with one block per group a run was seen in which none did)
    if layout == "team_hint":
        assert on[5]["gave_up"] > 0, on[5]


@pytest.mark.parametrize("n", [48, 64])
def test_smallest_shapes(n):
    on = _run(n, {}, 3)
    off = _run(n, OFF, 3)
    print(f"[hedge mark, {n} per half] counters {on[3]} hedge on {on[4]} off {off[4]} marks on {on[5]}")
    assert off[3]["refined"] > 0
    _assert_same(on, off)
    assert on[4]["hedged"] > 0 and off[4]["hedged"] > 0, (on[4], off[4])
    assert off[5] == dict(marked=0, gave_up=0), off[5]
    # (six half-steps of at most 2 x ceil(n / 32) hedge blocks each)
    assert 0 <= on[5]["gave_up"] <= on[5]["marked"] <= 6 * 2 * ((n + 31) // 32), on[5]
