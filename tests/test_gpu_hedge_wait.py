"""Team A's wait for a running hedge block (rvm_refine_impl.h hedge_wait_poll).

After pass 1, a team A whose open walkers' hedge blocks have ranked their slots but not yet stored pass 2 polls
for them before it publishes anything, and gives way when team B of the group arrives (or a needed block
stops, the group's done word is set, the safety bound passes).  RVM_HEDGE_WAIT at plan creation: 0 never waits
(the former path), unset or 1 waits, 2 skips the first look so that every trial goes through the poll loop --
deterministic coverage of the new path.  Nothing a caller sees may change: positions, log-probabilities, accept
counters and the plan's counters are those of a plan without the hedge (RVM_HEDGE=0), bit for bit, in every mode
and layout; rvm_plan_hedge_waits counts waited = late_hits + gave_way, all zero with the wait off and in the
layouts without teams.

The hedged instantiation of the refinement kernel (NW = 5) has no scratch, and the instantiations 4 and 8, which
every launch without a hedge runs, keep the register allocation of the commit before the wait (their source is
unchanged).  That commit's build (scripts/kernel_resources.py, gfx950), per (planets, D3), as
vgpr (AGPRs included) / agpr / vgpr_spill / sgpr_spill / scratch:
  NW = 4: (1, false) 343/87/16/887/0   (1, true) 364/108/16/969/0   (2, false) 384/128/20/1161/0
          (2, true) 404/148/20/1350/0  (3, false) 389/133/20/1373/0 (3, true) 411/155/20/1746/0
  NW = 8: (1, false) 256/0/103/924/356 (1, true) 256/0/119/1043/432 (2, false) 256/0/178/1156/512
          (2, true) 256/0/161/1370/556 (3, false) 256/0/159/1440/532 (3, true) 256/0/215/1737/600
"""
import os
import sys

import numpy as np
import pytest

from conftest import ROOT
from support import HEDGE_RUNS, LAYOUTS, OFF, assert_same_run, hedge_run, hedge_sampler, torch_or_fail, wide_walkers

gpu = pytest.mark.gpu

MODES = {"unset": None, "0": "0", "2": "2"}
ZERO = dict(waited=0, late_hits=0, gave_way=0)

# (vgpr, agpr, vgpr_spill, sgpr_spill, scratch) of refine_kernel<np, d3, nw> in the parent commit's build
PARENT = {
    (1, "false", 4): (343, 87, 16, 887, 0), (1, "true", 4): (364, 108, 16, 969, 0),
    (2, "false", 4): (384, 128, 20, 1161, 0), (2, "true", 4): (404, 148, 20, 1350, 0),
    (3, "false", 4): (389, 133, 20, 1373, 0), (3, "true", 4): (411, 155, 20, 1746, 0),
    (1, "false", 8): (256, 0, 103, 924, 356), (1, "true", 8): (256, 0, 119, 1043, 432),
    (2, "false", 8): (256, 0, 178, 1156, 512), (2, "true", 8): (256, 0, 161, 1370, 556),
    (3, "false", 8): (256, 0, 159, 1440, 532), (3, "true", 8): (256, 0, 215, 1737, 600),
}


def _waits(ens):
    return ens.plan.hedge_waits(reset=True)


def _sampler(X0, env):
    ens = hedge_sampler(X0, env)
    _waits(ens)
    return ens


_RUNS = {}


def _run(kind, layout, mode, iters):
    """As test_gpu_hedge._run, with the wait's mode set or unset at plan creation and its counters appended."""
    return hedge_run(_RUNS, kind, {**LAYOUTS[layout], "RVM_HEDGE_WAIT": MODES[mode]}, iters, _waits)


def _off(kind, layout, iters):
    """The run without the hedge, from (or into) test_gpu_hedge.py's cache."""
    return hedge_run(HEDGE_RUNS, kind, {**LAYOUTS[layout], **OFF}, iters)


def _check(tag, on, off):
    print(f"[hedge wait {tag}] counters {on[3]} hedge {on[4]} waits {on[5]}")
    assert_same_run(on, off)
    assert on[3]["handoff_timeouts"] == 0 and on[3]["nonfinite"] == off[3]["nonfinite"], on[3]
    w = on[5]
    assert w["waited"] == w["late_hits"] + w["gave_way"], w
    return w


@gpu
@pytest.mark.parametrize("mode", list(MODES))
def test_steady_state_bit_identical_with_teams(mode):
    off = _off("steady", "teams", 4)
    on = _run("steady", "teams", mode, 4)
    w = _check(f"steady teams mode {mode}", on, off)
    assert off[3]["refined"] > 0 and off[3]["handoff_timeouts"] == 0
    assert on[4]["hedged"] == 4 * 256, on[4]
    if mode == "0":
        assert w == ZERO, w
    if mode == "2":
        # (every commit passes through the poll loop, and the hedge holds a result in these iterations:
        # test_gpu_hedge sees replayed >= 1 here)
        assert on[4]["replayed"] >= 1 and w["late_hits"] >= 1, (on[4], w)


@gpu
@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("layout", ["split", "one_block"])
def test_steady_state_layouts_without_teams_never_wait(layout, mode):
    off = _off("steady", layout, 4)
    on = _run("steady", layout, mode, 4)
    w = _check(f"steady {layout} mode {mode}", on, off)
    assert w == ZERO, w
    assert on[4]["hedged"] == 4 * 256, on[4]


@gpu
@pytest.mark.parametrize("mode", ["unset", "2"])
@pytest.mark.parametrize("n", [48, 64])
def test_smallest_shapes(n, mode):
    """Every slot hedged, the last hedge group partial; groups mix ready, late and deeper (pass 3) walkers, so
    trials fail after a wait."""
    off = _off(n, "teams", 3)
    on = _run(n, "teams", mode, 3)
    _check(f"{n} per half mode {mode}", on, off)
    assert off[3]["refined"] > 0
    assert on[4]["hedged"] > 0, on[4]


@gpu
def test_hedged_launch_with_the_wait_captures_into_a_graph():
    """test_gpu_hedge.test_hedged_launch_captures_into_a_graph with every trial going through the poll loop:
    three replays of the captured launch give the bits of three plain launches without the hedge."""
    torch = torch_or_fail()
    X0 = wide_walkers(128, ball=0.3, seed=9)
    ens, ref = _sampler(X0, {"RVM_HEDGE_WAIT": "2"}), hedge_sampler(X0, OFF)
    ens.half_step(ens.pos[0], ens.lnp[0], ens.pos[1], 0)  # (a plain launch first: lazily created state is in place)
    ref.half_step(ref.pos[0], ref.lnp[0], ref.pos[1], 0)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            ens.half_step(ens.pos[0], ens.lnp[0], ens.pos[1], 0)
    torch.cuda.synchronize()
    for _ in range(3):
        g.replay()
        ref.half_step(ref.pos[0], ref.lnp[0], ref.pos[1], 0)
        torch.cuda.synchronize()
        np.testing.assert_array_equal(ens.pos[0].cpu().numpy(), ref.pos[0].cpu().numpy())
        np.testing.assert_array_equal(ens.lnp[0].cpu().numpy(), ref.lnp[0].cpu().numpy())
    np.testing.assert_array_equal(ens.naccepted.cpu().numpy(), ref.naccepted.cpu().numpy())
    assert ens.plan.faults() == ref.plan.faults()
    assert 0 < ens.plan.hedge_stats()["hedged"] <= 4 * 64
    w = ens.plan.hedge_waits()
    print(f"[hedge wait capture] waits {w}")
    assert w["waited"] == w["late_hits"] + w["gave_way"], w


def _resources():
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import kernel_resources as KR

    lib = os.path.join(ROOT, "rvel-mcmc_amd", "rvmcmc", "librvmcmc.so")
    if not os.path.exists(lib) or not os.path.exists(KR.READELF):
        pytest.skip("librvmcmc.so or llvm-readelf not available")
    ks = KR.kernels(lib)
    names = [n.split("(")[0].replace("void ", "") for n in KR.demangle([k["name"] for k in ks])]
    return dict(zip(names, ks))


@pytest.mark.parametrize("np_", [1, 2, 3])
@pytest.mark.parametrize("d3", ["false", "true"])
def test_hedged_instantiation_has_no_scratch(np_, d3):
    k = _resources()[f"rvm::refine_kernel<{np_}, {d3}, 5>"]
    assert k["scratch"] == 0, k
    assert k["max_wg"] == 256 and k["vgpr"] <= 512, k


@pytest.mark.parametrize("key", sorted(PARENT))
def test_other_instantiations_keep_the_parents_registers(key):
    np_, d3, nw = key
    k = _resources()[f"rvm::refine_kernel<{np_}, {d3}, {nw}>"]
    got = (k["vgpr"], k["agpr"], k["vgpr_spill"], k["sgpr_spill"], k["scratch"])
    assert got == PARENT[key], (key, got, PARENT[key])
