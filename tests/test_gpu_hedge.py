"""The hedged second halving pass (rvm_refine_impl.h hedge_kernel).

A fused stretch launch whose likelihood grid leaves CUs idle runs halving pass 2 of the walker slots
with the quickest pericentre passages beside the likelihood kernel, and the refinement kernel replays
that pass from the hedge's results where they are complete instead of integrating it.  Nothing a
caller sees may change: positions, log-probabilities, accept counters and the plan's counters are
those of a plan without the hedge (RVM_HEDGE=0), bit for bit,

  * at the bench chain's steady state (scripts/probe/ens_it2000.npy, seed 2017, 4 iterations: the
    oracle has pass-2 slots in iterations 1, 2 and 3, at ranks 62, 201 and 90) in the refinement
    kernel's three layouts, with at least one walker-direction replayed;
  * with one hedge group only (RVM_HEDGE_GROUPS=1): the pass-2 walkers of ranks beyond 32 miss the hedge;
  * on wide-ball walkers (two-pass walkers, deeper ones, encounters, prior rejections) through fused
    half-steps of 48 and 64 walkers: every slot hedged, the last hedge group partial, refinement
    groups that mix hedged-ready and deeper walkers;
  * stream-ordered and capturable, as every launch (include/rvmcmc.h "Conventions").
The hedge kernel itself has no scratch.
"""
import os
import sys

import numpy as np
import pytest

from conftest import ROOT
from support import HEDGE_RUNS, LAYOUTS, OFF, assert_same_run as _assert_same, hedge_run, hedge_sampler as _sampler
from support import torch_or_fail as _torch, wide_walkers

gpu = pytest.mark.gpu


def _run(kind, env, iters):
    return hedge_run(HEDGE_RUNS, kind, env, iters)


@gpu
@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_steady_state_bit_identical(layout):
    on = _run("steady", LAYOUTS[layout], 4)
    off = _run("steady", {**LAYOUTS[layout], **OFF}, 4)
    print(f"[hedge {layout}] counters {on[3]} hedge {on[4]}")
    assert off[3]["refined"] > 0 and off[3]["truncated"] > 0 and off[3]["handoff_timeouts"] == 0
    assert off[4] == dict(hedged=0, replayed=0, missed=0)
    _assert_same(on, off)
    assert on[4]["hedged"] == 4 * 256, on[4]
    assert on[4]["replayed"] >= 1, on[4]


@gpu
@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_miss_and_mixed_paths(layout):
    one = _run("steady", {**LAYOUTS[layout], "RVM_HEDGE_GROUPS": "1"}, 4)
    off = _run("steady", {**LAYOUTS[layout], **OFF}, 4)
    print(f"[hedge {layout}, one group] hedge {one[4]}")
    _assert_same(one, off)
    assert one[4]["hedged"] == 4 * 32, one[4]


@gpu
@pytest.mark.parametrize("layout", list(LAYOUTS))
@pytest.mark.parametrize("n", [48, 64])
def test_smallest_shapes(n, layout):
    on = _run(n, LAYOUTS[layout], 3)
    off = _run(n, {**LAYOUTS[layout], **OFF}, 3)
    print(f"[hedge {layout}, {n} per half] counters {on[3]} hedge {on[4]}")
    assert off[3]["refined"] > 0
    _assert_same(on, off)
    assert on[4]["hedged"] > 0, on[4]


@gpu
def test_hedged_launch_is_complete_when_the_stream_is():
    """A hedged half-step on a stream of the caller's: right after that stream is synchronised the
    caller overwrites the complement half, which the hedge blocks read, with NaN; the half-step's
    results, and those of the next one on restored walkers, equal a plan's without the hedge."""
    torch = _torch()
    X0 = wide_walkers(128, ball=0.3, seed=7)
    cs = torch.cuda.Stream()
    with torch.cuda.stream(cs):
        ens = _sampler(X0, {})
    ref = _sampler(X0, OFF)
    for _ in range(2):
        with torch.cuda.stream(cs):
            ens.half_step(ens.pos[0], ens.lnp[0], ens.pos[1], 0)
        cs.synchronize()
        keep = ens.pos_aos[1].clone()
        with torch.cuda.stream(cs):
            ens.pos_aos[1].fill_(float("nan"))  # (the caller is done with the complement)
        ref.half_step(ref.pos[0], ref.lnp[0], ref.pos[1], 0)
        torch.cuda.synchronize()
        ens.pos_aos[1].copy_(keep)
        torch.cuda.synchronize()
        np.testing.assert_array_equal(ens.pos[0].cpu().numpy(), ref.pos[0].cpu().numpy())
        np.testing.assert_array_equal(ens.lnp[0].cpu().numpy(), ref.lnp[0].cpu().numpy())
    assert ens.plan.faults() == ref.plan.faults()
    assert 0 < ens.plan.hedge_stats()["hedged"] <= 2 * 64  # (every slot within the prior bounds)


@gpu
def test_hedged_launch_captures_into_a_graph():
    """A hedged half-step (fork, hedge kernel, likelihood kernel, refinement kernel, join, generation
    bump) captured into a graph: three replays give the bits of three plain launches without the hedge."""
    torch = _torch()
    X0 = wide_walkers(128, ball=0.3, seed=9)
    ens, ref = _sampler(X0, {}), _sampler(X0, OFF)
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
    assert 0 < ens.plan.hedge_stats()["hedged"] <= 4 * 64  # (every slot within the prior bounds)


@pytest.mark.parametrize("np_", [1, 2, 3])
@pytest.mark.parametrize("d3", ["false", "true"])
def test_hedge_kernel_has_no_scratch(np_, d3):
    """As the other kernels in tests/test_kernel_resources.py (the code object's metadata; no GPU needed)."""
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import kernel_resources as KR

    lib = os.path.join(ROOT, "rvel-mcmc_amd", "rvmcmc", "librvmcmc.so")
    if not os.path.exists(lib) or not os.path.exists(KR.READELF):
        pytest.skip("librvmcmc.so or llvm-readelf not available")
    ks = KR.kernels(lib)
    names = [n.split("(")[0].replace("void ", "") for n in KR.demangle([k["name"] for k in ks])]
    k = dict(zip(names, ks))[f"rvm::hedge_kernel<{np_}, {d3}>"]
    assert k["scratch"] == 0 and k["vgpr_spill"] == 0, k
    assert k["max_wg"] == 256, k
    # one wave per SIMD and the block alone on its CU: its static LDS leaves the dynamic request (the
    # CU's remainder, rvm_refine_impl.h hedge_budget) room for the slots' keys
    assert k["lds"] <= 32 * 1024, k
