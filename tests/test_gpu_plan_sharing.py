"""Which plans the four device samplers run on, when they are built over one observation set.

Every sampler takes its plan from engine.plan_for_state, which spells the plan cache's key -- device,
stream, planet count, step, levels, hint, inclination, resolve tuple -- in one place.  On the S2
two-planet state, on one stream, in this order:

    EnsembleSampler(64)      the adaptive plan on the main stream (room for 3 x 32 walker slots)
    MhChains(64 chains)      the same plan
    PTSampler(2, 32)         the same plan
    SmalaChains(32 chains)   its fixed-step plan (the stencil; resolve (0, 0)) on the main stream and its
                             centre plan (adaptive) on its side stream; 32 chains: the eager centre launch

so the observation set holds three plans, one per distinct (stream, resolve) -- the count the code
before the factory creates for these lines.  A spelling that drifted between two sites would add a
plan, split the three samplers' shared one, or have SmalaChains.check_faults read the counters of a plan
that none of its launches ran on.

The samplers are built and stepped once, in a fresh process (this file run as a script prints what it
found as one JSON line), so that the count is that of these lines alone and the suite's process is left
as it was.  Built in the suite's process, these plans -- every refining plan creates a side stream of
its own -- changed a timing a later test asserts on: tests/test_gpu_refine_tail.py's team_hint case saw
0 of 22 marked hedge blocks stop on their marks in two whole-suite runs, and 22 of 22 run alone, with
this package and with the one before it alike (supposed cause: which hardware queue a new stream gets
depends on how many the process has created).
"""
import json
import os
import subprocess
import sys

import pytest

from conftest import S2_SCALES
from support import s2_state_and_obs, tight_ball

pytestmark = pytest.mark.gpu


def build_and_step():
    import torch
    from rvmcmc import engine
    from rvmcmc.ensemble import EnsembleSampler
    from rvmcmc.mcmc import MhChains
    from rvmcmc.smala import SmalaChains
    from rvmcmc.tempering import PTSampler

    s, obs = s2_state_and_obs()
    X0 = tight_ball(s, (64,), 0)
    ens = EnsembleSampler(64, s, obs, seed=1)
    ens.set_positions(X0)
    mh = MhChains(s, obs, S2_SCALES, 1e-3, n_chains=64, seed=2)
    pt = PTSampler(2, 32, s, obs, seed=3)
    pt.set_positions(X0.reshape(2, 32, s.Nvars))
    sm = SmalaChains(s, obs, eps=0.5, alpha=1e3, n_chains=32, seed=4)
    for sampler in (ens, mh, pt, sm):
        sampler.step()
    torch.cuda.synchronize()
    plans = obs._rvm_plans
    out = dict(n_plans=len(plans), n_stream_resolve=len({(k[1], k[-1]) for k in plans}),
               shared=ens.plan is mh.plan is pt.plan, ops_plan=ens.ops.plan is ens.plan)
    # SMALA: the plans of its two launches, found again by a second look-up and read by check_faults()
    fixed, centre = sm._plan_keep, sm._cplan
    out.update(two_plans=fixed is not centre, fixed_tol=fixed.resolve_tol, centre_tol=centre.resolve_tol,
               fixed_again=sm._fixed_plan((2 * sm.P + 1) * sm.n) is fixed, centre_again=sm._center_plan() is centre)
    read, inner = [], engine.LoglPlan.check_faults

    def spy(plan, *args, **kwargs):
        read.append((plan, torch.cuda.current_stream(plan.device).cuda_stream))
        return inner(plan, *args, **kwargs)

    engine.LoglPlan.check_faults = spy
    try:
        faults = sm.check_faults()
    finally:
        engine.LoglPlan.check_faults = inner
    out.update(read_fixed_then_centre=[p for p, _ in read] == [fixed, centre],
               fixed_on_its_stream=read[0][1] == fixed.stream,
               centre_on_side_stream=read[1][1] == sm._side.cuda_stream == centre.stream,
               bad=int(faults["handoff_timeouts"] + faults["nonfinite"]), n_plans_after=len(plans))
    return out


@pytest.fixture(scope="module")
def found():
    p = subprocess.run([sys.executable, os.path.abspath(__file__)], stdout=subprocess.PIPE, timeout=120, check=True)
    return json.loads(p.stdout.decode().strip().splitlines()[-1])


def test_plan_count(found):
    assert found["n_plans"] == 3
    assert found["n_stream_resolve"] == 3  # one per (stream, resolve)


def test_stretch_mh_and_tempering_share_one_plan(found):
    assert found["shared"] and found["ops_plan"]


def test_smala_reads_the_plans_it_launched_on(found):
    assert found["two_plans"] and found["fixed_tol"] == 0.0 and found["centre_tol"] > 0.0
    assert found["fixed_again"]   # a second look-up: the stencil launch's plan
    assert found["centre_again"]  # and the centre launch's, under the side stream
    assert found["read_fixed_then_centre"] and found["fixed_on_its_stream"] and found["centre_on_side_stream"]
    assert found["bad"] == 0
    assert found["n_plans_after"] == found["n_plans"]  # none of the look-ups made a plan


if __name__ == "__main__":
    print(json.dumps(build_and_step()))
