"""What the side benchmarks share (chain_bench.py, summary_bench.py, gls_bench.py, pt_bench.py): bench.py's
workload -- the 2-planet state of mcmc_benchmark_mh.py:32, np.random.seed(2017), FakeObservation(Npoints=100,
error=1.5e-4, errorVar=2.5e-5, tmax=120), walkers from the ball theta0 + 1e-3 * scales * N(0,1), untimed burn-in
iterations to the steady state, a recorder on the walkers bench.py records -- and the ways they time and report.
Importing it puts the package and the oracle on sys.path; torch and the package load at first use.
"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "rvel-mcmc_amd"), os.path.join(ROOT, "oracle")):
    if p not in sys.path:
        sys.path.insert(0, p)

S2_PLANETS = [{"m": 1.2e-3, "a": 0.88, "h": 0.218, "k": 0.015, "l": 0.3},
              {"m": 2.1e-3, "a": 1.44 + 0.11, "h": 0.16, "k": 0.02, "l": 2.2}]
S2_SCALES = {"m": 1.5e-3, "a": 0.3, "h": 0.1, "k": 0.1, "l": np.pi / 2.}


def s2_problem():
    """(state, obs, scales) on device 0; seeds numpy's global generator, which ball() then draws from."""
    import torch

    from rvmcmc.observations import FakeObservation
    from rvmcmc.state import State

    torch.cuda.set_device(0)
    state = State(planets=[dict(p) for p in S2_PLANETS])
    np.random.seed(2017)
    obs = FakeObservation(state, Npoints=100, error=1.5e-4, errorVar=2.5e-5, tmax=120.)
    return state, obs, np.array([S2_SCALES[k] for k in state.get_rawkeys()])


def ball(state, scales, *shape):
    """Positions [*shape][Nvars] around the state's parameters."""
    return state.get_params() + 0.1e-2 * scales * np.random.normal(size=shape + (state.Nvars,))


def burn_in(sampler, n, name):
    """n untimed iterations, with a line to stderr when 20 s have passed since the last."""
    t_prog = time.perf_counter()
    for i in range(n):
        sampler.step()
        if i % 64 == 0 and time.perf_counter() - t_prog > 20.0:
            t_prog = time.perf_counter()
            print(f"{name}: burn-in iteration {i}", file=sys.stderr, flush=True)


def steady_ensemble(args, name):
    """(state, obs, ens): EnsembleSampler of args.walkers walkers after args.burn_in iterations from the ball."""
    from rvmcmc.ensemble import EnsembleSampler

    state, obs, scales = s2_problem()
    X0 = ball(state, scales, args.walkers)
    ens = EnsembleSampler(args.walkers, state, obs, seed=2017)
    ens.set_positions(X0)
    ens.compute_lnprob()
    burn_in(ens, args.burn_in, name)
    ens.check_faults()
    return state, obs, ens


def subset_recorder(ens, capacity):
    """An empty ChainRecorder on bench.py's recorded subset (every 4th of 4096 walkers), without lnprob."""
    from rvmcmc.chain import ChainRecorder

    return ChainRecorder(ens, capacity=capacity, walker_stride=max(1, ens.nloc // 512), lnprob=False)


def steady_recorder(args, name):
    """(state, obs, ens, rec): steady_ensemble, then args.chain_steps iterations into subset_recorder."""
    import torch

    state, obs, ens = steady_ensemble(args, name)
    rec = subset_recorder(ens, args.chain_steps)
    ens.run_mcmc(args.chain_steps, rec)
    ens.check_faults()
    torch.cuda.synchronize()
    print(f"{name}: chain recorded", file=sys.stderr, flush=True)
    return state, obs, ens, rec


def timed(fn):
    """(seconds, result) of fn(): host clock around a device synchronise."""
    import torch

    torch.cuda.synchronize()
    a = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - a, r


def repeat(fn, n):
    """(first call's seconds, the next n calls' seconds, the last result): the first call allocates and loads."""
    first, r = timed(fn)
    rest = []
    for _ in range(n):
        dt, r = timed(fn)
        rest.append(dt)
    return first, rest, r


def events(fn, n):
    """Seconds of n calls of fn() between device events, after one call that is not counted."""
    import torch

    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    out = []
    for _ in range(n + 1):
        ev[0].record()
        fn()
        ev[1].record()
        torch.cuda.synchronize()
        out.append(ev[0].elapsed_time(ev[1]) * 1e-3)
    return out[1:]


def emit(result, out=None):
    """The result as one JSON line: written to `out` when given, then printed."""
    line = json.dumps(result)
    if out:
        with open(out, "w") as f:
            f.write(line + "\n")
    print(line)
