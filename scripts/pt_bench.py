#!/usr/bin/env python3
"""Throughput of the parallel-tempering ensemble (rvmcmc.tempering.PTSampler) on one MI355X, next to
the untempered ensemble's three-launch path at the same number of likelihood slots per launch.

Workload: bench.py's -- the 2-planet state of mcmc_benchmark_mh.py:32, np.random.seed(2017),
FakeObservation(Npoints=100, error=1.5e-4, errorVar=2.5e-5, tmax=120), the initial ball theta0 +
1e-3 * scales * N(0,1), --burn-in untimed iterations to the steady state, W warmup and K timed
iterations -- with
  * `pt`:       T = 8 temperatures x W = 512 walkers on the default ladder, an exchange sweep every
                iteration: two likelihood launches of T W / 2 = 2048 walkers per iteration;
  * `ensemble`: EnsembleSampler at 4096 walkers with fused = False (propose / likelihood / accept
                launches): two likelihood launches of 2048 walkers per iteration as well.
Each part runs in a child process of its own under its own time limit; a part that fails or runs
out of time ends the run (nothing more is started on the GPU).  Prints ONE JSON line.  The figures
are recorded (profiles/pt_bench.json), not asserted: hot temperatures propose wider moves, which
need more of the adaptive resolution's refinement per evaluation.

--adapt runs the `pt` part alone with the ladder adapting through the burn-in (PTSampler(adapt=True),
ptemcee's default lag and time unless given), freezes the ladder, times as above, then records the
lnp moments for --steps more iterations (mean lnp, the thermodynamic integral), and sets the figures
against the fixed ladder's in profiles/pt_bench.json.  It writes the line to --out
(profiles/pt_adapt_bench.json) as well.
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np
from side_bench import ROOT, ball, burn_in, emit, s2_problem

COUNTERS = ("refined", "unresolved", "nonfinite", "handoff_timeouts")


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ntemps", type=int, default=8)
    ap.add_argument("--walkers", type=int, default=512, help="walkers per temperature")
    ap.add_argument("--ensemble-walkers", type=int, default=4096, help="walkers of the untempered comparison")
    ap.add_argument("--swap-every", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--burn-in", type=int, default=4000, help="untimed iterations from the ball (bench.py's default)")
    ap.add_argument("--part-timeout", type=float, default=900.0,
                    help="seconds each part's process may take (the ladder's 4000-iteration burn-in alone takes "
                         "about ten minutes: the hot temperatures' first few hundred iterations out of the tight "
                         "ball run at 0.1-0.3 s each)")
    ap.add_argument("--adapt", action="store_true", help="adapt the ladder during the burn-in, then freeze it")
    ap.add_argument("--adaptation-lag", type=float, default=10000.0)
    ap.add_argument("--adaptation-time", type=float, default=100.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pt_adapt_bench.json"),
                    help="where --adapt writes its line")
    ap.add_argument("--part", choices=("pt", "ensemble"), default=None, help="(internal) run one part in this process")
    return ap.parse_args()


def run_part(args):
    import torch

    from rvmcmc.ensemble import EnsembleSampler
    from rvmcmc.tempering import PTSampler

    state, obs, scales = s2_problem()
    if args.part == "pt":
        T, W = args.ntemps, args.walkers
        X0 = ball(state, scales, T, W)
        smp = PTSampler(T, W, state, obs, seed=2017, swap_every=args.swap_every, adapt=args.adapt,
                        adaptation_lag=args.adaptation_lag, adaptation_time=args.adaptation_time)
        betas_start = [float(b) for b in smp.betas]
        nwalk = T * W
    else:
        T, W = 1, args.ensemble_walkers
        X0 = ball(state, scales, W)
        smp = EnsembleSampler(W, state, obs, seed=2017)
        smp.fused = False
        nwalk = W
    # the plan's counters are read here and reported; the periodic check would raise on the first
    # walker the adaptive resolution leaves UNRESOLVED, which a hot temperature may well propose
    smp.fault_check_every = 0
    smp.set_positions(X0)
    smp.compute_lnprob()
    t_burn = time.perf_counter()
    burn_in(smp, args.burn_in, f"pt_bench[{args.part}]")
    if args.part == "pt" and args.adapt:
        smp.freeze_ladder()  # the warmup and the timed iterations run on the adapted, fixed ladder
    for _ in range(args.warmup):
        smp.step()
    burn = smp.plan.faults(reset=True)
    t_burn = time.perf_counter() - t_burn
    if args.part == "pt":
        acc0, sw0, nsw0 = smp.naccepted.clone(), smp.nswapped.clone(), smp.nswaps
    else:
        acc0 = smp.naccepted.clone()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        smp.step()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    f = smp.plan.faults(reset=True)
    out = {"walkers_per_launch": nwalk // 2, "evals_per_s": nwalk * args.steps / dt,
           "ms_per_iteration": 1e3 * dt / args.steps, "steps": args.steps, "warmup": args.warmup,
           "burn_in": args.burn_in, "burn_in_and_warmup_s": t_burn,
           "per_iteration": {k: f[k] / float(args.steps) for k in COUNTERS},
           "burn_in_totals": {k: int(burn[k]) for k in COUNTERS}}
    if args.part == "pt":
        lnp = smp.lnprob()
        acc = (smp.naccepted - acc0).view(2, T, W // 2).sum((0, 2)).cpu().numpy() / float(W * args.steps)
        sweeps = max(smp.nswaps - nsw0, 1)
        out.update(ntemps=T, walkers=W, swap_every=args.swap_every, betas=[float(b) for b in smp.betas],
                   acceptance=[float(a) for a in acc],
                   swap_fraction=[float(v) for v in (smp.nswapped - sw0).sum(1).cpu().numpy() / float(sweeps * W)],
                   mean_lnprob=[float(v) for v in lnp.mean(1)], all_lnprob_finite=bool(np.isfinite(lnp).all()))
        if args.adapt:
            out.update(adapt=True, adaptation_lag=args.adaptation_lag, adaptation_time=args.adaptation_time,
                       betas_start=betas_start, ladder_updates=smp.nadapt, ladder_refusals=smp.ladder_refusals())
            smp.record_lnprob(True)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                smp.step()
            torch.cuda.synchronize()
            out["ms_per_iteration_recording"] = 1e3 * (time.perf_counter() - t0) / args.steps
            mean, std = smp.mean_lnprob()
            est, coarse = smp.log_evidence_ratio()
            out.update(recorded_mean_lnprob=[float(v) for v in mean], recorded_std_lnprob=[float(v) for v in std],
                       log_evidence_ratio=est, log_evidence_ratio_coarse=coarse)
    else:
        out.update(walkers=W, fused=False,
                   acceptance=float((smp.naccepted - acc0).sum().item()) / float(W * args.steps))
    print(json.dumps(out), flush=True)


def main():
    args = parse()
    if args.part is not None:
        run_part(args)
        return
    result = {"metric": "walker-logL evals/sec, parallel-tempering ensemble (2-planet, 100 obs, steady state)",
              "unit": "evals/s"}
    for part in (("pt",) if args.adapt else ("pt", "ensemble")):
        cmd = [sys.executable, os.path.abspath(__file__), "--part", part] + sys.argv[1:]
        try:
            p = subprocess.run(cmd, stdout=subprocess.PIPE, timeout=args.part_timeout, check=False)
        except subprocess.TimeoutExpired:
            sys.exit(f"pt_bench: part '{part}' exceeded its {args.part_timeout:.0f} s limit; stopping")
        if p.returncode != 0:
            sys.exit(f"pt_bench: part '{part}' ended with status {p.returncode}; stopping")
        result[part] = json.loads(p.stdout.decode().strip().splitlines()[-1])
    result["value"] = result["pt"]["evals_per_s"]
    if args.adapt:
        with open(os.path.join(ROOT, "profiles", "pt_bench.json")) as f:
            fixed = json.load(f)["pt"]
        result["fixed_ladder"] = {k: fixed[k] for k in ("betas", "swap_fraction", "ms_per_iteration", "evals_per_s")}
        result["min_swap_fraction"] = min(result["pt"]["swap_fraction"])
        result["fixed_ladder_min_swap_fraction"] = min(fixed["swap_fraction"])
    else:
        result["pt_over_ensemble"] = result["pt"]["evals_per_s"] / result["ensemble"]["evals_per_s"]
    emit(result, args.out if args.adapt else None)


if __name__ == "__main__":
    main()
