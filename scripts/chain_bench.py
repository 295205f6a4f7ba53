#!/usr/bin/env python3
"""What recording a chain on the device costs, and what its diagnostics cost against the host's.

Workload: bench.py's -- the 2-planet state of mcmc_benchmark_mh.py:32, np.random.seed(2017),
FakeObservation(Npoints=100, error=1.5e-4, errorVar=2.5e-5, tmax=120), 4096 walkers from the ball
theta0 + 1e-3 * scales * N(0,1), --burn-in untimed iterations to the steady state.  Then

  (i)  `record`: --rounds times, alternating, --steps iterations of the bare loop `for: ens.step()` and
       the same number through ens.run_mcmc(steps, recorder) recording EVERY step of ALL walkers
       (rvm_chain_record, two launches per iteration); host clock around a device synchronise; the median
       ms per iteration of each and every round's figures (the spread).
  (ii) `diagnostics`: a --chain-steps chain of the walkers bench.py records (every 4th of 4096), then
       recorder.diagnostics() (rvm_chain_moments + rvm_chain_autocov for the lags up to the first Sokal
       window; --repeat times, the first one apart as it allocates) against the host's way: the whole chain
       copied to the host and driver.ess (numpy FFT over all lags), copy and FFT timed separately.  The two
       sets of tau are compared.

Prints ONE JSON line and writes it to --out (profiles/chain_diag_bench.json).  Figures are recorded, not
asserted.
"""
import argparse
import os
import statistics
import time

import numpy as np
from side_bench import ROOT, emit, steady_ensemble, subset_recorder, timed


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--walkers", type=int, default=4096)
    ap.add_argument("--burn-in", type=int, default=4000, help="untimed iterations from the ball (bench.py's default)")
    ap.add_argument("--steps", type=int, default=200, help="iterations per timed window of part (i)")
    ap.add_argument("--rounds", type=int, default=5, help="alternating (bare, recorded) window pairs")
    ap.add_argument("--chain-steps", type=int, default=8000, help="recorded steps of part (ii)")
    ap.add_argument("--repeat", type=int, default=3, help="timed diagnostics() calls after the first")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "chain_diag_bench.json"))
    return ap.parse_args()


def main():
    args = parse()
    import torch

    from rvmcmc import driver
    from rvmcmc.chain import ChainRecorder

    _, _, ens = steady_ensemble(args, "chain_bench")
    W = args.walkers

    # ---- (i) the bare loop against run_mcmc with a recorder, alternating ------------------------------
    rec = ChainRecorder(ens, capacity=(args.rounds + 1) * args.steps)

    def bare():
        for _ in range(args.steps):
            ens.step()

    bare()
    ens.run_mcmc(args.steps, rec)  # (warm: both paths once, the recorder's kernel loaded)
    bare_ms, rec_ms = [], []
    for _ in range(args.rounds):
        bare_ms.append(1e3 * timed(bare)[0] / args.steps)
        rec_ms.append(1e3 * timed(lambda: ens.run_mcmc(args.steps, rec))[0] / args.steps)
    b, r = statistics.median(bare_ms), statistics.median(rec_ms)
    record = {"steps_per_window": args.steps, "rounds": args.rounds, "walkers_recorded": rec.n_walkers,
              "bytes_per_iteration": 8 * rec.n_walkers * (rec.n_params + 1),
              "bare_ms_per_iteration": b, "recorded_ms_per_iteration": r, "overhead_fraction": r / b - 1.0,
              "bare_ms_rounds": bare_ms, "recorded_ms_rounds": rec_ms,
              "timing": "host clock around a device synchronise, median over the rounds"}
    del rec
    torch.cuda.empty_cache()

    # ---- (ii) diagnostics() against the copy to the host and driver.ess --------------------------------
    rec = subset_recorder(ens, args.chain_steps)
    t_run = timed(lambda: ens.run_mcmc(args.chain_steps, rec))[0]
    ens.check_faults()
    first = timed(lambda: rec.diagnostics())[0]
    diag_s = []
    for _ in range(args.repeat):
        t0 = time.perf_counter()
        d = rec.diagnostics()
        diag_s.append(time.perf_counter() - t0)  # (diagnostics() ends in copies to the host: synchronised)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    c = rec.chain().permute(0, 2, 1).cpu().numpy()  # [steps][walkers][P], as bench.py hands it to driver.ess
    t_copy = time.perf_counter() - t0
    t0 = time.perf_counter()
    _, taus = driver.ess(c)
    t_fft = time.perf_counter() - t0
    diag = {"chain_steps": rec.n, "walkers_recorded": rec.n_walkers, "walker_stride": rec.walker_stride,
            "run_mcmc_ms_per_iteration": 1e3 * t_run / args.chain_steps,
            "diagnostics_first_call_s": first, "diagnostics_s": statistics.median(diag_s), "diagnostics_s_all": diag_s,
            "host_copy_s": t_copy, "host_driver_ess_s": t_fft, "host_total_s": t_copy + t_fft,
            "speedup": (t_copy + t_fft) / statistics.median(diag_s),
            "tau": [float(v) for v in d.tau], "window": [int(v) for v in d.window],
            "tau_host": [float(v) for v in taus],
            "tau_max_rel_diff": float(np.max(np.abs(d.tau - taus) / np.abs(taus))),
            "rhat_max": float(np.max(d.rhat)), "long_enough": d.long_enough,
            "ess_min_recorded_walkers": float(np.min(d.ess))}
    result = {"metric": "chain recording overhead and diagnostics time (2-planet, 100 obs, 4096 walkers, steady state)",
              "walkers": W, "burn_in": args.burn_in, "record": record, "diagnostics": diag}
    emit(result, args.out)


if __name__ == "__main__":
    main()
