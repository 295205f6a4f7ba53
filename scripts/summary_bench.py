#!/usr/bin/env python3
"""What the posterior summaries cost on the device against the host route they replace.

Workload: bench.py's -- the 2-planet state of mcmc_benchmark_mh.py:32, np.random.seed(2017),
FakeObservation(Npoints=100, error=1.5e-4, errorVar=2.5e-5, tmax=120), 4096 walkers from the ball
theta0 + 1e-3 * scales * N(0,1), --burn-in untimed iterations, then a --chain-steps chain of the walkers
bench.py records (every 4th of 4096).  On that chain, --repeat times each after a first call apart (it
allocates and loads the kernels):

  (i)   `summary`: recorder.summary(discard) -- rvm_chain_moments, rvm_rows_quantiles over the chain in
        place, rvm_chain_cov -- against the host's way: to_numpy() (the copy, timed apart), then np.quantile
        and np.cov on the [P][n W] samples.  The two sets of quantiles and covariances are compared.
  (ii)  `predict`: recorder.predict() on the 1000-point get_rv_plotting grid with 1024 samples against the
        host loop of scripts/posterior_ben21.py on the host copy of the chain: states picked with numpy,
        uploaded, one likelihood launch with rv_out, the RV matrix copied back, np.quantile per epoch.
  (iii) `select`: rvm_rows_quantiles alone on the chain (device events around the call): its achieved read
        bandwidth, passes x row bytes / time (8 passes over the retained steps), next to a torch copy of the
        same buffer timed in the same run (which reads AND writes every byte once).

Prints ONE JSON line and writes it to --out (profiles/summary_bench.json).  Figures are recorded, not
asserted.
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import side_bench
from side_bench import ROOT, emit, steady_recorder, timed
SELECT_PASSES = 8  # rvm_summary.hip: 8-bit digits of a 64-bit key


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--walkers", type=int, default=4096)
    ap.add_argument("--burn-in", type=int, default=4000, help="untimed iterations from the ball (bench.py's default)")
    ap.add_argument("--chain-steps", type=int, default=8000, help="recorded steps")
    ap.add_argument("--discard", type=int, default=1000, help="recorded steps left out of the summaries")
    ap.add_argument("--samples", type=int, default=1024, help="states behind the RV band")
    ap.add_argument("--grid", type=int, default=1000, help="epochs of the get_rv_plotting grid")
    ap.add_argument("--repeat", type=int, default=3, help="timed calls after the first")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "summary_bench.json"))
    return ap.parse_args()


def main():
    args = parse()
    import torch

    from rvmcmc import _lib, chain as chain_mod

    state, obs, ens, rec = steady_recorder(args, "summary_bench")
    W = args.walkers
    n, P, Wr, t0 = rec.n - args.discard, rec.n_params, rec.n_walkers, args.discard
    q = np.array(chain_mod.DEFAULT_Q)

    def repeat(fn):
        return side_bench.repeat(fn, args.repeat)

    def events(fn):
        return side_bench.events(fn, args.repeat)

    # ---- (i) summary() against to_numpy() + np.quantile + np.cov ------------------------------------------
    first, dev_s, sm = repeat(lambda: rec.summary(discard=t0))
    t_copy, c = timed(rec.to_numpy)                                   # [W][n][P]
    a = time.perf_counter()
    flat = np.ascontiguousarray(np.transpose(c[:, t0:], (2, 0, 1)).reshape(P, -1))  # [P][W n]
    t_flat = time.perf_counter() - a
    a = time.perf_counter()
    hq = np.quantile(flat, q, axis=1).T
    t_q = time.perf_counter() - a
    a = time.perf_counter()
    hc = np.cov(flat)
    t_c = time.perf_counter() - a
    host = t_copy + t_flat + t_q + t_c
    summary = {"steps": n, "walkers_recorded": Wr, "params": P, "chain_bytes": 8 * n * P * Wr,
               "device_first_call_s": first, "device_s": statistics.median(dev_s), "device_s_all": dev_s,
               "host_copy_s": t_copy, "host_layout_s": t_flat, "host_quantile_s": t_q, "host_cov_s": t_c,
               "host_total_s": host, "speedup": host / statistics.median(dev_s),
               "quantiles_max_rel_diff": float(np.max(np.abs(sm.quantiles - hq) / np.abs(hq))),
               "cov_max_rel_diff": float(np.max(np.abs(sm.cov - hc) / np.abs(hc))),
               "median": [float(v) for v in sm.quantiles[:, 2]], "sd": [float(v) for v in sm.sd]}
    print("summary_bench: summary done", file=sys.stderr, flush=True)

    # ---- (ii) predict() against the host loop ------------------------------------------------------------
    times = np.linspace(obs.tb[0], obs.tf[len(obs.tf) - 1], args.grid)  # State.get_rv_plotting's grid
    S = args.samples
    first, dev_s, bands = repeat(lambda: rec.predict(times, n_samples=S, discard=t0, seed=1))
    pobs = rec._epochs[1]  # (the host route gets the plan predict() built: neither side pays for it)

    def host_predict():
        rng = np.random.default_rng(1)
        ti, wi = rng.integers(t0, rec.n, S), rng.integers(0, Wr, S)
        X = torch.as_tensor(np.ascontiguousarray(c[wi, ti].T), device=rec.device)  # [P][S]
        _, st, rv = state.get_logp_batch(pobs, X, hill_factor=ens.hill_factor, want_rv=True, pmap=ens.pmap)
        ok = (st == 0).cpu().numpy()
        return np.quantile(rv.cpu().numpy()[:, ok], q, axis=1)

    h_first, host_s, hb = repeat(host_predict)
    width = bands.bands[3] - bands.bands[1]
    predict = {"epochs": len(times), "samples": S, "device_first_call_s": first, "device_s": statistics.median(dev_s),
               "device_s_all": dev_s, "host_loop_s": statistics.median(host_s), "host_loop_s_all": host_s,
               "host_copy_s": t_copy, "host_total_s": t_copy + statistics.median(host_s),
               "speedup_with_copy": (t_copy + statistics.median(host_s)) / statistics.median(dev_s),
               "speedup_without_copy": statistics.median(host_s) / statistics.median(dev_s),
               "n_valid_min": int(bands.n_valid.min()),
               "band68_width_median": float(np.median(width)),
               "median_curve_max_diff_in_band68_widths": float(np.max(np.abs(bands.bands[2] - hb[2]) / width))}
    print("summary_bench: predict done", file=sys.stderr, flush=True)

    # ---- (iii) the select alone, and a copy of the same bytes ----------------------------------------------
    x = rec.chain()[t0:]
    sel_s = events(lambda: chain_mod._rows_quantiles(rec.lib, x.data_ptr(), P, Wr, n, P * Wr, Wr, q, rec.device))
    dst = torch.empty_like(x)
    copy_s = events(lambda: dst.copy_(x))
    nbytes = 8 * n * P * Wr
    # (summary()'s other two launches, for the split of its time)
    mom_s = events(lambda: rec._moments(t0, rec.n, 0))
    center = rec._mean[0].mean(1).contiguous()
    cov = torch.empty((P, P), dtype=torch.float64, device=rec.device)
    ws = _lib.workspace(rec.lib.rvm_chain_cov_workspace_bytes(P, Wr), torch.float64, rec.device)
    cov_s = events(lambda: rec.lib.rvm_chain_cov(rec.chain().data_ptr(), P, Wr, t0, rec.n, center.data_ptr(),
                                                 cov.data_ptr(), ws.data_ptr(), torch.cuda.current_stream().cuda_stream))
    summary["device_moments_s"] = statistics.median(mom_s)
    summary["device_cov_s"] = statistics.median(cov_s)
    select = {"bytes": nbytes, "passes": SELECT_PASSES, "n_q": len(q), "select_s": statistics.median(sel_s),
              "select_s_all": sel_s, "select_read_GBps": SELECT_PASSES * nbytes / statistics.median(sel_s) / 1e9,
              "torch_copy_s": statistics.median(copy_s), "torch_copy_s_all": copy_s,
              "torch_copy_read_GBps": nbytes / statistics.median(copy_s) / 1e9,
              "torch_copy_read_plus_write_GBps": 2 * nbytes / statistics.median(copy_s) / 1e9,
              "timing": "device events around the call, median"}
    result = {"metric": "posterior summaries on the device against the host route (2-planet, 100 obs, 4096 walkers)",
              "walkers": W, "burn_in": args.burn_in, "chain_steps": rec.n, "discard": t0, "summary": summary,
              "predict": predict, "select": select}
    emit(result, args.out)


if __name__ == "__main__":
    main()
