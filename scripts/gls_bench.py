#!/usr/bin/env python3
"""What the residual periodogram costs on the device against the host route it replaces.

Workload: bench.py's -- the 2-planet state of mcmc_benchmark_mh.py:32, np.random.seed(2017),
FakeObservation(Npoints=100, error=1.5e-4, errorVar=2.5e-5, tmax=120), 4096 walkers from the ball
theta0 + 1e-3 * scales * N(0,1), --burn-in untimed iterations, then a --chain-steps chain of the walkers
bench.py records.  On that chain, for periodogram.freq_grid's default grid and one --finer times finer,
--repeat times each after a first call apart (it allocates and loads the kernels):

  `call`     recorder.residual_periodogram(grid, n_samples) -- draw, one likelihood launch with rv_out,
             rvm_gls_power twice (the residuals' and the data's own), rvm_rows_quantiles -- host clock around
             a device synchronise;
  `host`     the same rv matrix copied back, scipy.signal.lombscargle (weights, floating mean, normalised)
             looped over its columns, np.nanquantile per frequency; the largest difference of the two sets of
             bands;
  `kernels`  device events around rvm_gls_power on that matrix, around rvm_gls_basis alone on the same grid
             (the table kernel) and around rvm_gls_power of one model-less series (table + prepare, next to
             nothing else).  The product kernel is not an entry point of its own: its time is taken as the
             difference of the first and the last, which still holds the centre kernel's N S operations, 1 / F
             of the product's.  Its FP64 rate is 4 N F S flops over that time, against MI355X's 78.6 TFLOP/s
             vector FP64 peak.
  `product_large`  the same difference on the finer grid against --large-samples synthetic residual series, where
             the product is no longer launch-bound.

Prints ONE JSON line and writes it to --out (profiles/gls_bench.json).  Figures are recorded, not asserted.
"""
import argparse
import os
import statistics
import sys

import numpy as np
import side_bench
from side_bench import ROOT, emit, steady_recorder
PEAK_FP64_TFLOPS = 78.6  # MI355X vector FP64 (its matrix FP64 rate is the same)


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--walkers", type=int, default=4096)
    ap.add_argument("--burn-in", type=int, default=4000, help="untimed iterations from the ball (bench.py's default)")
    ap.add_argument("--chain-steps", type=int, default=1000, help="recorded steps")
    ap.add_argument("--samples", type=int, default=1024, help="states behind the bands")
    ap.add_argument("--finer", type=int, default=10, help="oversampling of the second grid over the default one")
    ap.add_argument("--large-samples", type=int, default=16384, help="series of the product kernel's own run")
    ap.add_argument("--repeat", type=int, default=5, help="timed calls after the first")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gls_bench.json"))
    return ap.parse_args()


def main():
    args = parse()
    import torch
    from scipy.signal import lombscargle

    from rvmcmc import _lib, engine, periodogram

    _, obs, _, rec = steady_recorder(args, "gls_bench")
    W = args.walkers

    lib = _lib.load()
    t, rvobs, er = engine.obs_arrays(obs)
    tau, w = periodogram.series_inputs(t, er)
    N, S = len(t), args.samples

    def repeat(fn):
        return side_bench.repeat(fn, args.repeat)

    def events(fn):
        return side_bench.events(fn, args.repeat)

    f0, df, F0 = periodogram.freq_grid(t)
    grids = {"default": (f0, df, F0), f"finer_x{args.finer}": (df / args.finer, df / args.finer, F0 * args.finer)}
    out = {}
    for name, grid in grids.items():
        F = grid[2]
        first, dev_s, pb = repeat(lambda: rec.residual_periodogram(grid=grid, n_samples=S, seed=1, return_samples=True))

        # ---- the host route on the same rv matrix ----
        def host():
            rv = pb.rv.cpu().numpy()
            ok = pb.status.cpu().numpy() == 0
            p = np.full((F, S), np.nan)
            for j in np.flatnonzero(ok):
                p[:, j] = lombscargle(t, rvobs - rv[:, j], 2.0 * np.pi * pb.freq, normalize=True, weights=1.0 / er ** 2,
                                      floating_mean=True)
            return np.nanquantile(p, pb.q, axis=1)

        h_first, host_s, hb = repeat(host)

        # ---- the launches alone ----
        dev = periodogram.upload_series(tau, w, rvobs, rec.device)
        model = pb.rv.contiguous()
        sh = torch.cuda.current_stream().cuda_stream
        f64 = dict(dtype=torch.float64, device=rec.device)
        power, freq = torch.empty((F, S), **f64), torch.empty(F, **f64)
        ws = torch.empty(lib.rvm_gls_workspace_bytes(N, F, S) // 8, **f64)
        cs, sn = torch.empty((F, N), **f64), torch.empty((F, N), **f64)

        def run_power(m, n_series):
            rc = lib.rvm_gls_power(dev[0].data_ptr(), dev[1].data_ptr(), N, dev[2].data_ptr(),
                                   m.data_ptr() if m is not None else 0, S, n_series, grid[0], grid[1], 0, F, 1,
                                   power.data_ptr(), S, freq.data_ptr(), ws.data_ptr(), sh)
            assert rc == 0, lib.rvm_last_error()

        def run_basis():
            rc = lib.rvm_gls_basis(dev[0].data_ptr(), N, grid[0], grid[1], 0, F, cs.data_ptr(), sn.data_ptr(),
                                   freq.data_ptr(), sh)
            assert rc == 0, lib.rvm_last_error()

        power_s = events(lambda: run_power(model, S))
        basis_s = events(run_basis)
        one_s = events(lambda: run_power(None, 1))
        product = statistics.median(power_s) - statistics.median(one_s)
        flops = 4.0 * N * F * S
        out[name] = {
            "n_obs": N, "n_freq": F, "samples": S, "f0": grid[0], "df": grid[1],
            "call_first_s": first, "call_s": statistics.median(dev_s), "call_s_all": dev_s,
            "host_s": statistics.median(host_s), "host_s_all": host_s,
            "speedup": statistics.median(host_s) / statistics.median(dev_s),
            "bands_max_abs_diff": float(np.nanmax(np.abs(pb.bands - hb))), "n_valid_min": int(pb.n_valid.min()),
            "median_band_peak_period_days": float(periodogram.period_days(pb.freq[np.argmax(pb.bands[2])])),
            "data_peak_period_days": float(periodogram.period_days(pb.freq[np.argmax(pb.data_power)])),
            "kernels": {"timing": "device events around the call, median",
                        "gls_power_s": statistics.median(power_s), "gls_power_s_all": power_s,
                        "gls_basis_s": statistics.median(basis_s), "gls_basis_s_all": basis_s,
                        "gls_power_one_series_s": statistics.median(one_s), "gls_power_one_series_s_all": one_s,
                        "product_s_by_difference": product, "product_flops": flops,
                        "product_fp64_TFLOPS": flops / product / 1e12,
                        "product_fraction_of_peak": flops / product / 1e12 / PEAK_FP64_TFLOPS,
                        "peak_fp64_TFLOPS": PEAK_FP64_TFLOPS}}
        print(f"gls_bench: {name} done", file=sys.stderr, flush=True)
    # ---- the product kernel where it is not launch-bound: the finer grid against --large-samples series -----
    SL, grid = args.large_samples, grids[f"finer_x{args.finer}"]
    F = grid[2]
    f64 = dict(dtype=torch.float64, device=rec.device)
    dev = periodogram.upload_series(tau, w, rvobs, rec.device)
    gen = torch.Generator(device=rec.device).manual_seed(1)
    model = dev[2][:, None] + 1e-4 * torch.randn((N, SL), generator=gen, **f64)
    power, ws = torch.empty((F, SL), **f64), torch.empty(lib.rvm_gls_workspace_bytes(N, F, SL) // 8, **f64)
    sh = torch.cuda.current_stream().cuda_stream

    def run_large(m, n_series):
        rc = lib.rvm_gls_power(dev[0].data_ptr(), dev[1].data_ptr(), N, dev[2].data_ptr(),
                               m.data_ptr() if m is not None else 0, SL, n_series, grid[0], grid[1], 0, F, 1,
                               power.data_ptr(), SL, 0, ws.data_ptr(), sh)
        assert rc == 0, lib.rvm_last_error()

    large_s = events(lambda: run_large(model, SL))
    one_s = events(lambda: run_large(None, 1))
    product = statistics.median(large_s) - statistics.median(one_s)
    flops = 4.0 * N * F * SL
    large = {"n_obs": N, "n_freq": F, "series": SL, "what": "synthetic residuals of the code's scale, device events",
             "gls_power_s": statistics.median(large_s), "gls_power_s_all": large_s,
             "gls_power_one_series_s": statistics.median(one_s), "product_s_by_difference": product,
             "product_flops": flops, "product_fp64_TFLOPS": flops / product / 1e12,
             "product_fraction_of_peak": flops / product / 1e12 / PEAK_FP64_TFLOPS}
    print("gls_bench: large product done", file=sys.stderr, flush=True)
    result = {"metric": "residual periodogram on the device against the host route (2-planet, 100 obs, 4096 walkers)",
              "walkers": W, "burn_in": args.burn_in, "chain_steps": rec.n, "grids": out, "product_large": large}
    emit(result, args.out)


if __name__ == "__main__":
    main()
