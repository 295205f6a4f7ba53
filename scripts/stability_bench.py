#!/usr/bin/env python3
"""What the stability screen costs on the device, per step, against the host route it replaces.

Workload: bench.py's posterior -- the 2-planet state of mcmc_benchmark_mh.py:32 sampled from the ball after
--burn-in untimed iterations, --chain-steps recorded -- and --samples states drawn from it.  For 2 planets those
states; for 3 planets the same states with a third planet (m = 1e-3, a = 2.6, h = 0.05, l = 1) added to each.

  `device`  rvm_stability_advance over --orbits orbits of the shortest period at --steps-per-orbit steps each, in
            one launch, device events around it (median of --repeat after one launch apart): Wisdom-Holman steps
            per second of one state and of all states together; `screen_call_s` the whole of
            stability.screen / ChainRecorder.stability for 2 planets, host clock, its chunking and reads included;
  `host`    tests/wh_ref.py's float run (the same map, one state after another on one CPU core) of the first
            --host-states states over --host-steps steps: steps per second of one state.
  `chunk`   the steps one launch of the 2-planet states runs in a second at the measured rate: what
            stability.DEFAULT_CHUNK_STEPS is chosen under.

Prints ONE JSON line and writes it to --out (profiles/stability_bench.json).  Figures are recorded, not asserted.
"""
import argparse
import math
import os
import statistics
import sys
import time

import numpy as np
import side_bench
from side_bench import ROOT, emit, steady_recorder

sys.path.insert(0, os.path.join(ROOT, "tests"))

THIRD = [1e-3, 2.6, 0.05, 0.0, 1.0]  # kernel rows m, a, h, k, l of the planet added for the 3-planet run


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--walkers", type=int, default=4096)
    ap.add_argument("--burn-in", type=int, default=4000, help="untimed iterations from the ball (bench.py's default)")
    ap.add_argument("--chain-steps", type=int, default=100, help="recorded steps")
    ap.add_argument("--samples", type=int, default=1024, help="states screened")
    ap.add_argument("--orbits", type=float, default=1e4)
    ap.add_argument("--steps-per-orbit", type=int, default=20)
    ap.add_argument("--repeat", type=int, default=3, help="timed launches after the first")
    ap.add_argument("--host-states", type=int, default=8)
    ap.add_argument("--host-steps", type=int, default=200)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "stability_bench.json"))
    return ap.parse_args()


def host_rate(K, n_planets, hill, h, n_states, n_steps):
    """Steps per second of one state: wh_ref.WH in float, K(h/2) [D K]^(n - 1) D K(h/2), one state after another."""
    import wh_ref as W

    cnt = [0, 0]
    t0 = time.perf_counter()
    for j in range(n_states):
        pl = [[float(K[5 * p + q, j]) for q in range(5)] + [0.0, 0.0] for p in range(n_planets)]
        s = W.WH(pl, False, hill)
        s.kick(h / 2)
        for i in range(n_steps):
            s.drift(h, cnt)
            s.kick(h / 2 if i == n_steps - 1 else h)
    return n_states * n_steps / (time.perf_counter() - t0)


def main():
    args = parse()
    import torch

    from rvmcmc import _lib, stability

    state, _, ens, rec = steady_recorder(args, "stability_bench")
    S = args.samples
    X, _ = rec.draw(S, 0, 1)
    K2 = ens.pmap.to_kernel(X).contiguous()
    third = torch.tensor(THIRD, dtype=torch.float64, device=K2.device)[:, None].expand(-1, S)
    hf = ens.hill_factor
    se = max(1, args.steps_per_orbit // 4)
    out = {}
    for npl, K in ((2, K2), (3, torch.cat([K2, third], 0).contiguous())):
        P, a, valid = stability.kepler_periods(K, npl, False)
        p_min, a_big = float(P[valid].min()), float(a[valid].max())
        h = p_min / args.steps_per_orbit
        blocks = math.ceil(args.orbits * args.steps_per_orbit / se)
        steps = blocks * se

        def launch():
            sc = stability.Screen(K, npl, False, hf).init()
            torch.cuda.synchronize()
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
            ev[0].record()
            sc.advance(h, se, blocks, 100.0 * a_big)
            ev[1].record()
            torch.cuda.synchronize()
            return ev[0].elapsed_time(ev[1]) * 1e-3, sc

        times = [launch() for _ in range(args.repeat + 1)]
        secs, sc = [t for t, _ in times[1:]], times[-1][1]
        med = statistics.median(secs)
        status = sc.status.cpu().numpy()
        done = int(sc.steps.sum().item())
        Kh = K.cpu().numpy()
        cpu = host_rate(Kh, npl, hf, h, args.host_states, args.host_steps)
        out[f"{npl}_planets"] = {
            "states": S, "steps_per_state": steps, "sample_every": se, "h": h, "orbits": args.orbits,
            "advance_s": med, "advance_s_all": secs, "advance_first_s": times[0][0],
            "fraction_ok": float(np.mean(status == _lib.RVM_STATUS_OK)), "state_steps_done": done,
            "steps_per_s_per_state": steps / med, "steps_per_s_aggregate": done / med,
            "host_float_steps_per_s_per_state": cpu, "host_states": args.host_states, "host_steps": args.host_steps,
            "aggregate_speedup_over_one_core": done / med / cpu}
        print(f"stability_bench: {npl} planets done", file=sys.stderr, flush=True)
    first, call_s, res = side_bench.repeat(
        lambda: rec.stability(n_samples=S, seed=1, orbits=args.orbits, steps_per_orbit=args.steps_per_orbit),
        args.repeat)
    rate = out["2_planets"]["steps_per_s_per_state"]
    result = {"metric": "stability screen on the device: Wisdom-Holman steps per second (bench posterior)",
              "walkers": args.walkers, "burn_in": args.burn_in, "chain_steps": rec.n, **out,
              "screen_call_first_s": first, "screen_call_s": statistics.median(call_s), "screen_call_s_all": call_s,
              "screen_fraction_stable": res.fraction_stable,
              "chunk": {"steps_in_one_second_at_the_measured_rate": rate,
                        "default_chunk_steps": stability.DEFAULT_CHUNK_STEPS,
                        "default_chunk_s": stability.DEFAULT_CHUNK_STEPS / rate}}
    emit(result, args.out)


if __name__ == "__main__":
    main()
