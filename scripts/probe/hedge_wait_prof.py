"""How late the hedged pass 2 arrives for team A (the RVM_PROFILE build, scripts/probe/librvmcmc_prof.so from
`make -C rvel-mcmc_amd profile`): the steady-state sampler of scripts/probe/steady_bench.py,
and for every refinement launch in which a team A had open walkers after pass 1 (rvm_refine_impl.h, the look
at the hedge): when the look came, when each hedge (group, direction) block it needed stored its completion
word -- or why it never did: no hedge index, stopped on its mark, cancelled, no record -- and when team B of
that group arrived at its wait with pass 2 done; for the hedge blocks, the time from entry to the first step
(the ranking prologue).  Times in us from the refinement kernel's first wave.  One JSON line per look, then a
summary line with the distributions (ITERS iterations, default 200)."""
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [os.path.join(ROOT, "rvel-mcmc_amd"), os.path.join(ROOT, "tests")]
import torch  # noqa: E402

from conftest import S2_PLANETS  # noqa: E402
from rvmcmc import _lib, engine  # noqa: E402

SLOTS, MAXW = 24, 4096


def quant(v):
    v = np.asarray(v, dtype=float)
    if not len(v):
        return None
    return {"n": int(len(v)), "mean": float(v.mean()),
            "q": [float(x) for x in np.quantile(v, [0, .1, .25, .5, .75, .9, 1])]}


def main():
    _lib.LIB_PATH = os.environ.get("RVM_LIB_PATH") or os.path.join(ROOT, "scripts", "probe", "librvmcmc_prof.so")
    lib = _lib.load()
    lib.rvm_rprof_copy.argtypes = [C.c_void_p, C.c_size_t]
    from rvmcmc.ensemble import EnsembleSampler
    from rvmcmc.observations import FakeObservation
    from rvmcmc.state import State

    state = State(planets=[dict(p) for p in S2_PLANETS])
    state.integrator = engine.IntegratorConfig(resolve_tol=5e-7)
    np.random.seed(2017)
    obs = FakeObservation(state, Npoints=100, error=1.5e-4, errorVar=2.5e-5, tmax=120.)
    X = np.load(os.path.join(ROOT, "scripts/probe/ens_it2000.npy"))
    ens = EnsembleSampler(len(X), state, obs, seed=2017)
    ens.set_positions(X)
    ens.compute_lnprob()
    for _ in range(3):
        ens.step()
    torch.cuda.synchronize()
    ens.plan.hedge_stats(reset=True)
    buf = np.zeros(MAXW * SLOTS, dtype=np.uint64)
    us = lambda x: float(x) / 100.0  # noqa: E731
    looks, prologue, hedge_start, hedge_len = [], [], [], []
    iters = int(os.environ.get("ITERS", "200"))
    for it in range(iters):
        lib.rvm_rprof_clear()
        torch.cuda.synchronize()
        ens.step()
        torch.cuda.synchronize()
        assert lib.rvm_rprof_copy(buf.ctypes.data, buf.nbytes) == 0
        b = buf.reshape(MAXW, SLOTS).astype(np.int64)
        b = b[b[:, 3] != 0]
        hb = b[((b[:, 9] >> 29) & 1) == 1]
        b = b[((b[:, 9] >> 29) & 1) == 0]
        if not len(b):
            continue
        t0 = b[:, 0].min()
        end = b[:, 3].max()
        if len(hb):
            hedge_start.append(us(hb[:, 0].min() - t0))
            for blk in set((hb[:, 9] & 0xFFFF).tolist()):
                r = hb[(hb[:, 9] & 0xFFFF) == blk]
                prologue.append(us((r[:, 1] - r[:, 0]).max()))
                hedge_len.append(us(r[:, 2].max() - r[:, 0].min()))
        team = (b[:, 9] >> 16) & 0xF
        grp = (b[:, 19] >> 32) & 0xFFFF
        for w in b[b[:, 18] != 0]:
            g = int((w[19] >> 32) & 0xFFFF)
            mask, untag = int(w[19] & 0xFFFF), int((w[19] >> 16) & 0xFF)
            barr = b[(team == 1) & (grp == g) & (b[:, 21] != 0)][:, 21]
            row = {"it": it, "group": g, "look_us": us(w[18] - t0), "took": int((w[19] >> 24) & 1),
                   "complete_at_look": int((w[19] >> 25) & 1), "no_index": untag,
                   "team_b_us": us(barr.max() - t0) if len(barr) else None,
                   "refine_end_us": us(end - t0), "blocks": []}
            for blk in range(16):
                if not (mask >> blk) & 1:
                    continue
                r = hb[(hb[:, 9] & 0xFFFF) == blk]
                e = {"block": blk, "wd": int((w[20] >> (4 * blk)) & 15)}
                if not len(r):
                    e["why"] = "no_record"
                elif r[:, 5].max() != 0:
                    e["complete_us"] = us(r[:, 5].max() - t0)
                    e["first_step_us"] = us(r[:, 1].max() - t0)
                    e["entry_us"] = us(r[:, 0].min() - t0)
                else:
                    e["why"] = "marked" if r[:, 4].max() else ("cancelled" if ((r[:, 9] >> 30) & 1).max() else "unfinished")
                row["blocks"].append(e)
            looks.append(row)
            print(json.dumps(row), flush=True)
    # the missed walker-directions (looks that did not take the hedge), by what became of their hedge block
    cls = dict.fromkeys(["no_index", "marked", "cancelled", "no_record", "unfinished", "complete_before_look",
                         "late_before_team_b", "late_after_team_b", "late_no_team_b_time"], 0)
    late_by, margin = [], []
    for r in looks:
        if r["took"]:
            continue
        cls["no_index"] += r["no_index"]
        for e in r["blocks"]:
            if "why" in e:
                cls[e["why"]] += e["wd"]
            elif e["complete_us"] <= r["look_us"]:
                cls["complete_before_look"] += e["wd"]
            elif r["team_b_us"] is None:
                cls["late_no_team_b_time"] += e["wd"]
            elif e["complete_us"] < r["team_b_us"]:
                cls["late_before_team_b"] += e["wd"]
                late_by += [e["complete_us"] - r["look_us"]] * e["wd"]
                margin += [r["team_b_us"] - e["complete_us"]] * e["wd"]
            else:
                cls["late_after_team_b"] += e["wd"]
    missed = sum(cls.values())
    # per look: would a wait have caught every needed block before team B arrived
    catch = [r for r in looks if not r["took"] and not r["no_index"] and r["team_b_us"] is not None and r["blocks"] and
             all("complete_us" in e and e["complete_us"] < r["team_b_us"] for e in r["blocks"])]
    print(json.dumps({"summary": True, "iterations": iters, "looks": len(looks),
                      "looks_taken": sum(r["took"] for r in looks),
                      "looks_complete_but_trial_failed": sum(1 for r in looks if not r["took"] and r["complete_at_look"]),
                      "missed_walker_directions": missed, "missed_by_cause": cls,
                      "share_missed_with_block_complete_before_team_b":
                          (cls["late_before_team_b"] + cls["complete_before_look"]) / max(1, missed),
                      "looks_a_wait_would_catch": len(catch),
                      "look_us": quant([r["look_us"] for r in looks]),
                      "team_b_us": quant([r["team_b_us"] for r in looks if r["team_b_us"] is not None]),
                      "late_by_us": quant(late_by), "team_b_minus_complete_us": quant(margin),
                      "catchable_saving_us": quant([r["team_b_us"] - max(e["complete_us"] for e in r["blocks"]) for r in catch]),
                      "hedge_entry_to_first_step_us": quant(prologue), "hedge_start_us": quant(hedge_start),
                      "hedge_block_length_us": quant(hedge_len),
                      "hedge_stats": ens.plan.hedge_stats(), "faults": ens.plan.faults(),
                      "lib": os.path.basename(_lib.LIB_PATH),
                      "hedge_wait_env": os.environ.get("RVM_HEDGE_WAIT")}), flush=True)


if __name__ == "__main__":
    main()
