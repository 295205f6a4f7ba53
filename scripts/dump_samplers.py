"""Dump what the Python samplers compute, one .npz per case, to compare two versions of rvmcmc/ bit for bit.

A refactor of the Python layer must leave every launch as it was, so every array
below must come out equal from the package before and the package after, over one librvmcmc.so:

    RVM_LIB_PATH=.../librvmcmc.so PYTHONPATH=<dir holding the other rvmcmc/> \
        python scripts/dump_samplers.py OUT_A
    python scripts/dump_samplers.py OUT_B --restore OUT_A     # the ck_* cases continue OUT_A's checkpoints
    python scripts/dump_samplers.py --compare OUT_A OUT_B     # np.array_equal of every array; exit 1 if not

The package is the first `rvmcmc` on PYTHONPATH, else this tree's.  All cases run on the S2 two-planet
state and its synthetic observations (tests/conftest.py), on one stream:

    ens_fused / ens_spec / ens_three / ens_injected   EnsembleSampler, W = 64, 4 iterations: fused half-steps,
                      speculative iterations, the three-launch path with Philox and with injected draws
    rec               ChainRecorder(thin=2) over ens_fused: chain, tau, quantiles
    pt                PTSampler(3, 32, adapt=True, swap_every=1): 4 iterations, freeze, record, 2 more
    mh_fused / mh_unfused                             MhChains, 64 chains, 4 steps
    smala_<hessian>_<fused|separate>, smala_fixed_*   SmalaChains, 32 chains, 3 steps; fixed: resolve_tol = 0
    ck_ens / ck_pt / ck_mh / ck_smala                 2 steps, checkpoint (kept beside the .npz), 2 more; with
                      --restore DIR the first two steps are replaced by restoring DIR's checkpoint
"""
import argparse
import dataclasses
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle")]
sys.path.append(os.path.join(ROOT, "rvel-mcmc_amd"))  # (after PYTHONPATH: another rvmcmc/ wins)
import torch  # noqa: E402
from conftest import S2_PLANETS, S2_SCALES, s2_obs_oracle  # noqa: E402

from rvmcmc import engine  # noqa: E402
from rvmcmc.chain import ChainRecorder  # noqa: E402
from rvmcmc.ensemble import EnsembleSampler  # noqa: E402
from rvmcmc.mcmc import MhChains  # noqa: E402
from rvmcmc.smala import SmalaChains  # noqa: E402
from rvmcmc.state import State  # noqa: E402
from rvmcmc.tempering import PTSampler  # noqa: E402

W = 64


def _state(**integrator):
    s = State(planets=[dict(p) for p in S2_PLANETS])
    if integrator:
        s.integrator = dataclasses.replace(engine.DEFAULT_CONFIG, **integrator)
    return s


def _ball(s, shape, seed=0):
    sc = np.array([S2_SCALES[k] for k in s.get_rawkeys()])
    return s.get_params() + 1e-3 * sc * np.random.default_rng(seed).standard_normal(tuple(shape) + (s.Nvars,))


def _ens_out(e):
    f = e.plan.faults()
    return dict(positions=e.gather_positions(), lnprob=e.gather_lnprob(), naccepted=e._gather_int(e.naccepted),
                faults=np.array([f[k] for k in sorted(f)]))


def ensemble(mode, obs, record=False):
    s = _state()
    e = EnsembleSampler(W, s, obs, seed=1)
    e.set_positions(_ball(s, (W,)))
    e.speculative = mode == "spec"
    e.fused = mode in ("fused", "spec")
    rec = ChainRecorder(e, capacity=2, thin=2) if record else None
    if mode == "injected":
        e.compute_lnprob()
        rng = np.random.default_rng(5)
        for _ in range(4):
            for half in (0, 1):
                dp, da = (torch.as_tensor(rng.random(n), device="cuda") for n in (W, W // 2))
                e.half_step(e.pos[half], e.lnp[half], e.pos[1 - half], half, draws_propose=dp, draws_accept=da)
            e.iteration += 1
    else:
        e.run_mcmc(4, rec)
    out = _ens_out(e)
    if record:
        out = dict(chain=rec.chain().cpu().numpy(), tau=rec.diagnostics().tau, quantiles=rec.summary().quantiles)
    return out


def _pt_out(p):
    return dict(positions=p.positions(), lnprob=p.lnprob(), naccepted=p.naccepted.cpu().numpy(),
                nswapped=p.nswapped.cpu().numpy(), betas=p.ladder(), ratios=p.last_swap_ratios(),
                moments=p._moments.cpu().numpy())


def _pt(obs):
    s = _state()
    p = PTSampler(3, 32, s, obs, seed=3, adapt=True, swap_every=1)
    p.set_positions(_ball(s, (3, 32)))
    return p


def tempering(obs):
    p = _pt(obs)
    p.run_mcmc(4)
    p.freeze_ladder()
    p.record_lnprob(True)
    p.run_mcmc(2)
    return _pt_out(p)


def _mh(obs):
    return MhChains(_state(), obs, S2_SCALES, 1e-3, 64, seed=2)


def _mh_out(m):
    return dict(X=m.X.cpu().numpy(), lnp=m.lnp.cpu().numpy(), accepted=m.accepted.cpu().numpy())


def mh(fused, obs):
    m = _mh(obs)
    for _ in range(4):
        m.step(fused=fused)
    return _mh_out(m)


def _smala(obs, hessian="gauss-newton", **integrator):
    return SmalaChains(_state(**integrator), obs, eps=0.5, alpha=1e3, n_chains=32, seed=4, hessian=hessian)


def _smala_out(sm):
    out = dict(X=sm.X.cpu().numpy(), accepted=sm.accepted.cpu().numpy(), failures=sm.failures.cpu().numpy())
    out.update({"cache_" + k: v.cpu().numpy() for k, v in sm.cache.items() if k != "_c"})
    return out


def smala(hessian, fused, obs, **integrator):
    sm = _smala(obs, hessian, **integrator)
    for _ in range(3):
        sm.step(fused=fused)
    return _smala_out(sm)


def checkpointed(name, build, out_of, out_dir, restore):
    """2 steps and a checkpoint (or another run's checkpoint restored), then 2 more."""
    smp = build()
    if restore:
        smp.restore(os.path.join(restore, name + ".ckpt.npz"))
    else:
        smp.run_mcmc(2)
    smp.checkpoint(os.path.join(out_dir, name + ".ckpt.npz"))
    smp.run_mcmc(2)
    return out_of(smp)


def _ck_ens(obs):
    s = _state()
    e = EnsembleSampler(W, s, obs, seed=1)
    e.set_positions(_ball(s, (W,)))
    return e


def dump(out_dir, restore):
    os.makedirs(out_dir, exist_ok=True)
    obs = s2_obs_oracle()
    cases = {"ens_" + m: (lambda m=m: ensemble(m, obs)) for m in ("fused", "spec", "three", "injected")}
    cases["rec"] = lambda: ensemble("fused", obs, record=True)
    cases["pt"] = lambda: tempering(obs)
    cases.update({"mh_" + ("fused" if f else "unfused"): (lambda f=f: mh(f, obs)) for f in (True, False)})
    for f in (True, False):
        how = "fused" if f else "separate"
        for h in ("gauss-newton", "exact"):
            cases[f"smala_{h}_{how}"] = lambda h=h, f=f: smala(h, f, obs)
        cases[f"smala_fixed_{how}"] = lambda f=f: smala("gauss-newton", f, obs, resolve_tol=0.0)
    for name, build, out_of in (("ck_ens", lambda: _ck_ens(obs), _ens_out), ("ck_pt", lambda: _pt(obs), _pt_out),
                                ("ck_mh", lambda: _mh(obs), _mh_out), ("ck_smala", lambda: _smala(obs), _smala_out)):
        cases[name] = lambda a=(name, build, out_of): checkpointed(*a, out_dir, restore)
    for name, run in cases.items():
        np.savez(os.path.join(out_dir, name + ".npz"), **run())
        torch.cuda.synchronize()
        print("dumped", name, flush=True)


def compare(a, b):
    names = sorted(f for f in os.listdir(a) if f.endswith(".npz") and not f.endswith(".ckpt.npz"))
    bad = 0
    for f in names:
        x, y = np.load(os.path.join(a, f)), np.load(os.path.join(b, f))
        diff = [k for k in sorted(set(x.files) | set(y.files))
                if k not in x.files or k not in y.files or not np.array_equal(x[k], y[k], equal_nan=x[k].dtype.kind == "f")]
        print(f"{f[:-4]:28s} {len(x.files):2d} arrays  " + ("equal" if not diff else f"DIFFERENT: {diff}"), flush=True)
        bad += bool(diff)
    print(f"{len(names)} cases, {bad} different")
    return 1 if bad or not names else 0


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("out", nargs="?", help="directory for the .npz files")
    ap.add_argument("--restore", metavar="DIR", help="continue the ck_* cases from DIR's checkpoints")
    ap.add_argument("--compare", nargs=2, metavar=("A", "B"), help="compare two dumps instead of dumping")
    args = ap.parse_args()
    if args.compare:
        sys.exit(compare(*args.compare))
    if not args.out:
        ap.error("an output directory (or --compare A B)")
    dump(args.out, args.restore)
