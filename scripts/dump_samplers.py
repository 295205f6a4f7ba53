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
    rec               ChainRecorder(thin=2) over ens_fused: chain, tau, quantiles; predict() and
                      residual_periodogram() over 64 drawn states, every field
    pt                PTSampler(3, 32, adapt=True, swap_every=1): 4 iterations, freeze, record, 2 more
    mh_fused / mh_unfused                             MhChains, 64 chains, 4 steps
    smala_<hessian>_<fused|separate>, smala_fixed_*   SmalaChains, 32 chains, 3 steps; fixed: resolve_tol = 0
    ck_ens / ck_pt / ck_mh / ck_smala                 2 steps, checkpoint (kept beside the .npz), 2 more; with
                      --restore DIR the first two steps are replaced by restoring DIR's checkpoint

and the read-outs on synthetic, fixed-seed inputs at the edges of the pieces they share:

    ro_chain          a chain [70][3][300]: moments, autocovariance over lag_blocks(70), summary(), draw(33)
    ro_quantiles      rvm_rows_quantiles through both load paths, an all-NaN row among the rows
    ro_gls            rvm_gls_power at N = 5 and 6, F = 65, S = 129, float_mean on and off, a NaN model column
    ro_ladder         rvm_pt_ladder_update at T = 3, W = 260 with the moments
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

from rvmcmc import _lib, engine, periodogram  # noqa: E402
from rvmcmc.chain import ChainRecorder, _rows_quantiles, lag_blocks  # noqa: E402
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
        t = engine.obs_arrays(obs)[0]
        out.update(_fields("predict_", rec.predict(np.linspace(t.min(), t.max(), 37), n_samples=64, seed=2,
                                                   return_samples=True)))
        out.update(_fields("residual_", rec.residual_periodogram(n_samples=64, seed=2, return_samples=True)))
    return out


def _fields(prefix, result):
    """Every field of a result dataclass as a host array (device tensors copied)."""
    d = {prefix + f.name: getattr(result, f.name) for f in dataclasses.fields(result)}
    return {k: v.cpu().numpy() if torch.is_tensor(v) else np.asarray(v) for k, v in d.items() if v is not None}


Q7 = (0.0, 0.025, 0.16, 0.5, 0.84, 0.975, 1.0)


def _f64(a, device="cuda"):
    return torch.as_tensor(np.ascontiguousarray(a, dtype=np.float64), device=device)


def ro_chain():
    """A synthetic chain [70][3][300]: two walker blocks of 256 with a partial one, the lags 0 .. 69 over tiles of 16
    with a partial one, an odd parameter count over the covariance's tiles of 2."""
    class Held:  # what a ChainRecorder asks of a sampler: a device and a segment's shape
        device = torch.device("cuda", torch.cuda.current_device())

        def _chain_segments(self):
            return [dict(x=torch.zeros((3, 300), dtype=torch.float64, device=self.device), n=300)]

    rec = ChainRecorder(Held(), capacity=70, lnprob=False)
    x = np.cumsum(np.random.default_rng(11).standard_normal((70, 3, 300)), 0)  # (random walks: the lags correlate)
    rec._chain.copy_(_f64(x * np.array([1.0, 1e-3, 40.0])[:, None] + np.array([0.5, -2.0, 1e3])[:, None]))
    rec.n = 70
    mean, m2 = (v.clone() for v in rec._moments(0, 70, 0))
    acov = np.concatenate([rec.autocov(0, 70, lo, hi - lo, mean).cpu().numpy() for lo, hi in lag_blocks(70)], 1)
    X, idx = rec.draw(33, discard=5, seed=9, draw_id=2)
    out = dict(mean=mean.cpu().numpy(), m2=m2.cpu().numpy(), acov=acov, draw_X=X.cpu().numpy(),
               draw_idx=idx.cpu().numpy())
    out.update(_fields("summary_", rec.summary(discard=5, q=Q7)))
    # the quantiles on the chain in place: 16-byte aligned, even strides -- the wide loads
    P, W = rec.n_params, rec.n_walkers
    qa, na = _rows_quantiles(rec.lib, rec._chain.data_ptr(), P, W, 70, P * W, W, np.array(Q7), rec.device)
    out.update(chain_quantiles=qa.cpu().numpy(), chain_n_valid=na.cpu().numpy())
    return out


def ro_quantiles():
    """rvm_rows_quantiles over [4][2500] (two segments of 2048, the second partial; row 1 all NaN, row 3 partly):
    16-byte aligned with an even stride, and the same values one double further on with an odd stride."""
    rng = np.random.default_rng(12)
    data = rng.standard_normal((4, 2500)) * np.array([1.0, 1.0, 1e-300, 1e5])[:, None]
    data[1], data[3, ::7], data[0, :3] = np.nan, np.nan, (np.inf, -np.inf, -0.0)
    wide = _f64(data)
    buf = torch.empty(1 + 4 * 2501, dtype=torch.float64, device="cuda")
    narrow = buf[1:].view(4, 2501)[:, :2500]
    narrow.copy_(wide)
    assert wide.data_ptr() % 16 == 0 and narrow.data_ptr() % 16 == 8 and narrow.stride(0) % 2 == 1
    out, lib = {}, _lib.load()
    for name, x in (("wide", wide), ("narrow", narrow)):
        qv, nv = _rows_quantiles(lib, x.data_ptr(), 4, x.stride(0), 1, x.stride(0), 2500, np.array(Q7), x.device)
        out.update({name + "_quantiles": qv.cpu().numpy(), name + "_n_valid": nv.cpu().numpy()})
    return out


def ro_gls():
    """rvm_gls_power at N = 5 and 6 (a table row padded to even, and not), F = 65 and S = 129 (one past the product
    kernel's tile of 64 x 128), with and without the floating mean, one model column all NaN."""
    lib, out = _lib.load(), {}
    sh = torch.cuda.current_stream().cuda_stream
    for N in (5, 6):
        rng = np.random.default_rng(13 + N)
        t, sigma = np.sort(rng.uniform(0.0, 30.0, N)), rng.uniform(0.5, 1.5, N)
        data, model = rng.standard_normal(N), 0.3 * rng.standard_normal((N, 129))
        model[:, 17] = np.nan
        for fm in (1, 0):
            tau, w = periodogram.series_inputs(t, sigma, bool(fm))
            d = [_f64(a) for a in (tau, w, data, model)]
            power, freq = torch.empty((65, 129), dtype=torch.float64, device="cuda"), _f64(np.zeros(65))
            ws = torch.empty(max(lib.rvm_gls_workspace_bytes(N, 65, 129) // 8, 2), dtype=torch.float64, device="cuda")
            _lib.check(lib.rvm_gls_power(d[0].data_ptr(), d[1].data_ptr(), N, d[2].data_ptr(), d[3].data_ptr(), 129,
                                         129, 0.01, 0.003, 2, 65, fm, power.data_ptr(), 129, freq.data_ptr(),
                                         ws.data_ptr(), sh), "rvm_gls_power")
            out.update({f"power_N{N}_fm{fm}": power.cpu().numpy(), f"freq_N{N}_fm{fm}": freq.cpu().numpy()})
    return out


def ro_ladder():
    """rvm_pt_ladder_update twice at T = 3, Wh = 130 (W = 260: the strided partials run past one block of 256),
    the moments on."""
    lib, rng, T, Wh = _lib.load(), np.random.default_rng(14), 3, 130
    i64 = dict(dtype=torch.int64, device="cuda")
    swapped = torch.as_tensor(rng.integers(0, 50, (T - 1, 2 * Wh)).astype(np.int32), device="cuda")
    lnp = [_f64(-50.0 + 5.0 * rng.standard_normal(T * Wh)) for _ in range(2)]
    betas, ratios, moments = _f64([1.0, 0.4, 0.05]), _f64(np.zeros(T - 1)), _f64(np.zeros((T, 2)))
    prev, refused, ws = torch.zeros(T - 1, **i64), torch.zeros(1, **i64), torch.empty(3 * T - 1, **i64)
    for _ in range(2):
        _lib.check(lib.rvm_pt_ladder_update(T, Wh, swapped.data_ptr(), lnp[0].data_ptr(), lnp[1].data_ptr(), 0.05,
                                            betas.data_ptr(), prev.data_ptr(), ratios.data_ptr(), refused.data_ptr(),
                                            moments.data_ptr(), ws.data_ptr(), torch.cuda.current_stream().cuda_stream),
                   "rvm_pt_ladder_update")
        swapped += torch.as_tensor(rng.integers(0, 3, (T - 1, 2 * Wh)).astype(np.int32), device="cuda")
    return {k: v.cpu().numpy() for k, v in dict(betas=betas, ratios=ratios, moments=moments, totals_prev=prev,
                                                refused=refused).items()}


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
    cases.update(ro_chain=ro_chain, ro_quantiles=ro_quantiles, ro_gls=ro_gls, ro_ladder=ro_ladder)
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
