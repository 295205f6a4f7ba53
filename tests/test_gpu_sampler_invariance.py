"""Do the sampler kernels, run for many iterations on the device's own Philox draws, leave a known target
invariant?  (tests/invariance_ref.py states the idea, the statistics and where every number comes from;
tests/test_invariance_ref_cpu.py shows that the reference passes and that every seeded slip of a rule is caught.)

Every case starts from an exact draw of its target, calls the propose / accept / swap / metric entry points
straight through the C ABI with draws = NULL, and evaluates the target's log-probability (gradient, Hessian)
between the launches in torch float64 -- no plan, no likelihood launch.  Asserted per case: every return code 0
(_lib.check), every output finite, the accept counters equal to the number of position changes, the swap counters
equal to the exchanges seen in the positions and log-probabilities, SMALA's ok flags set and its failure counters
0; every statistic within the LOOSE thresholds (p >= 1e-5, |z| <= 4.5: exact nulls, nothing measured); the
correlation with the start at most 0.15 and the acceptance fraction within 0.02 of the reference's (a frozen
sampler passes neither); the PT swap rates and the d = 1 MH acceptance within 4.5 measured sd of their analytic
values.  default_betas' "about 25 %" is, at d = 5, 0.449 analytically.  Every statistic is printed (pytest -s),
and so is the number of walkers whose final position differs from the CPU reference's (the two agree up to
decisions at ties and the last bits of torch's against numpy's log-probabilities; not asserted).

stretch17 runs 256 iterations where the other ensembles run 64: at d = 17 the correct move is still correlated
0.58 with its start after 64 (the reference, on the CPU), and the bound on that correlation stays at 0.15.
"""
import ctypes as C
import functools

import numpy as np
import pytest

import invariance_ref as I
from support import rvm_lib as _lib, to_device as _dev, torch_or_fail as _torch

pytestmark = pytest.mark.gpu

A = 2.0
KEYS = ("lp", "grad", "mu", "L", "G", "logdet", "ok")


class _Target:
    """The case's target in torch float64 on the device, positions [d][n] as the kernels hold them."""

    def __init__(self, case):
        self.t = I.target(case)
        self.quartic = isinstance(self.t, I.Quartic)
        self.M = _dev(self.t.R if self.quartic else self.t.prec)

    def lnp(self, x):
        if self.quartic:
            y = self.M @ x
            return -0.25 * ((y * y) * (y * y)).sum(0)
        return self.t.OFFSET - 0.5 * ((self.M @ x) * x).sum(0)

    def derivs(self, x):
        """(lp [C], grad [P][C], hess [P P][C]: element (i, j) of chain c at [i P + j][c])."""
        torch = _torch()
        y = self.M @ x
        P = x.shape[0]
        hess = -torch.einsum("ki,kc,kj->ijc", self.M, 3.0 * y * y, self.M).reshape(P * P, -1).contiguous()
        return self.lnp(x), -(self.M.T @ (y * y * y)).contiguous(), hess


def _finite(*ts):
    return sum((~_torch().isfinite(t)).sum() for t in ts)


# ---- the ensembles: rvm_stretch_propose / _accept, rvm_pt_stretch_propose / _accept, rvm_pt_swap -------------------

@functools.lru_cache(maxsize=None)
def _ensemble(case, plain, shards=((0.0, 1.0),)):
    """K iterations of a case on the device.  plain: the T = 1 entry points, each half in one call per shard
    (fractions of the half; s0_begin = h W/2 + the shard's first walker); else the tempered ones and, where the
    case has one, the sweep after every iteration."""
    torch = _torch()
    _lib_, lib = _lib()
    st = _lib_.stream_handle()
    c, tgt = I.CASES[case], _Target(case)
    X0 = I.start(case)
    d, T, W = X0.shape
    Wh, K, seed = W // 2, c["K"], c["seed"]
    n = T * Wh
    x = [_dev(X0[:, :, h * Wh:(h + 1) * Wh].reshape(d, n)) for h in (0, 1)]  # column t Wh + k
    lnp = [tgt.lnp(v) for v in x]
    betas = _dev(np.asarray(c["betas"], dtype=np.float64))
    acc = [torch.zeros(n, dtype=torch.int32, device="cuda") for _ in (0, 1)]
    swapped = torch.zeros((max(T - 1, 1), W), dtype=torch.int32, device="cuda")
    zero = torch.zeros((), dtype=torch.int64, device="cuda")
    moved, bad, unseen = zero.clone(), zero.clone(), zero.clone()
    cuts = [(int(round(a * Wh)), int(round(b * Wh))) for a, b in shards]
    assert not plain or T == 1
    for it in range(K):
        for h in (0, 1):
            before = x[h].clone()
            if plain:
                for b, e in cuts:
                    whole = (b, e) == (0, Wh)
                    xs, ls, as_ = (x[h], lnp[h], acc[h]) if whole else (x[h][:, b:e].contiguous(), lnp[h][b:e].clone(),
                                                                        acc[h][b:e].clone())
                    q = torch.full((d, e - b), float("nan"), dtype=torch.float64, device="cuda")
                    z = torch.full((e - b,), float("nan"), dtype=torch.float64, device="cuda")
                    _lib_.check(lib.rvm_stretch_propose(d, e - b, h * Wh + b, xs.data_ptr(), Wh, x[1 - h].data_ptr(), A,
                                                        seed, it, h, None, q.data_ptr(), z.data_ptr(), st), "propose")
                    lnew = tgt.lnp(q)
                    bad += _finite(q, z, lnew)
                    _lib_.check(lib.rvm_stretch_accept(d, e - b, h * Wh + b, xs.data_ptr(), ls.data_ptr(), q.data_ptr(),
                                                       lnew.data_ptr(), z.data_ptr(), seed, it, h, None, as_.data_ptr(),
                                                       st), "accept")
                    if not whole:
                        x[h][:, b:e], lnp[h][b:e], acc[h][b:e] = xs, ls, as_
            else:
                q = torch.full((d, n), float("nan"), dtype=torch.float64, device="cuda")
                z = torch.full((n,), float("nan"), dtype=torch.float64, device="cuda")
                _lib_.check(lib.rvm_pt_stretch_propose(d, T, Wh, x[h].data_ptr(), x[1 - h].data_ptr(), A, seed, it, h,
                                                       None, q.data_ptr(), z.data_ptr(), st), "pt propose")
                lnew = tgt.lnp(q)
                bad += _finite(q, z, lnew)
                _lib_.check(lib.rvm_pt_stretch_accept(d, T, Wh, betas.data_ptr(), x[h].data_ptr(), lnp[h].data_ptr(),
                                                      q.data_ptr(), lnew.data_ptr(), z.data_ptr(), seed, it, h, None,
                                                      acc[h].data_ptr(), st), "pt accept")
            moved += (x[h] != before).any(0).sum()
        if c["sweep"]:
            Xb = torch.cat([v.view(d, T, Wh) for v in x], 2)  # [d][T][W] before the sweep (a copy)
            Lb = torch.cat([v.view(T, Wh) for v in lnp], 1)
            sb = swapped.clone()
            _lib_.check(lib.rvm_pt_swap(d, T, Wh, betas.data_ptr(), x[0].data_ptr(), x[1].data_ptr(), lnp[0].data_ptr(),
                                        lnp[1].data_ptr(), seed, it, None, swapped.data_ptr(), st), "pt swap")
            delta = swapped - sb
            bad += ((delta != 0) & (delta != 1)).sum()
            for p in range(T - 2, -1, -1):  # the counted exchanges, replayed on the copy
                m = delta[p] != 0
                Xb[:, p, m], Xb[:, p + 1, m] = Xb[:, p + 1, m].clone(), Xb[:, p, m].clone()
                Lb[p, m], Lb[p + 1, m] = Lb[p + 1, m].clone(), Lb[p, m].clone()
            unseen += (Xb != torch.cat([v.view(d, T, Wh) for v in x], 2)).sum()
            unseen += (Lb != torch.cat([v.view(T, Wh) for v in lnp], 1)).sum()
    torch.cuda.synchronize()
    X = torch.cat([v.view(d, T, Wh) for v in x], 2).cpu().numpy()
    L = torch.cat([v.view(T, Wh) for v in lnp], 1).cpu().numpy()
    accepted = torch.cat([a.view(T, Wh) for a in acc], 1).cpu().numpy()
    sw = swapped.cpu().numpy()[:T - 1]
    return dict(X=X, lnp=L, accepted=accepted, swapped=sw, moved=int(moved), bad=int(bad), unseen=int(unseen),
                accept=accepted.sum() / (K * T * W), swap=sw.sum(1) / (K * W))


def _judge(case, res, differ_tol=0.0):
    """The assertions every case shares; returns the statistics' rows."""
    X = res["X"]
    assert np.isfinite(X).all() and res["bad"] == 0
    assert int(np.sum(res["accepted"])) == res["moved"], (int(np.sum(res["accepted"])), res["moved"])
    rows, move = I.evaluate(case, X, res)
    I.show(rows)
    ref = I.reference(case)
    differ = int((np.abs(X - ref["X"]) > differ_tol).reshape(X.shape[0], -1).any(0).sum())
    print(f"{case}: start rho {move['rho']:.3f} acceptance {move['accept']:.4f} (reference {ref['accept']:.4f}); "
          f"{differ} of {X[0].size} walkers differ from the reference's at iteration {I.CASES[case]['K']}", flush=True)
    I.count(case, rows)
    assert not I.misses(rows, I.P_MIN, I.Z_MAX), I.misses(rows, I.P_MIN, I.Z_MAX)
    assert move["rho"] <= I.RHO_MAX, move
    assert abs(move["accept"] - ref["accept"]) <= I.ACC_TOL, (move, ref["accept"])
    return rows


@pytest.mark.parametrize("case", ["stretch5", "stretch17"])
def test_stretch_move_leaves_the_gaussian_invariant(case):
    """W = 4096; d = 5 and d = 17; both halves, s0_begin 0 and n_half.  A full covariance of condition number 30:
    the move's affine invariance is what makes its acceptance that of the whitened target."""
    res = _ensemble(case, True)
    _judge(case, res)
    assert res["unseen"] == 0 and res["swapped"].size == 0


def test_stretch_sharded_keys_give_the_unsharded_run():
    """Each half in two calls (walkers [0, 733) and [733, 2048) of the half, s0_begin offset accordingly): the draws
    are keyed by the global walker index, so the run is the unsharded one bit for bit."""
    whole = _ensemble("stretch5", True)
    parts = _ensemble("stretch5", True, ((0.0, 733 / 2048), (733 / 2048, 1.0)))
    for k in ("X", "lnp", "accepted"):
        np.testing.assert_array_equal(parts[k], whole[k], err_msg=k)
    assert parts["moved"] == whole["moved"] and parts["bad"] == 0


def test_tempered_ladder_leaves_every_temperature_invariant():
    """T = 4 at default_betas(4, 5), the sweep after every iteration: every temperature t stays N(0, Sigma /
    beta_t), neighbouring temperatures stay independent, and the three swap rates are the analytic 0.4486 (sd
    over the reference's 16 seeds 1.3e-3 .. 1.75e-3; binomial 9.7e-4)."""
    res = _ensemble("pt4", False)
    _judge("pt4", res)
    assert res["unseen"] == 0
    assert (res["swapped"].sum(1) > 0).all()


def test_equal_betas_are_three_independent_ensembles():
    """T = 3 with every beta within 1e-12 of 1 and no sweep: three plain ensembles whose Philox items differ only
    in t W; a counter shared between temperatures shows in the t|t+1 statistics."""
    res = _ensemble("pt3equal", False)
    _judge("pt3equal", res)
    assert res["swapped"].sum() == 0


# ---- rvm_mh_propose / rvm_mh_accept ---------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _mh(case):
    torch = _torch()
    _lib_, lib = _lib()
    st = _lib_.stream_handle()
    c, tgt = I.CASES[case], _Target(case)
    x = _dev(I.start(case), copy=True)
    P, n = x.shape
    lnp = tgt.lnp(x)
    scales = _dev(np.asarray(c["scales"], dtype=np.float64))
    acc = torch.zeros(n, dtype=torch.int32, device="cuda")
    zero = torch.zeros((), dtype=torch.int64, device="cuda")
    moved, bad = zero.clone(), zero.clone()
    for it in range(c["K"]):
        q = torch.full((P, n), float("nan"), dtype=torch.float64, device="cuda")
        _lib_.check(lib.rvm_mh_propose(P, n, c["begin"], x.data_ptr(), scales.data_ptr(), c["step"], c["seed"], it,
                                       None, q.data_ptr(), st), "mh propose")
        lnew = tgt.lnp(q)
        bad += _finite(q, lnew)
        before = x.clone()
        _lib_.check(lib.rvm_mh_accept(P, n, c["begin"], x.data_ptr(), lnp.data_ptr(), q.data_ptr(), lnew.data_ptr(),
                                      c["seed"], it, None, acc.data_ptr(), st), "mh accept")
        moved += (x != before).any(0).sum()
    torch.cuda.synchronize()
    accepted = acc.cpu().numpy()
    return dict(X=x.cpu().numpy(), accepted=accepted, moved=int(moved), bad=int(bad),
                accept=accepted.sum() / (c["K"] * n), swap=np.zeros(0))


@pytest.mark.parametrize("case", ["mh1", "mh3"])
def test_metropolis_hastings_leaves_the_gaussian_invariant(case):
    """mh1: d = 1, N(0, 1), proposal sd 2.4, chain_begin 0; the acceptance is (2 / pi) atan(2 / 2.4) = 0.4423 (sd
    over the reference's 16 seeds 9.5e-4; binomial 6.9e-4).  mh3: d = 3, unequal scales, chain_begin 2^33 (the
    second counter word).  C = 8192 chains."""
    _judge(case, _mh(case), differ_tol=1e-9)


# ---- rvm_smala_metric / _propose / _accept / _metric_accept -------------------------------------------------------

def _cache(P, n):
    torch = _torch()
    _lib_, _ = _lib()
    shape = dict(lp=(n,), grad=(P, n), mu=(P, n), L=(P * P, n), G=(P * P, n), logdet=(n,))
    d = {k: torch.full(s, float("nan"), dtype=torch.float64, device="cuda") for k, s in shape.items()}
    d["ok"] = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    d["_c"] = _lib_.SmalaCache(*[d[k].data_ptr() for k in KEYS])
    return d


@functools.lru_cache(maxsize=None)
def _smala(fused):
    torch = _torch()
    _lib_, lib = _lib()
    st = _lib_.stream_handle()
    c, tgt = I.CASES["smala"], _Target("smala")
    x = _dev(I.start("smala"), copy=True)
    P, n = x.shape
    al, eps, seed, begin = c["alpha"], c["eps"], c["seed"], c["begin"]
    status = torch.zeros(n, dtype=torch.int32, device="cuda")
    cur, prop = _cache(P, n), _cache(P, n)
    acc = torch.zeros(n, dtype=torch.int32, device="cuda")
    fail = torch.zeros(n, dtype=torch.int32, device="cuda")
    zero = torch.zeros((), dtype=torch.int64, device="cuda")
    moved, bad, not_ok = zero.clone(), zero.clone(), zero.clone()
    lp, g, H = tgt.derivs(x)
    _lib_.check(lib.rvm_smala_metric(P, n, x.data_ptr(), lp.data_ptr(), status.data_ptr(), g.data_ptr(), H.data_ptr(),
                                     al, eps, C.byref(cur["_c"]), st), "metric")
    for it in range(c["K"]):
        xs = torch.full((P, n), float("nan"), dtype=torch.float64, device="cuda")
        _lib_.check(lib.rvm_smala_propose(P, n, begin, x.data_ptr(), C.byref(cur["_c"]), eps, seed, it, None,
                                          xs.data_ptr(), st), "propose")
        lp, g, H = tgt.derivs(xs)
        bad += _finite(xs, lp, g, H)
        before = x.clone()
        if fused:
            _lib_.check(lib.rvm_smala_metric_accept(P, n, begin, x.data_ptr(), xs.data_ptr(), lp.data_ptr(),
                                                    status.data_ptr(), g.data_ptr(), H.data_ptr(), al, eps,
                                                    C.byref(cur["_c"]), C.byref(prop["_c"]), seed, it, None,
                                                    acc.data_ptr(), fail.data_ptr(), st), "metric_accept")
        else:
            _lib_.check(lib.rvm_smala_metric(P, n, xs.data_ptr(), lp.data_ptr(), status.data_ptr(), g.data_ptr(),
                                             H.data_ptr(), al, eps, C.byref(prop["_c"]), st), "metric")
            _lib_.check(lib.rvm_smala_accept(P, n, begin, x.data_ptr(), C.byref(cur["_c"]), xs.data_ptr(),
                                             C.byref(prop["_c"]), eps, seed, it, None, acc.data_ptr(), fail.data_ptr(),
                                             st), "accept")
        moved += (x != before).any(0).sum()
        not_ok += (prop["ok"] != 1).sum() + (cur["ok"] != 1).sum()
        bad += _finite(*[prop[k] for k in KEYS[:-1]])
    torch.cuda.synchronize()
    accepted = acc.cpu().numpy()
    return dict(X=x.cpu().numpy(), accepted=accepted, moved=int(moved), bad=int(bad), not_ok=int(not_ok),
                failures=int(fail.sum()), cur={k: cur[k].cpu().numpy() for k in KEYS},
                accept=accepted.sum() / (c["K"] * n), swap=np.zeros(0))


def test_smala_leaves_the_quartic_invariant():
    """P = 3, alpha = 1, C = 8192, K = 48, exact (lp, grad, hess) of lnp = -sum (R x)_i^4 / 4: -H = R^T diag(3 y^2) R
    moves with the position and is not diagonal, so the Jacobi eigen-solver, SoftAbs (its 1 / alpha branch near
    y = 0), the Cholesky factor and log det all enter the law.  eps = 1.1: the reference accepts 53.5 %."""
    res = _smala(False)
    _judge("smala", res, differ_tol=1e-9)
    assert res["not_ok"] == 0 and res["failures"] == 0
    assert np.isfinite(np.concatenate([res["cur"][k].ravel() for k in KEYS[:-1]])).all()


def test_fused_smala_step_gives_the_separate_launches_run():
    sep, fused = _smala(False), _smala(True)
    np.testing.assert_array_equal(fused["X"], sep["X"])
    np.testing.assert_array_equal(fused["accepted"], sep["accepted"])
    for k in KEYS:
        np.testing.assert_array_equal(fused["cur"][k], sep["cur"][k], err_msg=k)
    assert fused["moved"] == sep["moved"] and fused["not_ok"] == 0 and fused["failures"] == 0 and fused["bad"] == 0


# ---- the whole file's chance of a false alarm ---------------------------------------------------------------------

def test_statistic_count_is_within_the_budget():
    """N statistics at p >= 1e-5 each: a correct sampler fails this file by chance less than once in 500 choices of
    the seeds.  Counts what the tests above asserted (all of them, when the file runs as a whole)."""
    n = I.budget()
    print(f"{n} statistics asserted, chance of a false alarm {n * I.P_MIN:.2e}", flush=True)
