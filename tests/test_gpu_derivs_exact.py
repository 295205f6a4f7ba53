"""The exact-derivative kernel (rvm_logl_derivs) against a 60-digit restatement, every variant.

Tier D0.  tests/test_gpu_derivs.py pins the kernel with finite differences in double
(D1 1e-6, Hessian against second differences 1e-3); this file compares logp, the gradient and the
Hessian with tests/golden/wh_derivs.json: central differences of tests/wh_ref.py's restatement of
the plan's discrete integrator in 60-digit arithmetic (truncation and roundoff ~1e-30), taken of the
per-epoch model RV, from which chi2, gradient and Hessian follow for any observation vector.

  * Bound: in the units of test_gpu_derivs.scaled_errors (gradient |dg_i| / sqrt|H_ii|, Hessian
    |dH_ij| / sqrt|H_ii H_jj|), T1_SENS_FACTOR (3) x the largest scaled error, over all entries of
    the case and vector, of the restatement's own hyper-dual run in double -- what an independent
    double-precision implementation of the same derivatives achieves.  It is measured on the
    reference, not on the kernel, and is at or below 1e-9 on every case (tests/test_wh_ref_cpu.py).
  * Cases (wh_ref.case_inputs): every instantiation class of launch_derivs -- 1 to 4 planets, planar
    and inclined, plans of 1, 3, 4, 5 and 6 levels (64-, 192-, 256-, 320- and 384-thread blocks,
    both MAXT) -- an epoch at t = 0, duplicate epochs, an empty direction, no step at all, a
    zero-inclination point, a scrambled sub-set of directions, and an e = 0.6 orbit at 8 steps per
    period whose steps take the bracketed Kepler solver and the Stumpff quartering loop.
  * Observation vectors: "fit" (truth + a 1-sigma offset) and "offset" (observed RV = 0: the
    residual is the whole signal, so the order-2 variations rv.ab carry a large share of the
    Hessian; a Hessian whose rv.a rv.b part alone is right passes "fit" whatever rv.ab is).  Where
    observed RV = 0 leaves r rv.ab below a quarter of more than half of the entries, the observed
    RVs lie further from the model (wh_ref.offset_factor: `three` 32x, `four_inclined` 64x,
    `one_level` 2x the signal).
  * logp keeps T1's form (t1_tol); rvm_logl_batch's rv_out on the same plan is held to the truth
    RVs within T1_RV_ABS's form.
  * Index mapping: `s2` runs its two walkers tiled to 7 chains (385 items, 32 per block),
    `five_levels_inclined` to 3 (84 items, 64 per block); every copy equals its original bit for bit.

$RVM_DERIVS_EXACT_REPORT (a path) appends per case the kernel's largest scaled errors, the double
restatement's and their ratio as JSON lines (profiles/derivs_exact_tier.jsonl).
"""
import numpy as np
import pytest
from mpmath import mp

import oracle as O
import wh_ref as R
from support import T1_SENS_FACTOR, report_line, t1_tol, torch_or_fail as _torch

pytestmark = pytest.mark.gpu

FX = R.load_fixture()
TILED = {"s2": 7, "five_levels_inclined": 3}
assert R.FLOOR_FACTOR == T1_SENS_FACTOR


def _make_plan(c, p):
    from rvmcmc import engine

    return engine.LoglPlan(np.array(c["epochs"]), np.array(p["obs_rv"]), np.array(p["sigma"]), p["npoints"],
                           len(c["walkers"][0]), c["dt"], tuple(c["levels"]), max_walkers=64,
                           period_hint=c["period_hint"], inclined=c["inclined"])


def _derivs(plan, c, walkers):
    torch = _torch()
    K = torch.as_tensor(R.kernel_rows(walkers, c["inclined"]), device="cuda")
    lp, g, H, st = plan.derivs(K, c["dir_rows"], hill_factor=c["hill"])
    lp_l, st_l, rv = plan.logl(K, hill_factor=c["hill"], want_rv=True)
    torch.cuda.synchronize()
    return [x.cpu().numpy() for x in (lp, g, H, st, lp_l, st_l, rv)]


@pytest.mark.parametrize("vec", ["fit", "offset"])
@pytest.mark.parametrize("name", list(FX))
def test_derivs_match_the_high_precision_truth(name, vec):
    c = FX[name]
    W = len(c["walkers"])
    C = TILED.get(name, W)
    with mp.workdps(R.TRUTH_DPS):
        p = R.problem(c, vec)
        plan = _make_plan(c, p)
        lp, g, H, st, lp_l, st_l, rv = _derivs(plan, c, [c["walkers"][k % W] for k in range(C)])
        assert (st == 0).all() and (st_l == 0).all()
        for k in range(W, C):  # every copy equals its original bit for bit
            assert lp[k] == lp[k % W] and np.array_equal(g[:, k], g[:, k % W]) and np.array_equal(H[:, :, k], H[:, :, k % W])
        rv_tol = 1e-14 * float(np.abs(O.richardson_weights(tuple(c["levels"]))).sum())  # T1_RV_ABS's form
        eg = eH = elp = erv = 0.0
        for w in range(W):
            lp_ref, g_ref, H_ref = p["truth"][w]
            assert np.array_equal(H[:, :, w], H[:, :, w].T)
            a, b = R.scaled_errors(g[:, w], H[:, :, w], g_ref, H_ref)
            eg, eH = max(eg, a), max(eH, b)
            elp = max(elp, float(abs(mp.mpf(float(lp[w])) - lp_ref) / max(1, abs(lp_ref))))
            erv = max(erv, max(float(abs(mp.mpf(float(rv[e, w])) - mp.mpf(c["walkers_out"][w]["truth"]["rv"][e])))
                               for e in range(len(c["epochs"]))))
    ratio = max(eg, eH) / max(p["floor_grad"], p["floor_hess"])
    print(f"{name}/{vec}: kernel scaled errors grad {eg:.2e} hess {eH:.2e}; double restatement grad {p['floor_grad']:.2e} "
          f"hess {p['floor_hess']:.2e}; ratio {ratio:.2f} (bound {T1_SENS_FACTOR}); logp rel err {elp:.1e}; rv err {erv:.1e}")
    report_line("RVM_DERIVS_EXACT_REPORT", case=name, vector=vec, chains=C, kernel_grad=eg, kernel_hess=eH,
                restatement_grad=p["floor_grad"], restatement_hess=p["floor_hess"], ratio=ratio, bound=p["bound"],
                logp_rel_err=elp, logp_tol=t1_tol(tuple(c["levels"])), rv_abs_err=erv, rv_tol=rv_tol)
    assert p["bound"] <= 1e-9
    assert elp <= t1_tol(tuple(c["levels"])), elp
    assert erv <= rv_tol, erv
    assert eg <= p["bound"] and eH <= p["bound"], (eg, eH, p["bound"])


def test_status_walkers_leave_the_good_ones_unchanged():
    """`s2` with a prior walker (a = 0.01) and an encounter walker (planet 2 on planet 1's orbit)
    appended: they carry the likelihood kernel's status and NaN derivatives; the good chains' values
    are unchanged bit for bit by their presence."""
    c = FX["s2"]
    with mp.workdps(R.TRUTH_DPS):
        p = R.problem(c, "fit")
    plan = _make_plan(c, p)
    good = [c["walkers"][k % 2] for k in range(TILED["s2"])]
    lp0, g0, H0, st0 = _derivs(plan, c, good)[:4]
    lp, g, H, st, lp_l, st_l, _ = _derivs(plan, c, good + R.s2_bad_walkers(c))
    n = len(good)
    assert list(st) == list(st_l) == [0] * n + [1, 2] and (st0 == 0).all()
    assert np.array_equal(lp[:n], lp0) and np.array_equal(g[:, :n], g0) and np.array_equal(H[:, :, :n], H0)
    assert np.isneginf(lp[n:]).all() and np.isnan(g[:, n:]).all() and np.isnan(H[:, :, n:]).all()
