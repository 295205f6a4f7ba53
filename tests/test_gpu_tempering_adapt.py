"""The adaptive ladder and the evidence on the device (rvm_pt_ladder_update, rvmcmc/tempering.py)
against the numpy restatement tests/pt_adapt_ref.py.

The device and the restatement run the same operations in the same order and differ only in exp, by
<= 1 ulp on each side: <= ~2 ulp in each temperature gap and each beta, so betas are compared at
rtol 1e-12 (three orders above that, nine below the 1e-3 movement a wrong rule produces).  The moments
have <= 516 same-signed terms: the summation-order error is <= 516 * 1.1e-16, compared at rtol 1e-12.
tests/test_tempering_adapt_cpu.py runs the full-iteration input through the restatement with the
oracle alone and asserts that no decision is near a tie (margins 3.4e-4 and 2.5e-2, against the
~1e-11 a beta error of 1e-12 moves a decision statistic): the comparisons here have no exemptions.
"""
import numpy as np
import pytest

import pt_adapt_ref as R
import pt_ref
from support import PT_ADAPT_CASE as CASE, s2_state_and_obs, state_scales as _scales, torch_or_fail as _torch

pytestmark = pytest.mark.gpu

RTOL = 1e-12


def _state_and_obs():
    return s2_state_and_obs(fixed_step=True)


# ---- 1. the update alone ----------------------------------------------------------------------------

def _update_device(betas, swapped, prev, lnp, kappa, moments=None, n_refused=0):
    """rvm_pt_ladder_update on host arrays (swapped [T-1][W], lnp [T][W], moments [T][2] or None)
    -> (rc, betas, prev, ratios, n_refused, moments)."""
    torch = _torch()
    from rvmcmc import _lib

    lib = _lib.load()
    T, W = lnp.shape
    Wh = W // 2
    dev = lambda a, dt: torch.as_tensor(np.ascontiguousarray(a, dtype=dt), device="cuda")  # noqa: E731
    b, sw, pv = dev(betas, np.float64), dev(swapped, np.int32), dev(prev, np.int64)
    l = [dev(lnp[:, h * Wh:(h + 1) * Wh].reshape(T * Wh), np.float64) for h in (0, 1)]
    ratios = torch.full((T - 1,), -7.0, dtype=torch.float64, device="cuda")
    nref = dev([n_refused], np.int64)
    mom = dev(moments, np.float64) if moments is not None else None
    work = torch.full((3 * T - 1,), float("nan"), dtype=torch.float64, device="cuda")
    rc = lib.rvm_pt_ladder_update(T, Wh, sw.data_ptr(), l[0].data_ptr(), l[1].data_ptr(), kappa, b.data_ptr(),
                                  pv.data_ptr(), ratios.data_ptr(), nref.data_ptr(),
                                  mom.data_ptr() if mom is not None else 0, work.data_ptr(), _lib.stream_handle())
    torch.cuda.synchronize()
    return (rc, b.cpu().numpy(), pv.cpu().numpy(), ratios.cpu().numpy(), int(nref.item()),
            mom.cpu().numpy() if mom is not None else None)


@pytest.mark.parametrize("T,W", [(2, 2), (3, 24), (5, 516), (16, 24)])
def test_update_matches_numpy(T, W):
    rng = np.random.default_rng(100 * T + W)  # (ladders the restatement accepts: the refusal has its own test)
    betas = np.sort(rng.uniform(0.05, 1.0, T))[::-1].copy()
    betas[0] = 1.0
    assert np.all(np.diff(betas) < 0)
    prev_counts = rng.integers(0, 40, (T - 1, W))  # cumulative counters and the previous totals start non-zero
    swapped = prev_counts + (rng.random((T - 1, W)) < rng.uniform(0.1, 0.9, (T - 1, 1)))  # each pair at its own rate
    prev = prev_counts.sum(1)
    lnp = -3.0 - 50.0 * rng.random((T, W))
    mom0 = np.stack([-1e3 * rng.random(T), 1e5 * rng.random(T)], 1)  # the accumulators start non-zero too
    want_b, want_A, want_prev, want_ref = R.update(betas, swapped, prev, W, 0.5)
    assert want_ref == 0
    out = [_update_device(betas, swapped, prev, lnp, 0.5, moments=mom0, n_refused=3) for _ in range(2)]
    rc, b, pv, A, nref, mom = out[0]
    assert rc == 0 and nref == 3
    np.testing.assert_array_equal(A, want_A)
    np.testing.assert_array_equal(pv, want_prev)
    assert b[0] == betas[0] and b[-1] == betas[-1]
    np.testing.assert_allclose(b, want_b, rtol=RTOL, atol=0)
    if T == 2:
        np.testing.assert_array_equal(b, betas)  # no interior temperature
    else:
        assert (np.abs(want_b - betas)[1:-1] > 1e-3).any()  # the rule moved the ladder: a no-op kernel fails
    np.testing.assert_allclose(mom, mom0 + R.moments(lnp), rtol=RTOL, atol=0)
    # the same bits from run to run
    np.testing.assert_array_equal(out[1][1], b)
    np.testing.assert_array_equal(out[1][5], mom)
    # without the accumulator the rest is the same
    rc, b2, pv2, A2, _, none = _update_device(betas, swapped, prev, lnp, 0.5)
    assert rc == 0 and none is None
    np.testing.assert_array_equal(b2, b)
    np.testing.assert_array_equal(pv2, pv)
    np.testing.assert_array_equal(A2, A)


def test_update_refusal_and_no_drive_leave_the_ladder_bit_identical():
    rng = np.random.default_rng(3)
    W = 24
    lnp = -rng.random((3, W))
    betas = np.array([1.0, 0.5000001, 0.5])
    sw = np.zeros((2, W), dtype=int)
    sw[0] = 1  # counts [24, 0]: the interior overshoots the hottest temperature
    assert R.update(betas, sw, np.zeros(2), W, 20.0)[3] == 1
    rc, b, pv, A, nref, _ = _update_device(betas, sw, np.zeros(2), lnp, 20.0)
    assert rc == 0 and nref == 1
    np.testing.assert_array_equal(b, betas)
    np.testing.assert_array_equal(A, [1.0, 0.0])
    np.testing.assert_array_equal(pv, [W, 0])
    # no drive: kappa = 0 with unequal ratios, and equal ratios with a gain; neither is a refusal
    lad = np.array([1.0, 0.7, 0.3, 0.1, 0.07])
    lnp5 = -rng.random((5, W))
    sw5 = rng.integers(0, 2, (4, W))
    sw5[3] = 0
    mom0 = np.zeros((5, 2))
    rc, b, _, A, nref, mom = _update_device(lad, sw5, np.zeros(4), lnp5, 0.0, moments=mom0)
    assert rc == 0 and nref == 0 and len(set(A)) > 1
    np.testing.assert_array_equal(b, lad)
    np.testing.assert_allclose(mom, R.moments(lnp5), rtol=RTOL, atol=0)
    rc, b, _, A, nref, _ = _update_device(lad, np.ones((4, W), dtype=int), np.zeros(4), lnp5, 50.0)
    assert rc == 0 and nref == 0
    np.testing.assert_array_equal(A, np.ones(4))
    np.testing.assert_array_equal(b, lad)


# ---- 2. full iterations against the restatement -----------------------------------------------------

def _case(s):
    return pt_ref.case_inputs(s.get_params(), _scales(s), CASE["T"], CASE["W"], CASE["iters"], seed=CASE["seed"])


def _sampler(s, obs, X, **kw):
    from rvmcmc.tempering import PTSampler

    pt = PTSampler(CASE["T"], CASE["W"], s, obs, seed=1, **kw)
    pt.set_positions(X)
    return pt


ADAPT = dict(adapt=True, adaptation_lag=CASE["lag"], adaptation_time=CASE["time"])


def test_full_adaptive_steps_match_numpy():
    """After every half-step and sweep the device's positions and lnp equal the restatement's exactly
    (it takes the device's proposal lnp, and keeps its OWN betas); after every update the device's
    ladder equals the restatement's at rtol 1e-12 and the ratios exactly.  No exemptions."""
    from rvmcmc.tempering import default_betas

    s, obs = _state_and_obs()
    T, W = CASE["T"], CASE["W"]
    Wh = W // 2
    X, draws = _case(s)
    pt = _sampler(s, obs, X, **ADAPT)
    pt.compute_lnprob()
    betas0 = default_betas(T, s.Nvars)
    lad = pt_ref.Ladder(X, betas0, lambda Q: (np.zeros(len(Q)), np.zeros(len(Q), dtype=int)))
    lad.lnp = pt.lnprob()
    nsw, prev = np.zeros((T - 1, W), dtype=np.int64), np.zeros(T - 1, dtype=np.int64)
    for it, d in enumerate(draws):
        for h in (0, 1):
            pt.half_step(h, np.stack([d["u1"][h].reshape(-1), d["u2"][h].reshape(-1)]), d["u3"][h])
            lnp_new = pt._lnp_new.cpu().numpy().reshape(T, Wh)
            assert np.isfinite(lnp_new).all() and (pt._status.cpu().numpy() == 0).all()
            lad.half_step(h, d["u1"][h], d["u2"][h], d["u3"][h], lnp_new=lnp_new)
            np.testing.assert_array_equal(pt.positions(), lad.pos, err_msg=f"iteration {it} half {h}")
            np.testing.assert_array_equal(pt.lnprob(), lad.lnp)
        pt.swap(d["swap"])
        nsw += lad.swap(d["swap"])
        np.testing.assert_array_equal(pt.positions(), lad.pos, err_msg=f"iteration {it} sweep")
        np.testing.assert_array_equal(pt.lnprob(), lad.lnp)
        assert pt.nadapt == it
        pt.adapt_ladder()
        lad.betas, A, prev, refused = R.update(lad.betas, nsw, prev, W, R.kappa(it, CASE["lag"], CASE["time"]))
        assert refused == 0
        np.testing.assert_array_equal(pt.last_swap_ratios(), A)
        got = pt.ladder()
        np.testing.assert_allclose(got, lad.betas, rtol=RTOL, atol=0, err_msg=f"iteration {it} update")
        np.testing.assert_array_equal(pt.betas, got)
        assert got[0] == betas0[0] and got[-1] == betas0[-1]
        np.testing.assert_array_equal(pt._swap_prev.cpu().numpy(), prev)
        pt.iteration += 1
    assert lad.accept_margin >= 1e-6 and lad.swap_margin >= 1e-6
    assert pt.ladder_refusals() == 0 and pt.nadapt == CASE["iters"]
    assert (np.abs(pt.ladder() - betas0)[1:-1] > 1e-3).all()
    # step(draws=...) is the same iteration, update included: replay the run
    pt2 = _sampler(s, obs, X, **ADAPT)
    for d in draws:
        pt2.step(draws=d)
    np.testing.assert_array_equal(pt2.positions(), pt.positions())
    np.testing.assert_array_equal(pt2.lnprob(), pt.lnprob())
    np.testing.assert_array_equal(pt2.ladder(), pt.ladder())


# ---- 3. adapt = False is the sampler as it was ------------------------------------------------------

def test_frozen_before_the_first_step_is_the_default_sampler():
    from rvmcmc.tempering import default_betas

    s, obs = _state_and_obs()
    X, _ = _case(s)
    a, b = _sampler(s, obs, X), _sampler(s, obs, X, **ADAPT)
    b.freeze_ladder()
    for _ in range(3):
        a.step()
        b.step()
    for f in ("positions", "lnprob", "ladder"):
        np.testing.assert_array_equal(getattr(a, f)(), getattr(b, f)())
    np.testing.assert_array_equal(a.naccepted.cpu().numpy(), b.naccepted.cpu().numpy())
    np.testing.assert_array_equal(a.nswapped.cpu().numpy(), b.nswapped.cpu().numpy())
    np.testing.assert_array_equal(a.ladder(), default_betas(CASE["T"], s.Nvars))
    assert a.nadapt == b.nadapt == 0 and a.ladder_refusals() == b.ladder_refusals() == 0
    assert 0 < a.nswapped.sum().item() < 3 * (CASE["T"] - 1) * CASE["W"]


# ---- 4. checkpoint in mid-adaptation ----------------------------------------------------------------

def test_checkpoint_in_mid_adaptation_continues_bit_identically(tmp_path):
    s, obs = _state_and_obs()
    X, _ = _case(s)
    a = _sampler(s, obs, X, **ADAPT)
    for _ in range(2):
        a.step()
    a.checkpoint(tmp_path / "pt.npz")
    mid = a.ladder()
    for _ in range(2):
        a.step()
    from rvmcmc.tempering import PTSampler

    r = PTSampler(CASE["T"], CASE["W"], s, obs, seed=999)  # adapt off, default settings: all from the file
    r.restore(tmp_path / "pt.npz")
    assert r.adapt and r.nadapt == 2 and r.adaptation_lag == CASE["lag"] and r.adaptation_time == CASE["time"]
    np.testing.assert_array_equal(r.ladder(), mid)
    for _ in range(2):
        r.step()
    for f in ("positions", "lnprob", "ladder", "last_swap_ratios", "ladder_refusals", "swap_fraction"):
        np.testing.assert_array_equal(getattr(r, f)(), getattr(a, f)())
    np.testing.assert_array_equal(r._swap_prev.cpu().numpy(), a._swap_prev.cpu().numpy())
    assert r.nadapt == a.nadapt == 4
    assert (a.ladder() != mid)[1:-1].all()  # the ladder went on moving after the checkpoint


# ---- 5. moments and the evidence --------------------------------------------------------------------

def test_moments_and_evidence_on_the_frozen_ladder(tmp_path):
    s, obs = _state_and_obs()
    X, _ = _case(s)
    T, W = CASE["T"], CASE["W"]
    pt = _sampler(s, obs, X, **ADAPT)
    with pytest.raises(ValueError, match="freeze_ladder"):
        pt.record_lnprob(True)
    pt.step()
    pt.freeze_ladder()
    frozen = pt.ladder()
    pt.record_lnprob(True)
    snaps, mom = [], np.zeros((T, 2))
    for _ in range(3):
        pt.step()
        snaps.append(pt.lnprob())
        mom = mom + R.moments(snaps[-1])
    np.testing.assert_array_equal(pt.ladder(), frozen)  # recording passes kappa = 0
    assert pt.nrecorded == 3 and pt.nadapt == 1
    allv = np.stack(snaps).transpose(1, 0, 2).reshape(T, -1)  # [T][3 W]
    mean, std = pt.mean_lnprob()
    np.testing.assert_allclose(mean, allv.mean(1), rtol=RTOL, atol=0)
    rmean, rstd = R.mean_std(mom, 3 * W)
    np.testing.assert_allclose(mean, rmean, rtol=RTOL, atol=0)
    # std: E[l^2] - mean^2 cancels; a relative error e of the two terms becomes e E[l^2] / var in the
    # variance and half that in its root
    amp = (allv * allv).mean(1) / allv.var(1)
    print(f"std {std}, numpy's {allv.std(1)}, amplification {amp}")
    assert (np.abs(std - allv.std(1)) <= RTOL * amp * allv.std(1)).all()
    est, coarse = pt.log_evidence_ratio()
    np.testing.assert_allclose([est, coarse], R.evidence(frozen, rmean), rtol=RTOL, atol=0)
    assert est != coarse and np.isfinite([est, coarse]).all()
    # the accumulators travel with a checkpoint
    pt.checkpoint(tmp_path / "pt.npz")
    r = _sampler(s, obs, X)
    r.restore(tmp_path / "pt.npz")
    assert r.recording and r.nrecorded == 3 and not r.adapt
    np.testing.assert_array_equal(r.mean_lnprob()[0], mean)
    pt.record_lnprob(False)
    pt.step()
    np.testing.assert_array_equal(pt.mean_lnprob()[0], mean)  # off: nothing more is added
