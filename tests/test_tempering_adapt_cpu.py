"""The adaptive ladder and the evidence, the parts that need no GPU: the constructor's and the entry
point's refusals, the numpy restatement's edge cases (tests/pt_adapt_ref.py), and the input of
tests/test_gpu_tempering_adapt.py run through the restatement with the oracle as the likelihood."""
import ctypes as C

import numpy as np
import pytest

import pt_adapt_ref as R
import pt_ref
from conftest import S2_PLANETS, s2_obs_oracle
from support import PT_ADAPT_CASE as CASE, oracle_logl_fn as _oracle_fn, s2_state_and_obs, state_scales

from rvmcmc import _lib, state
from rvmcmc.tempering import PTSampler, default_betas, log_evidence_ratio


# ---- 1. refusals without a device -----------------------------------------------------------------

def test_constructor_refuses_bad_adaptation_settings_before_any_device_use():
    s = state.State(planets=[dict(p) for p in S2_PLANETS])
    obs = s2_obs_oracle()
    for bad in (0, -1.0, float("inf"), float("nan")):
        with pytest.raises(ValueError, match="adaptation_lag"):
            PTSampler(3, 24, s, obs, adapt=True, adaptation_lag=bad)
        with pytest.raises(ValueError, match="adaptation_time"):
            PTSampler(3, 24, s, obs, adaptation_time=bad)
    assert "_rvm_plans" not in obs.__dict__  # no plan was asked for: nothing reached the device


def test_recording_while_adapting_is_refused():
    pt = PTSampler.__new__(PTSampler)  # record_lnprob reads host attributes only
    pt.ntemps, pt.adapt, pt.recording = 3, True, False
    with pytest.raises(ValueError, match="freeze_ladder"):
        pt.record_lnprob(True)
    assert pt.recording is False
    pt.record_lnprob(False)  # turning it off is always allowed
    pt.adapt = False
    pt.record_lnprob(True)
    assert pt.recording is True
    pt.ntemps = 1  # one temperature has no ladder to integrate over (and the entry point launches nothing)
    with pytest.raises(ValueError, match="two temperatures"):
        pt.record_lnprob(True)


def test_ladder_update_refuses_bad_arguments_without_a_device():
    lib = _lib.load()
    buf = (C.c_double * 16)(*([0.5] * 16))
    p = C.cast(buf, C.c_void_p)
    names = ("swapped", "lnp0", "lnp1", "betas", "swap_totals_prev", "ratios_out", "n_refused", "workspace")

    def update(n_temps=3, n_half=1, kappa=0.5, lnp_moments=p, **null):
        a = {k: (None if k in null else p) for k in names}
        return lib.rvm_pt_ladder_update(n_temps, n_half, a["swapped"], a["lnp0"], a["lnp1"], kappa, a["betas"],
                                        a["swap_totals_prev"], a["ratios_out"], a["n_refused"], lnp_moments,
                                        a["workspace"], None)

    def refused(rc, word):
        msg = lib.rvm_last_error()
        assert rc < 0 and word in msg and b"rvm_pt_ladder_update" in msg, (rc, msg)

    refused(update(n_temps=0), b"n_temps")
    refused(update(n_half=0), b"n_half")
    refused(update(n_temps=1 << 16, n_half=1 << 15), b"int32")  # n_temps * W = 2^32
    refused(update(kappa=-1e-300), b"kappa")
    refused(update(kappa=float("nan")), b"kappa")
    refused(update(kappa=float("inf")), b"kappa")
    for k in names:
        refused(update(**{k: True}), k.encode())
    # one temperature has no ladder: 0 without a launch, whatever the arrays
    assert lib.rvm_pt_ladder_update(1, 4, None, None, None, 0.5, None, None, None, None, None, None, None) == 0
    refused(lib.rvm_pt_ladder_update(1, 4, None, None, None, -1.0, None, None, None, None, None, None, None), b"kappa")


# ---- 2. the restatement's edge cases --------------------------------------------------------------

def test_restatement_two_temperatures_change_nothing():
    b = np.array([1.0, 0.37])
    new, A, total, refused = R.update(b, np.full((1, 24), 3), np.array([12]), 24, 20.0)
    np.testing.assert_array_equal(new, b)
    np.testing.assert_array_equal(A, [(72 - 12) / 24.0])
    np.testing.assert_array_equal(total, [72])
    assert refused == 0
    np.testing.assert_array_equal(R.ladder_rule([1.0], [], 1.0)[0], [1.0])


def test_restatement_refuses_an_interior_that_overshoots_the_hottest_temperature():
    b = np.array([1.0, 0.5000001, 0.5])
    sw = np.zeros((2, 24), dtype=int)
    sw[0] = 1  # counts [24, 0] of W = 24
    new, A, total, refused = R.update(b, sw, np.zeros(2, dtype=np.int64), 24, 20.0)
    np.testing.assert_array_equal(A, [1.0, 0.0])
    # 1 / (1 + (1/0.5000001 - 1) e^20) ~ 2e-9: far below the fixed hottest beta 0.5
    assert 1.0 / (1.0 + (1.0 / b[1] - 1.0) * np.exp(20.0)) < b[2]
    assert refused == 1
    np.testing.assert_array_equal(new, b)
    np.testing.assert_array_equal(total, [24, 0])


def test_restatement_worked_example():
    b = np.array([1.0, 0.6, 0.3, 0.1])
    sw = np.zeros((3, 24), dtype=int)
    sw[0] = 1
    sw[2, :12] = 1  # counts [24, 0, 12]
    new, A, _, refused = R.update(b, sw, np.zeros(3, dtype=np.int64), 24, 1.0)
    assert refused == 0
    np.testing.assert_array_equal(A, [1.0, 0.0, 0.5])
    assert new[0] == 1.0 and new[3] == 0.1
    # by hand: T = 1, 5/3, 10/3, 10; dT = (2/3) e, (5/3) e^-0.5
    t1 = 1.0 + (2.0 / 3.0) * np.e
    t2 = t1 + (5.0 / 3.0) * np.exp(-0.5)
    np.testing.assert_allclose(new[1:3], [1.0 / t1, 1.0 / t2], rtol=1e-14)
    np.testing.assert_allclose(new[1:3], [0.35559502, 0.26156973], rtol=2e-8)


def test_restatement_equal_ratios_and_zero_gain_leave_the_ladder_bit_identical():
    rng = np.random.default_rng(11)
    for T in (3, 5, 16):
        b = np.sort(rng.uniform(0.05, 1.0, T))[::-1].copy()
        b[0] = 1.0
        new, refused = R.ladder_rule(b, np.full(T - 1, 0.375), 50.0)
        np.testing.assert_array_equal(new, b)
        assert refused == 0
        new, refused = R.ladder_rule(b, rng.random(T - 1), 0.0)  # kappa = 0: what record_lnprob passes
        np.testing.assert_array_equal(new, b)
        assert refused == 0
        moved, refused = R.ladder_rule(b, np.linspace(0.1, 0.9, T - 1), 0.5)  # hotter pairs exchange more
        assert refused == 0 and moved[0] == b[0] and moved[-1] == b[-1]
        assert (moved[1:-1] > b[1:-1]).all() and (np.diff(moved) < 0).all()  # ... so the interior moves colder


def test_restatement_moments_and_evidence():
    rng = np.random.default_rng(5)
    lnp = -40.0 * rng.random((3, 516))
    m = R.moments(lnp)
    np.testing.assert_allclose(m[:, 0], lnp.sum(1), rtol=516 * 1.2e-16)
    np.testing.assert_allclose(m[:, 1], (lnp * lnp).sum(1), rtol=516 * 1.2e-16)
    mean, std = R.mean_std(2.0 * m, 2 * 516)
    np.testing.assert_allclose(mean, lnp.mean(1), rtol=1e-13)
    np.testing.assert_allclose(std, lnp.std(1), rtol=1e-11)
    # the trapezoid of a straight line is exact, fine and coarse, for odd and even T
    for T in (2, 3, 4, 5, 8):
        b = np.sort(rng.uniform(0.05, 1.0, T))[::-1].copy()
        b[0] = 1.0
        fine, coarse = R.evidence(b, 3.0 * b - 7.0)
        exact = 1.5 * (1.0 - b[-1] ** 2) - 7.0 * (1.0 - b[-1])
        np.testing.assert_allclose([fine, coarse], exact, rtol=1e-13)
        f2, c2 = R.evidence(b, -1.0 / b)  # a curved integrand: the coarse rule differs
        assert T < 3 or f2 != c2
        np.testing.assert_array_equal(log_evidence_ratio(b, -1.0 / b), (f2, c2))  # the package's is the same sum


# ---- 3. the GPU test's input through the restatement, the oracle as likelihood --------------------

def test_restatement_adapts_on_the_gpu_tests_input():
    """The input of test_gpu_tempering_adapt.py's full iterations (S2, fixed-step plan, T = 4, W = 24,
    rng 0, 4 iterations, default ladder, lag 10, time 2, an update after every sweep) through the
    restatement with the oracle as the likelihood: every walker evaluates cleanly, no decision is near
    a tie, no update is refused, the interior betas move and the end betas do not."""
    s, obs = s2_state_and_obs(fixed_step=True)
    T, W, iters = CASE["T"], CASE["W"], CASE["iters"]
    X, draws = pt_ref.case_inputs(s.get_params(), state_scales(s), T, W, iters, seed=CASE["seed"])
    dt = s.integrator.plan_args(s.planets)[0]
    betas0 = default_betas(T, s.Nvars)
    lad = pt_ref.Ladder(X, betas0, _oracle_fn(s, obs, dt))
    assert (lad.status0 == 0).all() and np.isfinite(lad.lnp).all()
    nsw, prev, refusals, ladders = np.zeros((T - 1, W), dtype=np.int64), np.zeros(T - 1, dtype=np.int64), 0, [betas0]
    for n, d in enumerate(draws):
        for h in (0, 1):
            lad.half_step(h, d["u1"][h], d["u2"][h], d["u3"][h])
        nsw += lad.swap(d["swap"])
        lad.betas, A, prev, refused = R.update(lad.betas, nsw, prev, W, R.kappa(n, CASE["lag"], CASE["time"]))
        refusals += refused
        ladders.append(lad.betas)
        print(f"sweep {n}: counts {np.rint(A * W).astype(int)}, betas {lad.betas}")
    st = np.stack(lad.statuses)
    assert st.size == 2 * iters * T * (W // 2) and (st == 0).all()
    print(f"accept margin {lad.accept_margin:.3g}, swap margin {lad.swap_margin:.3g}")
    assert lad.accept_margin >= 1e-6 and lad.swap_margin >= 1e-6
    assert refusals == 0
    moved = np.abs(ladders[-1] - betas0)
    assert (moved[1:-1] > 1e-3).all(), moved
    assert ladders[-1][0] == betas0[0] and ladders[-1][-1] == betas0[-1]
    assert all((np.diff(b) < 0).all() for b in ladders)
