"""CPU half of the step-unit tier U0: the constants tests/step_ref.py writes down are what wh_ref's
float run attains against the 40-digit truth, the inputs are what the tier promises, and a float
restatement of the drift's solver choice predicts that every reachable path class is populated
(the GPU test takes the condition from the device's own path codes)."""
import math

import numpy as np
import pytest
from mpmath import mp, mpf

import step_ref as S


def test_written_constants_are_the_float_runs_measure():
    """K = 3 x the largest ratio of wh_ref's float run per entry point, and the stumpff_full yardstick;
    the float run is finite on every input."""
    assert np.isfinite(S.drift_problem()["float_ratio"]).all()
    for n, d in S.NP_D3:
        assert np.isfinite(S.setup_problem(n, d)["float_ratio"]).all(), (n, d)
        assert all(np.isfinite(S.kick_problem(n, d)[k][2]).all() for k in ("full", "half")), (n, d)
    assert np.isfinite(S.stumpff_problem()["float_err"]).all()
    measured = S.measured_constants()
    print("measured K_DRIFT, K_SETUP, K_KICK, STUMPFF_FULL_BOUND:", measured)
    for got, written in zip(measured, (S.K_DRIFT, S.K_SETUP, S.K_KICK, S.STUMPFF_FULL_BOUND)):
        assert abs(got - written) <= S.K_DIGITS * written, (measured, written)


def test_drift_inputs():
    p = S.drift_problem()
    X, n_planar = p["x"], p["n_planar"]
    assert len(X) <= 1536 and 0 < n_planar < len(X)
    assert (X[:n_planar, 2] == 0).all() and (X[:n_planar, 5] == 0).all()
    assert (X[n_planar:, 2] != 0).all() and (X[n_planar:, 5] != 0).all()
    assert (X[:, 7] > 0).sum() > 500 and (X[:, 7] < 0).sum() > 500  # both directions
    r = np.sqrt((X[:, :3] ** 2).sum(1))
    beta = 2 * X[:, 6] / r - (X[:, 3:6] ** 2).sum(1)
    assert (beta < 0).sum() >= 100  # hyperbolic states
    # |dt| from P/224 to 0.6 P on the bound orbits of the grid
    b = beta[:len(S.ECC[:-1]) * len(S.ANOM) * len(S.DT_P) * 2]
    per = 2 * math.pi * X[:len(b), 6] / b ** 1.5
    frac = np.abs(X[:len(b), 7]) / per
    assert abs(frac.min() * 224 - 1) < 1e-9 and abs(frac.max() / 0.6 - 1) < 1e-9


@pytest.mark.parametrize("variant", S.SHIPPED + S.VARIANT_BUILDS, ids=S.variant_name)
def test_predicted_path_classes_are_populated(variant):
    p = S.drift_problem()
    X = p["x"] if variant[2] else p["x"][:p["n_planar"]]
    c = S.predicted_counts(X, variant)
    print(S.variant_name(variant), dict(zip(S.PATH_NAMES, c)))
    for k in S.reachable(variant[1]):
        assert c[k] >= S.MIN_CLASS, (S.PATH_NAMES[k], c)
    if S.acc_of(variant[1]) not in (1, 2, 4):
        assert c[S.ZAWARE] == 0 and c[S.TAYLOR] == 0


@pytest.mark.parametrize("np_,inclined", S.NP_D3)
def test_setup_inputs(np_, inclined):
    walkers, rej = S.setup_items(np_, inclined)
    W = len(walkers)
    L = 1 if np_ == 1 else (2 if np_ == 2 else 4)
    per_wave = 64 // L
    assert W > per_wave and W % per_wave != 0  # more than one wave, the last partly filled
    assert any(rej) and not all(rej)
    assert any(rej[w] != rej[w + 1] and (w + 1) % per_wave for w in range(W - 1))  # rejected beside valid in one wave
    if np_ >= 3:
        assert rej[15] and rej[16] and not rej[0]  # a wave's last group and the next wave's first
    ok = [p for wk, b in zip(walkers, rej) if not b for p in wk]
    e = [math.hypot(p[2], p[3]) for p in ok]
    assert max(e) > 0.989 and max(abs(p[4]) for p in ok) > 999 and min(p[4] for p in ok) < -999
    for sh in (1, -1):
        for sk in (1, -1):
            assert any(p[2] * sh > 0 and p[3] * sk > 0 for p in ok)
    if inclined:
        assert max(math.hypot(p[5], p[6]) for p in ok) > 1.999
    for wk, b in zip(walkers, rej):
        assert b == (S.R.prior_hard(wk, inclined) or any(not math.isfinite(p[4]) for p in wk))


@pytest.mark.parametrize("np_,inclined", S.NP_D3)
def test_kick_inputs_decide_the_encounter_bit(np_, inclined):
    p = S.kick_problem(np_, inclined)
    assert min(p["margin"]) >= 1e-9
    assert any(p["enc"]) and not all(p["enc"])
    close = [m for m in p["margin"] if m < 2 * S.EXIT_MARGIN]
    assert len(close) >= len(p["items"]) // 2 - 1  # just inside and just outside the exit distance
    ms = [m for it in p["items"] for m in it[2]]
    assert min(ms) == 5e-6 and max(ms) <= 1e-2 and max(ms) > 5e-3


def test_item_counts():
    assert sum(S.SETUP_W[n] for n, _ in S.NP_D3) <= 1536
    assert len(S.stumpff_items()) == 1536 and len(S.recip_items()) == 1536
    z = S.stumpff_items()
    assert z.min() == -40 and z.max() == 40 and (np.abs(z) <= 0.1).sum() > 400


def test_series_bound_holds_for_a_plain_horner_evaluation():
    """The derived STUMPFF23_BOUND holds for the same Horner chain in plain double (two roundings per
    step where the kernel's fma has one: the bound's inner terms are small enough to cover both)."""
    sp = S.stumpff_problem()
    with mp.workdps(S.DPS):
        for nt, B in S.STUMPFF_B.items():
            worst = 0.0
            for z, t in zip(sp["z"], sp["truth"]):
                if abs(z) <= B:
                    c2, c3 = S._series(float(z), nt)
                    worst = max(worst, float(abs(mpf(c2) - t[2]) / abs(t[2])) / S.U, float(abs(mpf(c3) - t[3]) / abs(t[3])) / S.U)
            print(nt, worst)
            assert worst <= S.STUMPFF23_BOUND, (nt, worst)


def test_probe_library_is_built_and_separate():
    """build() leaves rvmcmc/librvm_step_probe.so beside librvmcmc.so: it exports the five entry
    points, refuses an instantiation that does not exist before any HIP call, and the product
    library neither exports its symbols nor is loaded through it."""
    import ctypes as C
    import os

    import rvmcmc
    from rvmcmc import _lib

    lib = C.CDLL(os.path.join(os.path.dirname(os.path.abspath(rvmcmc.__file__)), "librvm_step_probe.so"))
    names = ("rvm_probe_drift", "rvm_probe_stumpff", "rvm_probe_recip", "rvm_probe_setup", "rvm_probe_kick")
    for f in names:
        assert hasattr(lib, f), f
    assert lib.rvm_probe_drift(5, 1, 0, 0, 1, 64, None, None, None, None, None, None) == -1  # no NT = 5
    assert lib.rvm_probe_drift(6, 2, 1, 0, 1, 64, None, None, None, None, None, None) == -1  # ACC 1 is planar only
    assert lib.rvm_probe_drift(6, 1, 0, 0, 1, 0, None, None, None, None, None, None) == -1   # no items
    assert lib.rvm_probe_setup(5, 0, 1, None, C.c_double(1.0), None, None) == -1
    product = _lib.load()
    assert not any(hasattr(product, f) for f in names)
    assert not any(f.startswith("rvm_probe") for f in _lib.SIGNATURES)
