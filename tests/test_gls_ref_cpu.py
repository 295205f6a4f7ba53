"""tests/gls_ref.py, the restatement the periodogram kernels are held to, checked on the host: against
scipy.signal.lombscargle (weights, floating mean, normalised) with mpmath's sin/cos rounded to double standing
in for the device's basis, its exact fma against hand-worked cases, and its invariance under the reference
time.  No library, no device."""
import math
import os

import numpy as np
import pytest
from scipy.signal import lombscargle

import gls_ref as G
import oracle as O
from conftest import GOLDEN, S2_PLANETS, s2_obs_oracle

SCIPY_TOL = 1e-12  # absolute, on powers in [0, 1]: scipy's own rounding (measured gap: 7e-15 on HD155358)

_cache = {}


def _hd():
    """HD155358: (t, rv, sigma, f0, df, n_freq) with f = k / (5 T), 305 frequencies up to N / (2 T)."""
    if "hd" not in _cache:
        obs = O.obs_from_file(os.path.join(GOLDEN, "HD155358.vels"))
        t, rv, er = obs.t, obs.rv, obs.err
        T = float(t.max() - t.min())
        df = 1.0 / (5.0 * T)
        _cache["hd"] = (t, rv, er, df, df, int(math.floor(len(t) / (2.0 * T) / df + 1e-9)))
    return _cache["hd"]


def _hd_power(float_mean):
    key = ("hd_power", float_mean)
    if key not in _cache:
        t, rv, er, f0, df, F = _hd()
        _cache[key] = G.gls_host(t, rv, er, f0, df, F, float_mean)
    return _cache[key]


def _scipy(t, y, sigma, freq, float_mean):
    return lombscargle(t, y, 2.0 * np.pi * freq, normalize=True, weights=1.0 / sigma ** 2, floating_mean=float_mean)


@pytest.mark.parametrize("float_mean", [True, False])
def test_hd155358_against_scipy(float_mean):
    t, rv, er, f0, df, F = _hd()
    assert len(t) == 122 and F == 305
    freq, p = _hd_power(float_mean)
    gap = float(np.max(np.abs(p - _scipy(t, rv, er, freq, float_mean))))
    print(f"HD155358 float_mean={float_mean}: max |restatement - scipy| = {gap:.2e}")
    assert gap <= SCIPY_TOL
    if float_mean:
        best = 1.0 / (freq[np.argmax(p)] * 0.01720)
        assert abs(best - 193.9) < 0.5  # HD155358 b


@pytest.mark.parametrize("float_mean", [True, False])
@pytest.mark.parametrize("N", [4, 5, 17, 64])
def test_random_epochs_against_scipy(N, float_mean):
    rng = np.random.default_rng(N)
    t = np.sort(rng.uniform(0.0, 50.0, N))
    sigma = rng.uniform(0.5, 2.0, N) * 1e-4
    y = 1e-3 * np.sin(2 * np.pi * t / 7.3 + 0.4) + sigma * rng.standard_normal(N)
    T = float(t.max() - t.min())
    df = 1.0 / (5.0 * T)
    F = int(math.floor(N / (2.0 * T) / df + 1e-9))
    freq, p = G.gls_host(t, y, sigma, df, df, F, float_mean)
    gap = float(np.max(np.abs(p - _scipy(t, y, sigma, freq, float_mean))))
    print(f"N={N} float_mean={float_mean}: max |restatement - scipy| = {gap:.2e}")
    assert gap <= SCIPY_TOL


def test_reference_time_invariance():
    t, rv, er, f0, df, F = _hd()
    _, p = _hd_power(True)
    _, shifted = G.gls_host(t, rv, er, f0, df, F, True, t_ref=float(t.min()) - 3.0)
    gap = float(np.max(np.abs(p - shifted)))
    print(f"reference time moved by half the span + 3: max |dp| = {gap:.2e}")
    assert gap <= 1e-10


def test_exact_fma_hand_worked():
    u = 2.0 ** -52
    # (1 + u)(1 - u) = 1 - u^2: a rounded product gives 1 and the sum 0; the fma keeps -u^2
    assert (1.0 + u) * (1.0 - u) - 1.0 == 0.0
    assert G.fma(1.0 + u, 1.0 - u, -1.0) == -(2.0 ** -104)
    # a product that cancels c exactly, to the last bit: +0, whatever the signs
    for x, y, c in ((3.0, 5.0, -15.0), (-3.0, 5.0, 15.0), (1.0 + u, 2.0, -(2.0 + 2 * u))):
        r = G.fma(x, y, c)
        assert r == 0.0 and math.copysign(1.0, r) == 1.0
    # one rounding: 2^53 + 1 is not a double; the exact sum rounds to even
    assert G.fma(2.0 ** 27, 2.0 ** 26, 1.0) == 2.0 ** 53
    assert G.fma(2.0 ** 27, 2.0 ** 26, 3.0) == 2.0 ** 53 + 4.0
    assert G.fma(0.1, 10.0, -1.0) == 2.0 ** -54  # 0.1 = (1 + 2^-54 ...)/10 above a tenth: the product's excess
    # zeros: the sum of zeros of one sign keeps it, anything else is +0
    for x, y, c, neg in ((0.0, 1.0, 0.0, False), (-0.0, 1.0, -0.0, True), (0.0, -1.0, -0.0, True),
                         (-0.0, -1.0, -0.0, False), (-0.0, 1.0, 0.0, False), (0.0, 1.0, -0.0, False)):
        r = G.fma(x, y, c)
        assert r == 0.0 and (math.copysign(1.0, r) < 0) == neg, (x, y, c, r)
    assert G.fma(0.0, 5.0, -2.5) == -2.5 and G.fma(-0.0, 5.0, 2.5) == 2.5
    # subnormals: the smallest one squared underflows to a zero of the product's sign; exact sums of them
    tiny = 5e-324
    assert G.fma(tiny, tiny, 0.0) == 0.0 and math.copysign(1.0, G.fma(-tiny, tiny, 0.0)) < 0
    assert G.fma(tiny, 1.0, tiny) == 1e-323
    assert G.fma(tiny, 0.5, 0.0) == 0.0  # half the smallest subnormal: the tie goes to even
    assert G.fma(tiny, 0.5, tiny) == 1e-323  # 1.5 of them: the tie goes to even, two
    assert G.fma(2.0 ** -537, 2.0 ** -537, 0.0) == 2.0 ** -1074
    assert G.fma(2.0 ** -1022, 0.5, 2.0 ** -1074) == 2.0 ** -1023 + 2.0 ** -1074
    # non-finite
    assert G.fma(1e308, 10.0, 0.0) == math.inf and G.fma(-1e308, 10.0, 0.0) == -math.inf
    assert G.fma(math.inf, 1.0, 1.0) == math.inf and math.isnan(G.fma(math.inf, 0.0, 1.0))
    assert math.isnan(G.fma(math.inf, 1.0, -math.inf)) and G.fma(1.0, 1.0, -math.inf) == -math.inf
    assert math.isnan(G.fma(math.nan, 1.0, 1.0)) and math.isnan(G.fma(1.0, 1.0, math.nan))


def test_phase_is_reduced_exactly():
    tau = np.array([-3.75, 0.0, 0.1, 1e3 + 0.5, 123456.789])
    f, x, r = G.phase(tau, 0.25, 0.125, 7, range(3))
    np.testing.assert_array_equal(f, [0.25 + 7 * 0.125, 0.25 + 8 * 0.125, 0.25 + 9 * 0.125])
    np.testing.assert_array_equal(x, f[:, None] * tau[None, :])
    assert np.all(np.abs(r) <= 0.5)
    from fractions import Fraction

    for xv, rv in zip(x.ravel(), r.ravel()):
        assert Fraction(float(xv)) - Fraction(float(rv)) == round(Fraction(float(xv)) - Fraction(float(rv)))


def test_end_to_end_seed_on_the_oracle():
    """The case tests/test_gpu_gls.py runs end to end, on the host: the residuals of the oracle's one-planet RV
    curve (planet 1's true parameters) peak within 1 / T of planet 2's orbital frequency."""
    obs = s2_obs_oracle(G.E2E_SEED, G.E2E_NPOINTS)
    t = np.concatenate([obs.tf, obs.tb])
    rv = np.concatenate([obs.rvf, obs.rvb])
    er = np.concatenate([obs.errorf, obs.errorb])
    model, st, _ = O.get_rv_ias15([dict(S2_PLANETS[0])], t, hill_factor=0.0)
    assert st == 0
    f2 = G.orbital_frequency(S2_PLANETS[1])
    f0, df, F = G.grid_around(t, f2)
    tau = t - (t.min() + t.max()) / 2.0
    f, _, r = G.phase(tau, f0, df, 0, range(F))
    s, c = G.trig_double(r)
    p = G.power(c, s, G.normalised_weights(er), rv, np.asarray(model)[:, None], True)[:, 0]
    T = float(t.max() - t.min())
    print(f"peak at {f[np.argmax(p)]:.5f}, planet 2 at {f2:.5f}, 1/T = {1 / T:.5f}, power {p.max():.3f}")
    assert f[0] < f2 < f[-1]
    assert abs(f[np.argmax(p)] - f2) <= 1.0 / T
