"""Restatement of the periodogram kernels (rvm_gls.hip, rvmcmc/periodogram.py) from the definition in
include/rvmcmc.h.  Nothing here touches the device or the library.

fma: exact -- for finite arguments float(Fraction(a) * Fraction(b) + Fraction(c)), one rounding; the sign of a
zero result and non-finite arguments by IEEE's rules.  About 8 us a call, so a case stays within 3e5 restated
fmas (2 N F S): restate chosen k of a long call.
phase: f_k, x, r of step 1 in float64, bit for bit what the device computes.
trig_mp / trig_double: sin and cos of 2 pi r in 50-digit mpmath, the truth for the device's sincospi, and the
same rounded to double, which stands in for the basis where no device is at hand.
power: steps 2-4 on a given basis, bit for bit.
"""
import math
from fractions import Fraction

import numpy as np

U = 2.0 ** -53

# max |device - mpmath| / 2^-53 of the device library's sincospi(2 r) over tests/test_gpu_gls.py's arguments
# (test_basis_trig_against_mpmath), sin and cos together.  Measured on an MI355X, ROCm 7.2.0, 2026-10-21.
# The test asserts 2 x this: the factor is for arguments the sample does not hit.
E_TRIG_MEASURED = 0.7205
# whether the device's values at 2 r in {0, +-1/2, +-1} were exactly 0 or +-1 in that run
TRIG_EXACT_AT_QUARTERS = True


def fma(a, b, c):
    """a * b + c with one rounding (float64, round to nearest even)."""
    a, b, c = float(a), float(b), float(c)
    if not (math.isfinite(a) and math.isfinite(b) and math.isfinite(c)):
        if math.isnan(a) or math.isnan(b) or math.isnan(c):
            return math.nan
        if math.isinf(a) or math.isinf(b):
            if a == 0.0 or b == 0.0:
                return math.nan  # 0 x inf
            p = math.copysign(math.inf, math.copysign(1.0, a) * math.copysign(1.0, b))
            return math.nan if math.isinf(c) and c != p else p
        return c  # a finite product and an infinite c
    exact = Fraction(a) * Fraction(b) + Fraction(c)
    if exact == 0:
        # an exact zero: the common sign of the product and c when both are zeros of one sign, else +0
        sp = math.copysign(1.0, a) * math.copysign(1.0, b)
        if (a == 0.0 or b == 0.0) and c == 0.0 and sp < 0 and math.copysign(1.0, c) < 0:
            return -0.0
        return 0.0
    try:
        return float(exact)  # correctly rounded, subnormals included; a negative that underflows gives -0
    except OverflowError:
        return math.inf if exact > 0 else -math.inf


def phase(tau, f0, df, k0, ks):
    """(f [K], x [K][N], r [K][N]) of step 1 for the frequency indices ks (relative to k0)."""
    tau = np.asarray(tau, dtype=np.float64)
    f = np.array([fma(float(int(k0) + int(k)), df, f0) for k in ks], dtype=np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        x = f[:, None] * tau[None, :]
        r = x - np.rint(x)
    return f, x, r


def trig_mp(r):
    """(sin, cos) of 2 pi r as lists of 50-digit mpf."""
    import mpmath

    with mpmath.workdps(50):
        a = [2 * mpmath.pi * mpmath.mpf(float(v)) for v in np.asarray(r, dtype=np.float64).ravel()]
        return [mpmath.sin(v) for v in a], [mpmath.cos(v) for v in a]


def trig_double(r):
    """(sin, cos) of 2 pi r rounded to double from mpmath, in r's shape."""
    r = np.asarray(r, dtype=np.float64)
    s, c = trig_mp(r)
    return (np.array([float(v) for v in s]).reshape(r.shape), np.array([float(v) for v in c]).reshape(r.shape))


def trig_error_units(got_sin, got_cos, r):
    """max |got - mpmath| / 2^-53 over sin and cos at the arguments r."""
    import mpmath

    s, c = trig_mp(r)
    with mpmath.workdps(50):
        worst = mpmath.mpf(0)
        for got, want in ((np.asarray(got_sin).ravel(), s), (np.asarray(got_cos).ravel(), c)):
            for g, t in zip(got, want):
                worst = max(worst, abs(mpmath.mpf(float(g)) - t))
        return float(worst / mpmath.mpf(2) ** -53)


def frequency_sums(c, s, w, float_mean):
    """Step 2 for one frequency: (u [N], v [N], CC, SS, CS) from c, s, w [N] (Python floats)."""
    C = S = 0.0
    if float_mean:
        for wi, ci, si in zip(w, c, s):
            C = fma(wi, ci, C)
            S = fma(wi, si, S)
    CC = SS = CS = 0.0
    u, v = [], []
    for wi, ci, si in zip(w, c, s):
        ct, st = ci - C, si - S
        ui, vi = wi * ct, wi * st
        CC = fma(ui, ct, CC)
        SS = fma(vi, st, SS)
        CS = fma(ui, st, CS)
        u.append(ui)
        v.append(vi)
    return u, v, CC, SS, CS


def series_sums(y, w, float_mean):
    """Step 3 for one series: (z [N], YY) from y, w [N]."""
    m = 0.0
    if float_mean:
        for wi, yi in zip(w, y):
            m = fma(wi, yi, m)
    z, YY = [], 0.0
    for wi, yi in zip(w, y):
        zi = yi - m
        z.append(zi)
        YY = fma(wi * zi, zi, YY)
    return z, YY


def _div(a, b):
    a, b = np.float64(a), np.float64(b)
    with np.errstate(all="ignore"):
        return float(a / b)


def power(c, s, w, data, model=None, float_mean=True, n_series=None):
    """Steps 2-4: p [K][S] float64 from the basis c, s [K][N], the weights w [N], data [N] and model [N][S]
    (None: data alone, n_series columns of it, default 1)."""
    c, s = np.asarray(c, dtype=np.float64), np.asarray(s, dtype=np.float64)
    w = [float(v) for v in np.asarray(w, dtype=np.float64)]
    data = np.asarray(data, dtype=np.float64)
    if model is None:
        S = 1 if n_series is None else int(n_series)
        Y = np.repeat(data[:, None], S, 1)
    else:
        model = np.asarray(model, dtype=np.float64)
        S = model.shape[1]
        with np.errstate(invalid="ignore", over="ignore"):
            Y = data[:, None] - model
    series = []
    for j in range(S):
        col = [float(v) for v in Y[:, j]]
        if model is None and j > 0:
            series.append(series[0])
        else:
            series.append(series_sums(col, w, float_mean))
    out = np.empty((c.shape[0], S))
    for k in range(c.shape[0]):
        u, v, CC, SS, CS = frequency_sums([float(x) for x in c[k]], [float(x) for x in s[k]], w, float_mean)
        D = CC * SS - CS * CS
        for j, (z, YY) in enumerate(series):
            if model is None and j > 0:
                out[k, j] = out[k, 0]
                continue
            YC = YS = 0.0
            for ui, vi, zi in zip(u, v, z):
                YC = fma(ui, zi, YC)
                YS = fma(vi, zi, YS)
            num = ((SS * YC) * YC + (CC * YS) * YS) - (2.0 * (CS * YC)) * YS
            out[k, j] = _div(num, YY * D)
    return out


def normalised_weights(sigma):
    """w = (1 / sigma^2) / sum, as rvmcmc/periodogram.py forms it."""
    sigma = np.asarray(sigma, dtype=np.float64)
    iv = 1.0 / (sigma * sigma)
    return iv / iv.sum()


def gls_host(t, y, sigma, f0, df, n_freq, float_mean=True, t_ref=None):
    """The whole periodogram on the host with mpmath's sin/cos rounded to double as the basis: (freq, p)."""
    t = np.asarray(t, dtype=np.float64)
    tau = t - ((t.min() + t.max()) / 2.0 if t_ref is None else t_ref)
    f, _, r = phase(tau, f0, df, 0, range(n_freq))
    s, c = trig_double(r)
    return f, power(c, s, normalised_weights(sigma), y, None, float_mean)[:, 0]


# ---- the end-to-end case tests/test_gpu_gls.py runs and tests/test_gls_ref_cpu.py checks on the host ----------
# conftest.s2_obs_oracle(E2E_SEED, E2E_NPOINTS): the S2 two-planet system observed, fitted with planet 1 alone
E2E_SEED, E2E_NPOINTS, E2E_NFREQ = 2017, 20, 24


def orbital_frequency(planet):
    """1 / (2 pi a^1.5 / sqrt(1 + m)), cycles per code time unit."""
    return 1.0 / (2.0 * math.pi * planet["a"] ** 1.5 / math.sqrt(1.0 + planet["m"]))


def grid_around(t, f_centre, n_freq=E2E_NFREQ, oversample=5):
    """(f0, df, n_freq): n_freq frequencies of spacing 1 / (oversample T) centred on f_centre."""
    t = np.asarray(t, dtype=np.float64)
    df = 1.0 / (oversample * float(t.max() - t.min()))
    k_lo = max(int(round(f_centre / df)) - n_freq // 2, 1)
    return k_lo * df, df, n_freq
