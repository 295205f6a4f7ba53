"""Restatement of the recorded chain's kernels and diagnostics (rvm_chain.hip, rvmcmc/chain.py) in
np.longdouble (64-bit significand on x86-64: 2^-11 of a double's rounding unit, so its own error is
three orders below every bound the tests derive from u = 2^-53), with an mpmath restatement of the
autocovariance that tests/test_chain_ref_cpu.py holds the longdouble one against.

Nothing here touches the device or the library: record is numpy indexing; moments, autocov, the doubling
window search and split-R-hat follow the definitions in include/rvmcmc.h and driver.integrated_time.
"""
import math

import numpy as np

LD = np.longdouble
U = 2.0 ** -53

# (n, W, phi, offset): x = offset + 1e-3 AR(1), default_rng(index).  The offsets put the cancellation of
# the mean subtraction of real parameters (a ~ 0.88 moving by 1e-3) into the inputs.
AR1_CASES = [(400, 6, 0.8, 0.88), (257, 65, 0.5, 1.55), (1000, 3, 0.95, 2.2), (37, 200, 0.0, 1e-3), (64, 1, 0.6, 0.3)]


def ar1_case(index):
    """x [n][W] float64 of case `index`: a stationary AR(1) per walker, z_0 = e_0 / sqrt(1 - phi^2),
    z_t = phi z_t-1 + e_t with e ~ N(0, 1) drawn [n][W] from default_rng(index)."""
    n, W, phi, offset = AR1_CASES[index]
    e = np.random.default_rng(index).standard_normal((n, W))
    z = np.empty((n, W))
    z[0] = e[0] / math.sqrt(1.0 - phi * phi)
    for t in range(1, n):
        z[t] = phi * z[t - 1] + e[t]
    return offset + 1e-3 * z


def short_trend(W=3):
    """x [5][W]: five steps of the trend 0.25 t, walker w shifted by 0.125 w -- a chain too short for a
    Sokal window (taus = 1, 1.8, 1.6, 0.8, 0: m < 5 taus[m] up to m = 3, so the search ends at n - 1)."""
    return 0.25 * np.arange(5.0)[:, None] + 0.125 * np.arange(float(W))[None, :]


def record(src, src_col0, col_stride, n_cols):
    """rvm_chain_record's gather of src [..., ld]: columns src_col0 + j col_stride, j < n_cols."""
    return np.asarray(src)[..., src_col0:src_col0 + (n_cols - 1) * col_stride + 1:col_stride]


def moments(x, t0=0, t1=None):
    """(mean, m2) [P][W] longdouble of x [n][P][W] over the steps [t0, t1)."""
    y = np.asarray(x, dtype=np.float64)[t0:t1].astype(LD)
    mean = y.sum(0) / LD(y.shape[0])
    d = y - mean
    return mean, (d * d).sum(0)


def autocov(x, t0, t1, lag0, n_lags, with_bound=False):
    """acov [P][n_lags] longdouble of x [n][P][W] over [t0, t1): (1/W) sum_w sum_t y_t y_t+k with the
    exact (longdouble) column means.  with_bound: also the device's error bound per entry,
        mean_w[(n + 3) u A_kw + 2 n u X_w B_w] + (ceil(log2 W) + 2) u mean_w |S_kw|
    (X_w = max |x|, B_w = sum_t |y_t|, A_kw = sum_t |y_t y_t+k|, S_kw the walker's lag sum): the
    mean's error n u X enters every product twice, a walker's n fused multiply-adds and its
    subtractions give (n + 3) u A, the walker tree and the division the last term."""
    xs = np.asarray(x, dtype=np.float64)[t0:t1].astype(LD)
    n, P, W = xs.shape
    y = xs - xs.sum(0) / LD(n)
    X = np.abs(xs).max(0)
    B = np.abs(y).sum(0)
    acov = np.zeros((P, n_lags), dtype=LD)
    bound = np.zeros((P, n_lags), dtype=LD)
    lg = math.ceil(math.log2(W)) if W > 1 else 0
    for j in range(n_lags):
        k = lag0 + j
        prod = y[:n - k] * y[k:]
        S = prod.sum(0)
        acov[:, j] = S.sum(1) / LD(W)
        if with_bound:
            A = np.abs(prod).sum(0)
            bound[:, j] = ((n + 3) * U * A + 2 * n * U * X * B).sum(1) / LD(W) + (lg + 2) * U * np.abs(S).sum(1) / LD(W)
    return (acov, bound) if with_bound else acov


def autocov_mp(x, t0, t1, lag0, n_lags, dps=60):
    """The same autocovariance in mpmath (small inputs only), as floats of the exact result."""
    import mpmath as mp

    with mp.workdps(dps):
        xs = np.asarray(x, dtype=np.float64)[t0:t1]
        n, P, W = xs.shape
        out = np.zeros((P, n_lags))
        for p in range(P):
            cols = []
            for w in range(W):
                v = [mp.mpf(float(a)) for a in xs[:, p, w]]
                m = mp.fsum(v) / n
                cols.append([a - m for a in v])
            for j in range(n_lags):
                k = lag0 + j
                out[p, j] = float(mp.fsum(c[t] * c[t + k] for c in cols for t in range(n - k)) / W)
        return out


def lag_blocks(n, first=64):
    """The window search's lag ranges: [0, 64), [64, 128), [128, 256), ... up to the lag n - 1."""
    out, lo, hi = [], 0, first
    while lo < n:
        out.append((lo, min(hi, n)))
        lo, hi = hi, 2 * hi
    return out


def window_search(x, c=5.0, t0=0, t1=None):
    """The walker-averaged-ACF Sokal window of one parameter x [n][W], the autocovariance asked for block
    by block and no further than the first window: (tau, window, margin, lags computed).  tau = nan
    with window -1 when acov[0] <= 0; taus[n - 1] when no window exists.  margin: the smaller
    |m - c tau(m)| of the window and the lag before it (how far the decision is from a tie; inf without
    a decision)."""
    xs = np.asarray(x, dtype=np.float64)[t0:t1]
    if xs.ndim == 1:
        xs = xs[:, None]
    n = xs.shape[0]
    a0, s, taus = None, LD(0), []
    for lo, hi in lag_blocks(n):
        a = autocov(xs[:, None, :], 0, n, lo, hi - lo)[0]
        if a0 is None:
            a0 = a[0]
            if not a0 > 0:
                return float("nan"), -1, float("inf"), hi
        for j in range(hi - lo):
            s = s + a[j] / a0
            taus.append(2 * s - 1)
            m = lo + j
            if not m < c * taus[m]:
                margin = abs(m - c * taus[m])
                if m > 0:
                    margin = min(margin, abs((m - 1) - c * taus[m - 1]))
                return float(taus[m]), m, float(margin), hi
    return float(taus[n - 1]), n - 1, float("inf"), n


def split_rhat(x, t0=0, t1=None):
    """Plain split-R-hat of one parameter x [n][W]: the first and the last n // 2 steps of every walker
    as 2 W chains of length h; sqrt(((h - 1)/h Wv + B/h) / Wv), Wv the mean within-chain variance, B/h
    the variance of the chain means (both with n - 1 denominators).  nan below h = 2."""
    xs = np.asarray(x, dtype=np.float64)[t0:t1].astype(LD)
    n = xs.shape[0]
    h = n // 2
    if h < 2:
        return float("nan")
    parts = np.concatenate([xs[:h], xs[n - h:]], 1)  # [h][2 W]
    m = parts.sum(0) / LD(h)
    d = parts - m
    within = ((d * d).sum(0) / LD(h - 1)).sum() / LD(parts.shape[1])
    mm = m.sum() / LD(len(m))
    between_over_h = ((m - mm) ** 2).sum() / LD(len(m) - 1)
    if not within > 0:
        return float("nan")
    return float(np.sqrt((LD(h - 1) / LD(h) * within + between_over_h) / within))
