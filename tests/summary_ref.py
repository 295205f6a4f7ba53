"""Restatement of the posterior-summary kernels (rvm_summary.hip, rvmcmc/chain.py summary / draw / predict)
from the definitions in include/rvmcmc.h.  Nothing here touches the device or the library.

quantile: the header's rule over np.sort of the non-NaN values, in float64 with every operation rounded
(the device must give the same bits).  np.sort puts -0 and +0 in input order; the device's order statistic
puts -0 first, so the zeros of the sorted array are rewritten in that order.
cov: in np.longdouble over the same rounded y = x - center (2^-11 of a double's rounding unit), with the
device's error bound per entry:  sum |y_p y_q| / (nW - 1)  times  u (n + 8 + ceil(W / 256) + 2) -- n
additions in the thread, 8 in the tree, the walker blocks in order, 2 for the product's rounding and the
division.
draw: the device's uniforms through philox_ref.uniform2_vec with stream 8, floor and clamp.
"""
import math

import numpy as np

import philox_ref

LD = np.longdouble
U = 2.0 ** -53
RNG_CHAIN_DRAW = 8


def key(v):
    """The order-preserving uint64 key of float64 values: all bits of a negative flipped, the sign bit of
    the others."""
    b = np.ascontiguousarray(np.asarray(v, dtype=np.float64)).view(np.uint64)
    neg = (b >> np.uint64(63)).astype(bool)
    return np.where(neg, ~b, b ^ np.uint64(1 << 63))


def order_statistics(x):
    """The non-NaN values of x ascending, -0 before +0."""
    v = np.asarray(x, dtype=np.float64).ravel()
    v = np.sort(v[~np.isnan(v)])
    zero = v == 0.0
    if zero.any():
        n_neg = int(np.signbit(v[zero]).sum())
        z = np.zeros(int(zero.sum()))
        z[:n_neg] = -0.0
        v[zero] = z
    return v


def quantile(x, q):
    """(out [n_q] float64, m) of the values x (any shape) for the quantiles q."""
    v = order_statistics(x)
    m = len(v)
    q = np.atleast_1d(np.asarray(q, dtype=np.float64))
    out = np.full(len(q), np.nan)
    if m == 0:
        return out, 0
    with np.errstate(invalid="ignore", over="ignore"):
        for j, qj in enumerate(q):
            h = np.float64(qj) * np.float64(m - 1)
            lo = int(math.floor(h))
            g = np.float64(h - lo)
            hi = min(lo + 1, m - 1)
            if g == 0.0 or v[hi] == v[lo]:
                out[j] = v[lo]
            else:
                step = np.float64(g * np.float64(v[hi] - v[lo]))
                out[j] = v[lo] + step
    return out, m


def rows_quantiles(x, q):
    """(out [n_rows][n_q], n_valid [n_rows]) of x [n_rows][...]: every row's values flattened."""
    x = np.asarray(x, dtype=np.float64)
    res = [quantile(x[r], q) for r in range(x.shape[0])]
    return np.stack([r[0] for r in res]), np.array([r[1] for r in res], dtype=np.int64)


def chain_quantiles(chain, t0, t1, q):
    """The same for the parameters of a chain [n][P][W] over the steps [t0, t1)."""
    c = np.asarray(chain, dtype=np.float64)[t0:t1]
    return rows_quantiles(np.transpose(c, (1, 0, 2)), q)


def cov(chain, t0, t1, center, with_bound=False):
    """cov [P][P] longdouble of chain [n][P][W] over [t0, t1) around center [P] (float64: y is rounded as
    on the device); nW = 1 gives NaN.  with_bound: also the device's error bound per entry."""
    x = np.asarray(chain, dtype=np.float64)[t0:t1]
    n, P, W = x.shape
    y = (x - np.asarray(center, dtype=np.float64)[None, :, None]).astype(LD)  # float64 subtraction, then widened
    out = np.full((P, P), np.nan, dtype=LD)
    bound = np.full((P, P), np.nan, dtype=LD)
    if n * W > 1:
        for p in range(P):
            for r in range(P):
                prod = y[:, p, :] * y[:, r, :]
                out[p, r] = prod.sum() / LD(n * W - 1)
                bound[p, r] = np.abs(prod).sum() / LD(n * W - 1) * U * (n + 8 + math.ceil(W / 256) + 2)
    return (out, bound) if with_bound else out


def draw_indices(n, W, t0, S, seed=0, draw_id=0, draws=None):
    """(t [S], w [S]) of rvm_chain_draw over the steps [t0, t0 + n) of W walkers."""
    if draws is None:
        u1, u2 = philox_ref.uniform2_vec(seed, np.arange(S, dtype=np.uint64), draw_id, RNG_CHAIN_DRAW)
    else:
        u1, u2 = np.asarray(draws, dtype=np.float64)

    def index(u, k):
        d = np.floor(u * np.float64(k))
        return np.where(d >= k, k - 1, np.where(d > 0, d, 0)).astype(np.int64)

    return t0 + index(u1, n), index(u2, W)


def draw(chain, t0, t1, S, seed=0, draw_id=0, draws=None):
    """(x_out [P][S], idx [S]) of rvm_chain_draw on chain [n][P][W]."""
    c = np.asarray(chain, dtype=np.float64)
    t, w = draw_indices(t1 - t0, c.shape[2], t0, S, seed, draw_id, draws)
    return c[t, :, w].T.copy(), t * c.shape[2] + w
