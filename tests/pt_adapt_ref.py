"""Plain-numpy restatement of the ladder dynamics, the lnp moments and the thermodynamic integral
(rvm_tempering.hip pt_ladder_stats_kernel / pt_ladder_adapt_kernel, rvmcmc/tempering.py).

Every expression is evaluated in the device's order (left to right, Python floats, no fused
multiply-add); the only operation that may differ from the device's is exp, by <= 1 ulp on each side.
"""
import math

import numpy as np

BLOCK = 256  # threads of one row's block in pt_ladder_stats_kernel


def kappa(n, lag, time):
    """The gain of update n (n updates done before it)."""
    return (lag / (n + lag)) / time


def _exp(x):
    try:
        return math.exp(x)
    except OverflowError:  # the device's exp gives +inf
        return math.inf


def ladder_rule(betas, A, kap):
    """The dynamics on betas [T] from the ratios A [T-1] -> (new betas, refused: 0 or 1).  Both end
    temperatures stay; no drive (every dS == 0) or T <= 2 returns the ladder itself, bit for bit; a
    result that is not finite or not strictly decreasing is refused and the ladder returned as is."""
    b = [float(v) for v in betas]
    T = len(b)
    if T < 3:
        return np.array(b), 0
    new = list(b)
    ok, driven = True, False
    tm = 1.0 / b[0]
    acc, prev = tm, b[0]
    for i in range(T - 2):
        dS = kap * (float(A[i]) - float(A[i + 1]))
        if dS != 0.0:
            driven = True
        tn = 1.0 / b[i + 1]
        dT = (tn - tm) * _exp(dS)
        acc = acc + dT
        nb = 1.0 / acc if acc != 0.0 else math.inf
        if not math.isfinite(nb) or not prev > nb:
            ok = False
        new[i + 1] = nb
        prev, tm = nb, tn
    if not prev > b[T - 1]:
        ok = False
    if not driven:
        return np.array(b), 0
    if not ok:
        return np.array(b), 1
    return np.array(new), 0


def update(betas, swapped, prev_totals, W, kap):
    """One rvm_pt_ladder_update without the moments: swapped [T-1][W] cumulative counters,
    prev_totals int64 [T-1] -> (new betas, ratios [T-1], new prev_totals, refused)."""
    total = np.asarray(swapped, dtype=np.int64).reshape(len(betas) - 1, -1).sum(1)
    count = total - np.asarray(prev_totals, dtype=np.int64)
    A = count.astype(np.float64) / float(W)
    new, refused = ladder_rule(betas, A, kap)
    return new, A, total, refused


def _block_sum(v):
    """The device's order: thread i adds v[i], v[i + 256], ... in turn, then a tree over 256 slots."""
    v = np.asarray(v, dtype=np.float64)
    slots = np.zeros(BLOCK)
    for j0 in range(0, len(v), BLOCK):
        chunk = v[j0:j0 + BLOCK]
        slots[:len(chunk)] = slots[:len(chunk)] + chunk
    s = BLOCK // 2
    while s > 0:
        slots[:s] = slots[:s] + slots[s:2 * s]
        s //= 2
    return float(slots[0])


def moments(lnp):
    """lnp [T][W] (half 0's walkers first, as PTSampler.lnprob() gives them) -> [T][2]: sum lnp, sum lnp^2."""
    lnp = np.asarray(lnp, dtype=np.float64)
    return np.array([[_block_sum(r), _block_sum(r * r)] for r in lnp])


def mean_std(mom, n):
    """Accumulated moments [T][2] over n values per temperature -> (mean [T], std [T])."""
    mean = mom[:, 0] / float(n)
    return mean, np.sqrt(np.maximum(mom[:, 1] / float(n) - mean * mean, 0.0))


def evidence(betas, mean):
    """(estimate, coarse): the trapezoid of mean over beta from betas[-1] up to betas[0], hottest
    interval first, over every temperature and over every second one (0, 2, ..., and the hottest)."""
    b, m = [float(v) for v in betas], [float(v) for v in mean]

    def trap(idx):
        s = 0.0
        for k in range(len(idx) - 1, 0, -1):
            i, j = idx[k - 1], idx[k]
            s = s + (b[i] - b[j]) * (0.5 * (m[i] + m[j]))
        return s

    fine = list(range(len(b)))
    coarse = [i for i in fine if i % 2 == 0]
    if coarse[-1] != fine[-1]:
        coarse.append(fine[-1])
    return trap(fine), trap(coarse)
