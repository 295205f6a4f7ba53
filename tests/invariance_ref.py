"""Exact invariance tests of the sampler rules: targets, float64 restatements of the transitions with seeded
slips, statistics with known null laws and the analytic rates (tests/test_invariance_ref_cpu.py,
tests/test_gpu_sampler_invariance.py).  numpy, scipy and the other restatements; no torch.

The idea.  A correct transition leaves its target invariant: a state drawn exactly from pi (an ensemble: from
pi^W; a ladder: from prod_t pi_beta_t^W) is, after K transitions, still exactly so distributed.  The W walkers
(C chains) at iteration K are then independent draws from a known law -- no burn-in, no autocorrelation to
estimate -- and every statistic below has a known null distribution.  A wrong rule drifts towards its own
stationary law and misses by many sigma.  The bit-for-bit tests (stretch_ref, pt_ref, smala_ref, philox_ref)
ask whether a kernel does what its restatement says; this asks whether that samples the target, and whether
draws that should be independent are (a shared Philox counter is the same on both sides of a bit comparison).

Layout.  Positions are parameter-major as on the device: an ensemble is X [d][T][W] with lnp [T][W] (T = 1: the
plain stretch move, whose Philox items the tempered ones then are), half h the walkers [h W/2, (h + 1) W/2);
chains are X [P][C].  The draws are the device's: philox_ref.uniform2_vec with the device's items, streams and
iteration.  The log-probabilities are evaluated here in numpy and on the device side of the GPU tests in torch:
the two chains agree up to the last bits of those, that is up to decisions at ties and, for the Gaussian
draws, the last bits of cos(2 pi u).

Thresholds.  Under the null a p-value is uniform and a z-score N(0, 1) (the sums behind the z-scores have at
least 2048 terms).  LOOSE (the device, and what a mutant must miss): every p >= 1e-5, every |z| <= 4.5; with
N statistics over the whole GPU file a correct sampler fails by chance with probability N 1e-5 <= 2e-3
(P(|z| > 4.5) = 6.8e-6 is below 1e-5), which budget() asserts.  STRICT (the reference at the committed seeds):
p >= 1e-3, |z| <= 3.3.  The Philox seeds of CASES were chosen so: a seed at which the reference alone missed
STRICT was replaced by the next one (the claim is that a correct rule passes and every mutant misses by many
sigma, not that any seed passes).  Nothing here was measured on a device.
"""
import functools
import math

import numpy as np
from scipy import integrate, linalg, special, stats

import philox_ref
import pt_ref
import stretch_ref

P_MIN, Z_MAX = 1e-5, 4.5          # loose
P_STRICT, Z_STRICT = 1e-3, 3.3    # strict
BUDGET = 2e-3                     # N P_MIN of a whole GPU file
RHO_MAX = 0.15                    # |correlation with the start|: a frozen sampler has 1
ACC_TOL = 0.02                    # acceptance fraction against the reference's for the same case
# (a rate against its analytic value is a z-score in units of the rate's measured sd, held to Z_MAX like the others)

MUTANTS = {
    "exponent_dim": "stretch accept with dim ln z in place of (dim - 1) ln z",
    "z_uniform": "z uniform on [1/a, a] in place of g(z) ~ 1/sqrt(z)",
    "no_beta": "tempered accept without beta",
    "swap_factor": "exchange factor x 1.15",
    "swap_sign": "exchange sign reversed",
    "mh_no_old": "MH accept on lnp_new alone",
    "no_logdet": "SMALA log q without log det",
    "drift_eps2": "SMALA drift with eps^2 in place of eps^2 / 2 (in the cache: proposal and log q alike)",
    "shared_counter": "accept uniform taken from the propose stream (u3 = u1)",
}


def _orthogonal(rng, d):
    Q, R = np.linalg.qr(rng.standard_normal((d, d)))
    return Q * np.sign(np.diag(R))


def _sym(A):
    return 0.5 * (A + A.T)


# ---- targets --------------------------------------------------------------------------------------------------

class Gauss:
    """N(0, Sigma), Sigma = Q diag(1 .. cond) Q^T full (the stretch move's affine invariance is exercised;
    d = 1: N(0, 1)).  pi_beta = N(0, Sigma / beta).  whiten: sqrt(beta) chol(Sigma)^-1 x, iid N(0, 1).
    lnp = OFFSET - x^T Sigma^-1 x / 2: a correct rule reads differences of log-probabilities only, while a rule
    that reads one alone (MH on exp(lnp_new) > u) happens to be reversible when max lnp = 0 and is not with an
    offset above 0."""

    OFFSET = 2.0

    def __init__(self, d, seed, cond=30.0):
        rng = np.random.default_rng([seed, d])
        self.d = d
        Q = _orthogonal(rng, d)
        self.cov = _sym(Q @ np.diag(np.geomspace(1.0, cond, d) if d > 1 else np.ones(1)) @ Q.T)
        self.chol = np.linalg.cholesky(self.cov)
        self.prec = _sym(np.linalg.inv(self.cov))

    def sample(self, rng, n, beta=1.0):
        return self.chol @ rng.standard_normal((self.d, n)) / math.sqrt(beta)

    def lnp(self, x):
        return self.OFFSET - 0.5 * ((self.prec @ x) * x).sum(0)

    def whiten(self, x, beta=1.0):
        return math.sqrt(beta) * linalg.solve_triangular(self.chol, x, lower=True)

    def unit(self, v):
        """Whitened coordinates [d][n] -> (coordinates of unit variance, a per-walker energy of mean 0 and
        variance 1: (r^2 - d) / sqrt(2 d))."""
        return v, ((v * v).sum(0) - self.d) / math.sqrt(2.0 * self.d)

    def stats(self, v, tag):
        d, n = v.shape
        r2 = (v * v).sum(0)
        out = [(f"{tag} ks x{i}", "p", stats.kstest(v[i], "norm").pvalue) for i in range(d)]
        out.append((f"{tag} ks r2", "p", stats.kstest(r2, stats.chi2(d).cdf).pvalue))
        out += [(f"{tag} mean x{i}", "z", v[i].mean() * math.sqrt(n)) for i in range(d)]
        out.append((f"{tag} sum r2", "z", (r2.sum() - n * d) / math.sqrt(2.0 * n * d)))
        return out


class Quartic:
    """lnp(x) = -sum_i y_i^4 / 4, y = R x, R orthogonal.  Exact draws y_i = +-(4 Gamma(1/4, 1))^(1/4);
    E y^2 = 2 Gamma(3/4) / Gamma(1/4), E y^4 = 1, E y^8 = 5; CDF 1/2 + sgn(v) P(1/4, v^4 / 4) / 2;
    sum_i y_i^4 / 4 ~ Gamma(P/4).  -H = R^T diag(3 y^2) R depends on the position and is not diagonal."""

    M2 = 2.0 * math.gamma(0.75) / math.gamma(0.25)

    def __init__(self, P, seed):
        self.d = P
        self.R = _orthogonal(np.random.default_rng([seed, P, 4]), P)

    def sample(self, rng, n, beta=1.0):
        y = (4.0 * rng.gamma(0.25, 1.0, (self.d, n))) ** 0.25 * np.where(rng.random((self.d, n)) < 0.5, -1.0, 1.0)
        return self.R.T @ y

    def lnp(self, x):
        y = self.R @ x
        return -0.25 * ((y * y) * (y * y)).sum(0)

    def grad(self, x):
        y = self.R @ x
        return -(self.R.T @ (y * y * y))

    def hess(self, x):
        """[P][P][C]"""
        y = self.R @ x
        return -np.einsum("ki,kc,kj->ijc", self.R, 3.0 * y * y, self.R)

    def whiten(self, x, beta=1.0):
        return self.R @ x

    @staticmethod
    def cdf(v):
        return 0.5 + 0.5 * np.sign(v) * special.gammainc(0.25, v ** 4 / 4.0)

    def unit(self, y):
        return y / math.sqrt(self.M2), ((y ** 4).sum(0) / 4.0 - self.d / 4.0) / math.sqrt(self.d / 4.0)

    def stats(self, y, tag):
        P, n = y.shape
        out = [(f"{tag} ks y{i}", "p", stats.kstest(y[i], self.cdf).pvalue) for i in range(P)]
        out.append((f"{tag} ks sum y4/4", "p", stats.kstest((y ** 4).sum(0) / 4.0, stats.gamma(P / 4.0).cdf).pvalue))
        out += [(f"{tag} mean y{i}", "z", y[i].mean() * math.sqrt(n / self.M2)) for i in range(P)]
        out.append((f"{tag} mean y2", "z", ((y ** 2).mean() - self.M2) * math.sqrt(n * P / (1.0 - self.M2 ** 2))))
        out.append((f"{tag} mean y4", "z", ((y ** 4).mean() - 1.0) * math.sqrt(n * P / 4.0)))
        return out


def pair_stats(tgt, va, vb, tag):
    """Independence of two sets of whitened walkers a_k, b_k (same shape [d][n]) that should be independent:
    z = sum a b / sqrt(d n) over the unit-variance coordinates ("lin": a shared or mirrored position) and
    z = sum e_a e_b / sqrt(n) over the unit-variance energies ("sq": a shared scale, such as one z for two
    walkers, which leaves the coordinates uncorrelated).  Mean 0 and variance 1 exactly under the null (the
    moments are the target's, not the sample's: the correlation estimate with null N(0, 1/n), times sqrt(n))."""
    (a, ea), (b, eb) = tgt.unit(va), tgt.unit(vb)
    return [(f"{tag} lin", "z", (a * b).sum() / math.sqrt(a.size)),
            (f"{tag} sq", "z", (ea * eb).sum() / math.sqrt(ea.size))]


def start_rho(v0, v):
    """Largest |sample correlation| of a whitened coordinate with its start value."""
    return max(abs(float(np.corrcoef(v0[i], v[i])[0, 1])) for i in range(v.shape[0]))


def misses(rows, p_min, z_max):
    return [(n, k, v) for n, k, v in rows if not ((k == "p" and v >= p_min) or (k == "z" and abs(v) <= z_max))]


def show(rows):
    """One line per statistic, as tests/test_gpu_stability.py prints its figures (pytest -s)."""
    for n, k, v in rows:
        print(f"{n}: {k} {v:.3e}" if k == "p" else f"{n}: {k} {v:+.2f}", flush=True)


COUNTED = {}


def count(case, rows):
    """Note the statistics a GPU test asserts; budget() holds their number to the chance a correct sampler has."""
    COUNTED[case] = len(rows)


def budget():
    n = sum(COUNTED.values())
    assert n * P_MIN <= BUDGET, (n, COUNTED)
    return n


# ---- analytic rates ---------------------------------------------------------------------------------------------

def default_betas(T, d):
    """rvmcmc.tempering.default_betas (test_invariance_ref_cpu.py holds the two together)."""
    r = 1.0 + 2.0 * math.sqrt(math.log(4.0)) / math.sqrt(d)
    return np.array([r ** -t for t in range(T)], dtype=np.float64)


@functools.lru_cache(maxsize=None)
def _swap_rate(ratio, d):
    k = 0.5 * d
    norm = 1.0 / (2.0 ** k * math.gamma(k))
    top = float(stats.chi2(d).isf(1e-14))

    def pdf(c):
        return norm * c ** (k - 1.0) * math.exp(-0.5 * c) if c > 0.0 else 0.0

    def f(c2, c1):
        return min(1.0, math.exp(0.5 * ((1.0 - 1.0 / ratio) * c1 - (ratio - 1.0) * c2))) * pdf(c1) * pdf(c2)

    # the integrand has a kink on c2 = c1 / ratio: the two sides of it are integrated apart
    lo, _ = integrate.dblquad(f, 0.0, top, 0.0, lambda c1: c1 / ratio, epsabs=1e-9, epsrel=1e-9)
    hi, _ = integrate.dblquad(f, 0.0, top, lambda c1: c1 / ratio, top, epsabs=1e-9, epsrel=1e-9)
    return lo + hi


def swap_rate(b1, b2, d):
    """E min(1, exp((b1 - b2)(L2 - L1))), L_t = -chi2_d / (2 b_t) independent: the exchange rate between
    N(0, Sigma / b1) and N(0, Sigma / b2) at stationarity, b1 > b2.  The exponent is ((1 - b2/b1) c1 -
    (b1/b2 - 1) c2) / 2: the rate depends on the ratio alone (rounded to 12 digits for the cache, so a geometric
    ladder is integrated once)."""
    return _swap_rate(round(b1 / b2, 12), d)


def swap_rate_closed(b1, b2, d):
    """The same by detailed balance: E min(1, r) = 2 P(r > 1) = 2 P(chi2_d / chi2_d' > b1 / b2), an F(d, d) tail."""
    return 2.0 * stats.f(d, d).sf(b1 / b2)


def mh_rate(s):
    """Random-walk acceptance on N(0, 1) with proposal sd s: E min(1, exp((x^2 - (x + s g)^2) / 2))."""
    return 2.0 / math.pi * math.atan(2.0 / s)


# ---- the device's draws -------------------------------------------------------------------------------------------

def normals(seed, items, iteration, base, P):
    """[P][n]: Box-Muller sqrt(-2 ln u0) cos(2 pi u1) of stream base | p << 8 (rvm_stretch.h box_muller)."""
    out = np.empty((P, len(items)))
    for p in range(P):
        u0, u1 = philox_ref.uniform2_vec(seed, items, iteration, base | (p << 8))
        out[p] = np.sqrt(-2.0 * np.log(u0)) * np.cos(2.0 * np.pi * u1)
    return out


# ---- transitions -------------------------------------------------------------------------------------------------

def ensemble_iteration(tgt, X, lnp, betas, seed, it, a=2.0, sweep=True, mutant=None, counts=None):
    """Both stretch half-steps of every temperature, then the exchange sweep (rvm_pt_stretch_propose / _accept,
    rvm_pt_swap; T = 1, beta = 1: rvm_stretch_propose / _accept with s0_begin = h W/2).  In place on X [d][T][W],
    lnp [T][W]; counts: accepted [T] and swapped [T-1] are added to."""
    d, T, W = X.shape
    Wh = W // 2
    b = np.asarray(betas, dtype=np.float64)[:, None]
    rows = np.arange(T)[:, None]
    for h in (0, 1):
        s, o = slice(h * Wh, (h + 1) * Wh), slice((1 - h) * Wh, (2 - h) * Wh)
        items = pt_ref.items(T, W, h).reshape(-1)
        u1, u2 = (u.reshape(T, Wh) for u in philox_ref.uniform2_vec(seed, items, it,
                                                                     philox_ref.RNG_STRETCH_PROPOSE | (h << 8)))
        u3 = philox_ref.uniform2_vec(seed, items, it, philox_ref.RNG_STRETCH_ACCEPT | (h << 8))[0].reshape(T, Wh)
        if mutant == "shared_counter":
            u3 = u1
        z = 1.0 / a + (a - 1.0 / a) * u1 if mutant == "z_uniform" else stretch_ref.stretch_z(u1, a)
        j = stretch_ref.stretch_j(u2, Wh)
        x = X[:, :, s]
        q = stretch_ref.stretch_q(X[:, :, o][:, rows, j], z[None], x)
        lnew, lold = tgt.lnp(q.reshape(d, -1)).reshape(T, Wh), lnp[:, s]
        e = float(d if mutant == "exponent_dim" else d - 1)
        diff = e * np.log(z) + lnew - lold if mutant == "no_beta" else e * np.log(z) + b * lnew - b * lold
        acc = diff > np.log(u3)
        X[:, :, s] = np.where(acc[None], q, x)
        lnp[:, s] = np.where(acc, lnew, lold)
        if counts is not None:
            counts["accepted"] += acc.sum(1)
    if sweep and T > 1:
        u = philox_ref.uniform2_vec(seed, pt_ref.swap_items(T, W).reshape(-1), it, philox_ref.RNG_PT_SWAP)[0]
        swapped = pt_sweep(X, lnp, b[:, 0], u.reshape(T - 1, W), mutant)
        if counts is not None:
            counts["swapped"] += swapped.sum(1)


def pt_sweep(X, lnp, betas, u, mutant=None):
    """The exchange sweep, pairs T-2 .. 0, in place on X [d][T][W], lnp [T][W] -> swapped [T-1][W] bool
    (pt_ref.swap in this layout, with the two seeded slips)."""
    T, W = lnp.shape
    f = {"swap_factor": 1.15, "swap_sign": -1.0}.get(mutant, 1.0)
    swapped = np.zeros((T - 1, W), dtype=bool)
    for p in range(T - 2, -1, -1):
        dd = (betas[p] - betas[p + 1]) * (lnp[p + 1] - lnp[p])
        s = (dd if f == 1.0 else f * dd) > np.log(u[p])
        X[:, p, s], X[:, p + 1, s] = X[:, p + 1, s].copy(), X[:, p, s].copy()
        lnp[p, s], lnp[p + 1, s] = lnp[p + 1, s].copy(), lnp[p, s].copy()
        swapped[p] = s
    return swapped


def mh_step(tgt, X, lnp, scales, step, seed, it, begin, mutant=None, counts=None):
    """rvm_mh_propose / rvm_mh_accept, in place on X [P][C], lnp [C]."""
    P, C = X.shape
    items = np.uint64(begin) + np.arange(C, dtype=np.uint64)
    g = normals(seed, items, it, philox_ref.RNG_MH_PROPOSE, P)
    q = X + (step * np.asarray(scales, dtype=np.float64))[:, None] * g
    lnew = tgt.lnp(q)
    u = philox_ref.uniform2_vec(seed, items, it, philox_ref.RNG_MH_ACCEPT)[0]
    acc = np.exp(lnew if mutant == "mh_no_old" else lnew - lnp) > u
    X[:, acc], lnp[acc] = q[:, acc], lnew[acc]
    if counts is not None:
        counts["accepted"] += acc.sum()


def smala_cache(tgt, X, alpha, eps, mutant=None):
    """rvm_smala_metric from the target's (lp, grad, hess) at X [P][C]: the SoftAbs metric of -H, its inverse's
    Cholesky factor, the drift, log det G^-1 (mcmc.py:135-150), chain-major [C][...]."""
    H = np.moveaxis(tgt.hess(X), 2, 0)
    lam, Q = np.linalg.eigh(-0.5 * (H + np.swapaxes(H, 1, 2)))
    al = alpha * lam
    with np.errstate(divide="ignore", invalid="ignore"):
        lt = np.where(np.abs(al) < 1e-8, 1.0 / alpha, lam / np.tanh(al))
    G = np.einsum("cik,ck,cjk->cij", Q, lt, Q)
    Ginv = np.einsum("cik,ck,cjk->cij", Q, 1.0 / lt, Q)
    half = eps * eps if mutant == "drift_eps2" else 0.5 * eps * eps
    return dict(lp=tgt.lnp(X), mu=X.T + half * np.einsum("cij,jc->ci", Ginv, tgt.grad(X)), G=G,
                L=np.linalg.cholesky(Ginv), logdet=-np.log(lt).sum(1))


def _logq(y, cache, eps, mutant):
    """log N(y; mu, eps^2 G^-1) (mcmc.py:158-162; rvm_smala.hip mvn_logpdf); y [C][P]."""
    dy = y - cache["mu"]
    maha = np.einsum("ci,cij,cj->c", dy, cache["G"], dy)
    P = y.shape[1]
    logdet = 0.0 if mutant == "no_logdet" else cache["logdet"]
    return -0.5 * (maha / (eps * eps) + P * math.log(eps * eps) + logdet + P * math.log(2.0 * math.pi))


def smala_step(tgt, X, cur, alpha, eps, seed, it, begin, mutant=None, counts=None):
    """rvm_smala_propose, rvm_smala_metric at x*, rvm_smala_accept (mcmc.py:144-187): in place on X [P][C] and
    on the current cache."""
    P, C = X.shape
    items = np.uint64(begin) + np.arange(C, dtype=np.uint64)
    zs = normals(seed, items, it, philox_ref.RNG_SMALA_PROPOSE, P)
    xs = cur["mu"] + eps * np.einsum("cij,jc->ci", cur["L"], zs)
    prop = smala_cache(tgt, np.ascontiguousarray(xs.T), alpha, eps, mutant)
    u = philox_ref.uniform2_vec(seed, items, it, philox_ref.RNG_SMALA_ACCEPT)[0]
    ratio = np.exp(prop["lp"] - cur["lp"] + _logq(X.T, prop, eps, mutant) - _logq(xs, cur, eps, mutant))
    acc = ratio > u
    X[:, acc] = xs.T[:, acc]
    for k in cur:
        cur[k][acc] = prop[k][acc]
    if counts is not None:
        counts["accepted"] += acc.sum()


# ---- the cases -----------------------------------------------------------------------------------------------

TARGET_SEED = 7
SMALA_EPS = 1.1   # chosen on the reference for an acceptance of 50 - 75 % (test_invariance_ref_cpu.py)
EQUAL_BETAS = (1.0, 1.0 - 2.5e-13, 1.0 - 5e-13)  # strictly decreasing, within 1e-12 of 1: three ensembles
BIG_BEGIN = 2 ** 33

CASES = {
    "stretch5": dict(kind="ens", d=5, T=1, W=4096, K=64, betas=(1.0,), sweep=False, seed=101),
    # (K = 256: the stretch move's autocorrelation time grows with d, and at d = 17 the reference itself is still
    # correlated 0.58 with its start after 64 iterations and 0.21 after 192, against RHO_MAX = 0.15)
    "stretch17": dict(kind="ens", d=17, T=1, W=4096, K=256, betas=(1.0,), sweep=False, seed=102),
    "pt4": dict(kind="ens", d=5, T=4, W=4096, K=64, betas=tuple(default_betas(4, 5)), sweep=True, seed=103),
    "pt3equal": dict(kind="ens", d=5, T=3, W=4096, K=64, betas=EQUAL_BETAS, sweep=False, seed=104),
    "mh1": dict(kind="mh", d=1, C=8192, K=64, scales=(1.0,), step=2.4, begin=0, seed=105),
    "mh3": dict(kind="mh", d=3, cond=3.0, C=8192, K=64, scales=(0.9, 1.3, 1.8), step=1.0, begin=BIG_BEGIN, seed=106),
    "smala": dict(kind="smala", d=3, C=8192, K=48, alpha=1.0, eps=SMALA_EPS, begin=0, seed=107),
}


@functools.lru_cache(maxsize=None)
def target(case):
    c = CASES[case]
    return Quartic(c["d"], TARGET_SEED) if c["kind"] == "smala" else Gauss(c["d"], TARGET_SEED, c.get("cond", 30.0))


def start(case, n=None):
    """The exact draw a case starts from: [d][T][W] or [P][C] (n: another number of walkers or chains)."""
    c, tgt = CASES[case], target(case)
    rng = np.random.default_rng([TARGET_SEED, c["seed"]])
    if c["kind"] == "ens":
        return np.stack([tgt.sample(rng, n or c["W"], b) for b in c["betas"]], 1)
    return tgt.sample(rng, n or c["C"])


def whitened(case, X):
    """[d][n] per temperature (a list) for an ensemble, [[P][C]] for chains."""
    c, tgt = CASES[case], target(case)
    if c["kind"] == "ens":
        return [tgt.whiten(X[:, t], b) for t, b in enumerate(c["betas"])]
    return [tgt.whiten(X)]


def run(case, mutant=None, seed=None, n=None):
    """The reference's K transitions of a case from start(): dict(X, accept (fraction), swap (rates [T-1]))."""
    c, tgt = CASES[case], target(case)
    seed = c["seed"] if seed is None else seed
    X = start(case, n)
    K = c["K"]
    if c["kind"] == "ens":
        d, T, W = X.shape
        lnp = tgt.lnp(X.reshape(d, -1)).reshape(T, W)
        counts = dict(accepted=np.zeros(T, dtype=np.int64), swapped=np.zeros(max(T - 1, 0), dtype=np.int64))
        for it in range(K):
            ensemble_iteration(tgt, X, lnp, c["betas"], seed, it, 2.0, c["sweep"], mutant, counts)
        return dict(X=X, accept=counts["accepted"].sum() / (K * T * W), swap=counts["swapped"] / (K * W))
    counts = dict(accepted=0)
    if c["kind"] == "mh":
        lnp = tgt.lnp(X)
        for it in range(K):
            mh_step(tgt, X, lnp, c["scales"], c["step"], seed, it, c["begin"], mutant, counts)
    else:
        cur = smala_cache(tgt, X, c["alpha"], c["eps"], mutant)
        for it in range(K):
            smala_step(tgt, X, cur, c["alpha"], c["eps"], seed, it, c["begin"], mutant, counts)
    return dict(X=X, accept=counts["accepted"] / (K * X.shape[1]), swap=np.zeros(0))


@functools.lru_cache(maxsize=None)
def reference(case):
    return run(case)


def analytic_rates(case):
    """[(name, analytic value)] of the rates a case is held to."""
    c = CASES[case]
    if case == "pt4":
        return [(f"swap rate {p}|{p + 1}", swap_rate(c["betas"][p], c["betas"][p + 1], c["d"])) for p in range(3)]
    if case == "mh1":
        return [("acceptance", mh_rate(c["step"] * c["scales"][0]))]
    return []


def measured_rates(case, res):
    return list(res["swap"]) if case == "pt4" else [res["accept"]] if case == "mh1" else []


# The sd of each rate over the K iterations of a run.  Decisions of successive iterations are identically
# distributed but not independent, so the binomial sd sqrt(r (1 - r) / (K n)) is only a lower bound; the sd
# used is measured on the reference over the 16 Philox seeds 1000 .. 1015 (test_invariance_ref_cpu.py
# re-derives these figures), never on a device.
#   pt4 swap rates, n = K W = 262144:  binomial 9.7e-4, measured 1.75e-3, 1.29e-3, 1.46e-3 (pairs 0|1, 1|2, 2|3)
#   mh1 acceptance, n = K C = 524288:  binomial 6.9e-4, measured 9.5e-4
RATE_SD_SEEDS = tuple(range(1000, 1016))
RATE_SD = {"pt4": (1.75e-3, 1.29e-3, 1.46e-3), "mh1": (9.5e-4,)}


def rate_sd(case):
    r = np.array([measured_rates(case, run(case, seed=s)) for s in RATE_SD_SEEDS])
    return r.std(axis=0, ddof=1)


def evaluate(case, X, res, sd=None):
    """Every statistic of a case's final state X against its start: (rows, movement) -- rows [(name, "p" | "z",
    value)] with exact nulls, movement dict(rho, accept).  res: dict(accept, swap) of the run that gave X."""
    c, tgt = CASES[case], target(case)
    V0, V = whitened(case, start(case, X.shape[-1])), whitened(case, X)
    rows = []
    for t, v in enumerate(V):
        tag = f"{case} t{t}" if len(V) > 1 else case
        rows += tgt.stats(v, tag)
    n = V[0].shape[1]
    cat = lambda f: np.concatenate([f(v) for v in V], 1)  # noqa: E731
    if c["kind"] == "ens":
        Wh = n // 2
        rows += pair_stats(tgt, cat(lambda v: v[:, 0:n:2]), cat(lambda v: v[:, 1:n:2]), f"{case} walker w|w+1")
        rows += pair_stats(tgt, cat(lambda v: v[:, :Wh]), cat(lambda v: v[:, Wh:]), f"{case} half 0|1")
        if len(V) > 1:
            rows += pair_stats(tgt, np.concatenate(V[:-1], 1), np.concatenate(V[1:], 1), f"{case} temperature t|t+1")
    else:
        rows += pair_stats(tgt, V[0][:, 0:n:2], V[0][:, 1:n:2], f"{case} chain c|c+1")
    sd = RATE_SD.get(case) if sd is None else sd
    for (name, want), got, s in zip(analytic_rates(case), measured_rates(case, res), sd or ()):
        print(f"{case} {name}: measured {got:.5f} analytic {want:.5f} sd {s:.2e}", flush=True)
        rows.append((f"{case} {name}", "z", (got - want) / s))
    rho = max(start_rho(v0, v) for v0, v in zip(V0, V))
    return rows, dict(rho=rho, accept=float(res["accept"]))
