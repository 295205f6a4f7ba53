"""High-precision restatement of the SMALA chain math (mcmc.py:135-187) in plain Python + mpmath.

The device kernels (rvm_smala.hip) do their own linear algebra -- a Jacobi eigen-solver, SoftAbs, a
Cholesky factorisation -- so their reference must not share float64 LAPACK's error: everything here
runs at 40 digits and is rounded to float64 only where a result leaves a function.

  metric_ref      SoftAbs metric G, G^-1, chol(G^-1), drift mu, log det G^-1, cond   (mcmc.py:135-150)
  gauss_newton    H = -(2/N) J^T W J from the +/- columns of a central-difference stencil
  gauss_newton_f64  the same sum with float64's roundings, and the bound between the two
  mvn_logq, accept_log_ratio                                                          (mcmc.py:158-187)
  metric_cases    deterministic named symmetric matrices -H for the kernel tests
  case_ref        metric_ref of one such case at its standard (x, lp, grad), cached
  accept_cases    synthetic current / proposal caches for the accept kernels, with the reference decision
  metric_numpy    the float64 (LAPACK) restatement the sampler tests use
"""
import functools
import zlib

import mpmath as mp
import numpy as np

DPS = 40
U = 2.0 ** -53                    # unit roundoff of float64
SOFTABS_SMALL = 1e-8              # |alpha lambda| below this: lambda~ = 1/alpha (mcmc.py:137)
COND_BULK, COND_GRADED = 1e4, 1e7  # cond limits of the two tolerance classes
EPS = 0.5


def _mpm(a):
    """float64 array -> mp.matrix, exactly (1-d arrays become columns)."""
    return mp.matrix(np.asarray(a, dtype=np.float64).tolist())


def _np(m, shape=None):
    a = np.array([float(v) for v in m], dtype=np.float64)
    return a.reshape(shape) if shape is not None else a


def metric_ref(x, lp, grad, H, alpha, eps):
    """mcmc.py:135-150 for one chain.  H: float64 [P][P] or an mp.matrix (gauss_newton's).
    Returns float64 G, Ginv, L (lower Cholesky factor of Ginv), mu, drift = mu - x, logdet
    (log det G^-1), cond = max lambda~ / min lambda~, lam, lam_twig, pivot (the smallest Cholesky
    pivot L_jj^2 relative to Ginv_jj), lp and grad as given, and under "mp" the unrounded values."""
    with mp.workdps(DPS):
        x = np.asarray(x, dtype=np.float64)
        P = len(x)
        Hm = H if isinstance(H, mp.matrix) else _mpm(H)
        A = -(Hm + Hm.T) / 2
        if P == 1:
            lam, Q = [A[0, 0]], mp.matrix([[1]])
        else:
            lam, Q = mp.eigsy(A)
            lam = list(lam)
        al = mp.mpf(alpha)
        lt = [1 / al if abs(al * l) < mp.mpf(SOFTABS_SMALL) else l * mp.coth(al * l) for l in lam]
        G = Q * mp.diag(lt) * Q.T
        Ginv = Q * mp.diag([1 / l for l in lt]) * Q.T
        G, Ginv = (G + G.T) / 2, (Ginv + Ginv.T) / 2
        scale = max(Ginv[j, j] for j in range(P))  # (mp.cholesky's positivity threshold is absolute)
        L = mp.cholesky(Ginv / scale) * mp.sqrt(scale)
        drift = (mp.mpf(eps) ** 2 / 2) * (Ginv * _mpm(grad))
        mu = _mpm(x) + drift
        logdet = -mp.fsum(mp.log(l) for l in lt)
        cond = max(lt) / min(lt)
        pivot = min(L[j, j] ** 2 / Ginv[j, j] for j in range(P))
        return dict(G=_np(G, (P, P)), Ginv=_np(Ginv, (P, P)), L=_np(L, (P, P)), mu=_np(mu), drift=_np(drift),
                    logdet=float(logdet), cond=float(cond), lam=_np(lam), lam_twig=_np(lt), pivot=float(pivot),
                    lp=lp, grad=np.asarray(grad, dtype=np.float64), x=x,
                    mp=dict(G=G, Ginv=Ginv, L=L, mu=mu, logdet=logdet, lam_twig=lt, Q=Q))


def fd_den(x, floor_, rel):
    """The realised central-difference step (x + e) - (x - e), e = rel max(|x|, floor), formed in
    float64 exactly as rvm_fd_params and rvm_smala_derive form it: an input of the arithmetic under test."""
    x = np.asarray(x, dtype=np.float64)
    e = rel * np.maximum(np.abs(x), floor_)
    return (x + e) - (x - e)


def gauss_newton(rv_stencil, inv_sigma2, den, npoints):
    """H = -(2/N) J^T W J as an mp.matrix for one chain: rv_stencil [n_obs][2P+1] (columns 1+2p / 2+2p
    the +/- points of parameter p), J[e][p] = (rv+ - rv-) / den_p, W = diag(inv_sigma2)."""
    with mp.workdps(DPS):
        rv = np.asarray(rv_stencil, dtype=np.float64)
        P = len(den)
        E = rv.shape[0]
        d = [mp.mpf(float(v)) for v in den]
        J = [[(mp.mpf(float(rv[e, 1 + 2 * p])) - mp.mpf(float(rv[e, 2 + 2 * p]))) / d[p] for p in range(P)]
             for e in range(E)]
        w = [mp.mpf(float(v)) for v in inv_sigma2]
        fac = mp.mpf(2) / mp.mpf(npoints)
        H = mp.zeros(P, P)
        for p in range(P):
            for q in range(p, P):
                H[p, q] = H[q, p] = -fac * mp.fsum(J[e][p] * w[e] * J[e][q] for e in range(E))
        return H


def gauss_newton_f64(rv_stencil, inv_sigma2, den, npoints):
    """The same H in float64 with the rounding steps of a plain epoch-ordered sum: J = (rv+ - rv-) / den,
    then sum_e (J_p w_e) J_q added one epoch after the other, times 2/N.  An entry of it differs from
    gauss_newton's by at most gauss_newton_rounding(n_obs) sqrt(H_pp H_qq): see there."""
    rv = np.asarray(rv_stencil, dtype=np.float64)
    P = len(den)
    J = (rv[:, 1:2 * P:2] - rv[:, 2:2 * P + 1:2]) / den
    acc = np.zeros((P, P))
    for e in range(rv.shape[0]):
        acc = acc + (J[e][:, None] * inv_sigma2[e]) * J[e][None, :]
    acc = np.triu(acc) + np.triu(acc, 1).T  # (J_p w) J_q for p <= q, mirrored
    return -((2.0 / npoints) * acc)


def gauss_newton_rounding(n_obs):
    """Relative rounding bound of one entry of the float64 Gauss-Newton sum against sum_e |J_p w J_q|
    <= sqrt(H_pp H_qq): two roundings in each J (difference, quotient), two in the product, one per
    addition, two for the factor 2/N -- (n_obs + 7) u to first order, with 1.01 for the higher orders."""
    return 1.01 * (n_obs + 7) * U


def mvn_logq(y, mu, G, logdet, eps):
    """log N(y; mu, eps^2 G^-1) from G and log det G^-1 (mcmc.py:158-162), as an mpf."""
    with mp.workdps(DPS):
        P = len(y)
        d = _mpm(y) - _mpm(mu)
        maha = (d.T * _mpm(G) * d)[0, 0]
        e2 = mp.mpf(eps) ** 2
        return -(maha / e2 + P * mp.log(e2) + mp.mpf(float(logdet)) + P * mp.log(2 * mp.pi)) / 2


def accept_log_ratio(x, xs, cur, prop, eps):
    """logp* - logp + log q(x | x*) - log q(x* | x) (mcmc.py:173-184) from two caches (dicts with
    float64 lp, mu, G, logdet), as an mpf."""
    with mp.workdps(DPS):
        q_ts_t = mvn_logq(xs, cur["mu"], cur["G"], cur["logdet"], eps)
        q_t_ts = mvn_logq(x, prop["mu"], prop["G"], prop["logdet"], eps)
        return mp.mpf(float(prop["lp"])) - mp.mpf(float(cur["lp"])) + q_t_ts - q_ts_t


def metric_numpy(lp, g, H, x, alpha, eps):
    """mcmc.py:135-150 restated in numpy (float64 LAPACK) for one chain: SoftAbs metric, G^-1, chol, drift."""
    lam, Q = np.linalg.eigh(-0.5 * (H + H.T))
    with np.errstate(divide="ignore", invalid="ignore"):
        lt = np.where(np.abs(alpha * lam) < 1e-8, 1.0 / alpha, lam / np.tanh(alpha * lam))
    G = Q @ np.diag(lt) @ Q.T
    Ginv = Q @ np.diag(1.0 / lt) @ Q.T
    L = np.linalg.cholesky(Ginv)
    mu = x + eps ** 2 * Ginv @ g / 2.0
    return dict(G=G, Ginv=Ginv, L=L, mu=mu, logdet=float(np.sum(np.log(1.0 / lt))))


# ---- case generator --------------------------------------------------------------------------

GENERIC = ("spd", "indefinite", "three_eye", "diagonal", "zeros", "eye_plus_rank1", "rank1", "blocks")
FAMILIES = GENERIC + ("graded_wide", "graded_hessian")
WELL_CONDITIONED = ("spd", "indefinite", "three_eye", "diagonal", "eye_plus_rank1", "blocks")


def _rng(*key):
    return np.random.default_rng(zlib.crc32(repr(key).encode()))


def _orthogonal(rng, P):
    Q, R = np.linalg.qr(rng.standard_normal((P, P)))
    return Q * np.sign(np.diag(R))


def _sym(A):
    return 0.5 * (A + A.T)


def _graded(P, lam, alpha):
    """Q diag(lam) Q^T with the first random rotation under which no Cholesky pivot of G^-1 comes
    near zero (at cond 1e7 a 2 x 2 rotated by 45 degrees has a relative pivot of 4e-7); a float64
    estimate picks the rotation, test_smala_ref_cpu.py asserts the condition on the reference."""
    for t in range(64):
        Q = _orthogonal(_rng("graded", P, t), P)
        A = _sym(Q @ np.diag(lam) @ Q.T)
        m = metric_numpy(0.0, np.zeros(P), -A, np.zeros(P), alpha, EPS)
        if (np.diag(m["L"]) ** 2 / np.diag(m["Ginv"])).min() > 4e-6:
            return A
    raise AssertionError("no rotation found")


def metric_cases(P):
    """Named symmetric float64 matrices A = -H with the alphas each is run at:
    [(name, A, alphas, cond_limit)].  Deterministic in P."""
    rng = _rng("metric_cases", P)
    Q = _orthogonal(rng, P)
    k = np.arange(P)
    u = rng.standard_normal(P)
    u *= 2.0 / np.linalg.norm(u)              # |u|^2 = 4: rank1's cond at alpha = 1e3 is 4e3
    sign = np.where(k % 2 == 0, 1.0, -1.0)    # indefinite as soon as P >= 2
    both = (1.0, 1e3)
    blocks = np.zeros((P, P))
    for i in range(0, P, 2):
        a, b = 2.0 + i, 0.5 + 0.25 * i        # equal diagonal pair: the rotation angle's theta is exactly 0
        blocks[i, i] = a
        if i + 1 < P:
            blocks[i + 1, i + 1] = a
            blocks[i, i + 1] = blocks[i + 1, i] = b
    out = [
        ("spd", _sym(Q @ np.diag(rng.uniform(0.5, 50.0, P)) @ Q.T), both, COND_BULK),
        ("indefinite", _sym(Q @ np.diag(sign * rng.uniform(0.5, 50.0, P)) @ Q.T), both, COND_BULK),
        ("three_eye", 3.0 * np.eye(P), both, COND_BULK),
        ("diagonal", np.diag(sign * (0.5 + 1.3 * k)), both, COND_BULK),
        ("zeros", np.zeros((P, P)), both, COND_BULK),
        ("eye_plus_rank1", 2.0 * np.eye(P) + np.outer(u, u), both, COND_BULK),   # a (P-1)-fold eigenvalue
        ("rank1", np.outer(u, u), both, COND_BULK),                              # null space: the 1/alpha branch
        ("blocks", blocks, both, COND_BULK),
        ("graded_wide", _graded(P, np.logspace(-6, 6, P), 1.0), (1.0,), COND_GRADED),
        # (the top eigenvalue a hair under 1e9: cond stays within COND_GRADED after the products' rounding)
        ("graded_hessian", _graded(P, np.minimum(np.logspace(2, 9, P), 1e9 * (1 - 1e-6)), 1e3), (1e3,), COND_GRADED),
    ]
    assert tuple(n for n, *_ in out) == FAMILIES
    return out


def case_inputs(P, name):
    """The standard point of a case: x away from 0, a non-zero gradient, a finite logp."""
    rng = _rng("case_inputs", P, name)
    x = rng.uniform(0.5, 2.0, P) * np.where(rng.random(P) < 0.5, -1.0, 1.0)
    grad = rng.standard_normal(P) * 3.0
    lp = float(-50.0 + 10.0 * rng.standard_normal())
    return x, lp, grad


@functools.lru_cache(maxsize=None)
def case_ref(P, name, alpha, eps=EPS):
    """metric_ref of metric_cases(P)[name] at case_inputs(P, name); "A" holds the matrix."""
    A = {n: a for n, a, *_ in metric_cases(P)}[name]
    x, lp, grad = case_inputs(P, name)
    r = metric_ref(x, lp, grad, -A, alpha, eps)
    r["A"] = A
    return r


def tolerances(P, cond):
    """(relative to max |G_ref|) for G, and (relative) for Ginv, L L^T, L, logdet, mu - x: an
    orthogonal-similarity eigen-solver perturbs eigenvalues by O(P u ||A||)."""
    return 4 * P * U, 4 * P * U * max(cond, 1.0)


# ---- synthetic caches for the propose / accept kernels -----------------------------------------

ACCEPT_CHAINS = 7


def accept_cases(P, eps=EPS):
    """Current and proposal caches of ACCEPT_CHAINS chains, valid and different per chain, from the
    generic cases at alpha = 1 (chain c: cur from case c, prop from case c + 3), with injected
    normals z and uniforms u and the reference log-ratio of every chain.  The proposal's logp is set
    so that the log-ratios spread around ln u: both outcomes occur.  Arrays are [C][...] float64."""
    C = ACCEPT_CHAINS
    rng = _rng("accept_cases", P)
    refs = [case_ref(P, n, 1.0, eps) for n in GENERIC]
    z = rng.standard_normal((C, P))
    u = rng.uniform(0.05, 0.95, C)
    shift = rng.uniform(0.05, 1.5, C) * np.where(np.arange(C) % 2 == 0, 1.0, -1.0)  # accept, reject, accept, ...
    x = np.empty((C, P))
    xs = np.empty((C, P))
    cur, prop = [], []
    logr = np.empty(C)
    for c in range(C):
        rc, rp = refs[c], refs[(c + 3) % len(refs)]
        x[c] = rc["x"]
        xs[c] = rc["mu"] + eps * rc["L"] @ z[c]
        cc = dict(lp=rc["lp"], grad=rc["grad"], mu=rc["mu"], L=rc["L"], G=rc["G"], logdet=rc["logdet"], ok=1)
        pc = dict(lp=0.0, grad=rp["grad"], mu=xs[c] + rp["drift"], L=rp["L"], G=rp["G"], logdet=rp["logdet"], ok=1)
        # logp* such that log-ratio - ln u = shift (up to float64 rounding of logp*)
        base = float(accept_log_ratio(x[c], xs[c], cc, pc, eps))
        pc["lp"] = float(np.log(u[c]) + shift[c] - base)
        logr[c] = float(accept_log_ratio(x[c], xs[c], cc, pc, eps))
        cur.append(cc)
        prop.append(pc)
    return dict(x=x, xs=xs, z=z, u=u, cur=cur, prop=prop, log_ratio=logr, accept=logr > np.log(u))
