"""Plain-numpy restatement of the parallel-tempering ensemble (rvmcmc/tempering.py, rvm_tempering.hip).

Walker-major arrays: positions [T][W][dim], lnp [T][W] (the UNtempered log-probabilities), halves
h = 0: walkers [0, W/2), h = 1: [W/2, W).  Every expression is evaluated as the device evaluates it
(left to right, no fused multiply-add), so fed the same uniforms and the same log-probabilities
the two agree bit for bit in the positions.
"""
import numpy as np

RNG_PT_SWAP = 7


def propose(x, c, u1, u2, a=2.0):
    """x, c: this half and the other half, [T][Wh][dim]; u1, u2 [T][Wh] -> (q [T][Wh][dim], z [T][Wh])."""
    T, Wh, _ = x.shape
    z = ((a - 1.0) * u1 + 1.0) * ((a - 1.0) * u1 + 1.0) / a
    j = np.clip(np.floor(u2 * float(Wh)).astype(int), 0, Wh - 1)
    cj = c[np.arange(T)[:, None], j]  # the partner: same temperature, other half
    return cj - z[..., None] * (cj - x), z


def accept(x, lnp, q, lnp_new, z, u3, betas):
    """One half's tempered accept (in place on x [T][Wh][dim], lnp [T][Wh]) -> (accepted [T][Wh] bool,
    margin |lnpdiff - ln u3|, accepted under the untempered rule)."""
    dim = x.shape[2]
    b = np.asarray(betas, dtype=np.float64)[:, None]
    with np.errstate(invalid="ignore"):
        lnpdiff = float(dim - 1) * np.log(z) + b * lnp_new - b * lnp
        plain = float(dim - 1) * np.log(z) + lnp_new - lnp > np.log(u3)
    acc = lnpdiff > np.log(u3)
    x[acc] = q[acc]
    lnp[acc] = lnp_new[acc]
    return acc, np.abs(lnpdiff - np.log(u3)), plain


def swap(pos, lnp, betas, u):
    """The exchange sweep, pairs T-2 .. 0 (in place on pos [T][W][dim], lnp [T][W]); u [T-1][W]
    -> (swapped [T-1][W] bool, margin |d - ln u| [T-1][W])."""
    T, W = lnp.shape
    swapped = np.zeros((max(T - 1, 0), W), dtype=bool)
    margin = np.full((max(T - 1, 0), W), np.inf)
    for p in range(T - 2, -1, -1):
        d = (betas[p] - betas[p + 1]) * (lnp[p + 1] - lnp[p])
        s = d > np.log(u[p])
        margin[p] = np.abs(d - np.log(u[p]))
        pos[p, s], pos[p + 1, s] = pos[p + 1, s].copy(), pos[p, s].copy()
        lnp[p, s], lnp[p + 1, s] = lnp[p + 1, s].copy(), lnp[p, s].copy()
        swapped[p] = s
    return swapped, margin


def items(T, W, half):
    """Philox items of half `half`'s walkers, [T][Wh]: g = t W + h Wh + k."""
    Wh = W // 2
    return (np.arange(T, dtype=np.uint64)[:, None] * np.uint64(W) + np.uint64(half * Wh)
            + np.arange(Wh, dtype=np.uint64)[None])


def swap_items(T, W):
    """Philox items of the exchange draws, [T-1][W]: p W + w."""
    return np.arange(max(T - 1, 0), dtype=np.uint64)[:, None] * np.uint64(W) + np.arange(W, dtype=np.uint64)[None]


def case_inputs(x0, scales, T, W, iters, seed=0, ball=1e-2):
    """The start and the injected uniforms of a full-step comparison, drawn in a fixed order from
    np.random.default_rng(seed): the start x0 + ball * scales * N(0,1) as [T][W][dim]; then per
    iteration u1, u2, u3 as (T, Wh) for half 0, the same for half 1, then u as (T-1, W)."""
    rng = np.random.default_rng(seed)
    Wh = W // 2
    X = np.asarray(x0)[None, None] + ball * np.asarray(scales) * rng.standard_normal((T, W, len(x0)))
    draws = []
    for _ in range(iters):
        d = dict(u1=[], u2=[], u3=[])
        for _h in (0, 1):
            for k in ("u1", "u2", "u3"):
                d[k].append(rng.random((T, Wh)))
        d = {k: np.stack(v) for k, v in d.items()}
        d["swap"] = rng.random((T - 1, W))
        draws.append(d)
    return X, draws


class Ladder:
    """The restated sampler on the host: positions [T][W][dim], lnp [T][W]; lnprob_fn maps [N][dim]
    positions to (logl [N], status [N])."""

    def __init__(self, X, betas, lnprob_fn, a=2.0):
        self.pos = np.array(X, dtype=np.float64)
        self.T, self.W, self.dim = self.pos.shape
        self.Wh = self.W // 2
        self.betas = np.asarray(betas, dtype=np.float64)
        self.fn = lnprob_fn
        self.a = a
        self.lnp, self.status0 = self._eval(self.pos)
        self.accept_margin, self.swap_margin = np.inf, np.inf
        self.n_tempered_differs = 0   # accept decisions that differ from the untempered rule
        self.statuses = []            # the proposals' statuses, per half-step
        self.swaps = []               # the swapped masks, per sweep

    def _eval(self, P):
        l, st = self.fn(P.reshape(-1, self.dim))
        return l.reshape(P.shape[:-1]), st.reshape(P.shape[:-1])

    def half(self, h):
        return slice(h * self.Wh, (h + 1) * self.Wh)

    def half_step(self, h, u1, u2, u3, lnp_new=None):
        """lnp_new [T][Wh]: the proposals' log-probabilities when the caller has them (the device's),
        else lnprob_fn evaluates them."""
        x, c = self.pos[:, self.half(h)].copy(), self.pos[:, self.half(1 - h)]
        lnp = self.lnp[:, self.half(h)].copy()
        q, z = propose(x, c, u1, u2, self.a)
        if lnp_new is None:
            lnp_new, st = self._eval(q)
            self.statuses.append(st)
        acc, margin, plain = accept(x, lnp, q, lnp_new, z, u3, self.betas)
        self.accept_margin = min(self.accept_margin, float(margin.min()))
        self.n_tempered_differs += int((acc != plain).sum())
        self.pos[:, self.half(h)], self.lnp[:, self.half(h)] = x, lnp
        return q, acc

    def swap(self, u):
        s, margin = swap(self.pos, self.lnp, self.betas, u)
        if margin.size:
            self.swap_margin = min(self.swap_margin, float(margin.min()))
        self.swaps.append(s)
        return s
