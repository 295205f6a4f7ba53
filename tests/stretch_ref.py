"""Restatement of the stretch-move kernels (rvm_stretch.h; rvm_samplers.hip stretch_propose_kernel,
stretch_accept_kernel, stretch_iteration_end_kernel; rvm_tempering.hip pt_stretch_propose_kernel,
pt_stretch_accept_kernel) and the synthetic cases tests/test_stretch_ref_cpu.py and
tests/test_gpu_stretch_kernels.py share.

Two levels:

  * Bit restatement (numpy float64, one rounding per operation, no fused multiply-add):
    z = ((a - 1) u1 + 1)^2 / a, j = clamp(floor(u2 n1), 0, n1 - 1), q = c_j - z (c_j - x), written as
    rvm_stretch.h writes them.  The kernels compile with fp contract(off), so z, q and every position
    they store must equal these bit for bit.

  * Exact decision margin (mpmath, 50 digits), from the float64 inputs:
        D = (dim - 1) ln z + beta lnp_new - beta lnp_old - ln u3          (beta = 1: the plain kernels)
    The walker accepts iff D > 0.  A non-finite lnp_new or lnp_old makes D itself +-inf or NaN by the
    IEEE rules, with no rounding in between; those walkers are decided by that value and have no margin.

Rounding bound.  B = 8 u ((dim - 1)|ln z| + beta |lnp_new| + beta |lnp_old| + |ln u3|), u = 2^-53.
The device evaluates lnpdiff = fl(fl(fl(d fl_log(z)) + fl(beta lnp_new)) - fl(beta lnp_old)) > fl_log(u3),
d = dim - 1 exact.  Take each device log to be within 2 ulp (OCML documents 1), and an ulp to be at most
2 u relative.  With A = (dim - 1) ln z, to first order in u:
    fl(d fl_log(z))   is off by at most 4u|A| (the log) + u|A| (the product)          = 5u|A|
    fl(beta lnp_new), fl(beta lnp_old) by u beta|lnp_new|, u beta|lnp_old|   (exact at beta = 1)
    the first sum  by u (|A| + beta|lnp_new|), the second by u (|A| + beta|lnp_new| + beta|lnp_old|)
    fl_log(u3) by 4u|ln u3|
in all 7u|A| + 3u beta|lnp_new| + 2u beta|lnp_old| + 4u|ln u3|: every coefficient is below 8, and the
slack covers the second-order terms.  (Counting the log's 2 ulp as 2u instead gives 5u|A| + ... +
2u|ln u3|, also below.)  The bound comes from this arithmetic, not from running the kernel.

A walker with |D| <= B is undecidable; the cases below are fixed by seed so that none is
(tests/test_stretch_ref_cpu.py asserts it for every case the GPU tests use).  bracket() builds
log-probabilities 64 B on either side of the threshold, so a wrong coefficient or a dropped term flips
decisions at the 1e-13 level, not only in gross cases.
"""
import functools

import mpmath as mp
import numpy as np

import philox_ref

U = 2.0 ** -53
DPS = 50
SEED = 12345
BRACKET = 64.0  # bracket(): bounds B between the proposal's log-probability and the threshold


# ---- bit restatement ----------------------------------------------------------------------------

def stretch_z(u1, a):
    u1 = np.asarray(u1, dtype=np.float64)
    return ((a - 1.0) * u1 + 1.0) * ((a - 1.0) * u1 + 1.0) / a


def stretch_j_unclamped(u2, n1):
    """floor(u2 n1) before the clamp: n1 at u2 = 1.0."""
    return np.floor(np.asarray(u2, dtype=np.float64) * float(n1)).astype(np.int64)


def stretch_j(u2, n1):
    j = stretch_j_unclamped(u2, n1)
    return np.where(j < 0, 0, np.where(j >= n1, n1 - 1, j))


def stretch_q(cj, z, x):
    return cj - z * (cj - x)


def propose(x, c, u1, u2, a):
    """x [P][n0], c [P][n1] (parameter-major, as rvm_stretch_propose takes them) -> (q [P][n0], z, j)."""
    z, j = stretch_z(u1, a), stretch_j(u2, c.shape[1])
    return stretch_q(c[:, j], z[None], x), z, j


def pt_propose(x, c, u1, u2, a, T, Wh):
    """x, c [P][T Wh], column t Wh + k -> (q, z, partner column t Wh + j)."""
    z, j = stretch_z(u1, a), stretch_j(u2, Wh)
    cj = np.repeat(np.arange(T), Wh) * Wh + j
    return stretch_q(c[:, cj], z[None], x), z, cj


# ---- the exact margin ---------------------------------------------------------------------------

def margin(dim, z, lnp_new, lnp_old, u3, beta=1.0):
    """(D, B) per walker as float64 (D rounded from 50 digits: its sign is exact).  Non-finite
    log-probabilities: D by the IEEE rules (+-inf or NaN), B = 0."""
    z, ln, lo, u3, beta = (np.asarray(v, dtype=np.float64) for v in np.broadcast_arrays(z, lnp_new, lnp_old, u3, beta))
    D, B = np.empty(z.shape), np.empty(z.shape)
    with mp.workdps(DPS):
        for i in np.ndindex(z.shape):
            if not (np.isfinite(ln[i]) and np.isfinite(lo[i])):
                with np.errstate(invalid="ignore"):
                    D[i] = float(dim - 1) * np.log(z[i]) + beta[i] * ln[i] - beta[i] * lo[i] - np.log(u3[i])
                B[i] = 0.0
                continue
            A, L3, b = (dim - 1) * mp.log(mp.mpf(z[i])), mp.log(mp.mpf(u3[i])), mp.mpf(beta[i])
            D[i] = float(A + b * mp.mpf(ln[i]) - b * mp.mpf(lo[i]) - L3)
            B[i] = float(8 * mp.mpf(U) * (abs(A) + b * abs(mp.mpf(ln[i])) + b * abs(mp.mpf(lo[i])) + abs(L3)))
    return D, B


def decide(dim, z, lnp_new, lnp_old, u3, beta=1.0):
    """(accepts, |D| / B) per walker; the ratio is inf where the decision has no margin (non-finite)."""
    D, B = margin(dim, z, lnp_new, lnp_old, u3, beta)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(B > 0.0, np.abs(D) / B, np.inf)
    return D > 0.0, ratio


def bracket(dim, z, lnp_old, u3, beta, sign):
    """lnp_new = fl(lnp_old + (ln u3 - (dim - 1) ln z) / beta) + sign * delta, delta = 64 B / beta with B
    taken at the threshold; then moved outward float by float while |D| < 64 B (the roundings of the
    centre and of the sum can leave it a fraction of B short).  sign = +1 accepts, -1 rejects."""
    z, lo, u3, beta, sign = (np.asarray(v, dtype=np.float64) for v in np.broadcast_arrays(z, lnp_old, u3, beta, sign))
    out = np.empty(z.shape)
    with mp.workdps(DPS):
        for i in np.ndindex(z.shape):
            centre = float(mp.mpf(lo[i]) + (mp.log(mp.mpf(u3[i])) - (dim - 1) * mp.log(mp.mpf(z[i]))) / mp.mpf(beta[i]))
            _, B = margin(dim, z[i], centre, lo[i], u3[i], beta[i])
            v = centre + sign[i] * (BRACKET * float(B) / beta[i])
            while True:
                D, B = margin(dim, z[i], v, lo[i], u3[i], beta[i])
                if abs(float(D)) >= BRACKET * float(B) and (float(D) > 0) == (sign[i] > 0):
                    break
                v = np.nextafter(v, sign[i] * np.inf)
            out[i] = v
    return out


def accept_ref(x, lnp, q, lnp_new, z, u3, accepted=None, beta=1.0):
    """The accept kernels' outputs, decided by D: x [P][n], lnp [n] (and accepted [n]) copies with the
    accepted walkers replaced -> dict(x, lnp, accepted, acc, ratio)."""
    acc, ratio = decide(x.shape[0], z, lnp_new, lnp, u3, beta)
    x2, l2 = x.copy(), lnp.copy()
    x2[:, acc], l2[acc] = q[:, acc], lnp_new[acc]
    return dict(x=x2, lnp=l2, accepted=None if accepted is None else accepted + acc.astype(np.int32), acc=acc,
                ratio=ratio)


# ---- rvm_stretch_iteration_end ------------------------------------------------------------------

def iteration_end_ref(dim, n, n_half, s0_begin, s1_begin, x0, x0_aos, dec_local, dec_all, x1, x1_aos, lnp1, c0, c1,
                      lnp_spec, st_spec, a, seed, iteration, accepted1):
    """x0, x1 [dim][n]; x0_aos, x1_aos [n][dim]; c0, c1 [n_half][dim]; lnp_spec, st_spec [3 n].
    Walker k of half 1 draws as item s1_begin + k, half 1; a partner j outside [s0_begin, s0_begin + n)
    as item j, half 0, both against n1 = n_half.  Nothing is modified; returns the outputs and, per
    walker, j, local, v, the partner position used, the decision and its |D| / B."""
    u1, u2, u3 = philox_ref.stretch_uniforms(seed, s1_begin, n, iteration, 1)
    z, j = stretch_z(u1, a), stretch_j(u2, n_half)
    jl = j - s0_begin
    local = (jl >= 0) & (jl < n)
    v = dec_all[j] != 0
    slot = (1 + v.astype(np.int64)) * n + np.arange(n)
    lnew, stnew = lnp_spec[slot], st_spec[slot]
    pu1, pu2 = philox_ref.uniform2_vec(seed, j.astype(np.uint64), iteration, philox_ref.RNG_STRETCH_PROPOSE)
    zp, jp = stretch_z(pu1, a), stretch_j(pu2, n_half)
    rebuilt = stretch_q(c1[jp].T, zp[None], c0[j].T)            # [dim][n]: the partner had it accepted
    partner = np.where(local[None], x0[:, np.clip(jl, 0, n - 1)], np.where(v[None], rebuilt, c0[j].T))
    acc, ratio = decide(dim, z, lnew, lnp1, u3)
    q = stretch_q(partner, z[None], x1)
    x1o, x1a, l1o = x1.copy(), x1_aos.copy(), lnp1.copy()
    x1o[:, acc], l1o[acc] = q[:, acc], lnew[acc]
    x1a[acc] = q[:, acc].T
    x0a = x0_aos.copy()
    ref = dec_local != 0
    x0a[ref] = x0[:, ref].T
    return dict(x1=x1o, x1_aos=x1a, lnp1=l1o, accepted1=accepted1 + acc.astype(np.int32), x0_aos=x0a,
                lnp_new_out=lnew, status_new_out=stnew, j=j, local=local, v=v, partner=partner, rebuilt=rebuilt,
                acc=acc, ratio=ratio, z=z, u3=u3)


def coverage(j, n, s0_begin, dec_all):
    """What an iteration-end case's partners j [n] cover: which of the window's four edge partners are
    drawn, and how many walkers fall in each of local / remote x v = 0 / 1."""
    jl = j - s0_begin
    local = (jl >= 0) & (jl < n)
    v = dec_all[j] != 0
    edges = {e: bool((j == e).any()) for e in (s0_begin - 1, s0_begin, s0_begin + n - 1, s0_begin + n)}
    cells = {(loc, vv): int(((local == loc) & (v == vv)).sum()) for loc in (True, False) for vv in (False, True)}
    return edges, cells


def required_coverage(n, n_half, s0_begin):
    """The part of coverage() a shape can have at all: the edge partners inside [0, n_half), the remote
    cells only when the window is not the whole half, and min(2, n // 4) walkers per cell (four cells
    of two need eight walkers; n = 5 can give one each, n = 1 none)."""
    edges = [e for e in (s0_begin - 1, s0_begin, s0_begin + n - 1, s0_begin + n) if 0 <= e < n_half]
    cells = [(loc, vv) for loc in ((True, False) if n < n_half else (True,)) for vv in (False, True)]
    return edges, cells, min(2, n // 4)


def covered(j, n, n_half, s0_begin, dec_all):
    edges, cells = coverage(j, n, s0_begin, dec_all)
    need_e, need_c, m = required_coverage(n, n_half, s0_begin)
    acc = outcomes(j, dec_all)
    return (all(edges[e] for e in need_e) and all(cells[c] >= m for c in need_c)
            and acc.sum() >= m and (~acc).sum() >= m)


def outcomes(j, dec_all):
    """The decisions iteration_end_case builds: variant 1 (partner rejected) accepts at even k, variant 2 at
    odd k.  find_case also asks for min(2, n // 4) walkers of each outcome."""
    return (np.arange(len(j)) % 2 == 0) != (dec_all[j] != 0)


def partners(seed, n, n_half, s1_begin, iteration):
    items = np.arange(s1_begin, s1_begin + n, dtype=np.uint64)
    _, u2 = philox_ref.uniform2_vec(seed, items, iteration, philox_ref.RNG_STRETCH_PROPOSE | (1 << 8))
    return stretch_j(u2, n_half)


def find_case(seed, n, n_half, s0_begin, dec_all, limit=200000):
    """The first iteration number (from 1) whose half-1 partners satisfy required_coverage()."""
    for it in range(1, limit):
        if covered(partners(seed, n, n_half, n_half + s0_begin, it), n, n_half, s0_begin, dec_all):
            return it
    raise AssertionError("no iteration covers the branches")


# ---- the cases (inputs fixed by seed; the GPU tests and the CPU checks of them read the same) -----

A_DEFAULT = 2.0
PROPOSE_P = (1, 10, 17, 28)
PROPOSE_SHAPES = ((1, 1), (257, 3), (64, 65), (300, 1))
PROPOSE_A = (2.0, 1.5, 1.0 + 2.0 ** -20, 100.0)
PINS_U1 = (2.0 ** -54, 1.0)
PINS_U2 = (2.0 ** -54, 1.0 - 2.0 ** -53, 1.0)  # -> j = 0, n1 - 1, n1 - 1
PT_SHAPES = ((1, 7), (3, 5), (4, 65))
ACCEPT_P = (1, 10, 28)
ACCEPT_N = (1, 255, 256, 257)
PT_ACCEPT_SHAPES = ((3, 1), (3, 85), (3, 86))  # 3, 255 and 258 columns
PT_BETAS = (1.0, 0.25, 1e-3)
BIG = 2 ** 32 + 7
ITER_END_DIMS = (1, 10, 16, 17, 28)
ITER_END_SHAPES = ((1, 1, 0), (129, 129, 0), (64, 192, 64), (5, 12, 5), (300, 900, 0))
# find_case(SEED, n, n_half, s0_begin, iteration_end_dec_all(n, n_half, s0_begin))
ITER_END_ITERATION = {(1, 1, 0): 1, (129, 129, 0): 4, (64, 192, 64): 38, (5, 12, 5): 411, (300, 900, 0): 66}


def _rng(*key):
    return np.random.default_rng([SEED] + [int(k) for k in key])


def pinned_draws(n0, rng):
    """[(u1 [n0], u2 [n0])]: random draws with every pin of PINS_U1 and PINS_U2 at some walker -- in one
    set when n0 has room for the five, else one set per pin."""
    pins = [(0, v) for v in PINS_U1] + [(1, v) for v in PINS_U2]
    sets = []
    if n0 >= len(pins):
        d = [rng.random(n0), rng.random(n0)]
        for (which, v), i in zip(pins, np.linspace(0, n0 - 1, len(pins)).astype(int)):
            d[which][i] = v
        sets.append(tuple(d))
    else:
        for which, v in pins:
            d = [rng.random(n0), rng.random(n0)]
            d[which][n0 - 1] = v
            sets.append(tuple(d))
    return sets


def propose_case(P, n0, n1, a):
    rng = _rng(1, P, n0, n1, int(a * 2 ** 20))
    return dict(x=rng.standard_normal((P, n0)), c=10.0 + rng.standard_normal((P, n1)), draws=pinned_draws(n0, rng))


def pt_propose_case(P, T, Wh):
    """Temperature t's columns of x and c lie in [1000 (t + 1), 1000 (t + 1) + 1): a q built from another
    temperature's partner lands outside (1000 (t + 1) - a, 1000 (t + 1) + 1 + a).  u2 = 1.0 at walker
    t % Wh of every temperature, the other pins wherever they fit."""
    rng = _rng(2, P, T, Wh)
    n = T * Wh
    base = 1000.0 * (np.repeat(np.arange(T), Wh) + 1)
    u1, u2 = rng.random(n), rng.random(n)
    free = [i for i in range(n) if i % Wh != (i // Wh) % Wh]
    for (which, v), i in zip([(0, PINS_U1[0]), (0, PINS_U1[1]), (1, PINS_U2[0]), (1, PINS_U2[1])], free):
        (u1, u2)[which][i] = v
    for t in range(T):
        u2[t * Wh + t % Wh] = 1.0
    return dict(x=base + rng.random((P, n)), c=base + rng.random((P, n)), u1=u1, u2=u2, base=base)


def _lnp_pair(rng, n):
    """Current log-probabilities with magnitudes from 1e-3 to 1e6, either sign."""
    return np.where(rng.random(n) < 0.8, -1.0, 1.0) * 10.0 ** rng.uniform(-3.0, 6.0, n)


@functools.lru_cache(maxsize=None)
def accept_case(P, n0, kind, T=1, betas=None, half=0, begin=None, iteration=0):
    """One accept launch of n = T n0 walkers and its reference.  kind "random": lnp_new = lnp + 3 N(0,1);
    "bracket": 64 B either side of the threshold, + at even walkers.  betas: per temperature (None: the
    plain kernel).  begin: None injects u3; a number takes u3 from the device's stream
    (RNG_STRETCH_ACCEPT | half << 8) of the items begin + i, or with T > 1 of the items t W + half n0 + k.
    The rejected walkers' q columns are NaN.  A one-walker launch accepts in the random case and rejects
    in the bracket case, so the pair holds both outcomes."""
    n = T * n0
    rng = _rng(3, P, n0, kind == "bracket", T, half, 0 if begin is None else begin % 1000003, iteration % 1000003)
    beta = np.repeat(np.asarray(betas if betas is not None else [1.0] * T, dtype=np.float64), n0)
    x, q = rng.standard_normal((P, n)), 5.0 + rng.standard_normal((P, n))
    z = stretch_z(rng.random(n), A_DEFAULT)
    if begin is None:
        u3 = rng.random(n)
    else:
        items = (np.arange(n, dtype=np.uint64) + np.uint64(begin) if T == 1 else
                 (np.repeat(np.arange(T, dtype=np.uint64), n0) * np.uint64(2 * n0) + np.uint64(half * n0)
                  + np.tile(np.arange(n0, dtype=np.uint64), T)))
        u3, _ = philox_ref.uniform2_vec(SEED, items, iteration, philox_ref.RNG_STRETCH_ACCEPT | (half << 8))
    lnp = _lnp_pair(rng, n)
    accepted = rng.integers(0, 6, n).astype(np.int32)
    if kind == "bracket":
        sign = np.where(np.arange(n) % 2 == 0, 1.0, -1.0)
        if n == 1:
            sign = -sign  # the lone walker rejects here and accepts in the random case
        lnp_new = bracket(P, z, lnp, u3, beta, sign)
    else:
        lnp_new = lnp + 3.0 * rng.standard_normal(n) / beta
        if n < 8:  # too few walkers to leave both outcomes to chance: + 50 / beta accepts, - 50 / beta rejects
            lnp_new = lnp + np.where(np.arange(n) % 2 == 0, 50.0, -50.0) / beta
    ref = accept_ref(x, lnp, q, lnp_new, z, u3, accepted, beta)
    q[:, ~ref["acc"]] = np.nan
    return dict(P=P, n=n, x=x, q=q, z=z, u3=u3, lnp=lnp, lnp_new=lnp_new, accepted=accepted, beta=beta, ref=ref)


NONFINITE_ROWS = ("acc", "new_ninf", "rej", "new_nan", "acc", "old_ninf", "rej", "both_ninf", "acc", "u3_one_acc",
                  "u3_one_rej", "rej")


@functools.lru_cache(maxsize=None)
def nonfinite_case(tempered):
    """The table of NONFINITE_ROWS, each non-finite walker between ordinary bracketed neighbours;
    tempered: lnp_old stays finite (include/rvmcmc.h), those two rows become ordinary ones."""
    P = 3
    rows = [("acc" if r == "old_ninf" else "rej" if r == "both_ninf" else r) if tempered else r for r in NONFINITE_ROWS]
    n = len(rows)
    rng = _rng(4, tempered)
    beta = np.full(n, 0.25 if tempered else 1.0)
    x, q = rng.standard_normal((P, n)), 5.0 + rng.standard_normal((P, n))
    z, u3, lnp = stretch_z(rng.random(n), A_DEFAULT), rng.random(n), -10.0 ** rng.uniform(0.0, 3.0, n)
    u3[[i for i, r in enumerate(rows) if r.startswith("u3_one")]] = 1.0
    sign = np.array([1.0 if r in ("acc", "u3_one_acc") else -1.0 for r in rows])
    lnp_new = bracket(P, z, lnp, u3, beta, sign)
    want = sign > 0
    for i, r in enumerate(rows):
        if r in ("new_ninf", "both_ninf"):
            lnp_new[i] = -np.inf
        if r == "new_nan":
            lnp_new[i] = np.nan
        if r in ("old_ninf", "both_ninf"):
            lnp[i] = -np.inf
        if r == "old_ninf":
            want[i] = True  # emcee's semantics: a walker that starts at -inf takes any finite proposal
    accepted = np.zeros(n, dtype=np.int32)
    ref = accept_ref(x, lnp, q, lnp_new, z, u3, accepted, beta)
    return dict(P=P, n=n, rows=rows, x=x, q=q, z=z, u3=u3, lnp=lnp, lnp_new=lnp_new, accepted=accepted, beta=beta,
                want=want, ref=ref)


def iteration_end_dec_all(n, n_half, s0_begin):
    """Random decisions of half 0, with the four edge partners pinned 0, 1, 0, 1 (those that exist), so both
    variants occur on each side of each edge of the window whatever the draw."""
    d = (_rng(5, n, n_half, s0_begin).random(n_half) < 0.5).astype(np.int32)
    for e, val in zip((s0_begin - 1, s0_begin, s0_begin + n - 1, s0_begin + n), (0, 1, 0, 1)):
        if 0 <= e < n_half:
            d[e] = val
    return d


@functools.lru_cache(maxsize=None)
def iteration_end_case(dim, n, n_half, s0_begin):
    """Inputs of one rvm_stretch_iteration_end launch and their reference.  lnp_spec[n + k] and
    lnp_spec[2 n + k] bracket walker k's threshold from opposite sides (slot 1 accepts at even k), so the
    wrong variant flips the decision; lnp_spec[0..n) is NaN; st_spec[s] = 100 + s; dec_pad [n_half] is
    drawn apart from dec_all and dec_local = dec_pad[s0_begin : s0_begin + n]; the mirrors start at the
    sentinel -7777."""
    s1_begin = n_half + s0_begin
    it = ITER_END_ITERATION[(n, n_half, s0_begin)]
    rng = _rng(6, dim, n, n_half, s0_begin)
    dec_all = iteration_end_dec_all(n, n_half, s0_begin)
    dec_pad = (rng.random(n_half) < 0.5).astype(np.int32)
    if n > 1:
        dec_pad[s0_begin], dec_pad[s0_begin + 1] = 1 - dec_all[s0_begin], 0  # differs from dec_all; one unrefreshed
    x0, x1 = rng.standard_normal((dim, n)), 3.0 + rng.standard_normal((dim, n))
    c0, c1 = 20.0 + rng.standard_normal((n_half, dim)), 40.0 + rng.standard_normal((n_half, dim))
    lnp1 = _lnp_pair(rng, n)
    u1, _, u3 = philox_ref.stretch_uniforms(SEED, s1_begin, n, it, 1)
    z = stretch_z(u1, A_DEFAULT)
    even = np.where(np.arange(n) % 2 == 0, 1.0, -1.0)
    lnp_spec = np.concatenate([np.full(n, np.nan), bracket(dim, z, lnp1, u3, 1.0, even),
                               bracket(dim, z, lnp1, u3, 1.0, -even)])
    st_spec = (100 + np.arange(3 * n)).astype(np.int32)
    accepted1 = rng.integers(0, 6, n).astype(np.int32)
    x0_aos, x1_aos = np.full((n, dim), -7777.0), np.full((n, dim), -7777.0)
    inp = dict(dim=dim, n=n, n_half=n_half, s0_begin=s0_begin, s1_begin=s1_begin, x0=x0, x0_aos=x0_aos,
               dec_local=dec_pad[s0_begin:s0_begin + n], dec_all=dec_all, x1=x1, x1_aos=x1_aos, lnp1=lnp1, c0=c0, c1=c1,
               lnp_spec=lnp_spec, st_spec=st_spec, a=A_DEFAULT, seed=SEED, iteration=it, accepted1=accepted1)
    return dict(inp, dec_pad=dec_pad, ref=iteration_end_ref(**inp))


def margin_cases():
    """(tag, ratios |D| / B, bracketed) of every case with a margin that the GPU tests run."""
    for P in ACCEPT_P:
        for n0 in ACCEPT_N:
            for kind in ("random", "bracket"):
                yield f"accept {kind} P={P} n0={n0}", accept_case(P, n0, kind)["ref"]["ratio"], kind == "bracket"
        for T, Wh in PT_ACCEPT_SHAPES:
            for kind in ("random", "bracket"):
                yield (f"pt accept {kind} P={P} T={T} Wh={Wh}",
                       accept_case(P, Wh, kind, T, PT_BETAS)["ref"]["ratio"], kind == "bracket")
    for tempered in (False, True):
        yield f"nonfinite tempered={tempered}", nonfinite_case(tempered)["ref"]["ratio"], True
    for half in (0, 1):
        yield f"philox accept half={half}", accept_case(10, 70, "bracket", 1, None, half, BIG, 5)["ref"]["ratio"], True
        yield (f"philox pt accept half={half}",
               accept_case(10, 23, "bracket", 3, PT_BETAS, half, 0, 5)["ref"]["ratio"], True)
    for dim in ITER_END_DIMS:
        for shape in ITER_END_SHAPES:
            yield f"iteration end dim={dim} shape={shape}", iteration_end_case(dim, *shape)["ref"]["ratio"], True
