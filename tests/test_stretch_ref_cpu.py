"""tests/stretch_ref.py checked on its own, and the conditions tests/test_gpu_stretch_kernels.py relies
on: the bit restatement against 50 digits and emcee's formula, no walker of any GPU case within the
rounding bound B of its threshold, brackets on their intended side, the committed find_case constants
against their coverage tables, and iteration_end_ref against two plain half-steps."""
import mpmath as mp
import numpy as np
import pytest

import philox_ref
import pt_ref
import stretch_ref as R

U = R.U


def test_bit_restatement_against_50_digits():
    """z within 6 u z of the exact value from the float64 u1 (two roundings in t = (a - 1) u1 + 1, counted
    twice in t t, one for the product, one for the quotient).  q against the exact value from the float64
    c, z, x: the difference c - x rounds once (u |c - x|), the product once more (2 u |z||c - x| so far), the
    last subtraction once (u |q|), so the error is at most u |q| + 2 u |z||c - x| to first order.  That is
    within 2 u (|c| + |z||c - x|) whenever |q| <= 2 |c|, and the test holds those walkers to that figure; where
    the stretch carries q further out than 2 |c| (a = 100 does) correctly rounded arithmetic can exceed it
    (found: c = 0.0187, x = 1.49, z = 90.9 gives q = 134.2 off by 3.38e-14 against 2.98e-14), and the derived
    bound stands alone."""
    rng = np.random.default_rng(0)
    n_near = 0
    for a in R.PROPOSE_A:
        u1 = np.concatenate([rng.random(200), R.PINS_U1])
        z = R.stretch_z(u1, a)
        c, x = rng.standard_normal(len(u1)) * 10.0 ** rng.uniform(-3, 3, len(u1)), rng.standard_normal(len(u1))
        q = R.stretch_q(c, z, x)
        with mp.workdps(R.DPS):
            for i in range(len(u1)):
                t = (mp.mpf(a) - 1) * mp.mpf(u1[i]) + 1
                assert abs(mp.mpf(z[i]) - t * t / mp.mpf(a)) <= 6 * U * z[i], (a, u1[i])
                ci, zi, xi = mp.mpf(c[i]), mp.mpf(z[i]), mp.mpf(x[i])
                err, far = abs(mp.mpf(q[i]) - (ci - zi * (ci - xi))), abs(zi) * abs(ci - xi)
                assert err <= (U * abs(mp.mpf(q[i])) + 2 * U * far) * (1 + mp.mpf(2) ** -40), (a, i)
                if abs(q[i]) <= 2 * abs(c[i]):
                    n_near += 1
                    assert err <= 2 * U * (abs(ci) + far), (a, i)
    assert n_near >= 100


def test_z_is_emcee_formula_bit_for_bit():
    u1 = np.random.default_rng(1).random(4096)
    for a in R.PROPOSE_A:
        np.testing.assert_array_equal(R.stretch_z(u1, a), ((a - 1.0) * u1 + 1.0) ** 2 / a)


def test_pinned_draws_reach_the_ends():
    """u2 = 2^-54, 1 - 2^-53, 1.0 give j = 0, n1 - 1, n1 - 1 -- the last only through the clamp: floor(1.0 n1)
    is n1, one past the complement.  The device's uniform does reach 1.0: its top value
    ((2^53 - 1) + 0.5) 2^-53 rounds there.  u1 = 2^-54, 1.0 give z at 1/a and a."""
    assert (float(2 ** 53 - 1) + 0.5) / 2.0 ** 53 == 1.0
    for n1 in (1, 3, 65, 900):
        np.testing.assert_array_equal(R.stretch_j(np.array(R.PINS_U2), n1), [0, n1 - 1, n1 - 1])
        assert R.stretch_j_unclamped(np.array([1.0]), n1)[0] == n1
    for a in R.PROPOSE_A:
        z = R.stretch_z(np.array(R.PINS_U1), a)
        assert abs(z[0] * a - 1.0) <= 4 * U + (a - 1.0) * 2.0 ** -52 and z[1] == a, (a, z)
    for n0 in (1, 3, 257):
        sets = R.pinned_draws(n0, np.random.default_rng(2))
        assert len(sets) == (1 if n0 >= 5 else 5)
        for which, v in [(0, p) for p in R.PINS_U1] + [(1, p) for p in R.PINS_U2]:
            assert any((s[which] == v).any() for s in sets), (n0, which, v)


def test_pt_propose_is_pt_ref_propose():
    for T, Wh in R.PT_SHAPES:
        c = R.pt_propose_case(10, T, Wh)
        q, z, cj = R.pt_propose(c["x"], c["c"], c["u1"], c["u2"], 2.0, T, Wh)
        as3 = lambda m: np.ascontiguousarray(m.T).reshape(T, Wh, -1)  # noqa: E731
        q3, z3 = pt_ref.propose(as3(c["x"]), as3(c["c"]), c["u1"].reshape(T, Wh), c["u2"].reshape(T, Wh), 2.0)
        np.testing.assert_array_equal(as3(q), q3)
        np.testing.assert_array_equal(z.reshape(T, Wh), z3)
        assert (cj // Wh == np.repeat(np.arange(T), Wh)).all()
        for t in range(T):
            assert (c["u2"][t * Wh:(t + 1) * Wh] == 1.0).any()
        lo = c["base"] - 2.0
        assert ((q > lo) & (q < c["base"] + 3.0)).all()  # each q next to its own temperature's range


def test_margin_against_the_float_expression():
    """D's sign agrees with the plain float64 expression wherever that expression is clear of B, and B
    is the stated multiple of the terms' magnitudes."""
    rng = np.random.default_rng(3)
    n, dim = 500, 10
    z, u3 = R.stretch_z(rng.random(n), 2.0), rng.random(n)
    lo = -10.0 ** rng.uniform(-3, 6, n)
    ln = lo + rng.standard_normal(n)
    beta = rng.choice(R.PT_BETAS, n)
    D, B = R.margin(dim, z, ln, lo, u3, beta)
    f = 9.0 * np.log(z) + beta * ln - beta * lo - np.log(u3)
    np.testing.assert_allclose(B, 8 * U * (9.0 * np.abs(np.log(z)) + beta * np.abs(ln) + beta * np.abs(lo)
                                           + np.abs(np.log(u3))), rtol=1e-12)
    assert (np.abs(D - f) <= B).all()
    # dim = 1: the ln z term vanishes whatever z is
    D1, _ = R.margin(1, z, ln, lo, u3)
    D1b, _ = R.margin(1, np.full(n, 1.0), ln, lo, u3)
    np.testing.assert_array_equal(D1, D1b)


def test_nonfinite_table():
    for tempered in (False, True):
        c = R.nonfinite_case(tempered)
        np.testing.assert_array_equal(c["ref"]["acc"], c["want"])
        finite = np.isfinite(c["lnp"]) & np.isfinite(c["lnp_new"])
        assert np.isinf(c["ref"]["ratio"][~finite]).all() and (c["ref"]["ratio"][finite] >= R.BRACKET).all()
        if tempered:
            assert np.isfinite(c["lnp"]).all()
        for i, r in enumerate(c["rows"]):
            assert c["want"][i] == (r in ("acc", "old_ninf", "u3_one_acc")), (i, r)
            if r.startswith("u3_one"):
                assert c["u3"][i] == 1.0
    plain = R.nonfinite_case(False)
    assert [r for r in plain["rows"] if r.endswith("ninf") or r.endswith("nan")] == ["new_ninf", "new_nan", "old_ninf",
                                                                                     "both_ninf"]


def test_no_gpu_case_has_a_walker_within_the_bound():
    """Zero undecidable walkers (|D| <= B) in every case the GPU tests run, 64 B for the bracketed ones;
    prints each group's smallest |D| / B."""
    groups = {}
    for tag, ratio, bracketed in R.margin_cases():
        finite = ratio[np.isfinite(ratio)]
        if finite.size == 0:
            continue
        assert (finite > 1.0).all(), (tag, finite.min())
        if bracketed:
            assert (finite >= R.BRACKET).all(), (tag, finite.min())
        key = tag.split(" P=")[0].split(" dim=")[0].split(" tempered=")[0].split(" half=")[0]
        groups[key] = min(groups.get(key, np.inf), float(finite.min()))
    for key, v in groups.items():
        print(f"\nRATIO min |D|/B {key}: {v:.4g}", flush=True)
    assert len(groups) == 8


def test_brackets_land_on_their_side_and_both_outcomes_occur():
    for P in R.ACCEPT_P:
        for n0 in R.ACCEPT_N:
            for T, betas in ((1, None), (3, R.PT_BETAS)):
                if T == 3 and (T, n0) not in R.PT_ACCEPT_SHAPES:
                    continue
                b, r = R.accept_case(P, n0, "bracket", T, betas), R.accept_case(P, n0, "random", T, betas)
                n = b["n"]
                want = (np.arange(n) % 2 == 0) if n > 1 else np.array([False])
                np.testing.assert_array_equal(b["ref"]["acc"], want)
                both = np.concatenate([b["ref"]["acc"], r["ref"]["acc"]]) if n == 1 else None
                for acc in ([both] if n == 1 else [b["ref"]["acc"], r["ref"]["acc"]]):
                    assert acc.any() and not acc.all(), (P, n0, T)
                for c in (b, r):  # the poison sits exactly on the rejected walkers' proposals
                    np.testing.assert_array_equal(np.isnan(c["q"]).all(axis=0), ~c["ref"]["acc"])
                    assert np.abs(np.log10(np.abs(c["lnp"]))).max() <= 6.0
    for T, Wh in R.PT_ACCEPT_SHAPES:
        assert set(R.accept_case(10, Wh, "bracket", T, R.PT_BETAS)["beta"]) == set(R.PT_BETAS)


@pytest.mark.parametrize("shape", R.ITER_END_SHAPES)
def test_find_case_constants_cover_every_branch(shape):
    n, n_half, s0 = shape
    dec_all = R.iteration_end_dec_all(*shape)
    it = R.ITER_END_ITERATION[shape]
    j = R.partners(R.SEED, n, n_half, n_half + s0, it)
    edges, cells = R.coverage(j, n, s0, dec_all)
    need_e, need_c, m = R.required_coverage(*shape)
    print(f"\ncoverage {shape} iteration {it}: edges {edges} cells {cells}", flush=True)
    for e in need_e:
        assert edges[e], (shape, e)
    for c in need_c:
        assert cells[c] >= m, (shape, c, cells)
    acc = R.outcomes(j, dec_all)
    assert acc.sum() >= m and (~acc).sum() >= m, (shape, acc)
    assert R.find_case(R.SEED, n, n_half, s0, dec_all) == it
    if shape in ((64, 192, 64), (300, 900, 0)):
        assert len(need_c) == 4 and m == 2 and len(need_e) == (4 if s0 else 3)
    # the case's reference saw the same partners, and its variants decide as built: slot 1 accepts at even k
    c = R.iteration_end_case(10, *shape)
    np.testing.assert_array_equal(c["ref"]["j"], j)
    np.testing.assert_array_equal(c["ref"]["acc"], (np.arange(n) % 2 == 0) != c["ref"]["v"])
    assert not np.array_equal(c["dec_local"], c["dec_all"][s0:s0 + n]) or n == 1


def _one_rank_iteration(dim, n, seed, it):
    """A whole iteration of one rank as two plain half-steps of the restatement (Philox draws, synthetic
    log-probabilities): the state before, after half 0, after half 1, and what half 1 was given."""
    rng = np.random.default_rng(dim * 1000 + n)
    X0, X1 = rng.standard_normal((dim, n)), 3.0 + rng.standard_normal((dim, n))
    lnp0, lnp1 = -10.0 ** rng.uniform(0, 3, n), -10.0 ** rng.uniform(0, 3, n)
    u1, u2, u3 = philox_ref.stretch_uniforms(seed, 0, n, it, 0)
    q0, z0, _ = R.propose(X0, X1, u1, u2, 2.0)
    h0 = R.accept_ref(X0, lnp0, q0, R.bracket(dim, z0, lnp0, u3, 1.0, rng.choice([-1.0, 1.0], n)), z0, u3)
    u1, u2, u3 = philox_ref.stretch_uniforms(seed, n, n, it, 1)
    z1 = R.stretch_z(u1, 2.0)
    even = np.where(np.arange(n) % 2 == 0, 1.0, -1.0)
    lnp_spec = np.concatenate([np.full(n, np.nan), R.bracket(dim, z1, lnp1, u3, 1.0, even),
                               R.bracket(dim, z1, lnp1, u3, 1.0, -even)])
    q1, z1b, j1 = R.propose(X1, h0["x"], u1, u2, 2.0)
    np.testing.assert_array_equal(z1, z1b)
    lnew = lnp_spec[(1 + h0["acc"][j1].astype(int)) * n + np.arange(n)]
    h1 = R.accept_ref(X1, lnp1, q1, lnew, z1, u3, np.zeros(n, np.int32))
    return dict(X0=X0, X1=X1, lnp1=lnp1, h0=h0, h1=h1, lnp_spec=lnp_spec, lnew=lnew, j1=j1)


@pytest.mark.parametrize("dim", [1, 10, 17])
def test_iteration_end_ref_is_two_plain_half_steps(dim):
    """One rank, every partner local: iteration_end_ref's x1, lnp1 and accepted1 are the second plain
    half-step's.  Then the same iteration seen through a window of the half (partners outside it rebuilt
    from the starting positions and their own draws) gives the window's walkers the same bits."""
    n, seed, it = 48, 99, 7
    s = _one_rank_iteration(dim, n, seed, it)
    dec = s["h0"]["acc"].astype(np.int32)
    st_spec = (100 + np.arange(3 * n)).astype(np.int32)
    c0, c1 = np.ascontiguousarray(s["X0"].T), np.ascontiguousarray(s["X1"].T)
    r = R.iteration_end_ref(dim, n, n, 0, n, s["h0"]["x"], c0.copy(), dec, dec, s["X1"], c1.copy(), s["lnp1"], c0, c1,
                            s["lnp_spec"], st_spec, 2.0, seed, it, np.zeros(n, np.int32))
    assert r["local"].all() and r["acc"].any() and not r["acc"].all()
    np.testing.assert_array_equal(r["x1"], s["h1"]["x"])
    np.testing.assert_array_equal(r["lnp1"], s["h1"]["lnp"])
    np.testing.assert_array_equal(r["accepted1"], s["h1"]["accepted"])
    np.testing.assert_array_equal(r["lnp_new_out"], s["lnew"])
    np.testing.assert_array_equal(r["x0_aos"], s["h0"]["x"].T)   # refreshed rows = accepted; the others were current
    np.testing.assert_array_equal(r["x1_aos"], s["h1"]["x"].T)
    lo, m = 16, 20  # the window [16, 36) of both halves
    w = slice(lo, lo + m)
    spec_w = np.concatenate([s["lnp_spec"][k * n:(k + 1) * n][w] for k in range(3)])
    rw = R.iteration_end_ref(dim, m, n, lo, n + lo, s["h0"]["x"][:, w], c0[w].copy(), dec[w], dec, s["X1"][:, w],
                             c1[w].copy(), s["lnp1"][w], c0, c1, spec_w, st_spec[:3 * m], 2.0, seed, it,
                             np.zeros(m, np.int32))
    assert (~rw["local"]).sum() >= 4 and (rw["v"] & ~rw["local"]).any() and (~rw["v"] & ~rw["local"]).any()
    np.testing.assert_array_equal(rw["j"], s["j1"][w])
    np.testing.assert_array_equal(rw["x1"], s["h1"]["x"][:, w])
    np.testing.assert_array_equal(rw["lnp1"], s["h1"]["lnp"][w])
    np.testing.assert_array_equal(rw["acc"], s["h1"]["acc"][w])
