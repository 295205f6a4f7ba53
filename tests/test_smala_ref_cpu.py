"""tests/smala_ref.py checked on its own: closed forms, identities at 40 digits, agreement with the
float64 restatement on well-conditioned matrices, and the conditions the GPU tests
(tests/test_gpu_smala_kernels.py) rely on -- cond limits, Cholesky pivots away from zero, and an empty
tie window in the accept cases."""
import mpmath as mp
import numpy as np
import pytest

import smala_ref as R

EPS = R.EPS


def test_closed_form_one_parameter():
    for a, alpha in ((2.5, 1.0), (-0.75, 1e3), (1e-12, 1e3), (0.0, 1.0)):
        x, g = np.array([1.25]), np.array([-3.0])
        r = R.metric_ref(x, -7.0, g, np.array([[-a]]), alpha, EPS)
        with mp.workdps(R.DPS):
            lt = 1 / mp.mpf(alpha) if abs(alpha * a) < 1e-8 else mp.mpf(a) * mp.coth(mp.mpf(alpha) * mp.mpf(a))
            assert r["G"][0, 0] == float(lt) and r["Ginv"][0, 0] == float(1 / lt)
            assert r["L"][0, 0] == float(1 / mp.sqrt(lt))
            assert r["mu"][0] == float(mp.mpf(1.25) + mp.mpf(EPS) ** 2 / 2 * mp.mpf(-3.0) / lt)
            assert r["logdet"] == float(-mp.log(lt))
        assert r["cond"] == 1.0 and r["lp"] == -7.0


def test_closed_form_diagonal():
    d = np.array([4.0, -2.0, 0.5, 1e-12, -7.25])
    alpha = 1e3
    r = R.metric_ref(np.ones(5), 0.0, np.ones(5), -np.diag(d), alpha, EPS)
    with mp.workdps(R.DPS):
        lt = [1 / mp.mpf(alpha) if abs(alpha * v) < 1e-8 else mp.mpf(float(v)) * mp.coth(alpha * mp.mpf(float(v)))
              for v in d]
        want = np.array([float(v) for v in lt])
        want_inv = np.array([float(1 / v) for v in lt])
        want_l = np.array([float(1 / mp.sqrt(v)) for v in lt])
    assert want[3] == 1.0 / alpha
    # eigsy orders the eigenvalues; G = diag(lambda~) exactly in the input's order
    np.testing.assert_array_equal(r["G"], np.diag(want))
    np.testing.assert_array_equal(r["Ginv"], np.diag(want_inv))
    np.testing.assert_array_equal(r["L"], np.diag(want_l))


def test_closed_form_two_by_two():
    """[[a, b], [b, a]]: eigenvectors (1, 1)/sqrt 2 and (1, -1)/sqrt 2, eigenvalues a + b and a - b."""
    a, b, alpha = 1.0, 3.0, 1.0  # indefinite: a - b = -2
    r = R.metric_ref(np.array([0.5, -0.5]), 0.0, np.array([1.0, 2.0]), -np.array([[a, b], [b, a]]), alpha, EPS)
    with mp.workdps(R.DPS):
        l1, l2 = mp.mpf(4) * mp.coth(4), mp.mpf(-2) * mp.coth(-2)
        G = np.array([[float((l1 + l2) / 2), float((l1 - l2) / 2)], [float((l1 - l2) / 2), float((l1 + l2) / 2)]])
        Gi = np.array([[float((1 / l1 + 1 / l2) / 2), float((1 / l1 - 1 / l2) / 2)],
                       [float((1 / l1 - 1 / l2) / 2), float((1 / l1 + 1 / l2) / 2)]])
        assert r["logdet"] == float(-mp.log(l1) - mp.log(l2))
        assert r["cond"] == float(l1 / l2)
    np.testing.assert_array_equal(r["G"], G)
    np.testing.assert_array_equal(r["Ginv"], Gi)


@pytest.mark.parametrize("P", [1, 4, 20])
def test_closed_form_zero_matrix(P):
    alpha = 1e3
    x, g = np.linspace(1, 2, P), np.linspace(-1, 1, P) + 0.25
    r = R.metric_ref(x, 0.0, g, np.zeros((P, P)), alpha, EPS)
    np.testing.assert_array_equal(r["G"], np.eye(P) / alpha)
    np.testing.assert_array_equal(r["Ginv"], np.eye(P) * alpha)
    with mp.workdps(R.DPS):
        assert r["logdet"] == float(P * mp.log(alpha))
        np.testing.assert_array_equal(r["L"], np.eye(P) * float(mp.sqrt(alpha)))
    np.testing.assert_allclose(r["mu"], x + EPS ** 2 / 2 * alpha * g, rtol=4 * R.U)
    assert r["cond"] == 1.0


@pytest.mark.parametrize("P,name,alpha", [(5, "indefinite", 1e3), (5, "rank1", 1e3), (3, "graded_wide", 1.0),
                                          (20, "graded_hessian", 1e3), (20, "eye_plus_rank1", 1.0)])
def test_identities_at_40_digits(P, name, alpha):
    m = R.case_ref(P, name, alpha)["mp"]
    with mp.workdps(R.DPS):
        eye = mp.eye(P)
        scale = mp.norm(m["G"], mp.inf) * mp.norm(m["Ginv"], mp.inf)
        assert mp.norm(m["G"] * m["Ginv"] - eye, mp.inf) < mp.mpf(10) ** -30 * scale
        assert mp.norm(m["L"] * m["L"].T - m["Ginv"], mp.inf) < mp.mpf(10) ** -35 * mp.norm(m["Ginv"], mp.inf)
        assert all(m["L"][i, j] == 0 for i in range(P) for j in range(i + 1, P))
        assert abs(m["logdet"] + mp.fsum(mp.log(l) for l in m["lam_twig"])) < mp.mpf(10) ** -35
        # log det G^-1 independently of the eigenvalues: 2 sum log L_jj
        assert abs(m["logdet"] - 2 * mp.fsum(mp.log(m["L"][j, j]) for j in range(P))) < mp.mpf(10) ** -30


@pytest.mark.parametrize("P", [2, 3, 5, 20])
def test_agrees_with_float64_restatement_where_well_conditioned(P):
    alphas = (1.0, 1e3) if P < 20 else (1.0,)
    for name in R.WELL_CONDITIONED:
        for alpha in alphas:
            r = R.case_ref(P, name, alpha)
            assert r["cond"] <= R.COND_BULK
            n = R.metric_numpy(r["lp"], r["grad"], -r["A"], r["x"], alpha, EPS)
            for k in ("G", "Ginv", "L", "mu"):
                np.testing.assert_allclose(n[k], r[k], rtol=0, atol=1e-12 * np.abs(r[k]).max(), err_msg=f"{name} {k}")
            assert abs(n["logdet"] - r["logdet"]) < 1e-12 * max(1.0, abs(r["logdet"]))


def _all_cases(P):
    for name, A, alphas, limit in R.metric_cases(P):
        for alpha in alphas:
            yield name, A, alpha, limit


@pytest.mark.parametrize("P", [1, 2, 3, 5, 19, 20])
def test_generator_matrices_are_what_they_claim(P):
    cases = {n: a for n, a, *_ in R.metric_cases(P)}
    assert tuple(cases) == R.FAMILIES
    again = {n: a for n, a, *_ in R.metric_cases(P)}
    for n, A in cases.items():
        np.testing.assert_array_equal(A, A.T)
        np.testing.assert_array_equal(A, again[n])  # deterministic
    lam = {n: np.linalg.eigvalsh(a) for n, a in cases.items()}
    assert lam["spd"].min() > 0
    assert not cases["zeros"].any() and not (cases["diagonal"] - np.diag(np.diag(cases["diagonal"]))).any()
    assert len(set(np.diag(cases["diagonal"]))) == P
    if P >= 2:
        assert lam["indefinite"].min() < -0.4 and lam["indefinite"].max() > 0.4
        assert np.abs(lam["rank1"][:-1]).max() < 1e-14 and abs(lam["rank1"][-1] - 4.0) < 1e-14
        np.testing.assert_allclose(lam["eye_plus_rank1"][:-1], 2.0, rtol=1e-14)
        b = cases["blocks"]
        assert b[0, 0] == b[1, 1] and b[0, 1] != 0.0


@pytest.mark.parametrize("P", [1, 2, 3, 5])
def test_generator_cond_limits_and_cholesky_pivots(P):
    n_bulk = n_all = 0
    for name, A, alpha, limit in _all_cases(P):
        r = R.case_ref(P, name, alpha)
        assert r["cond"] <= limit, (name, alpha, r["cond"])
        assert r["pivot"] > 1e-6, (name, alpha, r["pivot"])
        n_all += 1
        n_bulk += r["cond"] <= R.COND_BULK
    assert 2 * n_bulk > n_all  # the bulk of the cases sits in the 1e-10 tolerance class


def test_generator_cond_limits_at_the_largest_sizes():
    """P = 19, 20: cond of every case from the eigenvalues alone (the GPU test asserts the same, and the
    pivots, on the full reference it computes anyway); the full reference for the cases the accept
    tests use and the two graded ones."""
    for P in (19, 20):
        for name, A, alpha, limit in _all_cases(P):
            with mp.workdps(R.DPS):
                lam = mp.eigsy(mp.matrix(A.tolist()), eigvals_only=True)
                lt = [1 / mp.mpf(alpha) if abs(alpha * l) < mp.mpf(R.SOFTABS_SMALL) else l * mp.coth(alpha * l)
                      for l in lam]
                assert max(lt) / min(lt) <= limit, (P, name, alpha)
    for name, A, alpha, limit in _all_cases(20):
        if alpha == 1.0 or name == "graded_hessian":
            r = R.case_ref(20, name, alpha)
            assert r["cond"] <= limit and r["pivot"] > 1e-6, (name, alpha, r["cond"], r["pivot"])


@pytest.mark.parametrize("P", [1, 3, 20])
def test_accept_cases_have_an_empty_tie_window_and_both_outcomes(P):
    a = R.accept_cases(P)
    margin = np.abs(a["log_ratio"] - np.log(a["u"]))
    assert (margin >= 1e-9).all(), margin  # zero chains in the tie window: the GPU test exempts none
    assert a["accept"].any() and not a["accept"].all()
    for c in range(R.ACCEPT_CHAINS):  # caches valid and different per chain
        assert a["cur"][c]["ok"] == 1 and np.isfinite(a["prop"][c]["lp"])
        if P > 1:
            assert not np.array_equal(a["cur"][c]["G"], a["prop"][c]["G"])
        if c:
            assert not np.array_equal(a["cur"][c]["G"], a["cur"][c - 1]["G"])


def test_gauss_newton_closed_form():
    """Two epochs, two parameters, numbers exact in binary: -H = (2/N) J^T W J by hand."""
    rv = np.zeros((2, 5))
    rv[0, 1], rv[0, 2], rv[0, 3], rv[0, 4] = 1.0, 0.5, 2.0, 1.0   # J_0 = (0.5/den0, 1/den1)
    rv[1, 1], rv[1, 2], rv[1, 3], rv[1, 4] = 0.0, 1.0, 3.0, 3.0   # J_1 = (-1/den0, 0)
    den = np.array([0.5, 0.25])
    H = R.gauss_newton(rv, np.array([2.0, 4.0]), den, 4.0)
    J = np.array([[1.0, 4.0], [-2.0, 0.0]])
    want = -(2.0 / 4.0) * J.T @ np.diag([2.0, 4.0]) @ J
    np.testing.assert_array_equal(np.array([[float(H[i, j]) for j in range(2)] for i in range(2)]), want)
    assert R.gauss_newton(np.zeros((0, 5)), np.zeros(0), den, 4.0) == mp.zeros(2, 2)


@pytest.mark.parametrize("P,n_obs", [(1, 130), (3, 1), (3, 65), (20, 64)])
def test_gauss_newton_float64_sum_is_within_its_rounding_bound(P, n_obs):
    rng = np.random.default_rng(7 * P + n_obs)
    rv = 1e-4 * rng.standard_normal((n_obs, 2 * P + 1))
    w = 1e-3 * rng.uniform(0.5, 2.0, n_obs)
    den = R.fd_den(rng.uniform(0.05, 2.0, P), np.full(P, 0.5), 1e-6)
    H = R.gauss_newton(rv, w, den, 100.0)
    Hm = np.array([[float(H[i, j]) for j in range(P)] for i in range(P)])
    Hf = R.gauss_newton_f64(rv, w, den, 100.0)
    d = np.sqrt(-np.diag(Hm))
    assert (np.abs(Hf - Hm) <= R.gauss_newton_rounding(n_obs) * np.outer(d, d) + 1e-300).all()
    np.testing.assert_array_equal(Hf, Hf.T)


def test_fd_den_takes_both_branches():
    x = np.array([3.0, -1e-3, 0.0])
    fl = np.array([1.0, 1e-2, 1e-2])
    d = R.fd_den(x, fl, 1e-6)
    np.testing.assert_array_equal(d, [(3.0 + 3e-6) - (3.0 - 3e-6), (-1e-3 + 1e-8) - (-1e-3 - 1e-8), 1e-8 - -1e-8])


def test_mvn_logq_matches_scipy_free_closed_form():
    """One dimension: log N(y; mu, eps^2 / g)."""
    y, mu, g, eps = 0.7, 0.2, 3.0, 0.5
    got = float(R.mvn_logq(np.array([y]), np.array([mu]), np.array([[g]]), float(-np.log(g)), eps))
    var = eps ** 2 / g
    want = -0.5 * ((y - mu) ** 2 / var + np.log(2 * np.pi * var))
    assert abs(got - want) < 1e-15


def test_philox_normal_restates_box_muller():
    import philox_ref

    seed, item, it = (1 << 40) + 12345, (1 << 32) + 1, (1 << 32) + 5
    for base in (philox_ref.RNG_MH_PROPOSE, philox_ref.RNG_SMALA_PROPOSE):
        for p in (0, 27):
            u0, u1 = philox_ref.uniform2(seed, item, it, base | (p << 8))
            z = philox_ref.normal(seed, item, it, base, p)
            assert abs(z - np.sqrt(-2 * np.log(u0)) * np.cos(2 * np.pi * u1)) < 1e-14
    assert philox_ref.normal(seed, item, it, 3, 1) != philox_ref.normal(seed, item, it, 3, 0)
    assert philox_ref.normal(seed, item, it, 3, 1) != philox_ref.normal(seed, item, it, 5, 1)
    assert (philox_ref.RNG_SMALA_PROPOSE, philox_ref.RNG_SMALA_ACCEPT, philox_ref.RNG_PT_SWAP) == (5, 6, 7)
