"""tests/wh_ref.py and tests/golden/wh_derivs.json checked on their own, without a GPU: the
arbitrary-precision restatement against the C oracle (which also checks the oracle every T1 test
rests on), the float run against the mpf run, the HyperDual class on mpf against the
finite-difference truth, the fixture's regeneration, and the conditions the GPU tier
(tests/test_gpu_derivs_exact.py) relies on -- the branch counters of `eccentric`, the share of the
order-2 term in the "offset" Hessians, and every case's double-precision floor."""
import numpy as np
import pytest
from mpmath import mp, mpf

import oracle as O
import wh_ref as R

FX = R.load_fixture()
CASES = R.case_inputs()
WALKERS = [(n, w) for n, c in CASES.items() for w in range(len(c["walkers"]))]
RV_DPS = 30  # the comparisons with double need no more


def _oracle_rv(c, w):
    pl = np.ascontiguousarray(np.array(c["walkers"][w], dtype=np.float64))
    t = np.array(c["epochs"], dtype=np.float64)
    rv = np.full(len(t), np.nan)
    m, mp_ = O._mult(c["levels"])
    st = O.lib().rvo_whx_rv_seq(len(pl), O._p(pl), float(c["hill"]), O._p(t), len(t), float(c["dt"]), len(m), mp_, O._p(rv))
    return st, rv


def _rv_tol(c):
    return 1e-14 * float(np.abs(O.richardson_weights(tuple(c["levels"]))).sum())  # test_gpu_logl.T1_RV_ABS's form


@pytest.fixture(scope="module")
def mpf_runs():
    """One mpf run per case and walker, shared by the tests below."""
    out = {}
    with mp.workdps(RV_DPS):
        for n, w in WALKERS:
            c = CASES[n]
            out[n, w] = R.whx_rv(R.to_params(c["walkers"][w], mpf), c["inclined"], c["hill"], c["epochs"], c["dt"], c["levels"])
    return out


def test_fixture_holds_the_case_table():
    assert list(FX) == list(CASES)
    for n, c in CASES.items():
        assert {k: FX[n][k] for k in c} == c, n
        assert len(FX[n]["walkers_out"]) == len(c["walkers"])
    import support
    import test_gpu_derivs
    import test_gpu_logl
    from conftest import S2_PLANETS

    assert R.FLOOR == test_gpu_derivs.FLOOR and R.FLOOR_FACTOR == support.T1_SENS_FACTOR
    assert R.S2_PLANETS == S2_PLANETS and R.EXTRA_PLANETS == support.EXTRA_PLANETS
    assert R.S2_INCLINED == test_gpu_logl.S2_INCLINED
    assert R._ball(R.pal_rows(S2_PLANETS), 2, 1e-3, 0) == support.pal_ball(S2_PLANETS, 2, 1e-3, 0).tolist()


def test_mpf_restatement_matches_the_oracle(mpf_runs):
    worst = 0.0
    for n, w in WALKERS:
        c = CASES[n]
        st_o, rv_o = _oracle_rv(c, w)
        st, rv, _ = mpf_runs[n, w]
        assert st == st_o == R.OK, (n, w)  # every walker has status 0 in the reference
        with mp.workdps(RV_DPS):
            err = max(float(abs(a - mpf(float(b)))) for a, b in zip(rv, rv_o))
        worst = max(worst, err / _rv_tol(c))
        assert err <= _rv_tol(c), (n, w, err)
    print(f"largest |rv_mpf - rv_oracle| / (1e-14 sum|w|): {worst:.3f}")


def test_float_run_matches_the_mpf_run(mpf_runs):
    for n, w in WALKERS:
        c = CASES[n]
        st, rv, cnt = R.whx_rv(R.to_params(c["walkers"][w], float), c["inclined"], c["hill"], c["epochs"], c["dt"], c["levels"])
        assert st == R.OK and cnt == mpf_runs[n, w][2] == FX[n]["walkers_out"][w]["counters"]
        with mp.workdps(RV_DPS):
            err = max(float(abs(a - mpf(b))) for a, b in zip(mpf_runs[n, w][1], rv))
            # the fixture's truth RV is this function at 60 digits
            assert max(float(abs(a - mpf(b))) for a, b in zip(mpf_runs[n, w][1], FX[n]["walkers_out"][w]["truth"]["rv"])) < 1e-27
        assert err <= _rv_tol(c), (n, w, err)


def test_status_walkers_of_the_reference():
    c = CASES["s2"]
    bad = R.s2_bad_walkers(c)
    st = [R.whx_rv(R.to_params(wk, float), False, c["hill"], c["epochs"], c["dt"], c["levels"])[0] for wk in bad]
    assert st == [R.PRIOR, R.ENCOUNTER]
    P = np.array(bad)
    obs = O.OracleObs(tf=np.array(c["epochs"]), tb=np.zeros(0), rvf=np.zeros(6), rvb=np.zeros(0), errorf=np.ones(6),
                      errorb=np.zeros(0), Npoints=6)
    assert list(O.logl_whx_batch(P, 2, obs, c["dt"], tuple(c["levels"]), c["hill"])[1]) == st


def _scales(c, w):
    pr = 7 if c["inclined"] else 5
    return [max(abs(c["walkers"][w][r // pr][r % pr]), R.FLOOR[r % pr]) for r in c["dir_rows"]]


@pytest.mark.parametrize("name", R.REGENERATED)
def test_fixture_regenerates_and_hyperdual_on_mpf_matches_the_truth(name):
    """The stored digits come out of the committed generator's functions again; and the HyperDual
    class, run on mpf, agrees with the finite-difference truth to 1e-25 relative on every rv_i and
    rv_ij.  Entries that vanish identically (at t = 0 planet 1's velocity does not depend on planet
    2's elements) have no relative error: every entry is measured against max(|truth|, max|rv| /
    (s_i s_j)), s = max(|x|, FLOOR) the differencing's own unit, in which its roundoff
    (1e-60 / 1e-30) lies five orders below the bound."""
    c = CASES[name]
    with mp.workdps(R.TRUTH_DPS):
        for w in range(len(c["walkers"])):
            runs, cnt = {}, None
            for key, shifts in R.fd_points(c):
                st, runs[key], k = R.eval_point(c, w, shifts)
                assert st == R.OK
                cnt = k if key == "0" else cnt
            rec = R.make_walker_record(c, w, runs, cnt)
            have = FX[name]["walkers_out"][w]
            assert rec["truth"] == have["truth"] and rec["counters"] == have["counters"]
            for k in ("rv", "rv_i", "rv_ij"):  # (double results: equal up to the math library's last bits)
                a, b = np.array(rec["float_hd"][k]), np.array(have["float_hd"][k])
                np.testing.assert_allclose(a, b, rtol=1e-9, atol=1e-9 * np.abs(b).max())
            rv, rv_i, rv_ij = R.truth_from_runs(c, w, runs)
            hv, hv_i, hv_ij = R.hd_derivs(c, w, mpf)
            s, top = _scales(c, w), max(abs(x) for x in rv)
            worst = max(abs(a - b) / abs(b) for a, b in zip(hv, rv))
            for i in range(len(s)):
                worst = max([worst] + [abs(a - b) / max(abs(b), top / s[i]) for a, b in zip(hv_i[i], rv_i[i])])
                assert all(b != 0 for b in rv_i[i])
            p = 0
            for i in range(len(s)):
                for j in range(i + 1):
                    worst = max([worst] + [abs(a - b) / max(abs(b), top / (s[i] * s[j])) for a, b in zip(hv_ij[p], rv_ij[p])])
                    p += 1
            print(f"{name} walker {w}: HyperDual(mpf) vs truth, largest relative difference {float(worst):.1e}")
            assert worst < 1e-25


def test_eccentric_reaches_the_rare_branches():
    """From the reference alone: `eccentric` has steps on both sides of |beta| (dt/r0)^2 = 0.5 (the
    kernel's Halley iteration and its bracketed solver) and steps with |beta X^2| > 0.1 (the
    Stumpff quartering loop)."""
    c = FX["eccentric"]
    cnt = np.array(c["walkers_out"][0]["counters"])
    with mp.workdps(RV_DPS):
        _, _, again = R.whx_rv(R.to_params(c["walkers"][0], mpf), False, c["hill"], c["epochs"], c["dt"], c["levels"])
    assert again == cnt.tolist()
    n_steps = 0
    for sign in (1.0, -1.0):
        tprev = 0.0
        for at in sorted(abs(t) for t in c["epochs"] if (t >= 0.0) == (sign > 0)):
            n_steps += max(1, int(np.ceil((at - tprev) / c["dt"] - 1e-9))) if at > tprev else 0
            tprev = at
    total = n_steps * sum(c["levels"])
    assert 1 <= cnt[:, 0].sum() < total and cnt[:, 1].sum() >= 1
    e = np.hypot(c["walkers"][0][0][2], c["walkers"][0][0][3])
    assert abs(e - 0.6) < 1e-12


@pytest.mark.parametrize("name", list(CASES))
def test_offset_vector_weighs_the_second_order_term(name):
    """With observed RV = 0 the residual is the whole signal: r rv_ij carries more than a quarter of
    sum_e (|rv_i rv_j| + |r rv_ij|) / s^2 for at least half of the Hessian's entries, so a wrong rv.ab
    cannot hide behind rv.a rv.b (cases without a step are exempt).  Where observed RV = 0 does not
    reach that (cross-planet second derivatives are small: `three`, `four_inclined`; `one_level`),
    the observed RVs lie further from the model, (1 - f) x truth with f a power of two."""
    c = FX[name]
    obs = R.observation_vectors(c)
    f = R.offset_factor(c)
    assert 1.0 <= f <= 64.0
    assert np.abs(np.array(obs["offset"])).max() == 0.0 if f == 1.0 else name in ("three", "four_inclined", "one_level")
    truth = np.array([float(x) for x in c["walkers_out"][0]["truth"]["rv"]])
    z = (np.array(obs["fit"]) - truth) / R.SIGMA
    assert np.all(np.abs(z) < 4) and np.any(z != 0)
    if name in R.STEPLESS:
        return
    for rec in c["walkers_out"]:
        t = rec["truth"]
        share = np.array(R.second_order_share(t["rv"], t["rv_i"], t["rv_ij"], obs["offset"], [R.SIGMA] * len(truth)))
        print(f"{name}: offset factor {f:g}; entries with share > 0.25: {np.mean(share > 0.25):.2f}; median share {np.median(share):.2f}")
        assert np.mean(share > 0.25) >= 0.5


@pytest.mark.parametrize("vec", ["fit", "offset"])
@pytest.mark.parametrize("name", list(CASES))
def test_double_precision_floor_is_below_1e_9(name, vec):
    """The GPU tier's bound, 3 x the float hyper-dual restatement's largest scaled error against the
    truth, is at or below 1e-9 on every case: none is ill-conditioned."""
    with mp.workdps(R.TRUTH_DPS):
        p = R.problem(FX[name], vec)
    print(f"{name}/{vec}: float restatement scaled errors grad {p['floor_grad']:.2e} hess {p['floor_hess']:.2e}; bound {p['bound']:.2e}")
    assert 0 < p["bound"] <= 1e-9


@pytest.mark.parametrize("name", [n for n in CASES if n not in R.STEPLESS])
def test_bound_sees_a_small_error_in_the_second_order_variation(name):
    """What the tier is for: order-2 variations rv.ab wrong by 1e-7 relative (four orders below what
    second differences in double resolve) leave the "offset" bound, and order-1 variations wrong by as
    much leave both vectors', on every case that takes a step."""
    c = FX[name]
    with mp.workdps(R.TRUTH_DPS):
        for vec, key in (("offset", "rv_ij"), ("fit", "rv_i"), ("offset", "rv_i")):
            p = R.problem(c, vec)
            f = dict(c["walkers_out"][0]["float_hd"])
            f[key] = (np.array(f[key]) * (1 + 1e-7)).tolist()
            _, g, H = R.assemble(f["rv"], f["rv_i"], f["rv_ij"], p["obs_rv"], p["sigma"], p["npoints"], float)
            eg, eH = R.scaled_errors(g, H, p["truth"][0][1], p["truth"][0][2])
            assert max(eg, eH) > 10 * p["bound"], (vec, key, eg, eH, p["bound"])
