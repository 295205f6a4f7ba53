"""tests/invariance_ref.py judged on the CPU: the Philox restatement against the published vectors, the exact
samplers and analytic rates against themselves, the reference transitions against the STRICT thresholds, and
every seeded slip against the LOOSE ones.

Which statistic catches which mutant, and by how much (this file's runs; W = 4096 / C = 8192 as the GPU cases):

  mutant          case      caught by (largest)                      others that miss LOOSE
  exponent_dim    stretch5  sum r2 z = +18.2                         ks r2 p = 3e-47
  z_uniform       stretch5  sum r2 z = +17.5                         ks r2 p = 3e-56
  shared_counter  stretch5  sum r2 z = -35.6                         w|w+1 sq z = +15, half 0|1 sq z = +13, ks r2
  no_beta         pt4       swap rates z = +154, +274, +279          sum r2 of t1 .. t3 z = -53 .. -87
  swap_factor     pt4       swap rates z = -14, -17, -23             none: the variances move 2 - 3 sigma only
  swap_sign       pt4       sum r2 of t0 z = +656                    sq z-scores (to +2485), swap rates (to +248)
  mh_no_old       mh1       acceptance z = +174, sum r2 z = +68      ks r2 p = 0, ks x0 p = 7e-134
  no_logdet       smala     mean y2 z = -43, mean y4 z = -34         ks sum y4/4 p = 2e-311, ks y_i p = 1e-33
  drift_eps2      smala     acceptance fraction 0.604 against 0.535  none: see below

(The pair statistics use the target's moments, not the sample's, so a wrong marginal law moves them as well: they
are pure tests of independence only where the marginal statistics pass.)

What the test cannot see.  (1) drift_eps2: a slip in the proposal that the log q terms share (the drift, the step,
the metric itself) leaves the target invariant -- Metropolis-Hastings corrects any proposal -- so no
distributional statistic can catch it; only the acceptance fraction, held within ACC_TOL of the reference's,
moves (by 0.07 here).  A consistent slip that moves the acceptance by less than 0.02 passes.  (2) A strict
against a non-strict comparison (> for >=) differs at exact ties only, which have probability ~1e-16 per decision.
(3) A slip that changes the law by less than ~4.5 / sqrt(W d) relative in every moment tested.  (4) mh_no_old is
invisible on a target whose log-probability has its maximum at 0 (the rule min(1, exp(lnp_new)) is then
reversible); Gauss.OFFSET = 2 is what exposes it.
"""
import math

import mpmath as mp
import numpy as np
import pytest

import invariance_ref as I
import philox_ref
import pt_ref


# ---- Philox4x32-10 against the published known-answer vectors (Random123 kat_vectors) -------------------------

KAT = [
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
     (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
]


@pytest.mark.parametrize("ctr,key,want", KAT)
def test_philox_known_answer_vectors(ctr, key, want):
    assert philox_ref.philox4x32_10(ctr, *key) == want


@pytest.mark.parametrize("ctr,key,want", KAT)
def test_philox_vectorised_restatement_gives_the_same_words(ctr, key, want):
    """uniform2_vec builds its counter as (item lo, item hi, iteration lo, iteration hi & 0xFFFF | stream << 16) and
    returns ((x >> 5) 2^26 + (y >> 6) + 0.5) / 2^53 of the words: the same from the published ones."""
    item, it, stream = ctr[0] | (ctr[1] << 32), ctr[2] | ((ctr[3] & 0xFFFF) << 32), ctr[3] >> 16
    seed = key[0] | (key[1] << 32)
    x, y, z, w = want
    u = (((x >> 5) << 26 | (y >> 6)) + 0.5) / 2.0 ** 53, (((z >> 5) << 26 | (w >> 6)) + 0.5) / 2.0 ** 53
    assert philox_ref.uniform2(seed, item, it, stream) == u
    got = philox_ref.uniform2_vec(seed, np.array([item], dtype=np.uint64), it, stream)
    assert (float(got[0][0]), float(got[1][0])) == u


# ---- the exact samplers, the analytic rates ---------------------------------------------------------------------

@pytest.mark.parametrize("case", list(I.CASES))
def test_exact_sampler_passes_its_own_statistics(case):
    """The start of every case, and a second independent draw against it for the pair statistics."""
    c, tgt = I.CASES[case], I.target(case)
    V = I.whitened(case, I.start(case))
    rows = [r for t, v in enumerate(V) for r in tgt.stats(v, f"{case} start t{t}")]
    n = V[0].shape[1]
    rows += I.pair_stats(tgt, V[0][:, :n // 2], V[0][:, n // 2:], f"{case} start halves")
    I.show(rows)
    assert not I.misses(rows, I.P_STRICT, I.Z_STRICT)
    assert len(V) == (len(c["betas"]) if c["kind"] == "ens" else 1)


def test_quartic_moments_and_derivatives():
    tgt = I.Quartic(3, 1)
    with mp.workdps(30):
        assert math.isclose(tgt.M2, float(2 * mp.gamma(mp.mpf(3) / 4) / mp.gamma(mp.mpf(1) / 4)), rel_tol=1e-14)
        # E |y|^m = 4^(m/4) Gamma((m + 1) / 4) / Gamma(1/4): 1 at m = 4, 5 at m = 8
        assert math.isclose(float(16 * mp.gamma(mp.mpf(9) / 4) / mp.gamma(mp.mpf(1) / 4)), 5.0, rel_tol=1e-14)
    x = np.random.default_rng(0).standard_normal((3, 4))
    h = 1e-5
    for i in range(3):
        e = np.zeros((3, 1))
        e[i] = h
        np.testing.assert_allclose((tgt.lnp(x + e) - tgt.lnp(x - e)) / (2 * h), tgt.grad(x)[i], rtol=1e-8, atol=1e-9)
        np.testing.assert_allclose((tgt.grad(x + e) - tgt.grad(x - e)) / (2 * h), tgt.hess(x)[i], rtol=1e-8, atol=1e-9)
    lam = np.linalg.eigvalsh(-np.moveaxis(tgt.hess(x), 2, 0))
    np.testing.assert_allclose(lam, np.sort(3.0 * (tgt.R @ x).T ** 2, axis=1), rtol=1e-12, atol=1e-14)
    assert abs(tgt.hess(x)[0, 1]).min() > 1e-3  # not diagonal


def test_default_betas_is_the_package_ladder():
    from rvmcmc.tempering import default_betas

    np.testing.assert_array_equal(I.default_betas(4, 5), default_betas(4, 5))


def test_swap_rate_integral_closed_form_and_monte_carlo():
    """default_betas' "about 25 %" is the large-dimension limit; at d = 5 the neighbours exchange 44.9 % of the time."""
    b = I.default_betas(4, 5)
    want = I.swap_rate(b[0], b[1], 5)
    assert abs(want - 0.4486) < 5e-5
    assert abs(want - I.swap_rate_closed(b[0], b[1], 5)) < 1e-8
    assert abs(I.swap_rate(b[2], b[3], 5) - want) < 1e-12  # the ratio alone matters
    rng = np.random.default_rng(5)
    n = 2_000_000
    L1, L2 = -rng.chisquare(5, n) / (2 * b[0]), -rng.chisquare(5, n) / (2 * b[1])
    r = np.minimum(1.0, np.exp((b[0] - b[1]) * (L2 - L1)))
    z = (r.mean() - want) / (r.std() / math.sqrt(n))
    print(f"swap rate: integral {want:.6f} monte carlo {r.mean():.6f} z {z:+.2f}")
    assert abs(z) <= I.Z_STRICT
    # large dimension: the ladder's spacing approaches the rate its docstring names
    r = 1.0 + 2.0 * math.sqrt(math.log(4.0)) / math.sqrt(2000)
    assert abs(I.swap_rate_closed(1.0, 1.0 / r, 2000) - 0.25) < 0.02


def test_mh_rate_against_monte_carlo():
    s = 2.4
    rng = np.random.default_rng(6)
    n = 2_000_000
    x, g = rng.standard_normal(n), rng.standard_normal(n)
    r = np.minimum(1.0, np.exp(0.5 * (x * x - (x + s * g) ** 2)))
    z = (r.mean() - I.mh_rate(s)) / (r.std() / math.sqrt(n))
    print(f"mh rate: analytic {I.mh_rate(s):.6f} monte carlo {r.mean():.6f} z {z:+.2f}")
    assert abs(z) <= I.Z_STRICT


def test_sweep_is_pt_ref_swap():
    rng = np.random.default_rng(7)
    T, W, d = 4, 10, 3
    X, lnp, u = rng.standard_normal((d, T, W)), -rng.random((T, W)) * 5, rng.random((T - 1, W))
    betas = I.default_betas(T, d)
    pos, l2 = np.ascontiguousarray(np.moveaxis(X, 0, 2)), lnp.copy()
    want, _ = pt_ref.swap(pos, l2, betas, u)
    got = I.pt_sweep(X, lnp, betas, u)
    assert want.any() and not want.all()
    np.testing.assert_array_equal(got, want)
    np.testing.assert_array_equal(np.moveaxis(X, 0, 2), pos)
    np.testing.assert_array_equal(lnp, l2)


# ---- the reference passes STRICT, every mutant misses LOOSE -------------------------------------------------------

@pytest.mark.parametrize("case", list(I.CASES))
def test_reference_passes_the_strict_thresholds(case):
    res = I.reference(case)
    rows, move = I.evaluate(case, res["X"], res)
    I.show(rows)
    print(f"{case}: start rho {move['rho']:.3f} acceptance {move['accept']:.4f} swap {res['swap']}")
    assert not I.misses(rows, I.P_STRICT, I.Z_STRICT)
    assert move["rho"] <= I.RHO_MAX
    if case == "smala":
        assert 0.50 <= move["accept"] <= 0.75


def test_statistics_catch_a_repeated_ensemble():
    """The independence statistics on a state made dependent by hand: temperature 1 of the three equal-beta
    ensembles replaced by a copy of temperature 0 (what a Philox item without its t W term would give) passes every
    marginal statistic and misses the t|t+1 bounds."""
    res = I.reference("pt3equal")
    X = res["X"].copy()
    X[:, 1] = X[:, 0]
    missed = I.misses(I.evaluate("pt3equal", X, res)[0], I.P_MIN, I.Z_MAX)
    I.show(missed)
    assert missed and all("temperature" in n for n, _, _ in missed)


def test_statistic_count_of_the_gpu_file_is_within_the_budget():
    n = sum(len(I.evaluate(case, I.reference(case)["X"], I.reference(case))[0]) for case in I.CASES)
    print(f"{n} statistics, chance of a false alarm {n * I.P_MIN:.2e}")
    assert n * I.P_MIN <= I.BUDGET


MUTANT_CASE = dict(exponent_dim="stretch5", z_uniform="stretch5", shared_counter="stretch5", no_beta="pt4",
                   swap_factor="pt4", swap_sign="pt4", mh_no_old="mh1", no_logdet="smala", drift_eps2="smala")


def test_every_mutant_has_a_case():
    assert set(MUTANT_CASE) == set(I.MUTANTS)


@pytest.mark.parametrize("mutant", list(I.MUTANTS))
def test_mutant_misses_the_loose_thresholds(mutant):
    case = MUTANT_CASE[mutant]
    res = I.run(case, mutant=mutant)
    rows, move = I.evaluate(case, res["X"], res)
    missed = I.misses(rows, I.P_MIN, I.Z_MAX)
    I.show(missed)
    ref = I.reference(case)["accept"]
    print(f"{mutant}: {len(missed)} statistics miss; acceptance {move['accept']:.4f} against the reference's {ref:.4f}")
    if mutant == "drift_eps2":  # Metropolis-Hastings corrects a proposal's slip: the acceptance alone moves
        assert not missed
        assert abs(move["accept"] - ref) > 2.0 * I.ACC_TOL
    else:
        assert missed
        worst = max((abs(v) for _, k, v in missed if k == "z"), default=0.0)
        assert worst > 2.0 * I.Z_MAX or min(v for _, k, v in missed if k == "p") < 1e-10  # by many sigma


@pytest.mark.parametrize("case", list(I.RATE_SD))
def test_rate_sd_is_the_measured_one(case):
    """The committed sd of each rate, re-measured over the 16 seeds; always above the binomial bound."""
    sd = I.rate_sd(case)
    c = I.CASES[case]
    n = c["K"] * (c["W"] if case == "pt4" else c["C"])
    for (name, r), s, want in zip(I.analytic_rates(case), sd, I.RATE_SD[case]):
        print(f"{case} {name}: sd measured {s:.3e} committed {want:.3e} binomial {math.sqrt(r * (1 - r) / n):.3e}")
        assert abs(s - want) <= 0.05 * want
        assert want >= math.sqrt(r * (1 - r) / n)
