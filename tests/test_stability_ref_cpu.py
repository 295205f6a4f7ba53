"""The stability screen's restatement and its truth (tests/stability_ref.py, tests/golden/stability_truth.json).

No GPU: the fixture is what a fresh mpmath run gives, the float run decides every status and step count as the
truth does, the float run's errors are the constants the GPU tier's bound is taken from, and no decision of any
case lies within MARGIN of its threshold -- the reference alone decides them."""
import pytest

import stability_ref as R


@pytest.fixture(scope="module")
def fixture():
    return R.load_fixture()


@pytest.fixture(scope="module")
def float_runs(fixture):
    return {n: R.float_errors(c, fixture[n]["truth"]) for n, c in R.cases().items()}


def test_fixture_holds_the_case_table(fixture):
    cases = R.cases()
    assert list(fixture) == list(cases)
    for n, c in cases.items():
        assert {k: fixture[n][k] for k in c} == c, n
        assert len(fixture[n]["truth"]) == R.N_STATES


def test_case_table_covers_the_instantiations(fixture):
    seen = {(len(c["states"][0]), c["inclined"]) for c in fixture.values()}
    assert {(1, False), (2, False), (2, True), (3, False), (3, True), (4, False)} <= seen
    assert all(R.N_STATES % (64 // L) != 0 for L in (1, 2, 4))
    q = fixture["quiet3_inclined_256"]
    assert q["inclined"] and q["sample_every"] * q["n_blocks"] == 256 and all(t["status"] == R.OK for t in q["truth"])


@pytest.mark.parametrize("name", R.LIVE)
def test_truth_recomputed_live(fixture, name):
    runs = R.run_case(R.cases()[name], R.mpf)
    assert [R.record(r) for r in runs] == fixture[name]["truth"]


def test_named_cases_end_as_stated(fixture):
    """The encounter case ends in block 3 with the wide exit distance and survives 64 blocks with the narrow one;
    the escape case ends in block 6 at |r| = 3.109; the t = 0 states."""
    se = 4
    assert all((t["status"], t["steps"]) == (R.ENCOUNTER, 3 * se) for t in fixture["encounter_hill4"]["truth"])
    assert all((t["status"], t["steps"]) == (R.OK, 64 * se) for t in fixture["encounter_hill1"]["truth"])
    assert all((t["status"], t["steps"]) == (R.ESCAPE, 6 * se) for t in fixture["escape"]["truth"])
    nominal = fixture["escape"]["truth"][0]
    r2 = max(sum(float(x) ** 2 for x in p[:3]) for p in nominal["xv"])
    assert abs(r2 ** 0.5 - 3.109) < 5e-4
    assert [(t["status"], t["steps"]) for t in fixture["t0_status"]["truth"]] == [
        (R.OK, 32), (R.PRIOR, 0), (R.OK, 32), (R.ENCOUNTER, 0), (R.OK, 32)]
    assert fixture["t0_status"]["truth"][1]["xv"] is None and fixture["t0_status"]["truth"][3]["ext"] is None


def test_float_run_decides_as_the_truth(fixture, float_runs):
    for n, (runs, _) in float_runs.items():
        assert [(r.status, r.steps) for r in runs] == [(t["status"], t["steps"]) for t in fixture[n]["truth"]], n


def test_float_errors_are_the_recorded_ones(float_runs):
    """FLOAT_ERR, the constants behind the GPU tier's bound, are this float run's errors (to the 4 digits they are
    written with, and the last bits of another libm: 10 %)."""
    assert set(R.FLOAT_ERR) == set(float_runs)
    for n, (_, err) in float_runs.items():
        for k in R.KINDS:
            print(f"{n} {k}: measured {err[k]:.3e} recorded {R.FLOAT_ERR[n][k]:.3e}")
            assert err[k] == pytest.approx(R.FLOAT_ERR[n][k], rel=0.1), (n, k)


def test_no_decision_within_the_margin(fixture, float_runs):
    """Every d^2 / dmin2 at every kick and every |r| / r_max at every block end stays outside 1 +- MARGIN, in the
    truth and in the float run, in every case: none is excused."""
    for n, rec in fixture.items():
        ratios = [(t["enc_ratio"], t["esc_ratio"]) for t in rec["truth"]]
        ratios += [(r.enc_ratio, r.esc_ratio) for r in float_runs[n][0]]
        for enc, esc in ratios:
            assert enc is None or abs(enc - 1.0) > R.MARGIN, (n, enc)
            assert esc is None or abs(esc - 1.0) > R.MARGIN, (n, esc)
        # the tests were made: every integrated state of a case with an exit distance met a pair
        assert all(t["enc_ratio"] is not None for t in rec["truth"] if t["status"] != R.PRIOR), n
        assert all((t["esc_ratio"] is not None) == (rec["r_max"] > 0 and t["xv"] is not None) for t in rec["truth"]), n
