"""The stability screen on the device (rvm_stability.hip, rvmcmc/stability.py, ChainRecorder.stability) against
tests/stability_ref.py and its 40-digit truth (tests/golden/stability_truth.json).

Parity: status and steps equal the truth exactly; xv and ext agree with it within FLOOR_FACTOR = 3 x the float
restatement's own error, per case and quantity kind (stability_ref.FLOAT_ERR: measured on the CPU, never taken
from the kernel).  Then what the header promises bit for bit: the result does not depend on how the blocks are
split over launches, an ended state is never written again, and a state's bits do not depend on its column or its
neighbours.  Every case is a few hundred steps of at most a few dozen states."""
import math

import numpy as np
import pytest
import torch  # noqa: F401  (before librvmcmc.so is loaded: the process then holds one HIP runtime, torch's)

import stability_ref as R
import wh_ref as W
from conftest import S2_PLANETS, s2_obs_oracle
from support import rvm_lib, state_scales, to_device, torch_or_fail as _torch

gpu = pytest.mark.gpu


class Dev:
    """The five caller-owned arrays of n states and the two entry points on them, called directly."""

    def __init__(self, rows, n_planets, inclined, hill):
        torch = _torch()
        self.L, self.lib = rvm_lib()
        self.params = rows if torch.is_tensor(rows) else to_device(rows, np.float64, copy=True)
        self.np, self.inc, self.hill = n_planets, int(inclined), float(hill)
        self.n = n = int(self.params.shape[1])
        assert self.params.shape[0] == (7 if inclined else 5) * n_planets
        f64 = dict(dtype=torch.float64, device="cuda")
        self.xv, self.ext = torch.full((6, n_planets, n), -7.0, **f64), torch.full((3, n_planets, n), -7.0, **f64)
        self.status = torch.full((n,), -7, dtype=torch.int32, device="cuda")
        self.steps = torch.full((n,), -7, dtype=torch.int64, device="cuda")
        self.alive = torch.full((1,), -7, dtype=torch.int64, device="cuda")
        rc = self.lib.rvm_stability_init(n_planets, self.inc, n, self.params.data_ptr(), self.hill, self.xv.data_ptr(),
                                         self.ext.data_ptr(), self.status.data_ptr(), self.steps.data_ptr(),
                                         self.L.stream_handle())
        assert rc == 0, self.lib.rvm_last_error()

    def advance(self, h, sample_every, n_blocks, r_max=0.0, count=True):
        rc = self.lib.rvm_stability_advance(self.np, self.inc, self.n, self.params.data_ptr(), self.hill, h,
                                            sample_every, n_blocks, r_max, self.xv.data_ptr(), self.ext.data_ptr(),
                                            self.status.data_ptr(), self.steps.data_ptr(),
                                            self.alive.data_ptr() if count else 0, self.L.stream_handle())
        assert rc == 0, self.lib.rvm_last_error()
        return self

    def bits(self, col=None):
        """The five outputs as integer arrays (NaN compares by its bits), of every state or of one column."""
        out = [self.xv.cpu().numpy().view(np.int64), self.ext.cpu().numpy().view(np.int64),
               self.status.cpu().numpy(), self.steps.cpu().numpy()]
        return out if col is None else [a[..., col] for a in out]


def _same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


def _case_dev(name):
    c = R.cases()[name]
    return c, Dev(R.kernel_rows(c), len(c["states"][0]), c["inclined"], c["hill"])


@pytest.fixture(scope="module")
def fixture():
    return R.load_fixture()


@gpu
@pytest.mark.parametrize("name", list(R.cases()))
def test_parity_with_the_truth(fixture, name):
    c, d = _case_dev(name)
    truth = fixture[name]["truth"]
    st0 = d.status.cpu().numpy()
    assert np.all(d.steps.cpu().numpy() == 0)
    d.advance(c["h"], c["sample_every"], c["n_blocks"], c["r_max"])
    status, steps = R.truth_arrays(truth)
    assert np.array_equal(d.status.cpu().numpy(), status), (d.status.cpu().numpy(), status)
    assert np.array_equal(d.steps.cpu().numpy(), steps), (d.steps.cpu().numpy(), steps)
    assert int(d.alive.item()) == int((status == R.OK).sum())
    xv = d.xv.cpu().numpy().transpose(2, 1, 0)    # [n][np][6]
    ext = d.ext.cpu().numpy().transpose(2, 1, 0)  # [n][np][3]
    for i, t in enumerate(truth):
        if t["xv"] is None:  # not OK at t = 0: the setup's status, NaN in xv and ext
            assert st0[i] == t["status"] and np.all(np.isnan(xv[i])) and np.all(np.isnan(ext[i])), i
        else:
            assert st0[i] == R.OK and np.all(np.isfinite(xv[i])) and np.all(np.isfinite(ext[i])), i
            if not c["inclined"]:
                assert np.all(xv[i][:, 2] == 0.0) and np.all(xv[i][:, 5] == 0.0)
    err = R.errors(xv, ext, truth)
    for k in R.KINDS:
        print(f"{name} {k}: kernel {err[k]:.3e} float {R.FLOAT_ERR[name][k]:.3e} ratio {err[k] / R.FLOAT_ERR[name][k]:.2f}")
    for k in R.KINDS:
        assert err[k] <= R.FLOOR_FACTOR * R.FLOAT_ERR[name][k], (name, k, err[k], R.FLOAT_ERR[name][k])


@gpu
@pytest.mark.parametrize("name", ["one", "two_inclined", "three", "four", "encounter_hill4", "escape", "t0_status"])
def test_chunk_invariance_bit_for_bit(name):
    c = R.cases()[name]
    h, se, rm = c["h"], c["sample_every"], c["r_max"]
    whole = _case_dev(name)[1].advance(h, se, 8, rm).bits()
    split = _case_dev(name)[1].advance(h, se, 3, rm).advance(h, se, 5, rm).bits()
    ones = _case_dev(name)[1]
    for _ in range(8):
        ones.advance(h, se, 1, rm)
    assert _same(whole, split) and _same(whole, ones.bits())


@gpu
@pytest.mark.parametrize("name", ["encounter_hill4", "escape", "t0_status"])
def test_ended_states_are_frozen(name):
    c, d = _case_dev(name)
    h, se, rm = c["h"], c["sample_every"], c["r_max"]
    d.advance(h, se, 8, rm)
    ended = np.flatnonzero(d.status.cpu().numpy() != R.OK)
    assert len(ended) >= 2
    before = d.bits()
    d.advance(h, se, 3, rm).advance(h, se, 1, rm)
    after = d.bits()
    assert _same([a[..., ended] for a in before], [a[..., ended] for a in after])
    alive = np.flatnonzero(before[2] == R.OK)
    assert np.all(after[3][alive] == before[3][alive] + 4 * se)


def _mixed_two():
    """(target, neighbours, hill, h, sample_every, r_max): a quiet 2-planet state among states that end at t = 0
    (PRIOR, ENCOUNTER) and in different blocks (the escape case's outer planet started at different phases)."""
    target = W.pal_rows(R.ENCOUNTER_PLANETS)
    esc = [W.pal_rows([R.ESCAPE_PLANETS[0], dict(R.ESCAPE_PLANETS[1], l=l)]) for l in (2.0, 2.6, 3.2, 1.4, 0.8)]
    prior, enc = W.s2_bad_walkers(dict(walkers=[W.pal_rows(S2_PLANETS)]))
    return target, [prior, enc] + esc, 1.0, R.H20, 4, 3.0


def _mixed_three():
    planets = S2_PLANETS + W.EXTRA_PLANETS[:1]
    target = W.pal_rows(planets)
    prior = W.pal_rows(planets)
    prior[2][1] = 0.01
    return (target, [prior] + W._ball(target, 6, 2e-2, 11), 1.0, W.min_period(target) / 20.0, 3, 2.6)


@gpu
@pytest.mark.parametrize("mixed", [_mixed_two, _mixed_three])
def test_independent_of_column_and_neighbours(mixed):
    target, nbrs, hill, h, se, rm = mixed()
    npl, n, blocks = len(target), 40, 16

    def run(states, col):
        d = Dev(W.kernel_rows(states, False), npl, False, hill).advance(h, se, blocks, rm)
        return d, d.bits(col)

    def among(col):
        return [target if i == col else nbrs[i % len(nbrs)] for i in range(n)]

    _, alone = run([target], 0)
    d0, at0 = run(among(0), 0)
    _, at37 = run(among(37), 37)
    _, same_state = run([target] * n, 37)
    assert _same(alone, at0) and _same(alone, at37) and _same(alone, same_state)
    # the neighbours did end in different blocks, the wave's last one alive or not
    ends = set(d0.steps.cpu().numpy()[1:].tolist())
    assert len(ends) >= 4 and 0 in ends, ends
    assert int(d0.alive.item()) == int((d0.status.cpu().numpy() == R.OK).sum())


@gpu
def test_n_alive_is_the_count_of_ok_states():
    c, d = _case_dev("t0_status")
    d.advance(c["h"], c["sample_every"], 1, c["r_max"])
    assert int(d.alive.item()) == 3 == int((d.status.cpu().numpy() == R.OK).sum())
    d.alive.fill_(-7)
    d.advance(c["h"], c["sample_every"], 1, c["r_max"], count=False)
    assert int(d.alive.item()) == -7  # null n_alive_out: nothing written
    c, d = _case_dev("escape")
    d.advance(c["h"], c["sample_every"], 8, c["r_max"])
    assert int(d.alive.item()) == 0


@gpu
def test_recorder_stability_equals_the_abi():
    from rvmcmc import stability
    from rvmcmc.chain import ChainRecorder
    from rvmcmc.ensemble import EnsembleSampler
    from rvmcmc.state import State

    obs = s2_obs_oracle(2017, 20)
    s = State(planets=[dict(p) for p in S2_PLANETS])
    rng = np.random.default_rng(4)
    Wk = 64
    X0 = s.get_params() + 1e-3 * state_scales(s) * rng.standard_normal((Wk, s.Nvars))
    e = EnsembleSampler(Wk, s, obs, seed=6)
    e.set_positions(X0)
    rec = ChainRecorder(e, capacity=20)
    e.run_mcmc(20, rec)
    res = rec.stability(n_samples=32, orbits=50, return_samples=True)
    X, idx = rec.draw(32, 0, 0)
    assert torch.equal(idx, res.idx) and torch.equal(X, res.X)
    K = e.pmap.to_kernel(X).contiguous()
    Kh = K.cpu().numpy()
    a, m = Kh[1::5], Kh[0::5]
    p_min = float(np.min(2.0 * math.pi * np.sqrt(a * a * a / (1.0 + m))))
    assert res.h == pytest.approx(p_min / 20, rel=1e-14)
    se = 5
    blocks = math.ceil(50 * 20 / se - 1e-9)
    assert res.n_steps == blocks * se == 1000
    hf = getattr(e, "hill_factor", s.hillRadiusFactor)
    d = Dev(K, 2, False, hf).advance(res.h, se, blocks, 100.0 * float(a.max()))
    ext = d.ext.cpu().numpy()
    assert np.array_equal(res.status, d.status.cpu().numpy()) and np.array_equal(res.steps, d.steps.cpu().numpy())
    assert np.array_equal(res.a_min.view(np.int64), ext[0].view(np.int64))
    assert np.array_equal(res.a_max.view(np.int64), ext[1].view(np.int64))
    assert torch.equal(res.xv.view(torch.int64), d.xv.view(torch.int64))
    # the fields that follow from the arrays
    assert np.array_equal(res.stable, res.status == R.OK) and res.fraction_stable == float(np.mean(res.status == R.OK))
    assert np.all(res.steps[res.stable] == 1000) and res.fraction_stable > 0.5
    assert np.allclose(res.t_end_years, res.steps * res.h / (365.25 * 0.01720), rtol=1e-15)
    assert np.array_equal(res.e_max, np.sqrt(np.clip(ext[2], 0.0, None)))
    assert np.array_equal(res.unbound, np.any((ext[0] <= 0) | (ext[2] >= 1), axis=0))
    assert res.da_over_a.shape == (2, 32) and np.all(res.da_over_a[:, res.stable] < 0.1)
    # chunked and unchunked runs are equal
    chunked = rec.stability(n_samples=32, orbits=50, chunk_steps=130, return_samples=True)
    assert np.array_equal(chunked.status, res.status) and np.array_equal(chunked.steps, res.steps)
    assert torch.equal(chunked.xv.view(torch.int64), res.xv.view(torch.int64))
    assert torch.equal(chunked.ext.view(torch.int64), res.ext.view(torch.int64))
    # the caller's samples, through stability.screen
    direct = stability.screen(s, X, orbits=50, pmap=e.pmap, hill_factor=hf)
    assert direct.idx is None and np.array_equal(direct.status, res.status)
    assert np.array_equal(direct.a_max.view(np.int64), res.a_max.view(np.int64))
