"""The recorded chain on the device (rvm_chain.hip, rvmcmc/chain.py) against tests/chain_ref.py.

Record is compared bit for bit with numpy indexing.  Moments and autocovariance are compared with the
longdouble restatement under a bound derived from the arithmetic, not fitted: with u = 2^-53, X = max |x|
of a column, A_k = sum_t |y_t y_t+k| and B = sum_t |y_t|, the mean errs by <= n u X, a walker's lag sum
by <= (n + 3) u A_k + 2 n u X B, and the walker tree adds (ceil(log2 W) + 2) u mean_w |S_kw|
(chain_ref.autocov computes it per entry).  The tests assert |device - reference| <= 2 x that bound (the
factor covers second-order terms and the fused multiply-add) and that the bound itself is below
1e-6 acov[0]: a one-sample slip in a tail moves an entry by ~ acov[0] / n and cannot hide under it.
Every call runs twice and must give the same bits.

diagnostics(): tests/test_chain_ref_cpu.py shows that no window decision of the AR(1) cases is near a tie
(margins >= 0.19 against the ~1e-10 a device error of the bound above moves m - c tau(m)), so `window`
is compared exactly; tau and ess at rtol 1e-9, rhat at rtol 1e-10.
"""
import numpy as np
import pytest

import chain_ref as R
from conftest import S2_SCALES
from support import rvm_lib, s2_state_and_obs, tight_ball as _start, to_device, torch_or_fail as _torch

pytestmark = pytest.mark.gpu

U = 2.0 ** -53


def _dev(a, dtype=np.float64):
    return to_device(a, dtype, copy=True)  # (a copy: inputs stay read-only)


# ---- record -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("with_lnp", [True, False])
@pytest.mark.parametrize("n_cols", [1, 64, 65])
@pytest.mark.parametrize("col_stride,src_col0", [(1, 0), (3, 0), (1, 5), (3, 7)])
def test_record_is_numpy_indexing(col_stride, src_col0, n_cols, with_lnp):
    """Two segments (two sources) into one slot of a three-slot chain: the slot equals numpy's strided
    indexing bit for bit, everything else keeps its NaN fill."""
    torch = _torch()
    L, lib = rvm_lib()
    P, ld = 3, src_col0 + (n_cols - 1) * col_stride + 4
    rng = np.random.default_rng(1000 * col_stride + 10 * src_col0 + n_cols)
    srcs = [rng.standard_normal((P, ld)) for _ in range(2)]
    lnps = [rng.standard_normal(ld) for _ in range(2)]
    Wd = 2 * n_cols + 3  # (three columns no segment writes)
    chain = torch.full((3, P, Wd), float("nan"), dtype=torch.float64, device="cuda")
    lnp = torch.full((3, Wd), float("nan"), dtype=torch.float64, device="cuda")
    for seg in range(2):
        s, l = _dev(srcs[seg]), _dev(lnps[seg])
        rc = lib.rvm_chain_record(P, n_cols, s.data_ptr(), ld, src_col0, col_stride, chain[1].data_ptr(), Wd,
                                  seg * n_cols, l.data_ptr() if with_lnp else 0,
                                  lnp[1].data_ptr() if with_lnp else 0, L.stream_handle())
        assert rc == 0, lib.rvm_last_error()
    torch.cuda.synchronize()
    got, got_l = chain.cpu().numpy(), lnp.cpu().numpy()
    want = np.full((3, P, Wd), np.nan)
    want_l = np.full((3, Wd), np.nan)
    for seg in range(2):
        want[1, :, seg * n_cols:(seg + 1) * n_cols] = R.record(srcs[seg], src_col0, col_stride, n_cols)
        if with_lnp:
            want_l[1, seg * n_cols:(seg + 1) * n_cols] = R.record(lnps[seg], src_col0, col_stride, n_cols)
    np.testing.assert_array_equal(got, want)  # (NaN == NaN here; values bit for bit)
    np.testing.assert_array_equal(got_l, want_l)


# ---- moments and autocovariance ---------------------------------------------------------------------------

# (n, W, P, t0): n = 1, 2, 16, 17, 37, 257; W = 1, 63, 64, 65, 200 and 300 (two walker blocks); P = 1, 10
SHAPES = [(1, 1, 1, 0), (2, 63, 1, 0), (16, 64, 10, 0), (17, 65, 1, 2), (37, 200, 10, 0), (257, 65, 1, 3),
          (257, 1, 1, 0), (17, 300, 2, 1), (2, 1, 10, 1)]


def _lag_ranges(n):
    want = [(0, 1), (0, 16), (0, 17), (16, 33), (n - 2, n), (0, n)]
    return sorted({(lo, hi) for lo, hi in want if 0 <= lo < hi <= n})


_shape_cache = {}


def _shape_case(shape):
    """(x [t0 + n + 1][P][W] with a step before and after the range that must not be read as part of it,
    reference mean, m2, acov [P][n], bound [P][n]) -- computed once per shape, never modified."""
    if shape not in _shape_cache:
        n, W, P, t0 = shape
        rng = np.random.default_rng(n * 1000 + W)
        z = rng.standard_normal((t0 + n + 1, P, W))
        for t in range(1, z.shape[0]):
            z[t] = 0.5 * z[t - 1] + z[t]
        x = (0.5 + 0.25 * np.arange(P))[None, :, None] + 1e-3 * z
        x[t0 + n:] += 100.0  # (a read past t1 - 1 shows)
        if t0:
            x[:t0] -= 100.0
        mean, m2 = R.moments(x, t0, t0 + n)
        acov, bound = R.autocov(x, t0, t0 + n, 0, n, with_bound=True)
        for a in (x, mean, m2, acov, bound):
            a.setflags(write=False)
        _shape_cache[shape] = (x, mean, m2, acov, bound)
    return _shape_cache[shape]


def _device_moments(xd, P, W, t0, t1):
    torch = _torch()
    L, lib = rvm_lib()
    outs = []
    for _ in range(2):
        mean = torch.full((P * W + 4,), -7.0, dtype=torch.float64, device="cuda")
        m2 = torch.full((P * W + 4,), -7.0, dtype=torch.float64, device="cuda")
        rc = lib.rvm_chain_moments(xd.data_ptr(), P, W, t0, t1, mean.data_ptr(), m2.data_ptr(), L.stream_handle())
        assert rc == 0, lib.rvm_last_error()
        torch.cuda.synchronize()
        outs.append((mean, m2))
    for a, b in zip(outs[0], outs[1]):
        assert torch.equal(a, b)  # the same bits from run to run
        assert bool((a[P * W:] == -7.0).all())  # nothing written past the arrays
    return outs[0][0][:P * W].view(P, W), outs[0][1][:P * W].view(P, W)


def _device_autocov(xd, mean, P, W, t0, t1, lag0, n_lags):
    torch = _torch()
    L, lib = rvm_lib()
    nws = lib.rvm_chain_autocov_workspace_bytes(P, W, n_lags) // 8
    assert nws >= P * n_lags
    outs = []
    for _ in range(2):
        acov = torch.full((P * n_lags + 4,), -7.0, dtype=torch.float64, device="cuda")
        ws = torch.full((nws + 4,), float("nan"), dtype=torch.float64, device="cuda")
        ws[nws:] = -7.0
        rc = lib.rvm_chain_autocov(xd.data_ptr(), mean.data_ptr(), P, W, t0, t1, lag0, n_lags, acov.data_ptr(),
                                   ws.data_ptr(), L.stream_handle())
        assert rc == 0, lib.rvm_last_error()
        torch.cuda.synchronize()
        assert bool((acov[P * n_lags:] == -7.0).all()) and bool((ws[nws:] == -7.0).all())
        outs.append(acov[:P * n_lags].view(P, n_lags))
    assert torch.equal(outs[0], outs[1])
    return outs[0].cpu().numpy()


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "n%d-W%d-P%d-t%d" % s)
def test_moments_and_autocov_within_the_derived_bound(shape):
    n, W, P, t0 = shape
    x, mean_ref, m2_ref, acov_ref, bound = _shape_case(shape)
    xd = _dev(x)
    mean, m2 = _device_moments(xd, P, W, t0, t0 + n)
    X = np.abs(x[t0:t0 + n]).max(0)
    B = np.abs(x[t0:t0 + n].astype(R.LD) - mean_ref).sum(0)
    err_mean = np.abs(mean.cpu().numpy().astype(R.LD) - mean_ref)
    print(f"{shape}: mean err / (n u X) max {float((err_mean / (n * U * X)).max()):.3f}")
    assert np.all(err_mean <= n * U * X)
    bound_m2 = (n + 3) * U * m2_ref + 2 * n * U * X * B
    err_m2 = np.abs(m2.cpu().numpy().astype(R.LD) - m2_ref)
    assert np.all(err_m2 <= 2 * bound_m2)
    if n == 1:
        assert np.all(m2.cpu().numpy() == 0.0) and np.all(acov_ref == 0) and np.all(bound == 0)
    else:
        ratio = (bound / acov_ref[:, :1]).max()
        print(f"{shape}: bound / acov[0] max {float(ratio):.2e}")
        assert ratio < 1e-6
    for lo, hi in _lag_ranges(n):
        got = _device_autocov(xd, mean, P, W, t0, t0 + n, lo, hi - lo)
        err = np.abs(got.astype(R.LD) - acov_ref[:, lo:hi])
        b = bound[:, lo:hi]
        with np.errstate(invalid="ignore", divide="ignore"):
            worst = float(np.nanmax(np.where(b > 0, err / b, 0.0)))
        print(f"{shape} lags [{lo}, {hi}): err / bound max {worst:.3f}")
        assert np.all(err <= 2 * b), (lo, hi, worst)


# ---- diagnostics ------------------------------------------------------------------------------------------

class _Replay:
    """A sampler that only has positions: step() shows the next row of a prepared chain [n][P][W]."""

    def __init__(self, x):
        self.x = _dev(x)
        self.device = self.x.device
        self.iteration = 0
        self.cur = self.x[0]

    def step(self):
        self.cur = self.x[self.iteration]
        self.iteration += 1

    def _chain_segments(self):
        return [dict(x=self.cur, lnp=None, col0=0, n=self.cur.shape[1])]


def _recorded(x, **kw):
    from rvmcmc import chain

    sampler = _Replay(x)
    rec = chain.ChainRecorder(sampler, capacity=x.shape[0], lnprob=False, **kw)
    chain.run_mcmc(sampler, x.shape[0], rec)
    return rec


@pytest.mark.parametrize("index", range(len(R.AR1_CASES)))
def test_diagnostics_match_the_restatement(index):
    x0 = R.ar1_case(index)
    x = np.stack([x0, 3.0 - x0[::-1]], 1)  # [n][2][W]: the second parameter is the first one reversed in time
    n, _, W = x.shape
    rec = _recorded(x)
    assert rec.n == n and rec.n_walkers == W
    np.testing.assert_array_equal(rec.chain().cpu().numpy(), x)
    np.testing.assert_array_equal(rec.to_numpy(), np.transpose(x, (2, 0, 1)))
    d = rec.diagnostics()
    assert d.n_steps == n and d.n_walkers == W
    for p in range(2):
        tau, window, margin, _ = R.window_search(x[:, p, :])
        assert margin >= 0.1  # (the reversed copy too)
        rhat = R.split_rhat(x[:, p, :])
        print(f"case {index} param {p}: tau {d.tau[p]!r} vs {tau!r}, window {d.window[p]} vs {window}, "
              f"rhat {d.rhat[p]!r} vs {rhat!r}")
        assert d.window[p] == window
        assert abs(d.tau[p] - tau) <= 1e-9 * tau
        assert abs(d.ess[p] - n * W / tau) <= 1e-9 * n * W / tau
        assert abs(d.rhat[p] - rhat) <= 1e-10 * rhat
        assert abs(d.mean[p] - x[:, p, :].mean()) <= 1e-12 * abs(x[:, p, :].mean())
        assert abs(d.var[p] - x[:, p, :].var(ddof=1)) <= 1e-9 * x[:, p, :].var(ddof=1)
    assert d.long_enough == bool(n >= 50 * max(R.window_search(x[:, p, :])[0] for p in range(2)))
    # discard: the retained range moves
    d7 = rec.diagnostics(discard=min(7, n - 4))
    k = min(7, n - 4)
    assert d7.n_steps == n - k
    assert abs(d7.mean[0] - x[k:, 0, :].mean()) <= 1e-12 * abs(x[k:, 0, :].mean())
    assert abs(d7.rhat[1] - R.split_rhat(x[k:, 1, :])) <= 1e-10 * d7.rhat[1]


def test_diagnostics_edges():
    # a constant chain (1.5: its mean is exact): acov[0] = 0 -> tau nan, as integrated_time; rhat nan
    d = _recorded(np.full((16, 2, 5), 1.5)).diagnostics()
    assert np.isnan(d.tau).all() and np.isnan(d.ess).all() and np.isnan(d.rhat).all() and not d.long_enough
    assert (d.window == -1).all() and np.all(d.mean == 1.5) and np.all(d.var == 0.0)
    # too short for a window: taus[n - 1] (0 up to rounding, see tests/test_chain_ref_cpu.py: absolute)
    x = R.short_trend()
    d = _recorded(x[:, None, :]).diagnostics()
    tau, window, _, _ = R.window_search(x)
    assert window == 4 and d.window[0] == 4 and abs(d.tau[0] - tau) <= 1e-12
    # a single step: nothing to correlate
    d = _recorded(x[:1, None, :]).diagnostics()
    assert np.isnan(d.tau[0]) and np.isnan(d.rhat[0]) and d.n_steps == 1


def test_recorder_thin_stride_capacity():
    from rvmcmc import chain

    x = np.arange(10 * 2 * 7, dtype=np.float64).reshape(10, 2, 7)
    rec = _recorded(x[:9], thin=3, walker_stride=3)  # capacity 9, three of them used
    assert rec.n == 3 and rec.n_walkers == 3
    np.testing.assert_array_equal(rec.chain().cpu().numpy(), x[2:9:3, :, ::3])
    full = rec._chain.cpu().numpy()
    assert np.isnan(full[3:]).all()  # slots not pushed keep their NaN fill
    with pytest.raises(ValueError):
        rec.lnprob()
    s = _Replay(x)
    small = chain.ChainRecorder(s, capacity=2, lnprob=False)
    chain.run_mcmc(s, 2, small)
    with pytest.raises(ValueError, match="full"):
        small.push()
    assert small.n == 2
    with pytest.raises(ValueError):
        chain.run_mcmc(_Replay(x), 1, small)  # another sampler's recorder


# ---- end to end: fixed-step plan --------------------------------------------------------------------------

def _state_and_obs(**kw):
    return s2_state_and_obs(fixed_step=True, **kw)


def _run_pair(make, snapshot, n_steps=12, thin=3):
    """A sampler run with a recorder against a second one with the same seed stepped by hand: the
    recorded steps are the hand-gathered states after iterations thin, 2 thin, ..., bit for bit, and
    the recorder leaves the sampler's own bits alone."""
    torch = _torch()
    from rvmcmc.mcmc import ChainRecorder

    a, b = make(), make()
    rec = ChainRecorder(a, capacity=n_steps // thin + 2, thin=thin)
    assert a.run_mcmc(n_steps, rec) is rec
    want = []
    for i in range(n_steps):
        b.step()
        if (i + 1) % thin == 0:
            want.append(snapshot(b))
    torch.cuda.synchronize()
    assert rec.n == n_steps // thin and a.iteration == b.iteration == n_steps
    got, got_l = rec.chain().cpu().numpy(), rec.lnprob().cpu().numpy()
    for i, (pos, lnp) in enumerate(want):  # pos [W][dim], lnp [W]
        np.testing.assert_array_equal(got[i], pos.T)
        np.testing.assert_array_equal(got_l[i], lnp)
    assert len({w[0].tobytes() for w in want}) > 1  # the chain moved
    fa, fb = snapshot(a), snapshot(b)
    np.testing.assert_array_equal(fa[0], fb[0])
    np.testing.assert_array_equal(fa[1], fb[1])
    assert np.isnan(rec._chain[rec.n:].cpu().numpy()).all() and np.isnan(rec._lnp[rec.n:].cpu().numpy()).all()
    return rec


def test_ensemble_run_mcmc_records_the_hand_stepped_chain():
    from rvmcmc.ensemble import EnsembleSampler

    s, obs = _state_and_obs()
    X0 = _start(s, (64,), 11)

    def make():
        e = EnsembleSampler(64, s, obs, seed=5)
        e.set_positions(X0)
        return e

    rec = _run_pair(make, lambda e: (e.gather_positions(), e.gather_lnprob()))
    from rvmcmc.mcmc import ChainRecorder

    with pytest.raises(ValueError, match="set_positions"):
        ChainRecorder(EnsembleSampler(64, s, obs, seed=5), capacity=2)  # nothing to learn the layout from yet
    d = rec.diagnostics()  # four steps: too short for a window, so never long enough
    assert d.n_steps == 4 and d.n_walkers == 64 and d.tau.shape == (s.Nvars,)
    assert (d.window == 3).all() and not d.long_enough


def test_mh_chains_run_mcmc_records_the_hand_stepped_chain():
    from rvmcmc.mcmc import MhChains

    s, obs = _state_and_obs()
    _run_pair(lambda: MhChains(s, obs, S2_SCALES, 1e-3, 32, seed=3),
              lambda m: (m.X.t().cpu().numpy(), m.lnp.cpu().numpy()))


def test_pt_run_mcmc_records_the_cold_temperature():
    from rvmcmc.tempering import PTSampler

    s, obs = _state_and_obs(ignore_params=[["h", "k"], ["h", "k"]])  # 6 free parameters: 16 walkers suffice
    X0 = _start(s, (3, 16), 13)

    def make():
        pt = PTSampler(3, 16, s, obs, seed=7)
        pt.set_positions(X0)
        return pt

    _run_pair(make, lambda pt: (pt.positions()[0], pt.lnprob()[0]))


def test_smala_chains_run_mcmc_records_the_hand_stepped_chain():
    from rvmcmc.smala import SmalaChains

    s, obs = _state_and_obs()
    _run_pair(lambda: SmalaChains(s, obs, eps=0.5, alpha=1e3, n_chains=16, seed=3),
              lambda m: (m.X.t().cpu().numpy(), m.cache["lp"].cpu().numpy()), n_steps=4, thin=2)
