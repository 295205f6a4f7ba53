"""The posterior summaries on the device (rvm_summary.hip, rvmcmc/chain.py summary / draw / predict) against
tests/summary_ref.py.

Quantiles and draws are compared bit for bit (assert_array_equal: NaN matches NaN); the covariance with the
longdouble restatement under the bound summary_ref.cov derives, |device - reference| <= 2 x bound, and it
must be symmetric bit for bit.  Every call runs twice on a workspace filled with 0xFF bytes and must give
the same bits.

The select's size thresholds (rvm_summary.hip), each with a length on either side below:
  SEL_SEG = 2048         elements of a work unit along i: a line of 2048 is one unit, 2049 two, and
                         with them one block per row becomes two;
  SEL_MAX_BLOCKS = 2048  blocks of a launch over all rows: one row of 2048 units (lines) has a block per unit,
                         2049 units two units per block; five rows have 409 blocks each, so 409 | 410 lines.
Its two load paths: 16-byte loads when x is 16-byte aligned and both strides are even, 8-byte loads
otherwise -- the odd lengths and the misaligned case take the second.  There is no single-block path.
"""
import numpy as np
import pytest

import summary_ref as R
from conftest import S2_SCALES, s2_obs_oracle
from support import rvm_lib, s2_state, tight_ball, to_device, torch_or_fail as _torch

pytestmark = pytest.mark.gpu

SEL_SEG, SEL_MAX_BLOCKS = 2048, 2048
Q16 = np.array([0.0, 1.0, 0.5, 1.0 / 3.0, 0.25, 0.025, 0.16, 0.84, 0.975, 0.999, 1e-9, 0.75, 0.1, 0.9, 2.0 / 3.0, 0.6])
Q_SETS = [np.array([0.0]), np.array([1.0]), np.array([0.5]), np.array([1.0 / 3.0]), np.array([0.25]), Q16]


def _dev(a, dtype=np.float64):
    return to_device(a, dtype, copy=True)


def _device_quantiles(ptr, n_rows, row_stride, n_outer, outer_stride, n_inner, q):
    """rvm_rows_quantiles twice on a 0xFF-filled workspace: (out [n_rows][n_q], n_valid [n_rows])."""
    import ctypes as C

    torch = _torch()
    L, lib = rvm_lib()
    nws = lib.rvm_rows_quantiles_workspace_bytes(n_rows, len(q))
    assert nws > 0 and nws % 8 == 0
    qc = (C.c_double * len(q))(*q)
    outs = []
    for _ in range(2):
        out = torch.full((n_rows * len(q) + 4,), -7.0, dtype=torch.float64, device="cuda")
        nv = torch.full((n_rows + 4,), -7, dtype=torch.int64, device="cuda")
        ws = torch.full((nws + 32,), 0xFF, dtype=torch.uint8, device="cuda")
        rc = lib.rvm_rows_quantiles(ptr, n_rows, row_stride, n_outer, outer_stride, n_inner, qc, len(q), out.data_ptr(),
                                    nv.data_ptr(), ws.data_ptr(), L.stream_handle())
        assert rc == 0, lib.rvm_last_error()
        torch.cuda.synchronize()
        assert bool((out[n_rows * len(q):] == -7.0).all()) and bool((nv[n_rows:] == -7).all())
        assert bool((ws[nws:] == 0xFF).all())  # nothing written past the workspace
        outs.append((out[:n_rows * len(q)].view(n_rows, len(q)).cpu().numpy(), nv[:n_rows].cpu().numpy()))
    np.testing.assert_array_equal(outs[0][0].view(np.uint64), outs[1][0].view(np.uint64))  # the same bits
    np.testing.assert_array_equal(outs[0][1], outs[1][1])
    return outs[0]


def _from_bits(b):
    return np.asarray(b, dtype=np.uint64).view(np.float64)


def _contents(rng, shape):
    """name -> float64 array of `shape`: what a radix select can trip over."""
    n = int(np.prod(shape))
    two = np.where(rng.permutation(n) < (3 * n) // 10, -1.5, 2.25)
    low = _from_bits(np.float64(1.0).view(np.uint64) + rng.integers(0, 256, n).astype(np.uint64))
    # the top byte is the sign and seven exponent bits; the next exponent bits are 0, so no inf or NaN
    top = _from_bits((rng.integers(0, 256, n).astype(np.uint64) << np.uint64(56)) | np.uint64(0x0008000000000001))
    mixed = rng.standard_normal(n) * np.exp(rng.uniform(-30, 30, n))
    special = np.array([0.0, -0.0, np.inf, -np.inf, 5e-324, -5e-324, 2.2e-308, -2.2e-308, 1e-310, -1e-310])
    k = min(n, 3 * len(special))
    mixed[rng.choice(n, k, replace=False)] = np.resize(special, k)
    some_nan = rng.standard_normal(n)
    some_nan[rng.random(n) < 0.3] = np.nan
    out = {"gaussian": 0.88 + 1e-3 * rng.standard_normal(n), "equal": np.full(n, 3.25), "two": two, "low_byte": low,
           "top_byte": top, "mixed": mixed, "some_nan": some_nan, "all_nan": np.full(n, np.nan)}
    return {k: v.reshape(shape) for k, v in out.items()}


LENGTHS = [1, 2, 3, 255, 256, 257, SEL_SEG - 1, SEL_SEG, SEL_SEG + 1]


@pytest.mark.parametrize("n_rows", [1, 5])
@pytest.mark.parametrize("n", LENGTHS)
def test_contiguous_rows_bit_for_bit(n, n_rows):
    rng = np.random.default_rng(100 * n + n_rows)
    for name, x in _contents(rng, (n_rows, n)).items():
        xd = _dev(x)
        for q in (Q_SETS if name in ("gaussian", "mixed") else [Q16]):
            got, nv = _device_quantiles(xd.data_ptr(), n_rows, n, 1, n, n, q)
            want, m = R.rows_quantiles(x, q)
            np.testing.assert_array_equal(nv, m, err_msg=f"{name} n_valid")
            np.testing.assert_array_equal(got, want, err_msg=f"{name} q={q}")
            fin = ~np.isnan(want)  # (-0 and +0 compare equal above: their signs here)
            np.testing.assert_array_equal(np.signbit(got[fin]), np.signbit(want[fin]), err_msg=f"{name} signs")


def test_integer_h_is_the_order_statistic():
    x = np.random.default_rng(3).standard_normal((2, 257))
    xd = _dev(x)
    got, _ = _device_quantiles(xd.data_ptr(), 2, 257, 1, 257, 257, np.array([0.25, 0.5, 0.75]))
    np.testing.assert_array_equal(got, np.sort(x, axis=1)[:, [64, 128, 192]])


def test_misaligned_base_takes_the_narrow_loads():
    """Even strides from a base that is 8 but not 16 bytes aligned: the same bits as the aligned copy."""
    rng = np.random.default_rng(8)
    x = rng.standard_normal((5, 300))
    buf = _dev(np.concatenate([[1e30], x.ravel(), [-1e30]]))
    assert buf.data_ptr() % 16 == 0
    got, nv = _device_quantiles(buf.data_ptr() + 8, 5, 300, 1, 300, 300, Q16)
    want, m = R.rows_quantiles(x, Q16)
    np.testing.assert_array_equal(got, want)
    np.testing.assert_array_equal(nv, m)
    xd = _dev(x)
    aligned, _ = _device_quantiles(xd.data_ptr(), 5, 300, 1, 300, 300, Q16)
    np.testing.assert_array_equal(aligned, want)


def _chain_case(rng, n, P, W, t0, kind="gaussian"):
    """chain [t0 + n + 1][P][W]: parameter p within [10 p, 10 p + 1), the steps before t0 at -100 and the step
    after t1 at +100 (a stride slip or a read outside the range shows)."""
    x = 10.0 * np.arange(P)[None, :, None] + rng.random((t0 + n + 1, P, W))
    if kind == "some_nan":
        x[rng.random(x.shape) < 0.2] = np.nan
    x[:t0] = -100.0
    x[t0 + n:] = 100.0
    return x


@pytest.mark.parametrize("W", [1, 65, 300])
@pytest.mark.parametrize("n", [1, 17])
def test_chain_layout_bit_for_bit(n, W):
    P, t0 = 3, 2
    rng = np.random.default_rng(1000 * n + W)
    for kind in ("gaussian", "some_nan"):
        x = _chain_case(rng, n, P, W, t0, kind)
        xd = _dev(x)
        got, nv = _device_quantiles(xd.data_ptr() + 8 * t0 * P * W, P, W, n, P * W, W, Q16)
        want, m = R.chain_quantiles(x, t0, t0 + n, Q16)
        np.testing.assert_array_equal(nv, m)
        np.testing.assert_array_equal(got, want)
        if kind == "gaussian":
            assert np.all((got >= 10.0 * np.arange(P)[:, None]) & (got < 10.0 * np.arange(P)[:, None] + 1.0))


@pytest.mark.parametrize("P,n", [(1, SEL_MAX_BLOCKS), (1, SEL_MAX_BLOCKS + 1), (5, SEL_MAX_BLOCKS // 5),
                                 (5, SEL_MAX_BLOCKS // 5 + 1), (1, 3 * SEL_MAX_BLOCKS + 7)])
def test_units_per_block_threshold(P, n):
    """Lines of W = 3 are one work unit each: at most SEL_MAX_BLOCKS blocks share a launch's units."""
    W, t0 = 3, 1
    x = _chain_case(np.random.default_rng(n + P), n, P, W, t0)
    xd = _dev(x)
    got, nv = _device_quantiles(xd.data_ptr() + 8 * t0 * P * W, P, W, n, P * W, W, Q16)
    want, m = R.chain_quantiles(x, t0, t0 + n, Q16)
    np.testing.assert_array_equal(nv, m)
    np.testing.assert_array_equal(got, want)


def test_long_lines_several_units_per_block_and_line():
    """Lines of 2 SEL_SEG + 6 elements (three units each, the last one nearly empty), 1100 of them: 3300 units
    over at most 2048 blocks, so a block's two units cross line ends.  The wide loads."""
    W, n = 2 * SEL_SEG + 6, 1100
    rng = np.random.default_rng(77)
    x = rng.standard_normal((n, 1, W))
    x[rng.random(x.shape) < 0.01] = np.nan
    xd = _dev(x)
    got, nv = _device_quantiles(xd.data_ptr(), 1, W, n, W, W, Q16)
    want, m = R.chain_quantiles(x, 0, n, Q16)
    np.testing.assert_array_equal(nv, m)
    np.testing.assert_array_equal(got, want)


# ---- covariance -----------------------------------------------------------------------------------------

# (n, W, P, t0): the shapes of tests/test_gpu_chain.py's SHAPES
SHAPES = [(1, 1, 1, 0), (2, 63, 1, 0), (16, 64, 10, 0), (17, 65, 1, 2), (37, 200, 10, 0), (257, 65, 1, 3),
          (257, 1, 1, 0), (17, 300, 2, 1), (2, 1, 10, 1)]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "n%d-W%d-P%d-t%d" % s)
def test_cov_within_the_derived_bound(shape):
    torch = _torch()
    L, lib = rvm_lib()
    n, W, P, t0 = shape
    rng = np.random.default_rng(n * 1000 + W)
    z = rng.standard_normal((t0 + n + 1, P, W))
    for t in range(1, z.shape[0]):
        z[t] = 0.5 * z[t - 1] + z[t]
    z = z + 0.5 * z[:, ::-1, :]  # (the parameters correlate)
    x = (0.5 + 0.25 * np.arange(P))[None, :, None] + 1e-3 * z
    x[t0 + n:] += 100.0
    x[:t0] -= 100.0
    center = x[t0:t0 + n].transpose(1, 0, 2).reshape(P, -1).mean(1)
    want, bound = R.cov(x, t0, t0 + n, center, with_bound=True)
    xd, cd = _dev(x), _dev(center)
    nws = lib.rvm_chain_cov_workspace_bytes(P, W) // 8
    assert nws >= P * P
    outs = []
    for _ in range(2):
        cov = torch.full((P * P + 4,), -7.0, dtype=torch.float64, device="cuda")
        ws = torch.full((8 * (nws + 4),), 0xFF, dtype=torch.uint8, device="cuda").view(torch.float64)
        rc = lib.rvm_chain_cov(xd.data_ptr(), P, W, t0, t0 + n, cd.data_ptr(), cov.data_ptr(), ws.data_ptr(),
                               L.stream_handle())
        assert rc == 0, lib.rvm_last_error()
        torch.cuda.synchronize()
        assert bool((cov[P * P:] == -7.0).all())
        assert bool((ws.view(torch.uint8)[8 * nws:] == 0xFF).all())
        outs.append(cov[:P * P].view(P, P).cpu().numpy())
    np.testing.assert_array_equal(outs[0].view(np.uint64), outs[1].view(np.uint64))
    got = outs[0]
    np.testing.assert_array_equal(got.view(np.uint64), got.T.copy().view(np.uint64))  # symmetric bit for bit
    if n * W == 1:
        assert np.isnan(got).all()
        return
    err = np.abs(got.astype(R.LD) - want)
    with np.errstate(invalid="ignore", divide="ignore"):
        worst = float(np.max(np.where(bound > 0, err / bound, 0.0)))
    print(f"{shape}: err / bound max {worst:.3f}; bound / |cov| max {float((bound / np.abs(want)).max()):.2e}")
    assert np.all(err <= 2 * bound), worst
    assert np.all(np.diag(got) > 0)


# ---- draw -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("t0", [0, 3])
@pytest.mark.parametrize("W", [1, 65])
@pytest.mark.parametrize("n", [1, 37])
@pytest.mark.parametrize("S", [1, 64, 65, 300])
def test_draw_bit_for_bit(S, n, W, t0):
    torch = _torch()
    L, lib = rvm_lib()
    P = 3
    rng = np.random.default_rng(S + 10 * n + 100 * W + t0)
    x = rng.standard_normal((t0 + n + 1, P, W))
    xd = _dev(x)
    inj = rng.random((2, S))
    inj[0, 0] = 1.0  # exactly 1.0: the clamp
    inj[1, -1] = 1.0
    inj[1, 0] = 0.0
    for draws, seed, draw_id in ((None, 5, 0), (None, 5, 1), (inj, 0, 0)):
        dd = _dev(draws) if draws is not None else None
        outs = []
        for _ in range(2):
            xo = torch.full((P * S + 4,), -7.0, dtype=torch.float64, device="cuda")
            idx = torch.full((S + 4,), -7, dtype=torch.int64, device="cuda")
            rc = lib.rvm_chain_draw(xd.data_ptr(), P, W, t0, t0 + n, S, seed, draw_id,
                                    dd.data_ptr() if dd is not None else 0, xo.data_ptr(), idx.data_ptr(),
                                    L.stream_handle())
            assert rc == 0, lib.rvm_last_error()
            torch.cuda.synchronize()
            assert bool((xo[P * S:] == -7.0).all()) and bool((idx[S:] == -7).all())
            outs.append((xo[:P * S].view(P, S).cpu().numpy(), idx[:S].cpu().numpy()))
        np.testing.assert_array_equal(outs[0][0], outs[1][0])
        np.testing.assert_array_equal(outs[0][1], outs[1][1])
        want_x, want_i = R.draw(x, t0, t0 + n, S, seed, draw_id, draws)
        np.testing.assert_array_equal(outs[0][1], want_i)
        np.testing.assert_array_equal(outs[0][0], want_x)
        np.testing.assert_array_equal(outs[0][0], x.transpose(1, 0, 2).reshape(P, -1)[:, outs[0][1]])
        assert outs[0][1].min() >= t0 * W and outs[0][1].max() < (t0 + n) * W


# ---- end to end -----------------------------------------------------------------------------------------

_e2e = {}


def _recorded_ensemble():
    """The S2 system, 20 observations, 64 walkers, 20 recorded steps -- run once, shared, not modified."""
    if not _e2e:
        from rvmcmc.chain import ChainRecorder
        from rvmcmc.ensemble import EnsembleSampler

        s = s2_state()
        obs = s2_obs_oracle(Npoints=20)
        X0 = tight_ball(s, (64,), 11)
        e = EnsembleSampler(64, s, obs, seed=5)
        e.set_positions(X0)
        rec = ChainRecorder(e, capacity=20)
        e.run_mcmc(20, rec)
        _e2e.update(state=s, obs=obs, sampler=e, rec=rec, chain=rec.chain().cpu().numpy())
        _e2e["chain"].setflags(write=False)
    return _e2e


def test_summary_end_to_end():
    c = _recorded_ensemble()
    rec, x, s = c["rec"], c["chain"], c["state"]
    assert len({x[t].tobytes() for t in range(20)}) > 1  # the chain moved
    for discard in (0, 7):
        sm = rec.summary(discard=discard)
        n, P, W = 20 - discard, s.Nvars, 64
        assert sm.keys == s.get_rawkeys() and sm.n_steps == n and sm.n_walkers == W
        assert sm.quantiles.shape == (P, 5) and sm.cov.shape == (P, P)
        np.testing.assert_array_equal(np.transpose(rec.to_numpy(), (1, 2, 0)), x)
        want_q, _ = R.chain_quantiles(x, discard, 20, sm.q)
        np.testing.assert_array_equal(sm.quantiles, want_q)
        d = rec.diagnostics(discard=discard)
        np.testing.assert_array_equal(sm.mean.view(np.uint64), d.mean.view(np.uint64))
        want_c, bound = R.cov(x, discard, 20, sm.mean, with_bound=True)
        assert np.all(np.abs(sm.cov.astype(R.LD) - want_c) <= 2 * bound)
        np.testing.assert_array_equal(sm.cov, sm.cov.T)
        np.testing.assert_array_equal(sm.sd, np.sqrt(np.diag(sm.cov)))
        np.testing.assert_array_equal(np.diag(sm.corr), np.ones(P))
        np.testing.assert_allclose(sm.corr, want_c.astype(np.float64) / np.outer(sm.sd, sm.sd), rtol=1e-9, atol=1e-12)
        assert np.all(np.abs(sm.corr) <= 1.0 + 1e-12)
    one = rec.summary(q=[0.5])
    np.testing.assert_array_equal(one.quantiles, R.chain_quantiles(x, 0, 20, [0.5])[0])


def test_draw_end_to_end():
    c = _recorded_ensemble()
    rec, x = c["rec"], c["chain"]
    X, idx = rec.draw(128, discard=4, seed=9, draw_id=2)
    want_x, want_i = R.draw(x, 4, 20, 128, 9, 2)
    np.testing.assert_array_equal(idx.cpu().numpy(), want_i)
    np.testing.assert_array_equal(X.cpu().numpy(), want_x)
    with pytest.raises(ValueError):
        rec.draw(0)
    with pytest.raises(ValueError):
        rec.draw(4, discard=20)


def test_predict_end_to_end():
    torch = _torch()
    c = _recorded_ensemble()
    rec, x, s, e = c["rec"], c["chain"], c["state"], c["sampler"]
    times = np.linspace(-30.0, 60.0, 16)
    assert (times < 0).any() and (times > 0).any()
    S = 128
    b = rec.predict(times, n_samples=S, return_samples=True)
    assert b.bands.shape == (5, 16) and b.q.tolist() == [0.025, 0.16, 0.5, 0.84, 0.975]
    X, idx = b.X.cpu().numpy(), b.idx.cpu().numpy()
    np.testing.assert_array_equal(X, x.transpose(1, 0, 2).reshape(s.Nvars, -1)[:, idx])
    np.testing.assert_array_equal(idx, R.draw(x, 0, 20, S, 0, 0)[1])
    # the same launch again: the same bits
    _, st2, rv2 = s.get_logp_batch(rec._epochs[1], b.X, hill_factor=e.hill_factor, want_rv=True, pmap=e.pmap)
    assert torch.equal(st2, b.status)
    rv = b.rv.cpu().numpy()
    np.testing.assert_array_equal(rv.view(np.uint64), rv2.cpu().numpy().view(np.uint64))
    status = b.status.cpu().numpy()
    assert rv.shape == (16, S) and (status == 0).all()  # (states of the chain: every one was accepted)
    masked = np.where((status == 0)[None, :], rv, np.nan)
    want, m = R.rows_quantiles(masked, b.q)
    np.testing.assert_array_equal(b.bands, want.T)
    np.testing.assert_array_equal(b.n_valid, m)
    assert np.all(np.diff(b.bands, axis=0) >= 0) and np.ptp(b.bands) > 0
    # the centre of the band is the RV curve of a central state, up to the posterior's width
    ref = s.get_rv(times)
    assert np.all(np.abs(b.bands[2] - ref) < 0.2 * np.ptp(ref) + 1e-3)

    # the caller's samples, one with a negative mass: status PRIOR, left out of every epoch
    Xs = b.X.clone()
    ok = np.flatnonzero(status == 0)
    col = int(ok[len(ok) // 2])
    Xs[s.get_rawkeys().index("m"), col] = -1e-3
    b2 = rec.predict(times, samples=Xs, return_samples=True)
    st = b2.status.cpu().numpy()
    assert st[col] == 1 and b2.idx is None
    np.testing.assert_array_equal(np.delete(st, col), np.delete(status, col))
    assert np.all(b2.n_valid == S - 1)
    want2, _ = R.rows_quantiles(np.delete(masked, col, axis=1), b2.q)
    np.testing.assert_array_equal(b2.bands, want2.T)

    with pytest.raises(ValueError, match="RVM_MAX_EPOCHS_PER_DIRECTION"):
        rec.predict(np.linspace(1.0, 100.0, 1701), n_samples=4)
    with pytest.raises(ValueError, match="RVM_MAX_EPOCHS_PER_DIRECTION"):
        rec.predict(-np.linspace(1.0, 100.0, 1701), n_samples=4)
    with pytest.raises(ValueError):
        rec.predict(times, samples=Xs[:3])


# ---- predict() on the other three samplers ------------------------------------------------------------------

def _fixed_step_state(**kw):
    return s2_state(fixed_step=True, **kw)


def _make_mh():
    from rvmcmc.mcmc import MhChains

    return MhChains(_fixed_step_state(), s2_obs_oracle(Npoints=20), S2_SCALES, 1e-3, 32, seed=3)


def _make_pt():
    from rvmcmc.tempering import PTSampler

    s = _fixed_step_state(ignore_params=[["h", "k"], ["h", "k"]])  # 6 free parameters: 16 walkers suffice
    pt = PTSampler(3, 16, s, s2_obs_oracle(Npoints=20), seed=7)
    pt.set_positions(tight_ball(s, (3, 16), 13))
    return pt


def _make_smala():
    from rvmcmc.smala import SmalaChains

    return SmalaChains(_fixed_step_state(), s2_obs_oracle(Npoints=20), eps=0.5, alpha=1e3, n_chains=16, seed=3)


@pytest.mark.parametrize("make", [_make_mh, _make_pt, _make_smala], ids=["mh", "pt", "smala"])
def test_predict_on_the_other_samplers(make):
    from rvmcmc.chain import ChainRecorder

    sampler = make()
    rec = ChainRecorder(sampler, capacity=4)
    sampler.run_mcmc(4, rec)
    x = rec.chain().cpu().numpy()
    P = rec.n_params
    assert P == sampler.state.Nvars
    times = np.linspace(-10.0, 20.0, 8)
    b = rec.predict(times, n_samples=32, discard=1, seed=2, return_samples=True)
    idx, status, rv = b.idx.cpu().numpy(), b.status.cpu().numpy(), b.rv.cpu().numpy()
    np.testing.assert_array_equal(idx, R.draw(x, 1, 4, 32, 2, 0)[1])
    np.testing.assert_array_equal(b.X.cpu().numpy(), x.transpose(1, 0, 2).reshape(P, -1)[:, idx])
    assert (status == 0).all() and np.ptp(rv) > 0  # (recorded states: each was accepted, or the start)
    want, m = R.rows_quantiles(rv, b.q)
    np.testing.assert_array_equal(b.bands, want.T)
    np.testing.assert_array_equal(b.n_valid, m)
    sm = rec.summary(discard=1)
    assert sm.keys == sampler.state.get_rawkeys()
    np.testing.assert_array_equal(sm.quantiles, R.chain_quantiles(x, 1, 4, sm.q)[0])
