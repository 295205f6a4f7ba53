"""The restatement tests/chain_ref.py against driver.integrated_time and mpmath, the host half of
rvmcmc/chain.py (the block-fed window search), and the argument errors of the three chain entry points
-- none of which needs a device.

(b) below is what lets tests/test_gpu_chain.py compare `window` exactly: no window decision of the
AR(1) cases is near a tie.  Measured margins |m - c tau(m)| (window, lag before): 0.28 .. 0.76 in the
issue's prototype; this file asserts >= 0.1 on the inputs as generated here.
"""
import ctypes as C

import numpy as np
import pytest

import chain_ref as R
from support import refusal_text as _err
from rvmcmc import _lib, chain, driver

CASES = list(range(len(R.AR1_CASES)))


@pytest.mark.parametrize("index", CASES)
def test_restatement_tau_matches_integrated_time(index):
    x = R.ar1_case(index)
    tau, window, _, computed = R.window_search(x)
    want = driver.integrated_time(x)
    print(f"case {index}: tau {tau!r} vs integrated_time {want!r}, rel {abs(tau - want) / want:.2e}, "
          f"window {window}, lags computed {computed} of {x.shape[0]}")
    assert abs(tau - want) <= 1e-12 * abs(want)


@pytest.mark.parametrize("index", CASES)
def test_no_window_decision_is_near_a_tie(index):
    _, window, margin, _ = R.window_search(R.ar1_case(index))
    print(f"case {index}: window {window}, margin {margin:.3f}")
    assert window >= 1 and margin >= 0.1


@pytest.mark.parametrize("index", CASES)
def test_block_fed_search_is_integrated_time(index):
    """rvmcmc.chain.WindowSearch fed float64 autocovariance blocks gives the restatement's tau and window."""
    x = R.ar1_case(index)
    n = x.shape[0]
    s = chain.WindowSearch(n)
    assert chain.lag_blocks(n) == R.lag_blocks(n)
    for lo, hi in chain.lag_blocks(n):
        s.feed(R.autocov(x[:, None, :], 0, n, lo, hi - lo)[0].astype(np.float64))
        if s.done:
            break
    tau, window, _, _ = R.window_search(x)
    assert s.done and s.window == window and abs(s.tau - tau) <= 1e-12 * tau


def test_search_edges_are_integrated_time_s():
    # a constant chain (1.5: its mean is exact in every arithmetic): acov[0] = 0 -> nan
    s = chain.WindowSearch(8)
    s.feed(np.zeros(8))
    assert s.done and np.isnan(s.tau) and np.isnan(driver.integrated_time(np.full((8, 3), 1.5)))
    assert np.isnan(R.window_search(np.full((8, 3), 1.5))[0])
    # too short for a window: taus[n - 1].  With the walkers' own means subtracted the lag sums of a
    # walker add up to acov[0] / 2, so taus[n - 1] is 0 up to rounding and the comparison is absolute
    # (the taus are sums of acf values of order 1).  Five steps of a trend: taus = 1, 1.8, 1.6, 0.8, 0
    # and m < 5 taus[m] holds up to m = 3 (3 < 4: no tie).
    x = R.short_trend()
    n = x.shape[0]
    tau, window, _, _ = R.window_search(x)
    want = driver.integrated_time(x)
    assert window == n - 1 and abs(tau - want) <= 1e-12 and abs(tau) <= 1e-12
    s = chain.WindowSearch(n)
    s.feed(R.autocov(x[:, None, :], 0, n, 0, n)[0].astype(np.float64))
    assert s.done and s.window == n - 1 and abs(s.tau - want) <= 1e-12


def test_longdouble_autocov_matches_mpmath():
    x = R.ar1_case(0)[:40, None, :3] + np.zeros((1, 2, 1))
    x[:, 1] += 0.37
    a, bound = R.autocov(x, 3, 40, 2, 9, with_bound=True)
    mp = R.autocov_mp(x, 3, 40, 2, 9)
    # longdouble: 2^-64 per operation against the bound's 2^-53
    assert np.all(np.abs(a.astype(np.float64) - mp) <= bound.astype(np.float64) / 256 + 1e-16 * np.abs(mp))
    m, m2 = R.moments(x, 3, 40)
    np.testing.assert_allclose(m.astype(np.float64), x[3:40].mean(0), rtol=1e-14)
    np.testing.assert_allclose(m2.astype(np.float64), ((x[3:40] - x[3:40].mean(0)) ** 2).sum(0), rtol=1e-9)


def test_record_restatement_is_numpy_indexing():
    src = np.arange(3 * 40.0).reshape(3, 40)
    np.testing.assert_array_equal(R.record(src, 2, 3, 5), src[:, [2, 5, 8, 11, 14]])
    np.testing.assert_array_equal(R.record(src[0], 0, 1, 1), src[0, :1])


def test_split_rhat_of_identical_halves_is_below_one():
    x = R.ar1_case(1)
    r = R.split_rhat(x)
    assert 0.9 < r < 1.2
    assert np.isnan(R.split_rhat(np.full((10, 4), 1.5))) and np.isnan(R.split_rhat(x[:3]))


# ---- (c) argument errors: < 0 before any HIP call, the argument named ----------------------------------

def test_record_argument_errors():
    lib = _lib.load()
    d = 8  # (never dereferenced: every call below fails its checks first)
    rec = lambda **k: lib.rvm_chain_record(*[{**dict(n_params=2, n_cols=4, src=d, src_ld=16, src_col0=0,  # noqa: E731
                                                     col_stride=1, dst=d, dst_ld=8, dst_col0=0, lnp_src=0, lnp_dst=0,
                                                     stream=0), **k}[a]
                                             for a in ("n_params", "n_cols", "src", "src_ld", "src_col0", "col_stride",
                                                       "dst", "dst_ld", "dst_col0", "lnp_src", "lnp_dst", "stream")])
    assert b"n_params" in _err(rec(n_params=0))
    assert b"n_cols" in _err(rec(n_cols=0))
    assert b"null src" in _err(rec(src=0))
    assert b"null dst" in _err(rec(dst=0))
    assert b"col_stride" in _err(rec(col_stride=0))
    assert b"src_col0" in _err(rec(src_col0=-1))
    assert b"dst_col0" in _err(rec(dst_col0=-1))
    assert b"src_ld" in _err(rec(src_col0=4, col_stride=4))  # last column 16 of a 16-column source
    assert b"dst_ld" in _err(rec(dst_col0=5))
    assert b"lnp_dst" in _err(rec(lnp_src=d))
    assert b"lnp_src" in _err(rec(lnp_dst=d))


def test_moments_argument_errors():
    lib = _lib.load()
    d = 8
    assert b"null chain" in _err(lib.rvm_chain_moments(0, 2, 4, 0, 5, d, d, 0))
    assert b"n_params" in _err(lib.rvm_chain_moments(d, 0, 4, 0, 5, d, d, 0))
    assert b"n_cols" in _err(lib.rvm_chain_moments(d, 2, -1, 0, 5, d, d, 0))
    assert b"t0" in _err(lib.rvm_chain_moments(d, 2, 4, -1, 5, d, d, 0))
    assert b"t1" in _err(lib.rvm_chain_moments(d, 2, 4, 5, 5, d, d, 0))
    assert b"mean_out" in _err(lib.rvm_chain_moments(d, 2, 4, 0, 5, 0, d, 0))
    assert b"m2_out" in _err(lib.rvm_chain_moments(d, 2, 4, 0, 5, d, 0, 0))


def test_autocov_argument_errors():
    lib = _lib.load()
    d = 8
    ac = lambda *a: lib.rvm_chain_autocov(*a, 0)  # noqa: E731
    assert b"null chain" in _err(ac(0, d, 2, 4, 0, 10, 0, 4, d, d))
    assert b"null mean" in _err(ac(d, 0, 2, 4, 0, 10, 0, 4, d, d))
    assert b"n_params" in _err(ac(d, d, 0, 4, 0, 10, 0, 4, d, d))
    assert b"n_cols" in _err(ac(d, d, 2, 0, 0, 10, 0, 4, d, d))
    assert b"t0" in _err(ac(d, d, 2, 4, -2, 10, 0, 4, d, d))
    assert b"t1" in _err(ac(d, d, 2, 4, 3, 3, 0, 4, d, d))
    assert b"lag0" in _err(ac(d, d, 2, 4, 0, 10, -1, 4, d, d))
    assert b"n_lags" in _err(ac(d, d, 2, 4, 0, 10, 0, 0, d, d))
    assert b"lag0 + n_lags" in _err(ac(d, d, 2, 4, 0, 10, 7, 4, d, d))  # lag 10 of 10 steps
    assert b"lag0 + n_lags" in _err(ac(d, d, 2, 4, 2, 10, 0, 9, d, d))  # t0 shortens the range
    assert b"acov_out" in _err(ac(d, d, 2, 4, 0, 10, 0, 4, 0, d))
    assert b"workspace" in _err(ac(d, d, 2, 4, 0, 10, 0, 4, d, 0))
    # [P][lags rounded up to 16][blocks of 256 walkers] doubles; 0 on bad arguments
    wsb = lib.rvm_chain_autocov_workspace_bytes
    assert wsb(10, 200, 17) == 8 * 10 * 32 * 1 and wsb(3, 257, 16) == 8 * 3 * 16 * 2 and wsb(1, 1, 1) == 8 * 16
    assert wsb(0, 4, 4) == 0 and wsb(2, 0, 4) == 0 and wsb(2, 4, 0) == 0
    assert isinstance(C.c_size_t(wsb(1, 1, 1)).value, int)
