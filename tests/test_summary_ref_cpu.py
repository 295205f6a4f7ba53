"""The restatement tests/summary_ref.py against numpy, and the argument errors of the posterior-summary
entry points (rvm_rows_quantiles, rvm_chain_cov, rvm_chain_draw) -- none of which needs a device.

The quantile rule is numpy's 'linear' one up to its last roundings: numpy interpolates as
v_lo + g (v_hi - v_lo) or v_hi - (1 - g) (v_hi - v_lo) depending on g, each form with at most three
roundings of the magnitude |v_lo| + |v_hi|, so the two agree within 8 u (|v_lo| + |v_hi|), not bit for bit.
"""
import ctypes as C

import numpy as np
import pytest

import summary_ref as R
from support import refusal_text as _err
from rvmcmc import _lib

U = 2.0 ** -53
QS = np.array([0.0, 0.025, 0.16, 1.0 / 3.0, 0.5, 0.84, 0.975, 1.0])


def _special_values(rng, n):
    """n float64 values with denormals, +-0, +-inf and mixed signs among Gaussians."""
    v = rng.standard_normal(n) * np.exp(rng.uniform(-30, 30, n))
    special = np.array([0.0, -0.0, np.inf, -np.inf, 5e-324, -5e-324, 2.2e-308, -2.2e-308, 1e-310, -1e-310])
    k = min(n, 4 * len(special))
    v[rng.choice(n, k, replace=False)] = np.resize(special, k)
    return v


@pytest.mark.parametrize("n", [1, 2, 3, 4, 7, 100, 101, 1000, 5000])
def test_quantile_rule_against_numpy(n):
    rng = np.random.default_rng(n)
    for x in (rng.standard_normal(n), 0.88 + 1e-3 * rng.standard_normal(n), np.round(rng.standard_normal(n), 1)):
        got, m = R.quantile(x, QS)
        assert m == n
        want = np.quantile(x, QS)
        v = np.sort(x)
        for j, q in enumerate(QS):
            lo = int(np.floor(q * (n - 1)))
            hi = min(lo + 1, n - 1)
            assert abs(got[j] - want[j]) <= 8 * U * (abs(v[lo]) + abs(v[hi])), (n, q, got[j], want[j])
    # integer h: the order statistic itself
    assert R.quantile(np.arange(5.0)[::-1], [0.25, 0.5])[0].tolist() == [1.0, 2.0]


def test_quantile_rule_edges():
    nan = np.nan
    out, m = R.quantile([nan, nan], [0.5])
    assert m == 0 and np.isnan(out[0])
    out, m = R.quantile([nan, 3.0, nan, 1.0], [0.0, 0.5, 1.0])
    assert m == 2 and out.tolist() == [1.0, 2.0, 3.0]
    out, _ = R.quantile([0.0, -0.0, 0.0, -0.0], [0.0, 0.4, 1.0])  # -0 sorts before +0; equal values: v[lo]
    assert np.signbit(out).tolist() == [True, True, False]
    out, _ = R.quantile([-np.inf, 1.0, np.inf], [0.0, 0.25, 0.5, 1.0])
    assert out[0] == -np.inf and np.isnan(out[1]) and out[2] == 1.0 and out[3] == np.inf
    out, _ = R.quantile([np.inf, np.inf], [0.3])
    assert out[0] == np.inf
    out, m = R.rows_quantiles(np.array([[1.0, 2.0, 3.0], [nan, 5.0, nan]]), [0.5])
    assert out[:, 0].tolist() == [2.0, 5.0] and m.tolist() == [3, 1]


def test_key_orders_as_the_values_do():
    v = _special_values(np.random.default_rng(5), 5000)
    k = R.key(v)
    order = np.argsort(k, kind="stable")
    s = v[order]
    assert np.all(s[:-1] <= s[1:])
    # equal values with different keys are only the zeros, -0 first
    same = s[:-1] == s[1:]
    differ = k[order][:-1] != k[order][1:]
    both = same & differ
    assert np.all(s[:-1][both] == 0.0) and np.all(np.signbit(s[:-1][both])) and not np.any(np.signbit(s[1:][both]))
    np.testing.assert_array_equal(R.order_statistics(v), s)
    assert R.key([-0.0])[0] + 1 == R.key([0.0])[0]


def test_cov_against_numpy():
    rng = np.random.default_rng(9)
    n, P, W = 40, 4, 33
    mix = rng.standard_normal((P, P))
    x = np.einsum("pq,tqw->tpw", mix, rng.standard_normal((n + 3, P, W))) + np.arange(P)[None, :, None]
    c = x[2:n + 2]
    center = c.transpose(1, 0, 2).reshape(P, -1).mean(1)
    got, bound = R.cov(x, 2, n + 2, center, with_bound=True)
    want = np.cov(c.transpose(1, 0, 2).reshape(P, -1))
    np.testing.assert_allclose(got.astype(np.float64), want, rtol=1e-12)
    assert np.all(bound > 0) and np.all(bound < 1e-12 * np.abs(np.diag(want)).max())
    assert np.isnan(R.cov(x[:1, :, :1], 0, 1, x[0, :, 0])).all()


def test_draw_restatement():
    c = np.arange(7 * 2 * 5, dtype=np.float64).reshape(7, 2, 5)
    draws = np.array([[0.0, 0.5, 1.0, 0.999], [1.0, 0.0, 0.5, 0.2]])
    X, idx = R.draw(c, 3, 7, 4, draws=draws)
    assert idx.tolist() == [3 * 5 + 4, 5 * 5 + 0, 6 * 5 + 2, 6 * 5 + 1]
    np.testing.assert_array_equal(X, c.reshape(7, 2, 5).transpose(1, 0, 2).reshape(2, -1)[:, idx])
    t, w = R.draw_indices(37, 65, 3, 300, seed=4, draw_id=2)
    assert t.min() >= 3 and t.max() < 40 and w.min() >= 0 and w.max() < 65 and len(set(zip(t, w))) > 250
    t2, _ = R.draw_indices(37, 65, 3, 300, seed=4, draw_id=3)
    assert np.any(t != t2)


# ---- argument errors: < 0 before any HIP call, the argument named ---------------------------------------

def _q(*v):
    return (C.c_double * len(v))(*v)


def test_rows_quantiles_argument_errors():
    lib = _lib.load()
    d = 8  # (never dereferenced: every call below fails its checks first)
    names = ("x", "n_rows", "row_stride", "n_outer", "outer_stride", "n_inner", "q", "n_q", "out", "n_valid_out",
             "workspace", "stream")
    base = dict(x=d, n_rows=2, row_stride=10, n_outer=1, outer_stride=10, n_inner=10, q=_q(0.5), n_q=1, out=d,
                n_valid_out=0, workspace=d, stream=0)
    call = lambda **k: lib.rvm_rows_quantiles(*[{**base, **k}[a] for a in names])  # noqa: E731
    assert b"null x" in _err(call(x=0))
    assert b"n_rows" in _err(call(n_rows=0))
    assert b"n_rows" in _err(call(n_rows=65536))
    assert b"row_stride" in _err(call(row_stride=-1))
    assert b"n_outer" in _err(call(n_outer=0))
    assert b"outer_stride" in _err(call(outer_stride=-1))
    assert b"n_inner" in _err(call(n_inner=0))
    assert b"n_outer * n_inner" in _err(call(n_outer=1 << 16, n_inner=1 << 16))  # 2^32: one too many
    assert b"null q" in _err(call(q=None))
    assert b"n_q" in _err(call(n_q=0))
    assert b"n_q" in _err(call(q=_q(*[0.5] * 17), n_q=17))
    assert b"q must" in _err(call(q=_q(0.5, 1.5), n_q=2))
    assert b"q must" in _err(call(q=_q(-1e-9), n_q=1))
    assert b"q must" in _err(call(q=_q(float("nan")), n_q=1))
    assert b"null out" in _err(call(out=0))
    assert b"null workspace" in _err(call(workspace=0))
    assert b"aligned" in _err(call(workspace=12))
    wsb = lib.rvm_rows_quantiles_workspace_bytes
    assert wsb(1, 1) > 0 and wsb(3, 16) == 3 * wsb(1, 16) and wsb(1, 16) > wsb(1, 1) >= 2 * 256 * 4
    assert wsb(0, 1) == 0 and wsb(1, 0) == 0 and wsb(1, 17) == 0 and wsb(65536, 1) == 0


def test_chain_cov_argument_errors():
    lib = _lib.load()
    d = 8
    cov = lambda *a: lib.rvm_chain_cov(*a, 0)  # noqa: E731
    assert b"null chain" in _err(cov(0, 2, 4, 0, 5, d, d, d))
    assert b"n_params" in _err(cov(d, 0, 4, 0, 5, d, d, d))
    assert b"n_params" in _err(cov(d, 16385, 4, 0, 5, d, d, d))
    assert b"n_cols" in _err(cov(d, 2, 0, 0, 5, d, d, d))
    assert b"t0" in _err(cov(d, 2, 4, -1, 5, d, d, d))
    assert b"t1" in _err(cov(d, 2, 4, 5, 5, d, d, d))
    assert b"t1" in _err(cov(d, 2, 4, 5, 4, d, d, d))
    assert b"null center" in _err(cov(d, 2, 4, 0, 5, 0, d, d))
    assert b"null cov_out" in _err(cov(d, 2, 4, 0, 5, d, 0, d))
    assert b"null workspace" in _err(cov(d, 2, 4, 0, 5, d, d, 0))
    wsb = lib.rvm_chain_cov_workspace_bytes
    assert wsb(10, 200) == 8 * 100 * 200 and wsb(3, 257) == 8 * 9 * 257 and wsb(1, 1) == 8
    assert wsb(0, 4) == 0 and wsb(2, 0) == 0 and wsb(16385, 4) == 0 and wsb(2, 65535 * 64 + 1) == 0


def test_chain_draw_argument_errors():
    lib = _lib.load()
    d = 8
    draw = lambda *a: lib.rvm_chain_draw(*a, 0)  # noqa: E731
    assert b"null chain" in _err(draw(0, 2, 4, 0, 5, 3, 0, 0, 0, d, d))
    assert b"n_params" in _err(draw(d, 0, 4, 0, 5, 3, 0, 0, 0, d, d))
    assert b"n_cols" in _err(draw(d, 2, 0, 0, 5, 3, 0, 0, 0, d, d))
    assert b"t0" in _err(draw(d, 2, 4, -1, 5, 3, 0, 0, 0, d, d))
    assert b"t1" in _err(draw(d, 2, 4, 5, 5, 3, 0, 0, 0, d, d))
    assert b"n_samples" in _err(draw(d, 2, 4, 0, 5, 0, 0, 0, 0, d, d))
    assert b"null x_out" in _err(draw(d, 2, 4, 0, 5, 3, 0, 0, 0, 0, d))


def test_python_entry_points_exist():
    from rvmcmc import chain

    for name in ("summary", "draw", "predict"):
        assert callable(getattr(chain.ChainRecorder, name))
    assert chain.DEFAULT_Q == (0.025, 0.16, 0.5, 0.84, 0.975)
    with pytest.raises(ValueError):
        chain._q_array([])
    with pytest.raises(ValueError):
        chain._q_array([0.5] * 17)
    with pytest.raises(ValueError):
        chain._q_array([1.5])
