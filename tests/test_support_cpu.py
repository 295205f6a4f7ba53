"""tests/support.py checked on its own, without a GPU: the switch manager, the layout conversions, the tight
ball, the ensemble loader, and that importing the module loads neither torch nor the library."""
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle as O
import support
from conftest import ROOT, S2_SCALES

A, B, C = "RVM_SUPPORT_TEST_A", "RVM_SUPPORT_TEST_B", "RVM_SUPPORT_TEST_C"  # (names nothing reads)


@pytest.fixture
def three_states():
    """A absent, B present, C present (the block below unsets it); whatever they were is put back."""
    old = {k: os.environ.get(k) for k in (A, B, C)}
    os.environ.pop(A, None)
    os.environ[B], os.environ[C] = "before", "kept"
    yield {A: None, B: "before", C: "kept"}
    for k, v in old.items():
        if v is None:
            os.environ.pop(k, None)
        else:
            os.environ[k] = v


def _seen():
    return {k: os.environ.get(k) for k in (A, B, C)}


def test_switches_set_override_unset_and_restore(three_states):
    with support.switches({A: "1", B: "2", C: None}):
        assert _seen() == {A: "1", B: "2", C: None}
        with support.switches({}):  # (nothing named: nothing touched)
            assert _seen() == {A: "1", B: "2", C: None}
        with support.switches({A: None, C: "3"}):  # (nested: the inner block restores the outer's values)
            assert _seen() == {A: None, B: "2", C: "3"}
        assert _seen() == {A: "1", B: "2", C: None}
    assert _seen() == three_states


def test_switches_restore_after_an_exception(three_states):
    with pytest.raises(KeyError, match="inside"):
        with support.switches({A: "1", B: "2", C: None}):
            assert _seen() == {A: "1", B: "2", C: None}
            raise KeyError("inside")
    assert _seen() == three_states


@pytest.mark.parametrize("inclined", [False, True])
@pytest.mark.parametrize("n", [1, 2, 3, 4])
def test_layout_round_trip(n, inclined):
    rows = 7 if inclined else 5
    X = np.random.default_rng(10 * n + inclined).standard_normal((6, rows * n))  # flat kernel-row vectors
    P = support.oracle_params(X, n, inclined)
    assert P.shape == (6, n, 7)
    np.testing.assert_array_equal(P[:, :, :rows].reshape(6, -1), X)
    np.testing.assert_array_equal(P[:, :, rows:], 0.0)  # unused columns
    K = support.kernel_rows(P, rows)
    assert K.shape == (rows * n, 6) and K.flags.c_contiguous
    np.testing.assert_array_equal(K, X.T)
    np.testing.assert_array_equal(support.oracle_params(K.T, n, inclined), P)
    if not inclined:
        np.testing.assert_array_equal(P, O.kernel_params_to_oracle(K, n))
    assert support.oracle_params(X[:0], n, inclined).shape == (0, n, 7)


def test_free_parameters_reach_the_oracle_through_the_param_map():
    """A State with fixed rows: the fixed values come from the map's base, the free ones from the vector."""
    s = support.s2_state(ignore_params=[["h"], ["k", "l"]])
    pm = s.param_map()
    X = support.tight_ball(s, (5,), 2)
    P = support.free_params_to_oracle(pm, X)
    want = np.stack([O.kernel_params_to_oracle(pm.vector_to_kernel_np(x)[:, None], 2)[0] for x in X])
    np.testing.assert_array_equal(P, want)
    assert support.free_params_to_oracle(pm, X[:0]).shape == (0, 2, 7)


def test_tight_ball_is_the_literal_expression():
    s = support.s2_state()
    sc = np.array([S2_SCALES[k] for k in s.get_rawkeys()])
    np.testing.assert_array_equal(support.state_scales(s), sc)
    want = s.get_params() + 1e-3 * sc * np.random.default_rng(13).standard_normal((3, 16) + (s.Nvars,))
    np.testing.assert_array_equal(support.tight_ball(s, (3, 16), 13), want)
    rng = np.random.default_rng(4)  # a Generator is drawn from, and goes on where the ball left it
    want = s.get_params()[None] + 1e-2 * sc * np.random.default_rng(4).standard_normal((8, s.Nvars))
    np.testing.assert_array_equal(support.tight_ball(s, (8,), rng, 1e-2), want)
    assert rng.random() != np.random.default_rng(4).random()


def test_steady_ensembles_load():
    assert support.steady_ensemble("3planet").shape == (512, 15)
    assert support.steady_ensemble("hd155358").shape == (512, 10)
    assert support.steady_ensemble("s2").shape == (4096, 10)
    with pytest.raises(KeyError):
        support.steady_ensemble("ens_it2000.npy")


def test_import_loads_neither_torch_nor_the_library():
    code = ("import sys; sys.path.insert(0, 'tests'); import support; "
            "print([m for m in ('torch', 'rvmcmc._lib') if m in sys.modules])")
    p = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr[-2000:]
    assert p.stdout.strip() == "[]"
