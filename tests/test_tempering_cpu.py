"""Parallel tempering, the parts that need no GPU: the default ladder, the constructor's value
checks, the entry points' argument checks, and the numpy restatement (tests/pt_ref.py) run with the
oracle as the likelihood on the input tests/test_gpu_tempering.py compares the device against."""
import ctypes as C
import math

import numpy as np
import pytest

import pt_ref
from conftest import S2_PLANETS, s2_obs_oracle
from support import oracle_logl_fn as _oracle_fn, s2_state_and_obs, state_scales

from rvmcmc import _lib, state
from rvmcmc.tempering import PTSampler, default_betas


def test_default_betas_geometric():
    for T, dim in ((1, 10), (2, 10), (8, 10), (5, 15), (4, 1)):
        b = default_betas(T, dim)
        assert b.dtype == np.float64 and b.shape == (T,)
        assert b[0] == 1.0
        r = 1.0 + 2.0 * math.sqrt(math.log(4.0)) / math.sqrt(dim)
        np.testing.assert_allclose(b[:-1] / b[1:], r, rtol=1e-14)
        assert np.all(np.diff(b) < 0) and np.all(b > 0)
    np.testing.assert_array_equal(default_betas(1, 10), [1.0])


def test_constructor_refuses_bad_values_before_any_device_use():
    s = state.State(planets=[dict(p) for p in S2_PLANETS])
    obs = s2_obs_oracle()
    dim = s.Nvars
    assert dim == 10
    with pytest.raises(ValueError, match="even"):
        PTSampler(2, 21, s, obs)
    with pytest.raises(ValueError, match="twice the dimension"):
        PTSampler(2, 2 * dim - 2, s, obs)
    with pytest.raises(ValueError, match="strictly decreasing"):
        PTSampler(3, 24, s, obs, betas=[1.0, 0.5, 0.5])
    with pytest.raises(ValueError, match="strictly decreasing"):
        PTSampler(3, 24, s, obs, betas=[0.25, 0.5, 1.0])
    with pytest.raises(ValueError, match="> 0"):
        PTSampler(3, 24, s, obs, betas=[1.0, 0.5, 0.0])
    with pytest.raises(ValueError, match="> 0"):
        PTSampler(2, 24, s, obs, betas=[1.0, -0.5])
    with pytest.raises(ValueError, match="<= 1"):
        PTSampler(2, 24, s, obs, betas=[1.5, 0.5])
    with pytest.raises(ValueError, match="ntemps"):
        PTSampler(3, 24, s, obs, betas=[1.0, 0.5])
    assert "_rvm_plans" not in obs.__dict__  # no plan was asked for: nothing reached the device


def test_entry_points_refuse_bad_arguments_without_a_device():
    lib = _lib.load()
    one = (C.c_double * 4)(0.5, 0.5, 0.5, 0.5)
    ione = (C.c_int32 * 4)(0, 0, 0, 0)
    p = C.cast(one, C.c_void_p)
    ip = C.cast(ione, C.c_void_p)

    def propose(n_params=10, n_temps=2, n_half=1, x=p, c=p, a=2.0, half=0, q=p, z=p):
        return lib.rvm_pt_stretch_propose(n_params, n_temps, n_half, x, c, a, 0, 0, half, None, q, z, None)

    def accept(n_params=10, n_temps=2, n_half=1, betas=p, x=p, lnp=p, q=p, lnp_new=p, z=p, half=0):
        return lib.rvm_pt_stretch_accept(n_params, n_temps, n_half, betas, x, lnp, q, lnp_new, z, 0, 0, half, None,
                                         ip, None)

    def swap(n_params=10, n_temps=2, n_half=1, betas=p, x0=p, x1=p, lnp0=p, lnp1=p, swapped=ip):
        return lib.rvm_pt_swap(n_params, n_temps, n_half, betas, x0, x1, lnp0, lnp1, 0, 0, None, swapped, None)

    def refused(rc, word):
        msg = lib.rvm_last_error()
        assert rc < 0 and word in msg, (rc, msg)

    for name, fn in ((b"rvm_pt_stretch_propose", propose), (b"rvm_pt_stretch_accept", accept),
                     (b"rvm_pt_swap", swap)):
        refused(fn(n_temps=0), b"n_temps")
        assert name in lib.rvm_last_error()
        refused(fn(n_half=0), b"n_half")
        refused(fn(n_params=0), b"n_params")
        refused(fn(n_temps=1 << 16, n_half=1 << 16), b"int32")
    refused(propose(half=2), b"half")
    refused(accept(half=2), b"half")
    refused(propose(a=1.0), b"a must be > 1")
    refused(accept(betas=None), b"betas")
    refused(swap(betas=None), b"betas")
    refused(propose(x=None), b"null")
    refused(propose(z=None), b"null")
    refused(accept(lnp_new=None), b"null")
    refused(swap(x1=None), b"null")
    refused(swap(swapped=None), b"null")
    # one temperature has nobody to exchange with: 0 without a launch, whatever the arrays
    assert lib.rvm_pt_swap(10, 1, 4, None, None, None, None, None, 0, 0, None, None, None) == 0


def test_restatement_is_self_consistent_on_the_gpu_tests_input():
    """The input of test_gpu_tempering.py::test_full_steps_match_numpy (S2, T = 3, W = 24, rng 0, 3
    iterations) through the restatement with the oracle (the fixed-step plan's T1 twin) as the
    likelihood: every walker evaluates cleanly, no decision is near a tie, tempering changes
    decisions, and every pair both exchanges and keeps walkers -- so the GPU comparison can fail on a
    wrong beta, a wrong pairing or a swap that forgets lnp, and needs no exemptions."""
    s, obs = s2_state_and_obs(fixed_step=True)
    T, W, iters = 3, 24, 3
    X, draws = pt_ref.case_inputs(s.get_params(), state_scales(s), T, W, iters, seed=0)
    dt = s.integrator.plan_args(s.planets)[0]
    betas = default_betas(T, s.Nvars)
    lad = pt_ref.Ladder(X, betas, _oracle_fn(s, obs, dt))
    assert (lad.status0 == 0).all() and np.isfinite(lad.lnp).all()
    # conservation: a sweep only permutes walkers within one walker index
    for d in draws:
        for h in (0, 1):
            lad.half_step(h, d["u1"][h], d["u2"][h], d["u3"][h])
        before = np.sort(lad.lnp, axis=0)
        lad.swap(d["swap"])
        np.testing.assert_array_equal(np.sort(lad.lnp, axis=0), before)
    st = np.stack(lad.statuses)
    assert st.size == 2 * iters * T * (W // 2) == 216 and (st == 0).all()
    # the stored lnp is the lnp of the stored positions (a swap moved both or neither)
    np.testing.assert_array_equal(lad._eval(lad.pos)[0], lad.lnp)
    print(f"accept margin {lad.accept_margin:.3g}, swap margin {lad.swap_margin:.3g}, "
          f"{lad.n_tempered_differs} decisions differ from beta = 1, "
          f"swap fractions {np.stack(lad.swaps).mean(axis=(0, 2))}")
    assert lad.accept_margin >= 1e-6 and lad.swap_margin >= 1e-6
    assert lad.n_tempered_differs >= 10
    sw = np.stack(lad.swaps)  # [iters][T-1][W]
    for p in range(T - 1):
        assert sw[:, p].any() and not sw[:, p].all()


def test_restatement_swap_edge_cases():
    rng = np.random.default_rng(3)
    pos, lnp = rng.standard_normal((2, 4, 3)), -rng.random((2, 4))
    p0, l0 = pos.copy(), lnp.copy()
    s, _ = pt_ref.swap(pos, lnp, np.array([1.0, 1.0]), rng.random((1, 4)))  # d = 0 > ln u: always
    assert s.all()
    np.testing.assert_array_equal(pos, p0[::-1])
    np.testing.assert_array_equal(lnp, l0[::-1])
    one = pt_ref.swap(p0[:1].copy(), l0[:1].copy(), np.array([1.0]), np.zeros((0, 4)))
    assert one[0].shape == (0, 4)
