"""Parallel tempering on the device (rvmcmc/tempering.py, rvm_tempering.hip) against the numpy
restatement tests/pt_ref.py with injected uniforms, against the existing ensemble sampler at one
temperature, and against tests/philox_ref.py for the device's own draws.

Bit-exact tests use the fixed-step plan (resolve_tol = 0), whose T1 twin is the oracle's
logl_whx_batch.  tests/test_tempering_cpu.py runs the full-step input through the restatement with
the oracle alone and asserts that no decision is near a tie: the comparisons here have no exemptions.
"""
import numpy as np
import pytest

import oracle as O
import philox_ref
import pt_ref
from support import s2_state_and_obs as _state_and_obs, state_scales as _scales, tight_ball, torch_or_fail as _torch

pytestmark = pytest.mark.gpu


# ---- 1. the swap kernel alone ---------------------------------------------------------------------

def _swap_device(dim, T, W, betas, pos, lnp, u, swapped0, seed=0, iteration=0):
    """rvm_pt_swap on host arrays pos [T][W][dim], lnp [T][W] -> (rc, pos, lnp, swapped)."""
    torch = _torch()
    from rvmcmc import _lib

    lib = _lib.load()
    Wh = W // 2
    dev = lambda a: torch.as_tensor(np.ascontiguousarray(a), device="cuda")  # noqa: E731
    x = [dev(pos[:, h * Wh:(h + 1) * Wh].reshape(T * Wh, dim).T) for h in (0, 1)]
    l = [dev(lnp[:, h * Wh:(h + 1) * Wh].reshape(T * Wh)) for h in (0, 1)]
    b, du, sw = dev(np.asarray(betas, dtype=np.float64)), dev(u), dev(swapped0.astype(np.int32))
    rc = lib.rvm_pt_swap(dim, T, Wh, b.data_ptr(), x[0].data_ptr(), x[1].data_ptr(), l[0].data_ptr(), l[1].data_ptr(),
                         seed, iteration, du.data_ptr() if u is not None and u.size else 0, sw.data_ptr(),
                         _lib.stream_handle())
    torch.cuda.synchronize()
    P = np.concatenate([xx.t().cpu().numpy().reshape(T, Wh, dim) for xx in x], 1)
    L = np.concatenate([ll.cpu().numpy().reshape(T, Wh) for ll in l], 1)
    return rc, P, L, sw.cpu().numpy()


@pytest.mark.parametrize("dim,T,W", [(1, 2, 2), (10, 3, 24), (15, 5, 516)])
def test_swap_kernel_matches_numpy_sweep(dim, T, W):
    rng = np.random.default_rng(100 * T + W)
    pos = rng.standard_normal((T, W, dim))
    lnp = -3.0 * rng.random((T, W))
    betas = np.sort(rng.uniform(0.05, 1.0, T))[::-1].copy()
    assert np.all(np.diff(betas) < 0)
    u = rng.random((T - 1, W))
    start = rng.integers(0, 5, (T - 1, W))  # the counters start non-zero: the kernel adds to them
    rp, rl = pos.copy(), lnp.copy()
    swapped, margin = pt_ref.swap(rp, rl, betas, u)
    assert (margin >= 1e-9).all()  # no pair near a tie: nothing is exempt below
    rc, P, L, sw = _swap_device(dim, T, W, betas, pos, lnp, u, start)
    assert rc == 0
    np.testing.assert_array_equal(P, rp)
    np.testing.assert_array_equal(L, rl)
    np.testing.assert_array_equal(sw, start + swapped)
    if W > 2:
        assert swapped.any() and not swapped.all()
    # the same walkers, permuted within each walker index
    np.testing.assert_array_equal(np.sort(L, axis=0), np.sort(lnp, axis=0))


def test_swap_kernel_equal_betas_always_swap_and_one_temperature_is_a_noop():
    rng = np.random.default_rng(7)
    dim, W = 4, 12
    pos, lnp, u = rng.standard_normal((2, W, dim)), -rng.random((2, W)), rng.random((1, W))
    rc, P, L, sw = _swap_device(dim, 2, W, [1.0, 1.0], pos, lnp, u, np.zeros((1, W)))  # d = 0 > ln u
    assert rc == 0
    np.testing.assert_array_equal(P, pos[::-1])
    np.testing.assert_array_equal(L, lnp[::-1])
    np.testing.assert_array_equal(sw, np.ones((1, W), dtype=np.int32))
    rc, P, L, sw = _swap_device(dim, 1, W, [1.0], pos[:1], lnp[:1], np.zeros((0, W)), np.zeros((0, W)))
    assert rc == 0 and sw.shape == (0, W)
    np.testing.assert_array_equal(P, pos[:1])
    np.testing.assert_array_equal(L, lnp[:1])


# ---- 2. full steps against the restatement with injected draws --------------------------------------

def test_full_steps_match_numpy():
    """S2, T = 3, W = 24, rng 0, three iterations with a sweep after each: after every half-step and
    every sweep the device's positions equal the restatement's exactly (the restatement takes the
    device's log-probabilities, T1-equal to the oracle's; the CPU test shows the smallest decision
    margin of this input is 1.5e-2).  No exemptions."""
    from rvmcmc.tempering import PTSampler

    s, obs = _state_and_obs(fixed_step=True)
    T, W, iters = 3, 24, 3
    Wh = W // 2
    X, draws = pt_ref.case_inputs(s.get_params(), _scales(s), T, W, iters, seed=0)
    pt = PTSampler(T, W, s, obs, seed=1, swap_every=1)
    pt.set_positions(X)
    pt.compute_lnprob()
    np.testing.assert_array_equal(pt.positions(), X)
    pm = s.param_map()
    P = np.stack([O.kernel_params_to_oracle(pm.vector_to_kernel_np(x)[:, None], 2)[0] for x in X.reshape(-1, s.Nvars)])
    ref0, st0 = O.logl_whx_batch(P, 2, obs, pt.plan.dt, s.integrator.mult)
    assert (st0 == 0).all()
    t1 = 1e-11 * float(np.abs(O.richardson_weights(s.integrator.mult)).sum())
    np.testing.assert_allclose(pt.lnprob().reshape(-1), ref0, rtol=t1, atol=0)
    lad = pt_ref.Ladder(X, pt.betas, lambda Q: (np.zeros(len(Q)), np.zeros(len(Q), dtype=int)))
    lad.lnp = pt.lnprob()
    nacc = np.zeros((T, W), dtype=int)
    nsw = np.zeros((T - 1, W), dtype=int)
    for it, d in enumerate(draws):
        assert pt.iteration == it
        for h in (0, 1):
            pt.half_step(h, np.stack([d["u1"][h].reshape(-1), d["u2"][h].reshape(-1)]), d["u3"][h])
            lnp_new = pt._lnp_new.cpu().numpy().reshape(T, Wh)
            assert np.isfinite(lnp_new).all() and (pt._status.cpu().numpy() == 0).all()
            q, acc = lad.half_step(h, d["u1"][h], d["u2"][h], d["u3"][h], lnp_new=lnp_new)
            np.testing.assert_array_equal(pt._q.t().cpu().numpy().reshape(T, Wh, -1), q)
            np.testing.assert_array_equal(pt.positions(), lad.pos, err_msg=f"iteration {it} half {h}")
            np.testing.assert_array_equal(pt.lnprob(), lad.lnp)
            nacc[:, h * Wh:(h + 1) * Wh] += acc
        pt.swap(d["swap"])
        nsw += lad.swap(d["swap"])
        np.testing.assert_array_equal(pt.positions(), lad.pos, err_msg=f"iteration {it} sweep")
        np.testing.assert_array_equal(pt.lnprob(), lad.lnp)
        pt.iteration += 1
    assert lad.accept_margin >= 1e-6 and lad.swap_margin >= 1e-6
    assert lad.n_tempered_differs >= 10
    np.testing.assert_array_equal(pt.acceptance_fraction(), nacc / iters)
    np.testing.assert_array_equal(pt.swap_fraction(), nsw.sum(1) / (iters * W))
    assert ((nsw.sum(1) > 0) & (nsw.sum(1) < iters * W)).all()
    # step(draws=...) is the same iteration: replay the first one from the start
    pt2 = PTSampler(T, W, s, obs, seed=1)
    pt2.set_positions(X)
    pt2.step(draws=draws[0])
    pt3 = PTSampler(T, W, s, obs, seed=1)
    pt3.set_positions(X)
    pt3.compute_lnprob()
    for h in (0, 1):
        pt3.half_step(h, np.stack([draws[0]["u1"][h].reshape(-1), draws[0]["u2"][h].reshape(-1)]), draws[0]["u3"][h])
    pt3.swap(draws[0]["swap"])
    np.testing.assert_array_equal(pt2.positions(), pt3.positions())
    np.testing.assert_array_equal(pt2.lnprob(), pt3.lnprob())
    assert pt2.iteration == 1 and pt2.nevals == 2 * T * W


# ---- 3. one temperature is the existing sampler ---------------------------------------------------

def test_one_temperature_is_the_ensemble_sampler():
    torch = _torch()
    from rvmcmc.ensemble import EnsembleSampler
    from rvmcmc.tempering import PTSampler

    s, obs = _state_and_obs(fixed_step=True)
    W = 64
    rng = np.random.default_rng(4)
    X0 = tight_ball(s, (W,), rng, 1e-2)
    ens = EnsembleSampler(W, s, obs, seed=7)
    ens.fused = False
    ens.set_positions(X0)
    pt = PTSampler(1, W, s, obs, seed=7)
    np.testing.assert_array_equal(pt.betas, [1.0])
    pt.set_positions(X0[None])
    for _ in range(5):
        ens.step()
        pt.step()
    torch.cuda.synchronize()
    np.testing.assert_array_equal(pt.positions()[0], ens.gather_positions())
    np.testing.assert_array_equal(pt.lnprob()[0], ens.gather_lnprob())
    np.testing.assert_array_equal(pt.naccepted.reshape(-1).cpu().numpy(), ens.naccepted.cpu().numpy())
    acc = ens.naccepted.cpu().numpy().sum() / (5 * W)
    assert 0.0 < acc < 1.0
    assert pt.swap_fraction().shape == (0,)


# ---- 4. the device's Philox draws -----------------------------------------------------------------

def test_device_philox_matches_injected_draws():
    from rvmcmc.tempering import PTSampler

    s, obs = _state_and_obs(fixed_step=True)
    T, W, seed, it = 3, 24, 987654321987, 5
    X, _ = pt_ref.case_inputs(s.get_params(), _scales(s), T, W, 0, seed=2)
    d = dict(u1=[], u2=[], u3=[])
    for h in (0, 1):
        g = pt_ref.items(T, W, h).reshape(-1)
        u1, u2 = philox_ref.uniform2_vec(seed, g, it, philox_ref.RNG_STRETCH_PROPOSE | (h << 8))
        u3, _ = philox_ref.uniform2_vec(seed, g, it, philox_ref.RNG_STRETCH_ACCEPT | (h << 8))
        for k, v in (("u1", u1), ("u2", u2), ("u3", u3)):
            d[k].append(v.reshape(T, W // 2))
    d = {k: np.stack(v) for k, v in d.items()}
    d["swap"] = philox_ref.uniform2_vec(seed, pt_ref.swap_items(T, W).reshape(-1), it,
                                        pt_ref.RNG_PT_SWAP)[0].reshape(T - 1, W)
    runs = []
    for draws in (None, d):
        pt = PTSampler(T, W, s, obs, seed=seed)
        pt.set_positions(X)
        pt.compute_lnprob()
        pt.iteration = it
        pt.step(draws=draws)
        runs.append((pt.positions(), pt.lnprob(), pt.naccepted.cpu().numpy(), pt.nswapped.cpu().numpy()))
    for a, b in zip(*runs):
        np.testing.assert_array_equal(a, b)
    assert (runs[0][0] != X).any() and 0 < runs[0][3].sum() < (T - 1) * W


# ---- 5. bookkeeping and reproducibility with the default (adaptive) integrator --------------------

def test_bookkeeping_reproducibility_and_checkpoint(tmp_path):
    torch = _torch()
    from rvmcmc.tempering import PTSampler

    s, obs = _state_and_obs(fixed_step=False)
    T, W, iters = 4, 32, 10
    X, _ = pt_ref.case_inputs(s.get_params(), _scales(s), T, W, 0, seed=6)

    def run(n, pt=None):
        if pt is None:
            pt = PTSampler(T, W, s, obs, seed=11)
            pt.set_positions(X)
        for _ in range(n):
            pt.step()
        return pt

    a, b = run(iters), run(iters)
    for f in ("positions", "lnprob", "acceptance_fraction", "swap_fraction"):
        np.testing.assert_array_equal(getattr(a, f)(), getattr(b, f)())
    lnp = a.lnprob()
    assert lnp.shape == (T, W) and np.isfinite(lnp).all()
    assert a.iteration == iters and a.nevals == (iters + 1) * T * W
    # the stored lnp belongs to the stored positions, through every accept and exchange
    t1 = 1e-11 * float(np.abs(O.richardson_weights(s.integrator.mult)).sum())
    for h in (0, 1):
        again = a.plan.logl(a.pmap.to_kernel(a.pos[h]), hill_factor=a.hill_factor)[0]
        torch.cuda.synchronize()
        np.testing.assert_allclose(a.lnp[h].cpu().numpy(), again.cpu().numpy(), rtol=t1, atol=0)
    acc = a.acceptance_fraction()
    assert acc.shape == (T, W)
    assert ((acc.mean(1) > 0) & (acc.mean(1) < 1)).all()
    assert a.swap_fraction().shape == (T - 1,) and (a.swap_fraction() <= 1).all()
    f = a.check_faults()
    assert f["handoff_timeouts"] == 0 and f["nonfinite"] == 0 and f["unresolved"] == 0
    # checkpoint after 5 iterations, restore into a fresh sampler, 5 more == 10 uninterrupted
    c = run(5)
    c.checkpoint(tmp_path / "pt.npz")
    r = PTSampler(T, W, s, obs, seed=999)
    r.restore(tmp_path / "pt.npz")
    assert r.iteration == 5 and r.seed == 11
    run(5, r)
    for f in ("positions", "lnprob", "acceptance_fraction", "swap_fraction"):
        np.testing.assert_array_equal(getattr(r, f)(), getattr(a, f)())
    assert r.nevals == a.nevals
