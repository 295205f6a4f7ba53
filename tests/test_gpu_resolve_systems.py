"""The adaptive resolution beyond two planar planets (tests/test_gpu_resolve.py holds it for <2, planar>).

The refinement, eager and hedge kernels and the likelihood kernel's extension paths are compiled once per
planet count (1..4) and once more for inclined orbits; 3 and 4 planets run 16 walkers per group (4 lanes per
walker), 3 planar planets have a layout of their own (paired one-group blocks) and inclined plans carry a 7-row
state through the t = 0 hand-off and the lane save / load.  Here five systems -- 3 and 4 planar planets, 2, 3 and
4 inclined ones -- go through the same checks as the 2-planet system:

  * T1 of the adaptive kernel against the oracle's restatement of the rule (oracle.logl_whx_adapt_batch) at one
    launch size per likelihood layout, with a cap on how many walkers the comparison may excuse as sensitive,
    and the passes taken by the walkers clear of every bound counted against the oracle's stages;
  * the eager halving passes and the refinement kernel's layouts give the same bits;
  * one fused stretch half-step (the certain-reject cut, and at this size the hedged pass) against the oracle
    with the restated Philox draws.
The layouts the sizes are meant to reach are pinned on the host by tests/test_logl_layout_host_cpu.py.
"""
import functools

import numpy as np
import pytest

import ias15_parity as IP
import oracle as O
from conftest import S2_PLANETS, S2_SCALES
from support import EXTRA_PLANETS, RMAX, T1_REL, TOL, adaptive_plan, assert_t1_adaptive, launch as _run, oracle_params
from support import switches, torch_or_fail as _torch

pytestmark = pytest.mark.gpu

# name -> (planets, inclined)
SYSTEMS = {"p3": (3, False), "p4": (4, False), "i2": (2, True), "i3": (3, True), "i4": (4, True)}
BALL = 0.3


def system_planets(name):
    n, inclined = SYSTEMS[name]
    planets = [dict(p) for p in (S2_PLANETS + EXTRA_PLANETS)[:n]]
    if inclined:  # (as tests/test_gpu_logl.py test_t1_inclined_planet_counts)
        planets = [dict(p, ix=0.03 * (i + 1), iy=-0.02 * i) for i, p in enumerate(planets)]
    return planets


@functools.lru_cache(maxsize=None)
def system_obs(name):
    np.random.seed(2017)
    return O.fake_obs(system_planets(name), Npoints=100, error=1.5e-4, errorVar=2.5e-5, tmax=120.)


def _keys(name):
    return ["m", "a", "h", "k", "l"] + (["ix", "iy"] if SYSTEMS[name][1] else [])


def system_walkers(name, W, ball=BALL, seed=3):
    """tests/test_gpu_resolve.py wide_walkers for any system: half a ball x0 + ball * scales * N(0,1) (S2_SCALES
    per planet, 0.05 for ix and iy), half stretch proposals between its members (q = c - z (c - x), z in
    [1/2, 2]): [W][rows] in the kernel's row order (m, a, h, k, l (, ix, iy) per planet), which is also the
    State's free-parameter order of system_planets."""
    planets, keys = system_planets(name), _keys(name)
    x0 = np.array([p[k] for p in planets for k in keys])
    sc = np.array([S2_SCALES.get(k, 0.05) for _ in planets for k in keys])
    rng = np.random.default_rng(seed)
    n = W // 2
    X = x0 + ball * sc * rng.standard_normal((n, len(x0)))
    j = rng.integers(0, n, W - n)
    z = (rng.random(W - n) + 1.0) ** 2 / 2.0
    Q = X[j] - z[:, None] * (X[j] - X[np.arange(W - n) % n])  # (an odd W: one member proposes twice)
    return np.concatenate([X, Q])


def oracle_P(name, X):
    return oracle_params(X, *SYSTEMS[name])


def _plan(name, W):
    return adaptive_plan(system_planets(name), system_obs(name), W, (TOL, RMAX), SYSTEMS[name][1])


def sensitive_cap(n):
    """What the comparison may excuse: an eighth of the checked walkers (4 of 24).  The oracle alone, on these
    inputs, calls at most 16 of 192 and 2 of 24 sensitive."""
    return 4 if n <= 24 else n // 8


def checked_subset(W):
    """The walkers the oracle sees: all of a small launch; of a large one the first 64 slots, 64 around the
    middle (the ball's last members and the first proposals) and the last 64."""
    if W <= 256:
        return np.arange(W)
    return np.r_[0:64, W // 2 - 32:W // 2 + 32, W - 64:W]


def _ias15_difference(name, got, st, P, sensitive):
    """Largest |dlogL| against IAS15 over the OK, non-sensitive walkers (reported, not asserted: T2 on refining
    walkers of these systems)."""
    n, inclined = SYSTEMS[name]
    sel = (st == 0) & ~sensitive
    ias, st_ias = IP.ias15_logl(P[sel], n, system_obs(name), 1.0, int(inclined))
    both = st_ias == 0
    return float(np.max(np.abs(got[sel][both] - ias[both]), initial=0.0)), int(both.sum())


# The launch sizes, one per likelihood layout (rvm_plan_host.cpp choose_logl_layout, 256 CUs; 16 walkers per group,
# 32 for i2), pinned by tests/test_logl_layout_host_cpu.py:
#   24    below RVM_CX_MIN_WALKERS and RVM_EAGER_MIN: the extension runs after the main pass, no eager kernel
#   256   one group per block with the concurrent extension wave (cx), and the eager kernel
#   2304  144 groups of 16, more than one per two CUs: p4, i3 and i4 take the level-split layout with the extension
#         as a fifth level (lsx, 144 + 36 blocks); p3, which never takes lsx, the level-split layout of four levels
#         (144 + 48 blocks) with the extension after the main pass
#   3265  p3: 205 groups, the last with one walker, is the smallest launch the level-split layout does not fit
#         (205 + 52 blocks > 256 CUs): the paired one-group blocks with the extension wave (cx, two blocks per CU)
#   4097  i2 (72 groups of 32 at 2304 would stay cx): 129 groups, the last with one walker, is the smallest crowded
#         launch, and takes lsx (129 + 33 blocks)
# Measured on an MI355X over all 16 cases: largest error 0.24 T1_REL (p3 2304; elsewhere <= 0.06), sensitive 0-3 of
# 24, 9-17 of 256 and 5-10 of 192 (the oracle alone decides these), largest |dlogL| against IAS15 over the OK,
# non-sensitive walkers 8.4e-7 (i4 256; elsewhere <= 3.1e-7) -- within the 1e-6 the project promises.
T1_CASES = [(name, W) for name in SYSTEMS for W in (24, 256, 4097 if name == "i2" else 2304)] + [("p3", 3265)]


@pytest.mark.parametrize("name,W", T1_CASES, ids=[f"{n}-{w}" for n, w in T1_CASES])
def test_t1_adaptive_systems(name, W):
    n_planets, inclined = SYSTEMS[name]
    obs = system_obs(name)
    plan, dt, mult = _plan(name, W)
    assert plan.ext_mult == O.ext_multiplier(mult, RMAX) == max(mult) + 1
    X = system_walkers(name, W)
    got, st = _run(plan, X)
    f = plan.faults(reset=True)
    idx = checked_subset(W)
    n = len(idx)
    P = oracle_P(name, X[idx])
    rf, sensitive = assert_t1_adaptive(got[idx], st[idx], P, n_planets, obs, dt, mult, has_inc=int(inclined))
    ref, st_ref = O.logl_whx_adapt_batch(P, n_planets, obs, dt, mult, TOL, RMAX, has_inc=int(inclined))[:2]
    ok = (st[idx] == 0) & (st_ref == 0) & ~sensitive
    err = np.abs(got[idx][ok] - ref[ok]) / np.maximum(1.0, np.abs(ref[ok]))
    d_ias, n_ias = _ias15_difference(name, got[idx], st[idx], P, sensitive)
    print(f"{name} W={W} checked {n}: oracle walker-directions at the extension {int((rf == 1).sum())}, halved "
          f"{int((rf >= 2).sum())}, deepest stage {int(rf.max())}; kernel counters {f}, statuses "
          f"{np.bincount(st[idx], minlength=5).tolist()}, sensitive {int(sensitive.sum())}, max err / T1_REL "
          f"{err.max(initial=0.0) / T1_REL:.3f}, max |dlogL| vs IAS15 {d_ias:.3e} over {n_ias}")
    assert (rf == 1).sum() >= max(1, n // 20) and (rf >= 2).sum() >= max(1, n // 20), \
        "the wide ball must exercise both stages"
    assert sensitive.sum() <= sensitive_cap(n)
    assert f["refined"] > 0 and f["handoff_timeouts"] == 0 and f["nonfinite"] == 0
    assert f["unresolved"] == int((st == 4).sum())
    if W <= 256:
        # The stages themselves.  logL cannot see a direction that settled a stage early or late while within the
        # tolerance; the plan's `refined` counts one per walker-direction and pass (the extension and every
        # halving, include/rvmcmc.h), which is the oracle's stage.  Every decision of an OK walker the oracle does
        # not call sensitive is clear of its bound by far more than roundoff, so a launch of those walkers alone
        # counts exactly the oracle's stages -- and gives each the bits it had in the full launch.
        clean = (st[idx] == 0) & (st_ref == 0) & ~sensitive
        plan2, _, _ = _plan(name, W)
        got2, st2 = _run(plan2, X[idx][clean])
        f2 = plan2.faults(reset=True)
        print(f"{name} W={W}: {int(clean.sum())} clean walkers alone: refined {f2['refined']}, oracle stages "
              f"{int(rf[clean].sum())}")
        np.testing.assert_array_equal(st2, 0)
        np.testing.assert_array_equal(got2, got[idx][clean])
        assert f2["refined"] == int(rf[clean].sum())


def _fresh_launch(name, W, X, env):
    with switches(env):
        plan, _, _ = _plan(name, W)
        got, st = _run(plan, X)
        return got, st, plan.faults(reset=True)


@pytest.mark.parametrize("passes", ["1", "2"])
@pytest.mark.parametrize("name", ["p3", "i2", "i4"])
def test_eager_halving_passes_bit_identical_systems(name, passes):
    """tests/test_gpu_resolve.py test_eager_halving_passes_bit_identical per system: the eager kernel's passes
    replayed by the refinement kernel give the logL, status bits and plan counters of the refinement kernel
    integrating them itself (RVM_EAGER=0)."""
    W = 256
    X = system_walkers(name, W)
    res = [_fresh_launch(name, W, X, {"RVM_EAGER": e, "RVM_EAGER_PASSES": passes}) for e in ("1", "0")]
    np.testing.assert_array_equal(res[0][1], res[1][1])
    np.testing.assert_array_equal(res[0][0], res[1][0])
    assert res[0][2] == res[1][2], (res[0][2], res[1][2])
    assert res[0][2]["refined"] > 0


@pytest.mark.parametrize("name", ["p3", "i2", "i4"])
def test_refinement_layouts_bit_identical_plain_launch(name):
    """The plain-launch counterpart of tests/test_gpu_resolve.py test_refinement_layouts_bit_identical: the
    refinement kernel's team counts, one workgroup per direction or per walker group, and eight waves per
    workgroup instead of four take the same decisions with the same bits on one wide-ball launch."""
    W = 256
    X = system_walkers(name, W)
    envs = [{}, {"RVM_REFINE_TEAMS": "2"}, {"RVM_REFINE_TEAMS": "4"}, {"RVM_REFINE_TEAMS": "0"},
            {"RVM_REFINE_SPLIT": "0"}, {"RVM_REFINE_W4": "0"}]
    runs = [_fresh_launch(name, W, X, env) for env in envs]
    assert runs[0][2]["refined"] > 0 and runs[0][2]["handoff_timeouts"] == 0
    for env, (got, st, f) in zip(envs[1:], runs[1:]):
        np.testing.assert_array_equal(st, runs[0][1], err_msg=str(env))
        np.testing.assert_array_equal(got, runs[0][0], err_msg=str(env))
        assert f == runs[0][2], (env, f, runs[0][2])


# (ball, walker seed, sampler seed) of the fused half-step below.  The oracle alone (its own logL of the current
# positions as lnp0, the restated draws) cuts 62 (p3) and 53 (i4) walker-directions of the 256 proposals, and
# calls 11 and 8 proposals sensitive; with walker seeds 14 and 15 it cuts 55, 60 (p3) and 42, 41 (i4).
CUT_INPUTS = {"p3": (BALL, 13, 5), "i4": (BALL, 13, 5)}


@pytest.mark.parametrize("name", ["p3", "i4"])
def test_certain_reject_cut_matches_oracle_systems(name):
    """tests/test_gpu_resolve.py test_certain_reject_cut_matches_oracle per system, on 512 walkers: a fused
    stretch half-step of 256 proposals leaves CUs idle, so the hedged pass of the instantiation runs beside
    the refinement.  Every proposal's logL and status follow the oracle with the same accept inputs, the
    decisions are the emcee test on those values, and no accepted proposal is cut."""
    torch = _torch()
    from philox_ref import stretch_uniforms
    from rvmcmc.ensemble import EnsembleSampler
    from rvmcmc.state import State

    n_planets, inclined = SYSTEMS[name]
    W = 512
    ball, wseed, sseed = CUT_INPUTS[name]
    s = State(planets=system_planets(name))
    assert s.Nvars == n_planets * (7 if inclined else 5)
    obs = system_obs(name)
    X0 = system_walkers(name, W, ball=ball, seed=wseed)
    ens = EnsembleSampler(W, s, obs, seed=sseed)
    ens.set_positions(X0)
    ens.compute_lnprob()
    n, it = ens.nloc, ens.iteration
    before = ens.pos[0].t().cpu().numpy().copy()
    c = ens.pos[1].t().cpu().numpy().copy()
    lnp0 = ens.lnp[0].cpu().numpy().copy()
    ens.plan.faults(reset=True)
    ens.plan.hedge_stats(reset=True)
    ens.half_step(ens.pos[0], ens.lnp[0], ens.pos[1], 0)
    torch.cuda.synchronize()
    f = ens.plan.faults(reset=True)
    hedge = ens.plan.hedge_stats(reset=True)
    got, st = ens._lnp_new.cpu().numpy(), ens._status.cpu().numpy()
    after = ens.pos[0].t().cpu().numpy()
    u1, u2, u3 = stretch_uniforms(ens.seed, ens.global_begin(0), n, it, 0)
    q, z = IP.stretch_proposal(before, c, u1, u2, ens.a)
    plan = ens.plan
    ctx = dict(mode=np.ones(n, dtype=np.int32), dim=s.Nvars, z=z, u=u3, lnp0=lnp0)
    assert plan.ecc_guard > 0.0 and plan.inclined == inclined
    rf, sensitive, cut = assert_t1_adaptive(got, st, IP.to_oracle(s.param_map(), q), n_planets, obs, plan.dt,
                                            plan.mult, plan.resolve_tol, plan.resolve_max, has_inc=int(inclined),
                                            ctx=ctx, ecc_guard=plan.ecc_guard)
    ncut = int(cut.sum())
    print(f"{name} W={W}: directions extended {int((rf == 1).sum())}, halved {int((rf >= 2).sum())}, cut {ncut} "
          f"(oracle), sensitive {int(sensitive.sum())}; kernel {f}, hedge {hedge}")
    assert 0 < hedge["hedged"] <= n  # (the hedge kernel of this instantiation ran: tests/test_gpu_hedge.py)
    assert ncut >= 8 and abs(f["truncated"] - ncut) <= int(sensitive.sum())
    assert sensitive.sum() <= sensitive_cap(n)
    with np.errstate(invalid="ignore"):
        acc = (s.Nvars - 1.0) * np.log(z) + got - lnp0 > np.log(u3)
    np.testing.assert_array_equal(np.any(after != before, axis=1), acc)
    assert not np.any(acc & np.any(cut == 1, axis=1) & ~sensitive)
