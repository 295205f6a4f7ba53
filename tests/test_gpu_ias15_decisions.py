"""Sampler decisions on the device vs the same samplers driven by the IAS15 oracle.

The reference evaluates every proposal with REBOUND's IAS15 (state.py:36-110); the kernel
integrates Wisdom-Holman + Richardson.  Each test runs the PRODUCTION device path (Philox draws,
speculative stretch iterations on the bench shape), reconstructs the draws with
tests/philox_ref.py (or injects them), restates the reference sampler step in numpy with the IAS15
restatement as the likelihood, and compares every accept/reject decision
(tests/ias15_parity.py: near-margin walkers and status disagreements are exempt and counted;
everything else must be identical).  Each test prints one JSON line with the counts (and appends
it to $RVM_PARITY_REPORT when set; profiles/ keeps the round's report).

Cases: the bench config (2-planet synthetic, 4096 walkers, tight ball), a wide ball with prior
rejections and encounters, HD155358 (real data, `sol` of (Ex)HD155358.ipynb:64-66), 3 planets
(config 5's system), batched MH chains (mcmc.py:107-121) on S2 and HD155358, and one SMALA step
(mcmc.py:167-187; likelihood terms from IAS15, proposal-density terms from the device metric,
which test_gpu_derivs.py pins against IAS15 differences).
"""
import json

import numpy as np
import pytest

import ias15_parity as IP
import oracle as O
from conftest import S2_PLANETS, s2_obs_oracle
from philox_ref import stretch_uniforms
from support import THIRD, burned_in as _burned_in, hd_system as _hd, steady_ensemble, tight_ball
from support import torch_or_fail as _torch

pytestmark = pytest.mark.gpu

# T2 (|dlogL| <= 1e-6 absolute) on the proposals a sampler actually makes: they
# reach further from the plan's initial state than the tight balls of tests/test_gpu_logl.py
# (5e-8 there); measured max ~1e-7 on the bench config after a few iterations (reported per test)
T2_ABS = 1e-6


def _device_logl(ens_or_plan, pm, Q, hill):
    """Kernel logL + status of proposals Q [n][dim] (plain launch; bit-identical to the fused and
    speculative launches, test_gpu_samplers.py)."""
    torch = _torch()
    plan = ens_or_plan
    X = torch.as_tensor(np.ascontiguousarray(Q.T), device="cuda")
    lp, st, _ = plan.logl(pm.to_kernel(X), hill_factor=hill)
    torch.cuda.synchronize()
    return lp.cpu().numpy(), st.cpu().numpy()


def closest_approach_ratio(P, n_planets, obs, dt, hill=1.0, refine=32):
    """Closest pair approach of each walker's trajectory over the observation span, as a multiple of
    its exit distance (exit_min_distance, state.py:46): the Wisdom-Holman restatement at refine x
    finer steps than the plan's (one level), every pair checked at every kick -- the trajectory
    sampled ~densely, where REBOUND tests only at the ends of its IAS15 steps.  < 1: the planets do
    come inside the exit distance.  [W]."""
    return np.array([O.min_distance_ratio(P[i:i + 1], n_planets, obs, dt / refine, 1) for i in range(len(P))])


def stretch_parity(name, planets, obs, W, ball, iterations=2, warm=4, roundoff=False, seed=2017, ball_seed=0,
                   X0=None):
    """Run the device EnsembleSampler (default path) and compare its decisions, iteration by
    iteration, with emcee 2.2.1 restated in numpy on IAS15 logL and the same Philox draws.
    X0: start from these positions [W][dim] (e.g. a chain's steady state) instead of a ball."""
    torch = _torch()
    from rvmcmc.ensemble import EnsembleSampler
    from rvmcmc.state import State

    s = State(planets=[dict(p) for p in planets])
    pm = s.param_map()
    dim = s.Nvars
    if X0 is None:
        X0 = tight_ball(s, (W,), ball_seed, ball)
    ens = EnsembleSampler(W, s, obs, seed=seed)
    ens.set_positions(X0)
    ens.compute_lnprob()
    for _ in range(warm):
        ens.step()
    torch.cuda.synchronize()
    n, hk, hill, npl = ens.nloc, ens.halfk, ens.hill_factor, pm.n_planets
    lnp_ref = [IP.ias15_logl(IP.to_oracle(pm, p.t().cpu().numpy()), npl, obs, hill)[0] for p in ens.pos]
    tally = IP.Tally(name)
    for _ in range(iterations):
        it = ens.iteration
        before = [p.t().cpu().numpy().copy() for p in ens.pos]
        lnp_dev = [l.cpu().numpy().copy() for l in ens.lnp]
        spec = ens.speculating()
        ens.step()
        torch.cuda.synchronize()
        after = [p.t().cpu().numpy() for p in ens.pos]
        for h in (0, 1):
            c = before[1] if h == 0 else after[0]  # half 1 proposes against the updated half 0
            u1, u2, u3 = stretch_uniforms(ens.seed, ens.global_begin(h), n, it, h)
            q, z = IP.stretch_proposal(before[h], c, u1, u2, ens.a)
            lq_ref, sq_ref = IP.ias15_logl(IP.to_oracle(pm, q), npl, obs, hill)
            lq_dev, sq_dev = _device_logl(ens.plan, pm, q, hill)
            with np.errstate(invalid="ignore"):
                d_ref = (dim - 1.0) * np.log(z) + lq_ref - lnp_ref[h]
                d_dev = (dim - 1.0) * np.log(z) + lq_dev - lnp_dev[h]
                acc_ref = d_ref > np.log(u3)
                margin = np.abs(d_ref - np.log(u3))
                margin = np.where(np.isnan(margin), np.inf, margin)
            sens = None
            if roundoff:
                # the IAS15 logL's own roundoff sensitivity, for the proposals where it could matter
                # (a decision that differs, or an OK proposal beyond T2): chaotic ones are exempt
                sens = np.zeros(n)
                okk = (sq_dev == 0) & (sq_ref == 0)
                with np.errstate(invalid="ignore"):
                    look = (d_dev > np.log(u3)) != acc_ref
                    look |= okk & (np.abs(lq_dev - lq_ref) > IP.MARGIN)
                ix = np.nonzero(look & (sq_ref == 0))[0]
                sens[ix] = IP.ias15_roundoff(IP.to_oracle(pm, q[ix]), npl, obs, lq_ref[ix], hill)
            acc_dev = np.any(after[h] != before[h], axis=1)
            # the device sampler itself is exact: its decisions follow its own logL bit for bit
            np.testing.assert_array_equal(acc_dev, d_dev > np.log(u3))
            np.testing.assert_array_equal(after[h][acc_dev], q[acc_dev])
            cur = np.isneginf(lnp_dev[h]) != np.isneginf(lnp_ref[h])  # (e.g. UNRESOLVED vs OK)
            tally.add(acc_dev, acc_ref, margin, sq_dev, sq_ref, lq_dev, lq_ref, idx_offset=h * hk, roundoff=sens,
                      current_differs=cur)
            # proposals the device ends ENCOUNTER and IAS15 integrates (2/0): the kernel tests the exit
            # distance at every kick of every level, REBOUND only at the end of each IAS15 step
            # (state.py:46, mcmc.py:119-121).  Each such proposal's closest approach on a densely
            # sampled trajectory tells whether the planets really come inside the exit distance
            # (REBOUND's step-end test misses it) or the device's call is its own discretisation's
            e20 = np.nonzero((sq_dev == IP.ST_ENC) & (sq_ref == IP.ST_OK))[0]
            if len(e20):
                r = closest_approach_ratio(IP.to_oracle(pm, q[e20]), npl, obs, ens.plan.dt, hill)
                tally.enc_ratios = getattr(tally, "enc_ratios", []) + r.tolist()
            # (the proposals left UNRESOLVED, for the failure message: oracle replay in
            # scripts/probe/replay_parity.py)
            tally.unresolved_rows = getattr(tally, "unresolved_rows", []) + q[sq_dev == IP.ST_UNRESOLVED].tolist()
            if np.any(sq_dev == IP.ST_UNRESOLVED):
                print("unresolved proposals:", json.dumps(q[sq_dev == IP.ST_UNRESOLVED].tolist()))
            lnp_ref[h] = np.where(acc_dev, lq_ref, lnp_ref[h])  # follow the device chain
    er = np.array(getattr(tally, "enc_ratios", []))
    return tally, dict(walkers=W, ball=ball, iterations=iterations, warm_iterations=warm, speculative=bool(spec),
                       enc_2_0_inside_exit_distance=int((er < 1.0).sum()),
                       enc_2_0_outside_exit_distance=int((er >= 1.0).sum()),
                       enc_2_0_closest_approach_ratios=sorted(round(float(v), 4) for v in er))


def test_stretch_vs_ias15_bench_config():
    """The bench workload itself: 2-planet synthetic, 101 epochs, 4096 walkers, tight ball,
    speculative whole iterations (one 6144-slot launch)."""
    tally, info = stretch_parity("stretch/bench-config S2 4096 walkers", S2_PLANETS, s2_obs_oracle(), 4096, 1e-3)
    rep = tally.report(**info)
    assert info["speculative"]
    assert rep["mismatches_not_exempt"] == 0, tally.mismatch[:20]
    assert rep["exempt_status_disagreement"] == 0 and rep["differing_but_exempt"] == 0
    assert rep["max_abs_dlogl_ok_proposals"] <= T2_ABS
    assert rep["decisions"] == 2 * 4096 and rep["accepted_ias15"] > 1000


def test_stretch_vs_ias15_wide_ball_encounters():
    """A wide initial ball (0.6 x the emcee scales): prior rejections and close-encounter exits
    occur, and most proposals are far from the plan's period basis (short periods, eccentric or
    crossing orbits).  The adaptive resolution (IntegratorConfig.resolve_tol) keeps
    every OK proposal within T2 (1e-6) of IAS15 all the same; only proposals on which IAS15 itself
    is roundoff-sensitive (a 1e-15 input nudge moves its logL by > 1e-9 relative) are exempt, and
    counted.  (Round 2, fixed step: 580 OK proposals beyond 1e-6, max |dlogL| 81.)"""
    tally, info = stretch_parity("stretch/wide-ball S2 2048 walkers", S2_PLANETS, s2_obs_oracle(), 2048, 0.6,
                                 warm=0, roundoff=True, ball_seed=3)
    rep = tally.report(**info)
    assert rep["mismatches_not_exempt"] == 0, tally.mismatch[:20]
    # no proposal is left UNRESOLVED (a forced reject the reference never makes): device status 4 is
    # never exempt, and none occurs
    assert rep["unresolved_device"] == 0 and not any(k.startswith("4/") for k in rep["status_pairs_device/ias15"]), \
        tally.unresolved_rows
    assert rep["encounters_ias15"] > 20 and rep["prior_rejections"] > 20
    assert rep["exempt_status_disagreement"] <= max(4, rep["decisions"] // 100)
    assert rep["exempt_current_status_disagreement"] <= max(4, rep["decisions"] // 100)
    assert rep["differing_but_exempt"] <= max(4, rep["decisions"] // 500)
    assert rep["ok_proposals_dlogl_above_margin_not_roundoff"] == 0
    assert rep["max_abs_dlogl_ok_proposals_not_roundoff"] <= T2_ABS
    assert rep["exempt_ias15_roundoff_sensitive"] <= rep["decisions"] // 100


def test_stretch_vs_ias15_steady_state():
    """The bench chain at its steady state: 4096 walkers from the ensemble after 2000 iterations
    (scripts/probe/ens_it2000.npy, scripts/dump_bench_ensemble.py), where the posterior is wide in h, k
    (eccentricities to 0.45) and the plan's fixed step alone missed T2 on 668 of 5823 proposals.  Two
    speculative iterations of the real sampler; every decision and every OK proposal's logL against
    IAS15 (the adaptive resolution's regime: extensions, halving passes, certain rejects)."""
    X0 = steady_ensemble("s2")
    tally, info = stretch_parity("stretch/steady-state S2 4096 walkers (iteration 2000)", S2_PLANETS, s2_obs_oracle(),
                                 len(X0), 0.0, warm=0, roundoff=True, X0=X0)
    rep = tally.report(**info)
    assert info["speculative"]
    assert rep["mismatches_not_exempt"] == 0, tally.mismatch[:20]
    assert rep["unresolved_device"] == 0, tally.unresolved_rows
    assert rep["ok_proposals_dlogl_above_margin_not_roundoff"] == 0
    assert rep["max_abs_dlogl_ok_proposals_not_roundoff"] <= T2_ABS
    assert rep["exempt_status_disagreement"] <= max(4, rep["decisions"] // 500)
    assert rep["differing_but_exempt"] == 0 and rep["exempt_current_status_disagreement"] == 0


@pytest.mark.parametrize("case", ["HD155358", "3-planet"])
def test_stretch_vs_ias15_steady_state_other_systems(case):
    """HD155358 and the 3-planet system at the steady state of their own chains (1000 iterations
    of the device sampler from the tight ball): the adaptive resolution, and its eccentricity guard,
    calibrated on S2, must hold T2 on these posteriors too."""
    if case == "HD155358":
        planets, obs = _hd()
        W = 512
    else:
        np.random.seed(2017)
        planets = [dict(p) for p in S2_PLANETS] + [dict(THIRD)]
        obs = O.fake_obs(planets, Npoints=100, error=1.5e-4, errorVar=2.5e-5, tmax=120.)
        W = 512
    X0 = _burned_in(planets, obs, W, 1000)
    tally, info = stretch_parity(f"stretch/steady-state {case} {W} walkers (iteration 1000)", planets, obs, W, 0.0,
                                 warm=0, roundoff=True, X0=X0)
    rep = tally.report(**info)
    assert rep["mismatches_not_exempt"] == 0, tally.mismatch[:20]
    assert rep["unresolved_device"] == 0, tally.unresolved_rows
    assert rep["ok_proposals_dlogl_above_margin_not_roundoff"] == 0
    assert rep["max_abs_dlogl_ok_proposals_not_roundoff"] <= T2_ABS
    # the exempt status pairs (round 4: HD155358 23 of 1024, all 2/0) are bounded and none flips a
    # decision; each one's closest approach on a densely sampled trajectory is in the report
    # (enc_2_0_*: inside the exit distance = an approach between IAS15's step ends, REBOUND's test
    # misses it; outside = the device levels' own discretisation near a close approach)
    assert rep["exempt_status_disagreement"] <= rep["decisions"] // 32, rep["status_pairs_device/ias15"]
    assert set(rep["status_pairs_device/ias15"]) <= {"2/0"}, rep["status_pairs_device/ias15"]
    # a 2/0 pair is a forced reject: it flips the decision when IAS15 accepts the proposal (round 6:
    # 2 of HD155358's 1024 on one burn-in, 12 pairs all beyond the exit distance; 0 of 30 pairs in the
    # 2048-walker sweep, profiles/r06zi_parity_sweep_2048.jsonl)
    assert rep["differing_but_exempt"] <= max(2, rep["decisions"] // 400)
    assert rep["exempt_current_status_disagreement"] == 0


def test_stretch_vs_ias15_config2():
    """BASELINE config 2's own shape: 1024 walkers of the 2-planet synthetic config (512 per half,
    one speculative launch of 1536 walker slots per iteration), every proposal of two iterations."""
    tally, info = stretch_parity("stretch/config2 S2 1024 walkers", S2_PLANETS, s2_obs_oracle(), 1024, 1e-3)
    rep = tally.report(**info)
    assert info["speculative"]
    assert rep["decisions"] == 2 * 1024
    assert rep["mismatches_not_exempt"] == 0, tally.mismatch[:20]
    assert rep["exempt_status_disagreement"] == 0 and rep["differing_but_exempt"] == 0
    assert rep["max_abs_dlogl_ok_proposals"] <= T2_ABS


def test_stretch_vs_ias15_hd155358():
    planets, obs = _hd()
    tally, info = stretch_parity("stretch/HD155358 512 walkers", planets, obs, 512, 1e-3)
    rep = tally.report(**info)
    assert rep["mismatches_not_exempt"] == 0, tally.mismatch[:20]
    assert rep["exempt_status_disagreement"] == 0 and rep["differing_but_exempt"] == 0
    assert rep["max_abs_dlogl_ok_proposals"] <= T2_ABS


def test_stretch_vs_ias15_three_planets():
    """Config 5's system (S2 + the named third planet), 1024 walkers."""
    np.random.seed(2017)
    planets = [dict(p) for p in S2_PLANETS] + [dict(THIRD)]
    obs = O.fake_obs(planets, Npoints=100, error=1.5e-4, errorVar=2.5e-5, tmax=120.)
    tally, info = stretch_parity("stretch/3-planet 1024 walkers", planets, obs, 1024, 1e-3)
    rep = tally.report(**info)
    assert rep["mismatches_not_exempt"] == 0, tally.mismatch[:20]
    assert rep["exempt_status_disagreement"] == 0 and rep["differing_but_exempt"] == 0
    assert rep["max_abs_dlogl_ok_proposals"] <= T2_ABS


def mh_parity(name, planets, obs, chains, step, steps=3, seed=5):
    """MhChains (batched mcmc.Mh) with injected N(0,1) and U(0,1) vs mcmc.py:107-121 on IAS15."""
    torch = _torch()
    from rvmcmc.mcmc import MhChains
    from rvmcmc.state import State

    s = State(planets=[dict(p) for p in planets])
    scal = {"m": 1.e-3, "a": 0.3, "h": 0.5, "k": 0.5, "l": np.pi / 2.}  # mcmc_benchmark_mh.py:52
    mh = MhChains(s, obs, scal, step, chains, seed=seed)
    pm, dim, hill = mh.pmap, mh.dim, mh.state.hillRadiusFactor
    sc = np.array([scal[k] for k in mh.state.get_rawkeys()])
    X = mh.X.cpu().numpy().copy()  # [dim][C]
    lnp_ref = IP.ias15_logl(IP.to_oracle(pm, X.T), pm.n_planets, obs, hill)[0]
    rng = np.random.default_rng(seed)
    tally = IP.Tally(name)
    for _ in range(steps):
        g = rng.standard_normal((dim, chains))
        u = rng.random(chains)
        lnp_dev = mh.lnp.cpu().numpy().copy()
        mh.step(draws_propose=torch.as_tensor(g, device="cuda"), draws_accept=torch.as_tensor(u, device="cuda"))
        torch.cuda.synchronize()
        Q = X + (step * sc)[:, None] * g  # mcmc.py:89-93 (shift_params by step_size * scales * N(0,1))
        got = mh.X.cpu().numpy()
        np.testing.assert_array_equal(got[:, np.any(got != X, axis=0)], Q[:, np.any(got != X, axis=0)])
        lq_ref, sq_ref = IP.ias15_logl(IP.to_oracle(pm, Q.T), pm.n_planets, obs, hill)
        lq_dev, sq_dev = _device_logl(mh.plan, pm, Q.T, hill)
        with np.errstate(invalid="ignore", over="ignore"):
            # mcmc.py:112-121: priorHard / Encounter -> reject; accept if exp(lp* - lp) > U
            acc_ref = (sq_ref == IP.ST_OK) & (np.exp(lq_ref - lnp_ref) > u)
            margin = np.abs((lq_ref - lnp_ref) - np.log(u))
            margin = np.where(np.isnan(margin), np.inf, margin)
        acc_dev = np.any(got != X, axis=0)
        with np.errstate(over="ignore", invalid="ignore"):
            np.testing.assert_array_equal(acc_dev, np.exp(lq_dev - lnp_dev) > u)
        tally.add(acc_dev, acc_ref, margin, sq_dev, sq_ref, lq_dev, lq_ref)
        lnp_ref = np.where(acc_dev, lq_ref, lnp_ref)
        X = got.copy()
    return tally, dict(chains=chains, step_size=step, steps=steps)


@pytest.mark.parametrize("case", ["S2", "HD155358"])
def test_mh_vs_ias15(case):
    if case == "S2":
        planets, obs = S2_PLANETS, s2_obs_oracle()
    else:
        planets, obs = _hd()
    tally, info = mh_parity(f"mh/{case} 512 chains", planets, obs, 512, 2e-3)
    rep = tally.report(**info)
    assert rep["mismatches_not_exempt"] == 0, tally.mismatch[:20]
    assert rep["exempt_status_disagreement"] == 0 and rep["differing_but_exempt"] == 0
    assert rep["max_abs_dlogl_ok_proposals"] <= T2_ABS
    assert 0 < rep["accepted_ias15"] < rep["decisions"]


def smala_parity(name, hessian, C_, eps=0.5, alpha=1e3, warm=2):
    """One batched SMALA step (mcmc.py:167-187) with injected z, u: the accept ratio's likelihood
    terms from IAS15, its proposal-density terms from the device metric (exact derivatives, pinned
    against IAS15 differences in test_gpu_derivs.py, or config 4's Gauss-Newton metric from the
    FD stencil's per-epoch RVs)."""
    torch = _torch()
    from rvmcmc.smala import SmalaChains
    from rvmcmc.state import State

    s = State(planets=[dict(p) for p in S2_PLANETS])
    obs = s2_obs_oracle()
    dim = s.Nvars
    sm = SmalaChains(s, obs, eps=eps, alpha=alpha, n_chains=C_, seed=5, hessian=hessian)
    for _ in range(warm):
        sm.step()
    pm, hill = sm.pmap, sm.state.hillRadiusFactor
    rng = np.random.default_rng(6)
    z = rng.standard_normal((C_, dim))
    u = rng.random(C_)
    x0 = sm.X.cpu().numpy().copy()
    c0 = {k: v.cpu().numpy().copy() for k, v in sm.cache.items() if k != "_c"}
    acc0 = sm.accepted.cpu().numpy().copy()
    sm.step(z=torch.as_tensor(z, device="cuda"), u=torch.as_tensor(u, device="cuda"))
    torch.cuda.synchronize()
    xs = sm.Xs.cpu().numpy()
    p = {k: v.cpu().numpy() for k, v in sm.prop.items() if k != "_c"}
    acc_dev = (sm.accepted.cpu().numpy() - acc0) == 1
    l0_ref, s0_ref = IP.ias15_logl(IP.to_oracle(pm, x0.T), pm.n_planets, obs, hill)
    ls_ref, ss_ref = IP.ias15_logl(IP.to_oracle(pm, xs.T), pm.n_planets, obs, hill)
    _, ss_dev, _ = sm.state.get_logp_batch(obs, torch.as_tensor(xs, device="cuda"), hill_factor=hill, pmap=pm)
    ss_dev = ss_dev.cpu().numpy()
    ls_dev = p["lp"]  # the proposal's logp as the device step used it

    def logq(y, mu, G, logdet):
        d = y - mu
        return -0.5 * (d @ G @ d / eps ** 2 + dim * np.log(eps ** 2) + logdet + dim * np.log(2 * np.pi))

    acc_ref = np.zeros(C_, bool)
    margin = np.full(C_, np.inf)
    for i in range(C_):
        if not (c0["ok"][i] and p["ok"][i] and ss_ref[i] == 0):
            continue
        G0 = c0["G"][:, i].reshape(dim, dim)
        Gp = p["G"][:, i].reshape(dim, dim)
        lr = (ls_ref[i] - l0_ref[i] + logq(x0[:, i], p["mu"][:, i], Gp, p["logdet"][i])
              - logq(xs[:, i], c0["mu"][:, i], G0, c0["logdet"][i]))
        acc_ref[i] = np.exp(lr) > u[i]
        margin[i] = abs(lr - np.log(u[i]))
    tally = IP.Tally(name)
    tally.add(acc_dev, acc_ref, margin, ss_dev, ss_ref, ls_dev, ls_ref)
    return tally.report(chains=C_, eps=eps, alpha=alpha, hessian=hessian), tally


def test_smala_step_vs_ias15():
    """Exact-metric SMALA (the reference's Hessian, state.py:253-294), 128 chains."""
    rep, tally = smala_parity("smala/S2 128 chains exact metric", "exact", 128)
    assert rep["mismatches_not_exempt"] == 0, tally.mismatch[:20]
    # the logp the accept uses is the adaptive plan's (SmalaChains._center_start, beside the
    # derivative launch), so T2 holds on every OK proposal as on the other paths (eps = 0.5 in the
    # metric's units reaches several posterior widths; round 2, before the adaptive resolution: 1 of
    # 128 at 2.7e-6)
    assert rep["exempt_status_disagreement"] == 0 and rep["differing_but_exempt"] == 0
    assert rep["max_abs_dlogl_ok_proposals"] <= T2_ABS
    assert 0 < rep["accepted_ias15"]


def test_smala_fd_step_vs_ias15():
    """Config 4's own SMALA path (BASELINE.json configs[3]): 256 chains, the FD stencil formed in
    one likelihood launch (23 integrations per chain and step), Gauss-Newton + SoftAbs metric derived
    on the device (mcmc.py:144-187 with the FD/GN metric).  Likelihood terms of the accept ratio from
    IAS15, proposal-density terms from the device metric; the stencil's centre logL is the adaptive
    kernel's (T2 holds)."""
    rep, tally = smala_parity("smala/S2 256 chains FD Gauss-Newton (config 4)", "gauss-newton", 256)
    assert rep["mismatches_not_exempt"] == 0, tally.mismatch[:20]
    assert rep["exempt_status_disagreement"] == 0 and rep["differing_but_exempt"] == 0
    assert rep["max_abs_dlogl_ok_proposals"] <= T2_ABS
    assert 0 < rep["accepted_ias15"] < rep["decisions"]
