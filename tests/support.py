"""What the test modules share, each defined once: device access, environment switches, the S2 state and its
starting points, plans and a plain launch, layout conversions, the steady-state ensembles, the hedge tests'
sampler and cached runner, the tolerances and asserting helpers several modules hold their kernels to, and a few
small tools (the host-driver fixture's body, the JSON-lines report writer, a free port, a refusal's text).

Importing this module defines things and does nothing else: no torch, no librvmcmc.so, no GPU call, no
environment variable read (tests/test_gpu_a_dist.py needs a suite process that has made no GPU call by the time
it runs, and modules that sort before it import this one).  Test modules import from here, never from each other.
"""
import contextlib
import dataclasses
import json
import os
import re
import shutil
import socket
import subprocess
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import oracle as O
from conftest import GOLDEN, ROOT, S2_PLANETS, S2_SCALES, hd_planets, s2_obs_oracle

CSRC = os.path.join(ROOT, "rvel-mcmc_amd", "csrc")


# ---- device access ------------------------------------------------------------------------------------------

def torch_or_fail():
    import torch

    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


def rvm_lib():
    """(rvmcmc._lib, the loaded library)."""
    torch_or_fail()  # first: librvmcmc.so then binds to the HIP runtime torch has loaded, not to a second one
    from rvmcmc import _lib

    return _lib, _lib.load()


def to_device(a, dtype=None, copy=False):
    """A host array on the device, C-contiguous; copy=True always copies, so a read-only input stays read-only."""
    host = np.array(a, dtype=dtype, order="C") if copy else np.ascontiguousarray(a, dtype=dtype)
    return torch_or_fail().as_tensor(host, device="cuda")


# ---- environment switches -----------------------------------------------------------------------------------

@contextlib.contextmanager
def switches(env):
    """Environment switches read at plan creation ({name: value}, None: unset), restored on exit."""
    old = {k: os.environ.get(k) for k in env}
    try:
        for k, v in env.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


# ---- the S2 state, its scales, the tight ball ---------------------------------------------------------------

def s2_state(fixed_step=False, **kw):
    from rvmcmc import engine, state

    s = state.State(planets=[dict(p) for p in S2_PLANETS], **kw)
    if fixed_step:
        s.integrator = dataclasses.replace(engine.DEFAULT_CONFIG, resolve_tol=0.0)  # the fixed-step plan
    return s


def s2_state_and_obs(fixed_step=False, **kw):
    return s2_state(fixed_step, **kw), s2_obs_oracle()


def state_scales(s):
    return np.array([S2_SCALES[k] for k in s.get_rawkeys()])


def tight_ball(s, shape, seed, rel=1e-3):
    """shape + (Nvars,) starting points around the state's parameters; seed: an integer, or a Generator to draw
    from (and advance)."""
    rng = np.random.default_rng(seed)
    return s.get_params() + rel * state_scales(s) * rng.standard_normal(tuple(shape) + (s.Nvars,))


# ---- plans and a plain launch -------------------------------------------------------------------------------

TOL, RMAX = 5e-7, 4
T1_REL = 1e-11 * 35.0  # tests/test_gpu_logl.py: 1e-11 sum|w| (levels 4..7)
# default integrator (rvmcmc.engine.IntegratorConfig): level multipliers and base steps per orbit
LEVELS = (4, 5, 6, 7)
SPO = 8.0
# T1: roundoff floor.  ~1e-15 relative differences in the per-level model RV (FMA contraction on
# the GPU, a different Stumpff evaluation) are amplified by the Richardson weights (sum_k |w_k|:
# 6.2 at 4 levels, 26 at 6) and by the likelihood's conditioning (dlogL/drv ~ 2 sum|r|/(N sigma^2)
# ~ 1e4).  Tolerance: 1e-11 * sum|w| * max(1, |logL|)  (measured max 4e-11 at 4 levels).
T1_REL_PER_W = 1e-11
# T1 as used by the batch comparisons of tests/test_gpu_logl.py: 3x the oracle's own roundoff sensitivity over
# the batch (t1_tol_sens).  SURVEY.md §8c's 1e-12 is below that sensitivity for these walkers (the
# oracle itself moves by up to 7.5e-11 when an input changes by 1e-15 relative), so it cannot be
# met by any second implementation; t1_tol (the Sigma|w| form above) remains for the sampler and
# derivative tests that compare single values.
T1_SENS_FACTOR = 3.0


def t1_tol(nl=LEVELS):
    return T1_REL_PER_W * float(np.abs(O.richardson_weights(nl)).sum())


def adaptive_plan(planets, obs, W, resolve=(TOL, RMAX), inclined=False):
    """The default integrator's plan of W walkers with the adaptive resolution: (plan, dt, mult)."""
    from rvmcmc import engine

    dt, mult, hint = engine.IntegratorConfig().plan_args(planets)
    t, rv, er = engine.obs_arrays(obs)
    return engine.LoglPlan(t, rv, er, obs.Npoints, len(planets), dt, mult, W, period_hint=hint, inclined=inclined,
                           resolve=resolve), dt, mult


def fixed_plan(obs, planets, n_levels=LEVELS, steps=SPO, max_walkers=4096, inclined=False):
    from rvmcmc import engine

    pmin = engine.min_period(planets)
    dt = pmin / steps
    t, rv, er = engine.obs_arrays(obs)
    return engine.LoglPlan(t, rv, er, obs.Npoints, len(planets), dt, n_levels, max_walkers,
                           period_hint=pmin, inclined=inclined), dt


def launch(plan, X):
    """A plain launch of the walkers X [W][rows] (kernel row order): (logL [W], status [W]) on the host."""
    torch = torch_or_fail()
    K = torch.as_tensor(np.ascontiguousarray(np.asarray(X).T), device="cuda")
    lp, st, _ = plan.logl(K)
    torch.cuda.synchronize()
    return lp.cpu().numpy(), st.cpu().numpy()


# ---- layout conversions: kernel rows [rows * np][W] (m, a, h, k, l (, ix, iy) per planet), oracle [W][np][7] ----

def kernel_rows(P, rows=5):
    W, n, _ = P.shape
    return np.ascontiguousarray(np.concatenate([P[:, p, :rows].T for p in range(n)], 0))


def oracle_params(X, n_planets, inclined=False):
    """Flat kernel-row vectors X [W][rows * np] (kernel rows K: pass K.T) -> oracle parameters, unused columns 0."""
    rows = 7 if inclined else 5
    P = np.zeros((len(X), n_planets, 7))
    P[:, :, :rows] = np.asarray(X).reshape(-1, n_planets, rows)
    return P


def free_params_to_oracle(pm, X):
    """Free-parameter rows X [W][dim] of a State's ParamMap -> oracle layout [W][np][7]."""
    if len(X) == 0:
        return np.zeros((0, pm.n_planets, 7))
    K = np.stack([pm.vector_to_kernel_np(x) for x in np.asarray(X, dtype=np.float64)], 1)  # [rows][W]
    return oracle_params(K.T, pm.n_planets, pm.inclined)


def oracle_logl_fn(s, obs, dt):
    """X [W][dim] in the State's free-parameter order -> the oracle's (logL, status) with the kernel algorithm
    (the State's integrator level sequence)."""
    pm = s.param_map()

    def fn(X):
        return O.logl_whx_batch(free_params_to_oracle(pm, X), pm.n_planets, obs, dt, s.integrator.mult)

    return fn


# ---- the steady-state ensembles (scripts/probe/, where the scripts that wrote them read them) -------------------

STEADY = {"s2": "ens_it2000.npy", "hd155358": "ens_hd155358_it1000.npy", "3planet": "ens_3planet_it1000.npy"}


def steady_ensemble(name):
    return np.load(os.path.join(ROOT, "scripts", "probe", STEADY[name]))


def hd_system():
    return hd_planets(), O.obs_from_file(os.path.join(GOLDEN, "HD155358.vels"), Npoints=100)


def burned_in(planets, obs, W, iters, seed=2017):
    """An ensemble after `iters` iterations of the device sampler from the tight ball (the chain's
    steady state, the regime of the adaptive resolution)."""
    torch = torch_or_fail()
    from rvmcmc.ensemble import EnsembleSampler
    from rvmcmc.state import State

    s = State(planets=[dict(p) for p in planets])
    X0 = tight_ball(s, (W,), 1)
    ens = EnsembleSampler(W, s, obs, seed=seed + 1)
    ens.set_positions(X0)
    ens.compute_lnprob()
    for _ in range(iters):
        ens.step()
    torch.cuda.synchronize()
    ens.check_faults()
    return ens.gather_positions()


# ---- wide-ball walkers and the adaptive T1 comparison (tests/test_gpu_resolve.py) -------------------------------

THIRD = {"m": 1e-3, "a": 2.6, "h": 0.05, "k": 0.0, "l": 1.0}  # scripts/configs_bench.py config 5
EXTRA_PLANETS = [{"m": 1e-3, "a": 2.6, "h": 0.05, "k": 0.0, "l": 1.0},
                 {"m": 5e-4, "a": 4.1, "h": -0.03, "k": 0.02, "l": 4.0}]

# two prior-passing walkers of the S2 observation set (hill_factor 0: no encounter exit) whose
# halving passes blow up: [1] in pass 1 of its forward direction, [0] in pass 2 of both directions
# (found on the oracle by scripts/probe/find_nonfinite_pass.py; rows m, a, h, k, l per planet)
NONFINITE_WALKERS = np.array([
    [[0.02256103, 0.41693664, -0.97022551, -0.02642071, 0.3], [0.00259106, 0.65391134, -0.90235793, 0.40896047, 2.2]],
    [[0.00505582, 1.19118678, -0.39903947, 0.34994554, 0.3], [0.00316488, 1.01076266, -0.72163793, 0.31746809, 2.2]],
])


def pal_ball(planets, W, rel=1e-3, seed=0):
    rng = np.random.default_rng(seed)
    base = O.pal_params(planets)
    P = np.repeat(base[None], W, 0)
    P[:, :, :5] *= 1 + rel * rng.standard_normal((W, len(planets), 5))
    return P  # [W][np][7]


def s2_rows_and_scales():
    return np.array([p[k] for p in S2_PLANETS for k in "mahkl"]), np.array([S2_SCALES[k] for _ in S2_PLANETS
                                                                             for k in "mahkl"])


def wide_walkers(W, ball=0.6, seed=3):
    """Half a sampler-like ball (x0 + ball * scales * N(0,1), mcmc.py:45-51), half stretch
    proposals between its members (q = c - z (c - x), z in [1/2, 2]): [W][10] kernel rows."""
    x0, sc = s2_rows_and_scales()
    rng = np.random.default_rng(seed)
    n = W // 2
    X = x0 + ball * sc * rng.standard_normal((n, 10))
    j = rng.integers(0, n, W - n)
    z = (rng.random(W - n) + 1.0) ** 2 / 2.0
    Q = X[j] - z[:, None] * (X[j] - X[:W - n])
    return np.concatenate([X, Q])


def _par(fn, P, nt=16):
    idx = np.array_split(np.arange(len(P)), nt)
    with ThreadPoolExecutor(nt) as ex:
        parts = list(ex.map(lambda ix: fn(P[ix]), idx))
    return [np.concatenate([p[k] for p in parts]) for k in range(len(parts[0]))]


def _par_ix(fn, P, nt=16):
    """_par for fn(P_chunk, index_chunk)."""
    idx = np.array_split(np.arange(len(P)), nt)
    with ThreadPoolExecutor(nt) as ex:
        parts = list(ex.map(lambda ix: fn(P[ix], ix), idx))
    return [np.concatenate([p[k] for p in parts]) for k in range(len(parts[0]))]


def assert_t1_adaptive(got, st, P, n_planets, obs, dt, mult, tol=TOL, rmax=RMAX, has_inc=0, ctx=None, ecc_guard=0.0):
    """T1 of an adaptive-resolution launch against the oracle's restatement of the same rule
    (oracle.logl_whx_adapt_batch): statuses and logL, up to sensitivity.  Chaotic walkers (close
    approaches) and decisions at roundoff distance from their bound may legitimately go the other
    way in a second implementation: the oracle's own response to 1e-15 relative input nudges (of
    logL, of the status, of the stage reached and of the final estimate -- a difference of two
    extrapolations, which near a close approach moves by up to tens of percent under such a nudge),
    and its closest approach to any decision's bound.  ctx: the sampler's accept inputs (the
    certain-reject cut; oracle.logl_whx_adapt_batch).  Returns (stages [W][2], sensitive [W]) and,
    with ctx, the oracle's cut [W][2]."""
    W = len(got)

    def fn(p, ix=None):
        c = None if ctx is None else dict(ctx, **{k: np.asarray(ctx[k])[ix] for k in ("mode", "z", "u", "lnp0")})
        r = O.logl_whx_adapt_batch(p, n_planets, obs, dt, mult, tol, rmax, has_inc=has_inc, ctx=c, ecc_guard=ecc_guard)
        return r if ctx is not None else r + (np.zeros((len(p), 2), dtype=np.int32),)

    ref, st_ref, rf, est, margin, cut = _par_ix(fn, P)
    sens = np.zeros(W)
    flips = np.zeros(W, dtype=bool)
    for pl, par, sgn in [(0, 4, 1), (-1, 4, -1), (0, 1, 1)]:
        P2 = P.copy()
        P2[:, pl, par] *= 1 + sgn * 1e-15
        r2, s2, rf2, est2, _, cut2 = _par_ix(fn, P2)
        flips |= (s2 != st_ref) | np.any(rf2 != rf, axis=1) | np.any(cut2 != cut, axis=1)
        with np.errstate(invalid="ignore"):  # (an estimate whose roundoff response is not small
            # against its distance from the bound)
            flips |= np.any(np.abs(est2 - est) > 0.02 * np.abs(est - 0.5 * tol), axis=1)
        both = (st_ref == 0) & (s2 == 0)
        sens[both] = np.maximum(sens[both], np.abs(r2[both] - ref[both]) / np.maximum(1.0, np.abs(ref[both])))
    sensitive = flips | (sens > 1e-9) | (margin.min(axis=1) < 1e-6)
    mism = st != st_ref
    assert np.all(~mism | sensitive), np.nonzero(mism & ~sensitive)
    assert mism.sum() <= max(2, W // 100)
    ok = (st == 0) & (st_ref == 0)
    err = np.abs(got[ok] - ref[ok]) / np.maximum(1.0, np.abs(ref[ok]))
    bound = np.maximum(T1_REL, 1e3 * sens[ok])
    bad = (err > bound) & ~sensitive[ok]
    assert not bad.any(), (np.nonzero(ok)[0][bad][:10], err[bad][:10])
    assert np.mean(err <= T1_REL) > 0.9
    # walkers the oracle leaves UNRESOLVED are UNRESOLVED on the device too (up to sensitivity)
    assert np.all(((st == 4) == (st_ref == 4)) | sensitive)
    if ctx is not None:
        return rf, sensitive, cut
    return rf, sensitive


# ---- the hedge tests (test_gpu_hedge.py, test_gpu_hedge_wait.py, test_gpu_refine_tail.py) ------------------------

LAYOUTS = {"teams": {}, "split": {"RVM_REFINE_TEAMS": "0"}, "one_block": {"RVM_REFINE_SPLIT": "0"}}
OFF = {"RVM_HEDGE": "0"}
# test_gpu_hedge.py's runs; test_gpu_hedge_wait.py reads its references without the hedge from the same cache
HEDGE_RUNS = {}


def hedge_sampler(X0, env):
    from rvmcmc.ensemble import EnsembleSampler

    with switches(env):
        s = s2_state()
        ens = EnsembleSampler(len(X0), s, s2_obs_oracle(), seed=2017)  # (a fresh observation set: a fresh plan)
        ens.set_positions(X0)
        ens.compute_lnprob()
    ens.plan.faults(reset=True)
    ens.plan.hedge_stats(reset=True)
    return ens


def hedge_result(ens):
    torch_or_fail().cuda.synchronize()
    return (ens.gather_positions(), np.concatenate([l.cpu().numpy() for l in ens.lnp]), ens.naccepted.cpu().numpy(),
            ens.plan.faults(reset=True), ens.plan.hedge_stats(reset=True))


def hedge_run(cache, kind, env, iters, counter=None):
    """The sampler's result after `iters` iterations from the steady-state ensemble or a wide ball of n
    walkers per half (kind = n), under the switches env; computed once per (kind, env) and kept in the caller's
    cache.  counter(ens) reads and resets one more of the plan's counters: reset before the first iteration,
    appended to the result after the last."""
    key = (kind, tuple(sorted(env.items())), iters)
    if key not in cache:
        X0 = steady_ensemble("s2") if kind == "steady" else wide_walkers(2 * kind, ball=0.3, seed=5)
        ens = hedge_sampler(X0, env)
        if counter is not None:
            counter(ens)
        for _ in range(iters):
            ens.step()
        cache[key] = hedge_result(ens) + (() if counter is None else (counter(ens),))
    return cache[key]


def assert_same_run(got, want):
    np.testing.assert_array_equal(got[0], want[0])
    np.testing.assert_array_equal(got[1], want[1])
    np.testing.assert_array_equal(got[2], want[2])
    assert got[3] == want[3], (got[3], want[3])


# ---- include/rvmcmc.h as the ABI tests read it ---------------------------------------------------------------

def header_source():
    """include/rvmcmc.h without its comments."""
    src = open(os.path.join(ROOT, "include", "rvmcmc.h")).read()
    return re.sub(r"/\*.*?\*/", "", src, flags=re.S)


def header_prototypes():
    """{name: (return type, [(argument type, argument name), ...])} of every prototype the header declares;
    a type is its C spelling without `const` and without blanks (`double*`, `rvm_plan**`, `int32_t`)."""
    out = {}
    for ret, name, args in re.findall(r"^(int|void|size_t|const char\*)\s+(rvm_\w+)\s*\(([^)]*)\)\s*;",
                                      header_source(), flags=re.M):
        out[name] = (ret, [])
        for a in args.split(","):
            m = re.match(r"(.*?)(\w+)$", " ".join(a.split()))
            if m.group(0) != "void":
                out[name][1].append((m.group(1).replace("const ", "").replace(" ", ""), m.group(2)))
    return out


# ---- small tools --------------------------------------------------------------------------------------------

# the full-iteration case tests/test_tempering_adapt_cpu.py and tests/test_gpu_tempering_adapt.py share
PT_ADAPT_CASE = dict(T=4, W=24, iters=4, seed=0, lag=10.0, time=2.0)


def host_driver_report(tmp_path_factory, name, driver):
    """The output (JSON) of a small driver built with rvm_plan_host.cpp by the host compiler and run with every
    RVM_* variable stripped."""
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    d = tmp_path_factory.mktemp(name)
    src = d / "driver.cpp"
    src.write_text(driver)
    exe = d / "driver"
    b = subprocess.run([cxx, "-std=c++17", "-O1", "-I", CSRC, "-o", str(exe), str(src),
                        os.path.join(CSRC, "rvm_plan_host.cpp")], capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, b.stderr[-3000:]
    env = {k: v for k, v in os.environ.items() if not k.startswith("RVM_")}
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, r.stderr[-3000:]
    return json.loads(r.stdout)


def current_test():
    return os.environ.get("PYTEST_CURRENT_TEST", "").split(" ")[0]


def report_line(var, what=None, **fields):
    """Append one record to the JSON-lines file $var names, if it names one: the fields, behind the running test
    and `what` where a `what` is given."""
    path = os.environ.get(var)
    if path:
        d = {} if what is None else {"test": current_test(), "what": what}
        d.update(fields)
        with open(path, "a") as f:
            f.write(json.dumps(d) + "\n")


def free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def refusal_text(rc):
    from rvmcmc import _lib

    assert rc < 0
    return _lib.load().rvm_last_error()
