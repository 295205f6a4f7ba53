"""The SMALA and MH device kernels straight through the C ABI on synthetic inputs, against the
40-digit restatement tests/smala_ref.py (not float64 LAPACK) and tests/philox_ref.py.

No plan, no likelihood launch: rvm_smala_metric / _derive / _derive_sides / _propose / _accept /
_center_accept, rvm_mh_propose / _accept and rvm_fd_params get torch tensors; every chain of a launch has
a different matrix, so a wrong [(i P + j) C + c] index cannot hide.

Tolerances (smala_ref.tolerances; derived, not tuned on the kernel): an orthogonal-similarity
eigen-solver perturbs eigenvalues by O(P u ||A||), u = 2^-53, so G gets 4 P u max|G_ref| and G^-1,
L L^T, L, log det and mu - x get 4 P u cond relative (floor 4 P u).  mu is stored as x + drift, so
mu - x carries the half-ulp of that sum on top: u max|mu|.  Each comparison prints its largest
error / tolerance ("RATIO ..." lines, pytest -s).
"""
import ctypes as C

import numpy as np
import pytest

import philox_ref
import smala_ref as R
from support import rvm_lib as _lib, to_device as _dev, torch_or_fail as _torch

pytestmark = pytest.mark.gpu

EPS = R.EPS
KEYS = ("lp", "grad", "mu", "L", "G", "logdet", "ok")


def _new_cache(P, n, chains=None):
    """A device cache of n chains, poisoned (NaN, ok = -1) or filled from per-chain dicts
    (lp, grad [P], mu [P], L [P][P], G [P][P], logdet, ok)."""
    torch = _torch()
    _lib_, _ = _lib()
    if chains is None:
        host = dict(lp=np.full(n, np.nan), grad=np.full((P, n), np.nan), mu=np.full((P, n), np.nan),
                    L=np.full((P * P, n), np.nan), G=np.full((P * P, n), np.nan), logdet=np.full(n, np.nan),
                    ok=np.full(n, -1, dtype=np.int32))
    else:
        assert len(chains) == n
        host = dict(lp=np.array([c["lp"] for c in chains], dtype=np.float64),
                    grad=np.stack([c["grad"] for c in chains], 1), mu=np.stack([c["mu"] for c in chains], 1),
                    L=np.stack([np.asarray(c["L"]).reshape(P * P) for c in chains], 1),
                    G=np.stack([np.asarray(c["G"]).reshape(P * P) for c in chains], 1),
                    logdet=np.array([c["logdet"] for c in chains], dtype=np.float64),
                    ok=np.array([c["ok"] for c in chains], dtype=np.int32))
    d = {k: _dev(host[k], np.int32 if k == "ok" else np.float64) for k in KEYS}
    d["_c"] = _lib_.SmalaCache(*[d[k].data_ptr() for k in KEYS])
    return d


def _read(cache):
    _torch().cuda.synchronize()
    return {k: cache[k].cpu().numpy() for k in KEYS}


def _chain(out, P, c):
    return dict(lp=out["lp"][c], grad=out["grad"][:, c], mu=out["mu"][:, c], L=out["L"][:, c].reshape(P, P),
                G=out["G"][:, c].reshape(P, P), logdet=out["logdet"][c], ok=out["ok"][c])


def _run_metric(P, x, lp, status, grad, hess, alpha, eps=EPS):
    """x, grad [C][P], hess [C][P][P] (host, chain-major) -> the cache rvm_smala_metric writes."""
    _lib_, lib = _lib()
    n = len(lp)
    xd, gd = _dev(np.asarray(x).T), _dev(np.asarray(grad).T)
    hd = _dev(np.asarray(hess).reshape(n, P * P).T)
    lpd, std = _dev(lp, np.float64), _dev(status, np.int32)
    out = _new_cache(P, n)
    _lib_.check(lib.rvm_smala_metric(P, n, xd.data_ptr(), lpd.data_ptr(), std.data_ptr(), gd.data_ptr(),
                                     hd.data_ptr(), float(alpha), float(eps), C.byref(out["_c"]),
                                     _lib_.stream_handle()), "rvm_smala_metric")
    return _read(out)


def _metric_ratios(got, ref, P):
    """Largest error / tolerance of one chain's metric outputs against a smala_ref.metric_ref result,
    after the exact-structure checks (L lower-triangular, G symmetric)."""
    G, L = got["G"], got["L"]
    np.testing.assert_array_equal(L, np.tril(L))
    np.testing.assert_array_equal(G, G.T)
    tol_g, tol_r = R.tolerances(P, ref["cond"])
    amax = lambda a: float(np.abs(a).max())  # noqa: E731
    drift_tol = tol_r * amax(ref["drift"]) + R.U * amax(ref["mu"])
    return dict(
        G=amax(G - ref["G"]) / (tol_g * amax(ref["G"])),
        LLt=amax(L @ L.T - ref["Ginv"]) / (tol_r * amax(ref["Ginv"])),
        L=amax(L - ref["L"]) / (tol_r * amax(ref["L"])),
        mu=amax((got["mu"] - ref["x"]) - ref["drift"]) / drift_tol,
        logdet=abs(got["logdet"] - ref["logdet"]) / (tol_r * max(1.0, abs(ref["logdet"]))))


def _assert_ratios(ratios, tag, misses=None):
    """Print the ratios, then assert them (or, given a list, note the miss there for one assertion
    after every chain of the launch has been compared and printed)."""
    print(f"\nRATIO {tag} " + " ".join(f"{k}={v:.3g}" for k, v in ratios.items()), flush=True)
    good = all(np.isfinite(v) and v <= 1.0 for v in ratios.values())
    if misses is not None and not good:
        misses.append((tag, {k: float(f"{v:.3g}") for k, v in ratios.items() if not v <= 1.0}))
    else:
        assert good, (tag, ratios)


# ---- a. rvm_smala_metric vs the 40-digit reference ----------------------------------------------


@pytest.mark.parametrize("alpha", [1.0, 1e3])
@pytest.mark.parametrize("P", [1, 2, 3, 5, 19, 20])
def test_metric_matches_reference(P, alpha):
    """Measured on an MI355X: every family and size sits at 0 to 0.6 of its tolerance.  (Before the
    solver brought its eigenvectors back to unit length, graded_wide at P = 20, alpha = 1 missed G's
    bound at 1.08: rotations with a tangent below sqrt(ulp) only ever stretch Q's columns, and 12 sweeps
    had raised their squared norms by 98 u.  It now sits at 0.16.)"""
    cases = [(n, A) for n, A, alphas, _ in R.metric_cases(P) if alpha in alphas]
    limits = {n: lim for n, _, _, lim in R.metric_cases(P)}
    n = len(cases)
    assert n == 9  # every generic family and this alpha's graded one; neither a power of two nor the wave
    refs = [R.case_ref(P, name, alpha) for name, _ in cases]
    x = np.stack([r["x"] for r in refs])
    lp = np.array([r["lp"] for r in refs])
    grad = np.stack([r["grad"] for r in refs])
    out = _run_metric(P, x, lp, np.zeros(n, np.int32), grad, np.stack([-A for _, A in cases]), alpha)
    assert (out["ok"] == 1).all(), out["ok"]
    np.testing.assert_array_equal(out["lp"], lp)      # passed through bit-exact
    np.testing.assert_array_equal(out["grad"], grad.T)
    misses = []
    for c, (name, _) in enumerate(cases):
        ref = refs[c]
        assert ref["cond"] <= limits[name] and ref["pivot"] > 1e-6, (name, ref["cond"], ref["pivot"])
        _assert_ratios(_metric_ratios(_chain(out, P, c), ref, P), f"3a {name} P={P} alpha={alpha:g}", misses)
    assert not misses, misses


# ---- b. the ok flags of rvm_smala_metric --------------------------------------------------------


def _flag_inputs(P=5, alpha=1e3):
    names = R.GENERIC[:7]
    refs = [R.case_ref(P, n, alpha) for n in names]
    return dict(P=P, alpha=alpha, x=np.stack([r["x"] for r in refs]), lp=np.array([r["lp"] for r in refs]),
                grad=np.stack([r["grad"] for r in refs]), hess=np.stack([-r["A"] for r in refs]),
                status=np.zeros(len(names), np.int32))


@pytest.mark.parametrize("bad", ["status", "lp_neg_inf", "lp_nan", "grad_nan", "hess_inf"])
def test_metric_flags_a_bad_chain_and_leaves_its_neighbours_alone(bad):
    a = _flag_inputs()
    P, k = a["P"], 3
    keep = [c for c in range(len(a["lp"])) if c != k]
    b = {key: (v.copy() if isinstance(v, np.ndarray) else v) for key, v in a.items()}
    if bad == "status":
        b["status"][k] = 2
    elif bad == "lp_neg_inf":
        b["lp"][k] = -np.inf
    elif bad == "lp_nan":
        b["lp"][k] = np.nan
    elif bad == "grad_nan":
        b["grad"][k, P - 1] = np.nan
    else:
        b["hess"][k, 1, 2] = np.inf
    with_bad = _run_metric(P, b["x"], b["lp"], b["status"], b["grad"], b["hess"], b["alpha"])
    without = _run_metric(P, a["x"][keep], a["lp"][keep], a["status"][keep], a["grad"][keep], a["hess"][keep],
                          a["alpha"])
    assert with_bad["ok"][k] == 0
    assert (with_bad["ok"][keep] == 1).all() and (without["ok"] == 1).all()
    for key in KEYS:  # the neighbours to the bit, against a launch that does not contain the bad chain
        np.testing.assert_array_equal(with_bad[key][..., keep], without[key], err_msg=key)


def test_metric_on_a_matrix_whose_squares_overflow():
    """-H scaled by 1e200: the convergence test's sums of squares are inf.  The chain must either be
    flagged (ok = 0) or be right within the tolerances of (a); its neighbours are right either way.
    (Before the solver checked its sums for finiteness it left after zero sweeps with ok = 1 and a G
    1e14 tolerances off; it now reports ok = 0.)"""
    a = _flag_inputs(alpha=1.0)
    P, k = a["P"], 0  # the random SPD matrix
    a["hess"][k] *= 1e200
    out = _run_metric(P, a["x"], a["lp"], a["status"], a["grad"], a["hess"], a["alpha"])
    assert (np.delete(out["ok"], k) == 1).all()
    for c in range(1, len(a["lp"])):
        ref = R.case_ref(P, R.GENERIC[c], a["alpha"])
        _assert_ratios(_metric_ratios(_chain(out, P, c), ref, P), f"3b neighbour {R.GENERIC[c]}")
    print(f"RATIO 3b 1e200 ok={out['ok'][k]}", flush=True)
    if out["ok"][k] != 0:
        ref = R.metric_ref(a["x"][k], a["lp"][k], a["grad"][k], a["hess"][k], a["alpha"], EPS)
        _assert_ratios(_metric_ratios(_chain(out, P, k), ref, P), "3b 1e200")


# ---- c. rvm_smala_derive / rvm_smala_derive_sides on a synthetic stencil -------------------------

REL, NPOINTS, ALPHA_D = 1e-6, 100.0, 1e3


def _stencil(P, n_obs, n):
    """A synthetic central-difference stencil of n chains: x on both sides of the step's floor, random
    logp, model RVs at the 1e-4 scale, per-epoch weights."""
    rng = np.random.default_rng(1000 * P + n_obs)
    S = 2 * P + 1
    floor_ = np.full(P, 0.5)
    x = rng.uniform(0.05, 2.0, (P, n)) * np.where(rng.random((P, n)) < 0.5, -1.0, 1.0)
    x[0, 0], x[P - 1, n - 1] = 0.1, -1.7  # both branches of max(|x_p|, floor_p), whatever the draw
    return dict(P=P, n_obs=n_obs, n=n, floor=floor_, x=x, lp=10.0 * rng.standard_normal((S, n)),
                status=np.zeros((S, n), np.int32), rv=1e-4 * rng.standard_normal((n_obs, S, n)),
                w=1e-3 * rng.uniform(0.5, 2.0, n_obs))


def _run_derive(s, sides=False, lp=None, status=None):
    _lib_, lib = _lib()
    P, n, n_obs = s["P"], s["n"], s["n_obs"]
    xd, fd = _dev(s["x"]), _dev(s["floor"])
    lpd = _dev(s["lp"] if lp is None else lp)
    std = _dev(s["status"] if status is None else status, np.int32)
    rvd, wd = _dev(s["rv"]), _dev(s["w"])
    out = _new_cache(P, n)
    fn = lib.rvm_smala_derive_sides if sides else lib.rvm_smala_derive
    _lib_.check(fn(P, n, n_obs, xd.data_ptr(), REL, fd.data_ptr(), lpd.data_ptr(), std.data_ptr(),
                   rvd.data_ptr() if n_obs else None, wd.data_ptr() if n_obs else None, NPOINTS, ALPHA_D, EPS,
                   C.byref(out["_c"]), _lib_.stream_handle()), "rvm_smala_derive")
    return _read(out)


@pytest.mark.parametrize("n_obs", [0, 1, 63, 64, 65, 128, 130])
@pytest.mark.parametrize("P", [1, 3, 10, 20])
def test_derive_matches_reference_pipeline(P, n_obs):
    n = 7 if P <= 10 else 3
    s = _stencil(P, n_obs, n)
    ax = np.abs(s["x"])
    assert (ax > 0.5).any() and (ax < 0.5).any()
    out = _run_derive(s)
    assert (out["ok"] == 1).all()
    np.testing.assert_array_equal(out["lp"], s["lp"][0])
    # the other entry point: same bits apart from lp and ok, and the centre row is not read
    lp_poison = s["lp"].copy()
    lp_poison[0] = np.nan
    sides = _run_derive(s, sides=True, lp=lp_poison)
    assert (sides["ok"] == 1).all() and (sides["lp"] == 0.0).all()
    for key in ("grad", "mu", "L", "G", "logdet"):
        np.testing.assert_array_equal(sides[key], out[key], err_msg=key)
    for c in range(n):
        den = R.fd_den(s["x"][:, c], s["floor"], REL)
        grad = (s["lp"][1::2, c] - s["lp"][2::2, c]) / den
        np.testing.assert_array_equal(out["grad"][:, c], grad)  # bit for bit
        # the reference pipeline on gauss_newton's H in two links: the float64 sum of the same terms is
        # within its own rounding bound of it (entry by entry), and the kernel's metric is within the
        # tolerances of (a) of the pipeline on that sum.  ((a) bounds the eigen-solver for a given matrix;
        # at P = 1, where no solver runs, the 130-term sum's rounding alone is 1.4 times (a)'s 4 u.)
        H = R.gauss_newton(s["rv"][:, :, c], s["w"], den, NPOINTS)
        H64 = R.gauss_newton_f64(s["rv"][:, :, c], s["w"], den, NPOINTS)
        Hm = np.array([[float(H[i, j]) for j in range(P)] for i in range(P)])
        d = np.sqrt(-np.diag(Hm))
        assert (np.abs(H64 - Hm) <= R.gauss_newton_rounding(n_obs) * np.outer(d, d) + 1e-300).all()
        ref = R.metric_ref(s["x"][:, c], s["lp"][0, c], grad, H64, ALPHA_D, EPS)
        assert ref["cond"] <= R.COND_GRADED and ref["pivot"] > 1e-6, (ref["cond"], ref["pivot"])
        got = _chain(out, P, c)
        if n_obs < P:  # rank-deficient: the null space takes the 1/alpha branch
            assert (np.abs(ref["lam"]) < 1e-12 * np.abs(ref["lam"]).max() + 1e-300).sum() == P - n_obs
            assert np.isclose(ref["lam_twig"].min(), 1.0 / ALPHA_D, rtol=1e-15)
        if n_obs == 0:
            np.testing.assert_array_equal(got["G"], np.eye(P) / ALPHA_D)
        _assert_ratios(_metric_ratios(got, ref, P), f"3c P={P} n_obs={n_obs} chain={c} cond={ref['cond']:.3g}")


def test_derive_status_rows():
    """A non-zero status at a side point: ok = 0 from both entry points.  At the centre: ok = 0 from
    rvm_smala_derive; rvm_smala_derive_sides does not read that row."""
    s = _stencil(3, 65, 7)
    base = _run_derive(s)
    st = s["status"].copy()
    st[2, 1] = 2      # x - e_0 of chain 1
    st[6, 5] = 4      # x - e_2 (the last row) of chain 5
    st[0, 2] = 1      # the centre of chain 2
    lp_poison = s["lp"].copy()
    lp_poison[0] = np.nan
    full = _run_derive(s, status=st)
    sides = _run_derive(s, sides=True, lp=lp_poison, status=st)
    np.testing.assert_array_equal(full["ok"], [1, 0, 0, 1, 1, 0, 1])
    np.testing.assert_array_equal(sides["ok"], [1, 0, 1, 1, 1, 0, 1])
    for key in ("grad", "mu", "L", "G", "logdet"):  # the flags change nothing else
        np.testing.assert_array_equal(full[key], base[key], err_msg=key)
        np.testing.assert_array_equal(sides[key], base[key], err_msg=key)


# ---- d. rvm_smala_propose / _accept / _center_accept on synthetic caches --------------------------


def _accept_launch(a, P, cur_chains, prop_chains, center=None, counters=True, xs=None):
    """One accept launch on fresh device copies; returns x, the current cache, accepted, failures."""
    torch = _torch()
    _lib_, lib = _lib()
    n = len(cur_chains)
    x = _dev(a["x"].T)
    xsd = _dev((a["xs"] if xs is None else xs).T)
    cur, prop = _new_cache(P, n, cur_chains), _new_cache(P, n, prop_chains)
    u = _dev(a["u"])
    acc = torch.zeros(n, dtype=torch.int32, device="cuda")
    fail = torch.zeros(n, dtype=torch.int32, device="cuda")
    ap, fp = (acc.data_ptr(), fail.data_ptr()) if counters else (None, None)
    if center is None:
        _lib_.check(lib.rvm_smala_accept(P, n, 0, x.data_ptr(), C.byref(cur["_c"]), xsd.data_ptr(),
                                         C.byref(prop["_c"]), EPS, 1, 0, u.data_ptr(), ap, fp,
                                         _lib_.stream_handle()), "rvm_smala_accept")
    else:
        lpc, stc = _dev(center[0], np.float64), _dev(center[1], np.int32)
        _lib_.check(lib.rvm_smala_center_accept(P, n, 0, x.data_ptr(), xsd.data_ptr(), lpc.data_ptr(),
                                                stc.data_ptr(), C.byref(cur["_c"]), C.byref(prop["_c"]), EPS, 1, 0,
                                                u.data_ptr(), ap, fp, _lib_.stream_handle()),
                    "rvm_smala_center_accept")
    torch.cuda.synchronize()
    return x.cpu().numpy().T, _read(cur), acc.cpu().numpy(), fail.cpu().numpy()


def _assert_accept_state(a, P, cur_chains, prop_chains, decided, x, cur):
    """Accepted chains: x and every cache entry of cur are prop's bit for bit; rejected: unchanged."""
    for c, yes in enumerate(decided):
        src = prop_chains[c] if yes else cur_chains[c]
        np.testing.assert_array_equal(x[c], a["xs"][c] if yes else a["x"][c], err_msg=f"x of chain {c}")
        got = _chain(cur, P, c)
        for key in KEYS:
            np.testing.assert_array_equal(got[key], src[key], err_msg=f"{key} of chain {c}")


@pytest.mark.parametrize("P", [1, 3, 20])
def test_propose_with_injected_draws(P):
    _lib_, lib = _lib()
    a = R.accept_cases(P)
    n = R.ACCEPT_CHAINS
    chains = [dict(c) for c in a["cur"]]
    chains[2]["ok"] = 0  # no usable metric: the chain proposes x itself
    cur = _new_cache(P, n, chains)
    x, z = _dev(a["x"].T), _dev(a["z"].T)
    xs = _dev(np.full((P, n), np.nan))
    _lib_.check(lib.rvm_smala_propose(P, n, 0, x.data_ptr(), C.byref(cur["_c"]), EPS, 1, 0, z.data_ptr(),
                                      xs.data_ptr(), _lib_.stream_handle()), "rvm_smala_propose")
    _torch().cuda.synchronize()
    got = xs.cpu().numpy().T
    for c in range(n):
        if c == 2:
            np.testing.assert_array_equal(got[c], a["x"][c])
        else:
            np.testing.assert_allclose(got[c], chains[c]["mu"] + EPS * chains[c]["L"] @ a["z"][c], rtol=1e-13,
                                       atol=0)


@pytest.mark.parametrize("P", [1, 3, 20])
def test_accept_decisions_and_cache_copy(P):
    a = R.accept_cases(P)
    n = R.ACCEPT_CHAINS
    want = a["accept"]
    assert want.any() and not want.all()  # both outcomes (and no ties: test_smala_ref_cpu.py)
    x, cur, acc, fail = _accept_launch(a, P, a["cur"], a["prop"])
    np.testing.assert_array_equal(acc, want.astype(np.int32))
    np.testing.assert_array_equal(fail, 0)
    _assert_accept_state(a, P, a["cur"], a["prop"], want, x, cur)
    # null counters
    x0, cur0, _, _ = _accept_launch(a, P, a["cur"], a["prop"], counters=False)
    np.testing.assert_array_equal(x0, x)
    for key in KEYS:
        np.testing.assert_array_equal(cur0[key], cur[key])
    # the centre's logp and status arrive separately: same decisions, same state
    poisoned = [dict(c, lp=np.nan) for c in a["prop"]]
    lpc = np.array([c["lp"] for c in a["prop"]])
    xc, curc, accc, failc = _accept_launch(a, P, a["cur"], poisoned, center=(lpc, np.zeros(n, np.int32)))
    np.testing.assert_array_equal(accc, acc)
    np.testing.assert_array_equal(failc, 0)
    _assert_accept_state(a, P, a["cur"], a["prop"], want, xc, curc)
    # a non-zero centre status rejects
    yes = int(np.nonzero(want)[0][0])
    stc = np.zeros(n, np.int32)
    stc[yes] = 2
    xr, curr, accr, _ = _accept_launch(a, P, a["cur"], poisoned, center=(lpc, stc))
    decided = want.copy()
    decided[yes] = False
    np.testing.assert_array_equal(accr, decided.astype(np.int32))
    _assert_accept_state(a, P, a["cur"], a["prop"], decided, xr, curr)


@pytest.mark.parametrize("P", [1, 3, 20])
def test_accept_rejections_and_failure_counts(P):
    """Chains that would accept, spoiled one way each: the proposal's metric failed with a finite logp
    (failures += 1), its logp is -inf or NaN (rejected, not a failure, with or without a metric), or the
    current cache is not usable."""
    a = R.accept_cases(P)
    yes = np.nonzero(a["accept"])[0]
    assert len(yes) >= 4
    cur = [dict(c) for c in a["cur"]]
    prop = [dict(c) for c in a["prop"]]
    prop[yes[0]]["ok"] = 0
    prop[yes[1]]["lp"] = -np.inf
    prop[yes[2]]["lp"] = np.nan
    prop[yes[2]]["ok"] = 0
    cur[yes[3]]["ok"] = 0
    decided = a["accept"].copy()
    decided[yes[:4]] = False
    x, curo, acc, fail = _accept_launch(a, P, cur, prop)
    np.testing.assert_array_equal(acc, decided.astype(np.int32))
    want_fail = np.zeros(len(cur), np.int32)
    want_fail[yes[0]] = 1
    np.testing.assert_array_equal(fail, want_fail)
    _assert_accept_state(a, P, cur, prop, decided, x, curo)


# ---- e. the device's own Gaussians and accept uniforms vs philox_ref ------------------------------

SEED, BEGIN, ITER, NCH = (1 << 40) + 12345, (1 << 32) - 3, (1 << 32) + 5, 8  # chains straddle 2^32


def _normals(stream, P):
    return np.array([[philox_ref.normal(SEED, BEGIN + c, ITER, stream, p) for c in range(NCH)] for p in range(P)])


def test_smala_propose_draws_match_philox_restatement():
    _lib_, lib = _lib()
    P = 20
    eye = dict(lp=0.0, grad=np.zeros(P), mu=np.zeros(P), L=np.eye(P), G=np.eye(P), logdet=0.0, ok=1)
    cur = _new_cache(P, NCH, [eye] * NCH)
    x = _dev(np.zeros((P, NCH)))
    xs = _dev(np.full((P, NCH), np.nan))
    _lib_.check(lib.rvm_smala_propose(P, NCH, BEGIN, x.data_ptr(), C.byref(cur["_c"]), 1.0, SEED, ITER, None,
                                      xs.data_ptr(), _lib_.stream_handle()), "rvm_smala_propose")
    _torch().cuda.synchronize()
    np.testing.assert_allclose(xs.cpu().numpy(), _normals(philox_ref.RNG_SMALA_PROPOSE, P), rtol=1e-14, atol=1e-15)


def test_mh_propose_draws_match_philox_restatement():
    _lib_, lib = _lib()
    P = 28  # four inclined planets
    x, sc = _dev(np.zeros((P, NCH))), _dev(np.ones(P))
    q = _dev(np.full((P, NCH), np.nan))
    _lib_.check(lib.rvm_mh_propose(P, NCH, BEGIN, x.data_ptr(), sc.data_ptr(), 1.0, SEED, ITER, None, q.data_ptr(),
                                   _lib_.stream_handle()), "rvm_mh_propose")
    _torch().cuda.synchronize()
    np.testing.assert_allclose(q.cpu().numpy(), _normals(philox_ref.RNG_MH_PROPOSE, P), rtol=1e-14, atol=1e-15)


def _bracket(stream):
    """lnp_new = log(u (1 +/- 1e-6)) around the stream's own uniform: + accepts, - rejects."""
    u = np.array([philox_ref.uniform2(SEED, BEGIN + c, ITER, stream)[0] for c in range(NCH)])
    s = np.where(np.arange(NCH) % 2 == 0, 1.0, -1.0)
    return np.log(u * (1.0 + s * 1e-6)), s > 0


def test_mh_accept_uniform_matches_philox_restatement():
    torch = _torch()
    _lib_, lib = _lib()
    P = 3
    lnp_new, want = _bracket(philox_ref.RNG_MH_ACCEPT)
    rng = np.random.default_rng(0)
    x0, q0 = rng.standard_normal((P, NCH)), rng.standard_normal((P, NCH))
    x, q = _dev(x0), _dev(q0)
    lnp, lnew = _dev(np.zeros(NCH)), _dev(lnp_new)
    acc = torch.zeros(NCH, dtype=torch.int32, device="cuda")
    _lib_.check(lib.rvm_mh_accept(P, NCH, BEGIN, x.data_ptr(), lnp.data_ptr(), q.data_ptr(), lnew.data_ptr(), SEED,
                                  ITER, None, acc.data_ptr(), _lib_.stream_handle()), "rvm_mh_accept")
    torch.cuda.synchronize()
    np.testing.assert_array_equal(acc.cpu().numpy(), want.astype(np.int32))
    np.testing.assert_array_equal(x.cpu().numpy(), np.where(want[None], q0, x0))
    np.testing.assert_array_equal(lnp.cpu().numpy(), np.where(want, lnp_new, 0.0))


def test_smala_accept_uniform_matches_philox_restatement():
    """Both caches with one G and one logdet, cur.mu = x and prop.mu = x_prop: the two Mahalanobis terms
    are equal to the bit and the q-ratio cancels, leaving exp(logp* - logp) > u."""
    torch = _torch()
    _lib_, lib = _lib()
    P = 3
    lnp_new, want = _bracket(philox_ref.RNG_SMALA_ACCEPT)
    ref = R.case_ref(P, "spd", 1.0)
    rng = np.random.default_rng(1)
    x0 = rng.standard_normal((NCH, P))
    xs0 = x0 + 0.1 * rng.standard_normal((NCH, P))
    cur = [dict(lp=0.0, grad=ref["grad"], mu=x0[c], L=ref["L"], G=ref["G"], logdet=ref["logdet"], ok=1)
           for c in range(NCH)]
    prop = [dict(lp=lnp_new[c], grad=-ref["grad"], mu=xs0[c], L=ref["L"], G=ref["G"], logdet=ref["logdet"], ok=1)
            for c in range(NCH)]
    curd, propd = _new_cache(P, NCH, cur), _new_cache(P, NCH, prop)
    x, xs = _dev(x0.T), _dev(xs0.T)
    acc = torch.zeros(NCH, dtype=torch.int32, device="cuda")
    _lib_.check(lib.rvm_smala_accept(P, NCH, BEGIN, x.data_ptr(), C.byref(curd["_c"]), xs.data_ptr(),
                                     C.byref(propd["_c"]), EPS, SEED, ITER, None, acc.data_ptr(), None,
                                     _lib_.stream_handle()), "rvm_smala_accept")
    torch.cuda.synchronize()
    np.testing.assert_array_equal(acc.cpu().numpy(), want.astype(np.int32))
    np.testing.assert_array_equal(x.cpu().numpy().T, np.where(want[:, None], xs0, x0))


# ---- f. rvm_fd_params --------------------------------------------------------------------------


@pytest.mark.parametrize("P", [1, 20])
def test_fd_params_bit_exact(P):
    _lib_, lib = _lib()
    n, rel = 5, 1e-6
    rng = np.random.default_rng(P)
    x = rng.uniform(0.05, 2.0, (P, n)) * np.where(rng.random((P, n)) < 0.5, -1.0, 1.0)
    x[0, 1] = 0.0       # the floor branch at its extreme
    x[P - 1, 3] = 1.75  # and the |x| branch
    floor_ = np.full(P, 0.5)
    S = 2 * P + 1
    out = _dev(np.full((P, S * n), np.nan))
    xd, fd = _dev(x), _dev(floor_)
    _lib_.check(lib.rvm_fd_params(P, n, xd.data_ptr(), rel, fd.data_ptr(), out.data_ptr(), _lib_.stream_handle()),
                "rvm_fd_params")
    _torch().cuda.synchronize()
    e = rel * np.maximum(np.abs(x), floor_[:, None])
    want = np.repeat(x[:, None, :], S, axis=1)  # [P][S][n]
    for p in range(P):
        want[p, 1 + 2 * p] = x[p] + e[p]
        want[p, 2 + 2 * p] = x[p] - e[p]
    np.testing.assert_array_equal(out.cpu().numpy(), want.reshape(P, S * n))
