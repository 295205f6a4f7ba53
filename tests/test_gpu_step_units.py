"""Tier U0: the device functions under the likelihood kernel, one call at a time, against mpmath.

rvmcmc/librvm_step_probe.so (csrc/test/rvm_step_probe.hip) calls rvm_device.h's drift, Stumpff and
reciprocal functions, the kicks and rvm_walker.h's walker_setup on arrays of items; tests/step_ref.py
holds the inputs, the 40-digit truth (tests/wh_ref.py on mpf) and the bounds.  Every comparison
appends its largest ratio and the path-class counts to $RVM_STEP_REPORT (JSON lines;
profiles/step_unit_tier.jsonl is one run).
"""
import ctypes as C
import math
import os

import numpy as np
import pytest
from mpmath import mp, mpf

import step_ref as S
from support import report_line, to_device as _dev

pytestmark = pytest.mark.gpu

_dp = C.c_void_p
SIGNATURES = {
    "rvm_probe_drift": [C.c_int] * 6 + [_dp, _dp, _dp, _dp, _dp, C.c_void_p],
    "rvm_probe_stumpff": [C.c_int, _dp, _dp, C.c_void_p],
    "rvm_probe_recip": [C.c_int, _dp, _dp, C.c_void_p],
    "rvm_probe_setup": [C.c_int, C.c_int, C.c_int, _dp, C.c_double, _dp, C.c_void_p],
    "rvm_probe_kick": [C.c_int, C.c_int, C.c_int, _dp, _dp, _dp, C.c_double, _dp, _dp, C.c_void_p],
}


def report(what, **kw):
    report_line("RVM_STEP_REPORT", what, **kw)


@pytest.fixture(scope="module")
def probe():
    import torch

    import rvmcmc

    assert torch.cuda.is_available()
    path = os.path.join(os.path.dirname(os.path.abspath(rvmcmc.__file__)), "librvm_step_probe.so")
    lib = C.CDLL(path)  # (no fallback: a missing probe library is an error)
    for name, args in SIGNATURES.items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = C.c_int, args
    return lib


def _stream():
    from rvmcmc import _lib

    return _lib.stream_handle()


def run_drift(probe, variant, X, enc=None, np_=1):
    """X [n][8] -> (out [n][8] = rx ry rz vx vy vz r ir, bad [n], path [n])."""
    import torch

    nt, mode, d3, kg = variant
    n = len(X)
    xin = _dev(X.T, np.float64)
    e = _dev(np.zeros(n, np.int32) if enc is None else enc, np.int32)
    out = torch.full((8, n), float("nan"), dtype=torch.float64, device="cuda")
    bad = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    path = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    rc = probe.rvm_probe_drift(nt, mode, d3, kg, np_, n, xin.data_ptr(), e.data_ptr(), out.data_ptr(), bad.data_ptr(),
                               path.data_ptr(), _stream())
    assert rc == 0, (variant, rc)
    torch.cuda.synchronize()
    return out.cpu().numpy().T.copy(), bad.cpu().numpy(), path.cpu().numpy()


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def same_bits(a, b):
    return bits(a) == bits(b)


@pytest.fixture(scope="module")
def drift_base(probe):
    """Every instantiation on the batch as generated (planar instantiations: the planar items)."""
    p = S.drift_problem()
    runs = {}
    for v in S.SHIPPED + S.VARIANT_BUILDS:
        X = p["x"] if v[2] else p["x"][:p["n_planar"]]
        runs[v] = run_drift(probe, v, X)
    return runs


def class_counts(path):
    return [int((path == k).sum()) for k in range(8)]


# ---------------------------------------------------------------------------------------------
# drift
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", S.SHIPPED + S.VARIANT_BUILDS, ids=S.variant_name)
def test_drift_accuracy_and_coverage(drift_base, variant):
    """Every item's rx .. vz, r, ir within K_DRIFT u (|y|_block + sum |dy/dx| |x|) of the truth (the
    ungated drift: the items it does not flag), and every path class the instantiation can reach
    holds at least 32 items by the device's own codes."""
    p = S.drift_problem()
    out, bad, path = drift_base[variant]
    n = len(out)
    counts = class_counts(path)
    assert sum(counts) == n and set(np.unique(bad)) <= {0, 1}
    sel = None
    if variant[1] == 0:
        # the ungated verdict is the first Halley test's (no item is flagged as encountered here)
        assert ((bad == 0) == (path == S.FIRST)).all()
        sel = bad == 0
    else:
        assert (bad == 0).all()
    r = S.max_ratio(out, p["truth"][:n], p["scale"][:n], sel)
    per_class = {S.PATH_NAMES[k]: float(r[path == k].max(initial=0.0)) for k in range(8)}
    worst = int(r.max(1).argmax())
    report("drift", variant=S.variant_name(variant), K=S.K_DRIFT, max_ratio=float(r.max()), max_ratio_per_class=per_class,
           class_counts=dict(zip(S.PATH_NAMES, counts)), items=n, compared=int(n if sel is None else sel.sum()),
           worst_item=worst, worst_x=p["x"][worst].tolist())
    print(S.variant_name(variant), "max ratio", r.max(), "K", S.K_DRIFT, per_class, dict(zip(S.PATH_NAMES, counts)))
    for k in S.reachable(variant[1]):
        assert counts[k] >= S.MIN_CLASS, (S.PATH_NAMES[k], counts)
    if S.acc_of(variant[1]) not in (1, 2, 4):
        assert counts[S.ZAWARE] == 0 and counts[S.TAYLOR] == 0
    assert r.max() <= S.K_DRIFT, (worst, p["x"][worst].tolist(), S.PATH_NAMES[path[worst]], r[worst].tolist())


def test_drift_bit_identities(drift_base):
    """rvm_device.h: "good lanes compute bit-identical states either way" (ungated against gated),
    "ACC 3 gives exactly ACC 0's bits" (and ACC 4 ACC 1's; ACC 2 is ACC 1), and an inclined
    instantiation on a planar state is the planar one."""
    n_planar = S.drift_problem()["n_planar"]
    checked = 0
    for nt in (6, 7, 8):
        for d3 in (0, 1):
            ung, g0, g3 = (drift_base[(nt, m, d3, 0)] for m in (0, 1, 4))
            good = ung[1] == 0
            assert good.sum() >= S.MIN_CLASS
            assert same_bits(ung[0], g0[0])[good].all(), (nt, d3)
            assert same_bits(g3[0], g0[0]).all(), (nt, d3)
            assert (g3[2] == g0[2]).all() and (ung[2] == g0[2]).all()
            checked += 2
        for m in (0, 1, 4):  # D3 with rz = vz = 0 against planar (whose rz, vz are not computed: 0)
            a, b = drift_base[(nt, m, 0, 0)], drift_base[(nt, m, 1, 0)]
            inplane = [0, 1, 3, 4, 6, 7]
            assert same_bits(a[0][:, inplane], b[0][:n_planar, inplane]).all(), (nt, m)
            solved = np.isfinite(a[0][:, 0])  # (the ungated drift leaves a flagged lane's values as they fall)
            assert (solved | (a[1] == 1)).all() and (b[0][:n_planar, [2, 5]][solved] == 0.0).all(), (nt, m)
            assert (a[1] == b[1][:n_planar]).all() and (a[2] == b[2][:n_planar]).all()
        a1, a2, a4 = (drift_base[(nt, m, 0, 0)] for m in (2, 3, 5))
        assert same_bits(a2[0], a1[0]).all() and same_bits(a4[0], a1[0]).all(), nt
        assert (a2[2] == a1[2]).all() and (a4[2] == a1[2]).all()
        k0, k3 = drift_base[(nt, 1, 0, 1)], drift_base[(nt, 4, 0, 1)]
        assert same_bits(k3[0], k0[0]).all(), nt
    report("drift_bit_identities", pairs=checked)


@pytest.mark.parametrize("variant", S.SHIPPED + S.VARIANT_BUILDS, ids=S.variant_name)
def test_drift_lane_independence(probe, drift_base, variant):
    """rvm_device.h: "a walker's result never depends on the other lanes of the wave": the batch as
    generated, reversed, and every item that is not FIRST alone in a wave of FIRST items."""
    p = S.drift_problem()
    out, bad, path = drift_base[variant]
    n = len(out)
    X = p["x"][:n]
    rev = np.arange(n)[::-1]
    first = np.flatnonzero(path == S.FIRST)
    rest = np.flatnonzero(path != S.FIRST)
    alone = first[(np.arange(len(rest))[:, None] * 63 + np.arange(64)[None, :]) % len(first)]
    alone[np.arange(len(rest)), rest % 64] = rest
    for name, idx in (("reversed", rev), ("alone", alone.ravel())):
        o, b, q = run_drift(probe, variant, X[idx])
        assert same_bits(o, out[idx]).all(), (name, np.flatnonzero(~same_bits(o, out[idx]).all(1))[:5])
        assert (b == bad[idx]).all() and (q == path[idx]).all(), name
    report("drift_lane_independence", variant=S.variant_name(variant), alone_waves=int(len(rest)))


@pytest.mark.parametrize("mode", [0, 1, 4], ids=["ungated", "acc0", "acc3"])
def test_encountered_walker_changes_no_other_walker(probe, mode):
    """Two lanes per walker (NP = 2): flagging a walker as encountered leaves every other walker's bits
    alone; the flagged walker's lanes keep the first Halley step's update and raise no verdict."""
    p = S.drift_problem()
    X = p["x"][:p["n_planar"] & ~1]
    n = len(X)
    v = (6, mode, 0, 0)
    base = run_drift(probe, v, X, np_=2)
    one = run_drift(probe, (6, mode, 0, 0), X)  # one lane per walker: the same items
    assert same_bits(base[0], one[0]).all() and (base[2] == one[2]).all()
    enc = np.zeros(n, np.int32)
    walkers = np.arange(0, n // 2, 3)
    enc[2 * walkers + walkers % 2] = 1  # one item of every third walker, either lane in turn
    flagged = np.zeros(n, bool)
    flagged[2 * walkers] = flagged[2 * walkers + 1] = True
    assert (base[2][flagged] != S.FIRST).sum() >= S.MIN_CLASS  # walkers that would have gone to a second solve
    got = run_drift(probe, v, X, enc=enc, np_=2)
    assert same_bits(got[0], base[0])[~flagged].all()
    assert (got[1] == base[1])[~flagged].all() and (got[2] == base[2]).all()
    assert (got[1][flagged] == 0).all()
    first_step = run_drift(probe, (6, 0, 0, 0), X)[0]  # the ungated drift applies the first step on every lane
    assert same_bits(got[0], first_step)[flagged].all()
    report("drift_encounter_mask", mode=mode, walkers_flagged=int(len(walkers)))


# ---------------------------------------------------------------------------------------------
# stumpff, recip
# ---------------------------------------------------------------------------------------------
def test_stumpff(probe):
    """stumpff23<6/7/8> on |z| <= B(NT) within STUMPFF23_BOUND u of the truth, its two overloads the
    same bits; stumpff_full on [-40, 40] within STUMPFF_FULL_BOUND u of the majorant c_k(-|z|)."""
    import torch

    sp = S.stumpff_problem()
    z = sp["z"]
    n = len(z)
    out = torch.full((16, n), float("nan"), dtype=torch.float64, device="cuda")
    zd = _dev(z)
    assert probe.rvm_probe_stumpff(n, zd.data_ptr(), out.data_ptr(), _stream()) == 0
    torch.cuda.synchronize()
    o = out.cpu().numpy()
    res = {}
    with mp.workdps(S.DPS):
        for j, nt in enumerate((6, 7, 8)):
            assert same_bits(o[4 * j], o[4 * j + 2]).all() and same_bits(o[4 * j + 1], o[4 * j + 3]).all(), nt
            inb = np.abs(z) <= S.STUMPFF_B[nt]
            assert inb.sum() > 400
            for k in (2, 3):
                e = S.rel_err_u(o[4 * j + k - 2][inb], [t[k] for t, b in zip(sp["truth"], inb) if b])
                res[f"stumpff23<{nt}> c{k}"] = float(e.max())
        full = np.array([[float(abs(mpf(float(o[12 + k][i])) - sp["truth"][i][k]) / sp["major"][i][k]) / S.U
                          for k in range(4)] for i in range(n)])
    for k in range(4):
        res[f"stumpff_full c{k}"] = float(full[:, k].max())
    report("stumpff", bound23=S.STUMPFF23_BOUND, bound_full=S.STUMPFF_FULL_BOUND, max_err_u=res,
           float_run_full=sp["float_err"].max(0).tolist())
    print(res)
    assert np.isfinite(o).all()
    assert max(v for k, v in res.items() if "23" in k) <= S.STUMPFF23_BOUND, res
    assert full.max() <= S.STUMPFF_FULL_BOUND, (res, z[full.max(1).argmax()])


def test_recip(probe):
    """rcp_nr, rsq_nr, rcube_nr: "limited by rounding" -- within the bounds step_ref derives."""
    import torch

    x = S.recip_items()
    n = len(x)
    out = torch.full((3, n), float("nan"), dtype=torch.float64, device="cuda")
    xd = _dev(x)
    assert probe.rvm_probe_recip(n, xd.data_ptr(), out.data_ptr(), _stream()) == 0
    torch.cuda.synchronize()
    o = out.cpu().numpy()
    truth = S.recip_truth(x)
    with mp.workdps(S.DPS):
        err = [float(S.rel_err_u(o[k], truth[k]).max()) for k in range(3)]
    report("recip", bounds=[S.RCP_BOUND, S.RSQ_BOUND, S.RCUBE_BOUND], max_err_u=err)
    print(err)
    assert err[0] <= S.RCP_BOUND and err[1] <= S.RSQ_BOUND and err[2] <= S.RCUBE_BOUND, err


# ---------------------------------------------------------------------------------------------
# setup, kick
# ---------------------------------------------------------------------------------------------
def _lanes(np_):
    return 1 if np_ == 1 else (2 if np_ == 2 else 4)


@pytest.mark.parametrize("np_,inclined", S.NP_D3)
def test_setup(probe, np_, inclined):
    """walker_setup on every lane: the state, r, ir within K_SETUP of the truth; GM, dmin2 within their
    derived bounds; status exact; e2w one of the values h^2 + k^2 takes in double."""
    import torch

    p = S.setup_problem(np_, inclined)
    W, L, PR = len(p["walkers"]), _lanes(np_), 7 if inclined else 5
    rows = np.array([[wk[q][c] for wk in p["walkers"]] for q in range(np_) for c in range(PR)])
    out = torch.full((12, W * L), float("nan"), dtype=torch.float64, device="cuda")
    rd = _dev(rows)
    assert probe.rvm_probe_setup(np_, int(inclined), W, rd.data_ptr(), S.HILL_FACTOR, out.data_ptr(), _stream()) == 0
    torch.cuda.synchronize()
    o = out.cpu().numpy().reshape(12, W, L)
    worst, wgm, wd2 = 0.0, 0.0, 0.0
    with mp.workdps(S.DPS):
        for w in range(W):
            lo, hi, allv = p["e2w"][w]
            for q in range(L):
                pl = min(q, np_ - 1)  # (3 planets: the fourth lane shadows planet 3)
                y = o[:8, w, q]
                r = S.ratios(y, p["truth"][w][8 * pl:8 * pl + 8], p["scale"][w][8 * pl:8 * pl + 8])
                worst = max(worst, max(r))
                wgm = max(wgm, float(abs(mpf(float(o[8, w, q])) - p["GM"][w][pl]) / p["GM"][w][pl]) / S.U)
                wd2 = max(wd2, float(abs(mpf(float(o[9, w, q])) - p["dmin2"][w]) / p["dmin2"][w]) / S.U)
                assert o[11, w, q] == (1.0 if p["rejected"][w] else 0.0), (w, q)
                assert o[10, w, q] in allv and lo <= o[10, w, q] <= hi, (w, q, o[10, w, q], lo, hi)
    report("setup", np=np_, inclined=inclined, K=S.K_SETUP, max_ratio=worst, GM_err_u=wgm, dmin2_err_u=wd2, walkers=W,
           float_run_max_ratio=float(p["float_ratio"].max()))
    print("setup", np_, inclined, worst, wgm, wd2)
    assert worst <= S.K_SETUP and wgm <= S.GM_BOUND and wd2 <= S.DMIN2_BOUND, (worst, wgm, wd2)


@pytest.mark.parametrize("np_,inclined", S.NP_D3)
def test_kick(probe, np_, inclined):
    """kick (kick2 / kickN / kick_generic by NP), kick_generic and kick_prep + kick_apply (full and
    half) within K_KICK of the truth; the encounter verdicts exact and the same in all four; kick the
    same bits as kick_prep + kick_apply where the header shares the expressions (NP <= 2); star_vx."""
    import torch

    p = S.kick_problem(np_, inclined)
    items = p["items"]
    W, L = len(items), _lanes(np_)
    state = np.zeros((6, W, L))
    for w, (r, v, m, d2) in enumerate(items):
        for q in range(L):
            pl = min(q, np_ - 1)
            state[0:3, w, q], state[3:6, w, q] = r[pl], v[pl]
    mass = np.array([[it[2][q] for it in items] for q in range(np_)])
    dmin2 = np.array([it[3] for it in items])
    out = torch.full((16, W * L), float("nan"), dtype=torch.float64, device="cuda")
    star = torch.full((W * L,), float("nan"), dtype=torch.float64, device="cuda")
    sd, md, dd = _dev(state.reshape(6, -1)), _dev(mass), _dev(dmin2)  # (held until the launch has run)
    rc = probe.rvm_probe_kick(np_, int(inclined), W, sd.data_ptr(), md.data_ptr(), dd.data_ptr(), S.KICK_H, out.data_ptr(),
                              star.data_ptr(), _stream())
    assert rc == 0
    torch.cuda.synchronize()
    o = out.cpu().numpy().reshape(4, 4, W, L)  # [kick, generic, prep + apply, prep + half apply][vx vy vz enc]
    sv = star.cpu().numpy().reshape(W, L)
    worst = [0.0] * 4
    star_worst = 0.0
    with mp.workdps(S.DPS):
        for w in range(W):
            for q in range(L):
                pl = min(q, np_ - 1)
                for k in range(4):
                    truth, sc, _ = p["half" if k == 3 else "full"]
                    r = S.ratios(o[k, :3, w, q], truth[w][3 * pl:3 * pl + 3], sc[w][3 * pl:3 * pl + 3])
                    worst[k] = max(worst[k], max(r))
                    assert (o[k, 3, w, q] != 0.0) == p["enc"][w], (w, q, k, o[k, 3, w, q], p["margin"][w])
                star_worst = max(star_worst, float(abs(mpf(float(sv[w, q])) - p["star"][w])) / p["star_bound"][w])
    report("kick", np=np_, inclined=inclined, K=S.K_KICK, max_ratio=dict(zip(("kick", "kick_generic", "prep_apply", "prep_half"), worst)),
           star_vx_over_bound=star_worst, walkers=W, encounters=int(sum(p["enc"])),
           float_run_max_ratio=float(max(p["full"][2].max(), p["half"][2].max())))
    print("kick", np_, inclined, worst, star_worst)
    assert (o[0, 3] == o[2, 3]).all() and (o[0, 3] == o[3, 3]).all()  # kick's and kick_prep's bits of Lane::encm
    if np_ <= 2:
        assert same_bits(o[0, :3], o[2, :3]).all()
    if np_ == 1:
        assert same_bits(o[0, :3], o[1, :3]).all()  # kick is kick_generic
    assert max(worst) <= S.K_KICK and star_worst <= 1.0, (worst, star_worst)
