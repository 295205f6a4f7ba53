"""Restatement of the stability screen's block rule (include/rvmcmc.h, rvm_stability_init / rvm_stability_advance)
over wh_ref.WH, in ``float`` or ``mpmath.mpf``.

A state is integrated block by block: one block is K(h/2) [D K]^(sample_every - 1) D K(h/2), and at its end, in
this order: 1. a pair came within the exit distance at a kick of the block -> ENCOUNTER, xv and ext as at the
previous block end; 2. some planet's |r|, a or e2 is not finite -> NONFINITE, likewise; 3. ext is updated and xv
stored; 4. some planet's |r| > r_max -> ESCAPE (r_max <= 0: no test).  steps += sample_every in every case.

Elements of a planet from its Jacobi (r, v) and the interior mass GM of its coordinate: v2 = |v|^2,
beta = 2 GM / |r| - v2, a = GM / beta, e2 = 1 - |r x v|^2 beta / GM^2.

The run also records its decision margins: the d^2 / dmin2 closest to 1 over every pair at every kick it
evaluates (the t = 0 check included), and the |r| / r_max closest to 1 over every planet at every block end.  The
cases below are chosen so that both stay outside 1 +- MARGIN: the reference alone decides every status.

tests/golden/make_stability_truth.py writes tests/golden/stability_truth.json from cases() at TRUTH_DPS digits;
FLOAT_ERR holds the float run's own errors against that truth (measured by tests/test_stability_ref_cpu.py):
the GPU tier's bound is FLOOR_FACTOR times them (tests/test_gpu_stability.py).
"""
import json
import math
import os

import numpy as np
from mpmath import mp, mpf

import wh_ref as W

OK, PRIOR, ENCOUNTER, NONFINITE, ESCAPE = 0, 1, 2, 3, 6
TRUTH_DPS = 40
DIGITS = 30
MARGIN = 1e-9
FLOOR_FACTOR = 3.0  # the project's margin for a second double-precision implementation (tiers D0, U0)
KINDS = ("pos", "vel", "a", "e2")
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "stability_truth.json")


def _isfinite(x):
    return math.isfinite(x) if isinstance(x, float) else bool(mp.isfinite(x))


def elements(GM, r, v):
    """(|r|, a, e2) of one Jacobi coordinate."""
    r0 = W.sqrt(r[0] * r[0] + r[1] * r[1] + r[2] * r[2])
    v2 = v[0] * v[0] + v[1] * v[1] + v[2] * v[2]
    beta = 2 * GM / r0 - v2
    a = GM / beta
    hx, hy, hz = r[1] * v[2] - r[2] * v[1], r[2] * v[0] - r[0] * v[2], r[0] * v[1] - r[1] * v[0]
    e2 = 1 - (hx * hx + hy * hy + hz * hz) * beta / (GM * GM)
    return r0, a, e2


class Run:
    """One state's outcome: status, steps, xv [np][6] and ext [np][3] (None unless the state was OK at t = 0),
    enc_ratio / esc_ratio the decision ratios closest to 1 (None: no such test was made)."""

    def __init__(self):
        self.status, self.steps, self.xv, self.ext = OK, 0, None, None
        self.enc_ratio, self.esc_ratio = None, None

    def _near(self, name, ratio):
        cur = getattr(self, name)
        if cur is None or abs(ratio - 1.0) < abs(cur - 1.0):
            setattr(self, name, ratio)


def _pair_ratios(s):
    """d^2 / dmin2 of every pair at the state's positions (wh_ref.WH.kick's own distances)."""
    if s.dmin2 == 0.0:
        return []
    n = s.np
    zero = 0 * s.r[1][0]
    x, cm = [[zero] * 3], [zero] * 3
    for i in range(1, n + 1):
        x.append([s.r[i][c] + cm[c] / s.Mi[i - 1] for c in range(3)])
        cm = [cm[c] + s.m[i] * x[i][c] for c in range(3)]
    return [float(sum((x[j][c] - x[i][c]) ** 2 for c in range(3)) / s.dmin2) for i in range(n + 1)
            for j in range(i + 1, n + 1)]


def run_state(pl, inclined, hill_factor, h, sample_every, n_blocks, r_max, on_block=None):
    """pl [np][7] numbers of one type; h, r_max Python floats.  on_block(run, block index) after every block."""
    out = Run()
    if W.prior_hard(pl, inclined):
        out.status = PRIOR
        return out
    num = W._num(pl[0][1])
    s = W.WH(pl, inclined, hill_factor)

    def kick(step):
        for q in _pair_ratios(s):
            out._near("enc_ratio", q)
        s.kick(step, dry=step is None)

    kick(None)  # the check before the first step
    if s.enc:
        out.status = ENCOUNTER
        return out
    n = s.np
    el = [elements(s.Mi[i], s.r[i], s.v[i]) for i in range(1, n + 1)]
    out.xv = [list(s.r[i]) + list(s.v[i]) for i in range(1, n + 1)]
    out.ext = [[e[1], e[1], e[2]] for e in el]
    hh = num(h)
    cnt = [0, 0]
    for b in range(n_blocks):
        try:
            kick(hh / 2)
            for j in range(sample_every):
                s.drift(hh, cnt)
                kick(hh / 2 if j == sample_every - 1 else hh)
            el = [elements(s.Mi[i], s.r[i], s.v[i]) for i in range(1, n + 1)]
            finite = all(_isfinite(q) for e in el for q in e)
        except (ArithmeticError, ValueError):
            finite = False
        out.steps += sample_every
        if s.enc:
            out.status = ENCOUNTER
        elif not finite:
            out.status = NONFINITE
        else:
            for p, e in enumerate(el):
                out.ext[p] = [min(out.ext[p][0], e[1]), max(out.ext[p][1], e[1]), max(out.ext[p][2], e[2])]
            out.xv = [list(s.r[i]) + list(s.v[i]) for i in range(1, n + 1)]
            if r_max > 0.0:
                for e in el:
                    out._near("esc_ratio", float(e[0] / r_max))
                if any(e[0] > r_max for e in el):
                    out.status = ESCAPE
        if on_block is not None:
            on_block(out, b)
        if out.status != OK:
            break
    return out


def run_case(case, num=float, dps=TRUTH_DPS, states=None):
    """[Run] of the case's states (all, or the listed ones)."""
    with mp.workdps(dps):
        return [run_state(W.to_params(case["states"][i], num), case["inclined"], case["hill"], case["h"],
                          case["sample_every"], case["n_blocks"], case["r_max"])
                for i in (range(len(case["states"])) if states is None else states)]


# ---------------------------------------------------------------------------------------------
# cases (tests/golden/stability_truth.json)
# ---------------------------------------------------------------------------------------------
N_STATES = 5  # not a multiple of 64 / L for any lane packing
H20 = 2.0 * math.pi / 20.0
ENCOUNTER_PLANETS = [{"m": 1e-3, "a": 1.0, "l": 0.0}, {"m": 1e-3, "a": 1.25, "l": 1.0}]
ESCAPE_PLANETS = [{"m": 1e-3, "a": 1.0, "k": 0.3, "l": 0.0}, {"m": 2e-3, "a": 2.5, "h": 0.3, "l": 2.0}]
QUIET3_INCLINED = [{"m": 3e-4, "a": 1.0, "h": 0.02, "k": 0.01, "l": 0.4, "ix": 0.05, "iy": -0.02},
                   {"m": 5e-4, "a": 1.9, "h": -0.03, "k": 0.02, "l": 2.1, "ix": -0.03, "iy": 0.04},
                   {"m": 2e-4, "a": 3.4, "h": 0.01, "k": -0.04, "l": 4.4, "ix": 0.02, "iy": 0.06}]
THREE_INCLINED = W.S2_INCLINED + [dict(W.EXTRA_PLANETS[0], ix=-0.05, iy=0.07)]


def _states(planets, rel, seed):
    """The nominal state and N_STATES - 1 of a ball of relative width rel around it."""
    base = W.pal_rows(planets)
    return [base] + W._ball(base, N_STATES - 1, rel, seed)


def cases():
    """{name: dict(states [n][np][7], inclined, hill, h, sample_every, n_blocks, r_max)}."""
    def case(planets, states, hill, h, sample_every, n_blocks, r_max=0.0):
        inclined = any("ix" in p for p in planets)
        h = W.min_period(W.pal_rows(planets)) / 20.0 if h is None else h
        return dict(states=states, inclined=inclined, hill=hill, h=h, sample_every=sample_every, n_blocks=n_blocks,
                    r_max=r_max)

    s2 = W.S2_PLANETS
    bad = _states(s2, 1e-3, 7)
    bad[1], bad[3] = W.s2_bad_walkers(dict(walkers=[bad[0]]))  # a t = 0 PRIOR state and a t = 0 ENCOUNTER state
    return {
        "one": case(s2[:1], _states(s2[:1], 1e-3, 1), 1.0, None, 5, 13),
        "two": case(s2, _states(s2, 1e-3, 2), 1.0, None, 5, 13),
        "two_inclined": case(W.S2_INCLINED, _states(W.S2_INCLINED, 1e-3, 3), 1.0, None, 4, 16),
        "three": case(s2 + W.EXTRA_PLANETS[:1], _states(s2 + W.EXTRA_PLANETS[:1], 1e-3, 4), 1.0, None, 1, 64),
        "three_inclined": case(THREE_INCLINED, _states(THREE_INCLINED, 1e-3, 5), 1.0, None, 7, 9),
        "quiet3_inclined_256": case(QUIET3_INCLINED, _states(QUIET3_INCLINED, 1e-3, 6), 1.0, None, 8, 32),
        "four": case(s2 + W.EXTRA_PLANETS, _states(s2 + W.EXTRA_PLANETS, 1e-3, 8), 1.0, None, 5, 13),
        "encounter_hill4": case(ENCOUNTER_PLANETS, _states(ENCOUNTER_PLANETS, 1e-4, 9), 4.0, H20, 4, 64),
        "encounter_hill1": case(ENCOUNTER_PLANETS, _states(ENCOUNTER_PLANETS, 1e-4, 9), 1.0, H20, 4, 64),
        "escape": case(ESCAPE_PLANETS, _states(ESCAPE_PLANETS, 1e-4, 10), 1.0, H20, 4, 64, r_max=3.0),
        "t0_status": case(s2, bad, 1.0, None, 4, 8),
    }


LIVE = ("one", "encounter_hill4", "escape", "t0_status")  # cheap enough for the CPU test to recompute in mpf


def fmt(x):
    return mp.nstr(x, DIGITS, min_fixed=0, max_fixed=0)


def record(run):
    """The fixture's record of one state's truth (decimal strings)."""
    return dict(status=run.status, steps=run.steps,
                xv=None if run.xv is None else [[fmt(x) for x in p] for p in run.xv],
                ext=None if run.ext is None else [[fmt(x) for x in p] for p in run.ext],
                enc_ratio=run.enc_ratio, esc_ratio=run.esc_ratio)


def load_fixture():
    with open(FIXTURE) as f:
        return json.load(f)


def scales(truth):
    """{kind: the case's scale of that kind}: the largest |truth| over its states (e2: 1)."""
    pos = vel = a = 0.0
    for rec in truth:
        if rec["xv"] is None:
            continue
        for p, e in zip(rec["xv"], rec["ext"]):
            pos = max([pos] + [abs(float(x)) for x in p[:3]])
            vel = max([vel] + [abs(float(x)) for x in p[3:]])
            a = max([a] + [abs(float(x)) for x in e[:2]])
    return dict(pos=pos, vel=vel, a=a, e2=1.0)


def errors(xv, ext, truth):
    """{kind: the largest |value - truth| / scale over the case's states}: xv [n][np][6], ext [n][np][3] of floats
    (a state's entry is ignored where the truth has none); the differences are taken in mpf."""
    sc = scales(truth)
    out = dict.fromkeys(KINDS, 0.0)
    with mp.workdps(TRUTH_DPS):
        for i, rec in enumerate(truth):
            if rec["xv"] is None:
                continue
            for p in range(len(rec["xv"])):
                for c in range(6):
                    k = "pos" if c < 3 else "vel"
                    out[k] = max(out[k], float(abs(mpf(float(xv[i][p][c])) - mpf(rec["xv"][p][c]))) / sc[k])
                for c in range(3):
                    k = "a" if c < 2 else "e2"
                    out[k] = max(out[k], float(abs(mpf(float(ext[i][p][c])) - mpf(rec["ext"][p][c]))) / sc[k])
    return out


def float_errors(case, truth):
    """(runs, errors) of the float restatement against the truth."""
    runs = run_case(case, float)
    nan = float("nan")
    npl = len(case["states"][0])
    xv = [r.xv if r.xv is not None else [[nan] * 6] * npl for r in runs]
    ext = [r.ext if r.ext is not None else [[nan] * 3] * npl for r in runs]
    return runs, errors(xv, ext, truth)


def kernel_rows(case):
    return W.kernel_rows(case["states"], case["inclined"])


def truth_arrays(truth):
    """(status [n], steps [n]) as numpy arrays."""
    return (np.array([r["status"] for r in truth], dtype=np.int32), np.array([r["steps"] for r in truth], dtype=np.int64))


# The float restatement's own errors against the 40-digit truth, per case and kind (errors(); measured by
# tests/test_stability_ref_cpu.py::test_float_errors_are_the_recorded_ones, which fails when they move).
FLOAT_ERR = {
    "one": dict(pos=1.204e-13, vel=9.622e-14, a=4.412e-15, e2=1.343e-15),
    "two": dict(pos=3.074e-14, vel=6.887e-14, a=2.510e-15, e2=6.897e-16),
    "two_inclined": dict(pos=4.355e-14, vel=9.092e-14, a=2.796e-15, e2=9.919e-16),
    "three": dict(pos=6.100e-14, vel=1.861e-13, a=2.569e-15, e2=1.525e-15),
    "three_inclined": dict(pos=3.590e-14, vel=1.103e-13, a=2.428e-15, e2=8.749e-16),
    "quiet3_inclined_256": dict(pos=7.842e-14, vel=3.083e-13, a=3.571e-15, e2=5.965e-16),
    "four": dict(pos=9.320e-15, vel=2.152e-14, a=2.707e-15, e2=1.540e-15),
    "encounter_hill4": dict(pos=1.515e-15, vel=1.641e-15, a=1.491e-15, e2=4.553e-16),
    "encounter_hill1": dict(pos=6.120e-13, vel=7.793e-13, a=7.155e-15, e2=1.014e-15),
    "escape": dict(pos=5.615e-15, vel=1.560e-14, a=3.666e-15, e2=7.517e-16),
    "t0_status": dict(pos=9.571e-15, vel=1.622e-14, a=1.824e-15, e2=4.755e-16),
}
