"""Inputs, truth and yardsticks of the step-unit tier U0 (tests/test_gpu_step_units.py).

The device functions under the likelihood kernel (rvm_device.h drift, stumpff23, stumpff_full,
rcp_nr / rsq_nr / rcube_nr, the kicks; rvm_walker.h walker_setup) are called one step at a time
through rvmcmc/librvm_step_probe.so and held to tests/wh_ref.py run on mpmath.mpf at 40 digits.
Nothing of the integrator is stated again here: the truth of a drift is wh_ref.kepler_drift, of a
walker's state at t = 0 wh_ref.WH, of a kick wh_ref.WH.kick.

Yardstick (drift, setup, kick): first-order conditioning.  For outputs y of inputs x

    bound_i = K u (|y|_block + sum_j |dy_i/dx_j| |x_j|),     u = 2^-53,

|y|_block the norm of the position (velocity) for a position (velocity) component and |y_i| for a
scalar; the Jacobian by central differences of wh_ref's own float run with the relative step 1e-7.
K is 3 x the largest ratio that float run attains against the truth over the inputs below (the
project's margin for a second double-precision implementation: T1_SENS_FACTOR, tier D0's
FLOOR_FACTOR), written down here and re-measured by tests/test_step_ref_cpu.py.

Bounds from the operation count (in u, relative unless said otherwise):

  rcp_nr    r (1 + e + e^2), e = 1 - x r exact to ~u |e|: what is left is e^3 (|e| <~ 1e-7: 1e-21)
            and the final fma's rounding, 1 u.                                           RCP_BOUND 1.1
  rsq_nr    e = fma(-(x y), y, 1): the product x y is rounded, so e carries an absolute error u,
            which enters the result as u / 2; the final fma 1 u.                         RSQ_BOUND 1.6
  rcube_nr  y2 = y y rounded (d1), y3 = y2 y rounded (d2); e is the exact residual of the rounded y2,
            so the series corrects (x y2)^(-3/2) = x^(-3/2) y^-3 (1 - 3 d1 / 2): the result is
            x^(-3/2) (1 + d1 + d2 - 3 d1 / 2): 1.5 u, and the final fma 1 u.              RCUBE_BOUND 2.6
  stumpff23<NT> on |z| <= B(NT): Horner c = K0 + z (K1 + z (...)): the last fma rounds c itself
            (1 u), K0 is rounded (1 u; exact for c2), every inner coefficient and fma contributes
            2 u |K_j| |z|^j, in all 2 u (c(-|z|) - K0) / c(z) <= 0.12 u at |z| = 0.3, and the
            documented truncation 2e-17 = 0.2 u.                                     STUMPFF23_BOUND 2.5
  stumpff_full on [-40, 40]: error over the majorant c_k(-|z|) (c2 and c3 have zeros for z > 0),
            3 x what wh_ref.stumpff attains on float over the same z, floor 2 u: STUMPFF_FULL_BOUND.
"""
import math

import numpy as np
from mpmath import mp, mpf

import wh_ref as R

U = 2.0 ** -53
DPS = 40
REL_STEP = 1e-7
MARGIN = 3.0  # test_gpu_logl.T1_SENS_FACTOR, wh_ref.FLOOR_FACTOR

# 3 x the float run's largest ratio (tests/test_step_ref_cpu.py re-measures them; written to 5 digits)
K_DRIFT = 34.047
K_SETUP = 6.1452
K_KICK = 10.653
STUMPFF_FULL_BOUND = 41.334  # in u, over the majorant (wh_ref.stumpff's float run: 13.8 u in c3 at z = -1.03)
K_DIGITS = 1e-4  # the written constants' rounding

RCP_BOUND, RSQ_BOUND, RCUBE_BOUND, STUMPFF23_BOUND = 1.1, 1.6, 2.6, 2.5
GM_BOUND = 4.0     # M_p = 1 + m_1 + .. + m_p summed in double: at most 4 additions of 1 u each
DMIN2_BOUND = 12.0  # (hf a cbrt(m / 3))^2: m/3 (u / 3 after the root), cbrt (1 ulp = 2 u), two products
                    # (2 u), doubled by the square, the square's rounding: 2 (1/3 + 2 + 2) + 1 = 9.7 u
STUMPFF_B = {6: 0.1, 7: 0.3, 8: 0.3}  # rvm_device.h stumpff_bound

FIRST, ZAWARE, TAYLOR, SECOND8, RARE_HALLEY, SAFE_HARD, SAFE_FALLBACK, NAN_GUESS = range(8)
PATH_NAMES = ("FIRST", "ZAWARE", "TAYLOR", "SECOND8", "RARE_HALLEY", "SAFE_HARD", "SAFE_FALLBACK", "NAN_GUESS")
MIN_CLASS = 32

# drift instantiations of the probe: (nt, mode, d3, kg); mode 0 ungated, 1 + ACC gated
MODES = {"ungated": 0, "acc0": 1, "acc1": 2, "acc2": 3, "acc3": 4, "acc4": 5}
SHIPPED = [(nt, m, d3, 0) for nt in (6, 7, 8) for m in (0, 1, 4) for d3 in (0, 1)]
VARIANT_BUILDS = ([(nt, m, 0, 0) for nt in (6, 7, 8) for m in (2, 3, 5)] +
                  [(nt, m, 0, 1) for nt in (6, 7, 8) for m in (1, 4)])


def variant_name(v):
    nt, mode, d3, kg = v
    return f"nt{nt}-{[k for k, m in MODES.items() if m == mode][0]}-{'d3' if d3 else 'planar'}-kg{kg}"


def acc_of(mode):
    return max(mode - 1, 0)


def reachable(mode):
    """Path classes a mode can reach (SAFE_FALLBACK may stay empty: its count is reported)."""
    c = [FIRST, SECOND8, RARE_HALLEY, SAFE_HARD, NAN_GUESS]
    if acc_of(mode) in (1, 2, 4):
        c += [ZAWARE, TAYLOR]
    return c


# ---------------------------------------------------------------------------------------------
# the yardstick
# ---------------------------------------------------------------------------------------------
def conditioning(fn, x):
    """sum_j |dy_i/dx_j| |x_j| by central differences of fn's float run (relative step REL_STEP)."""
    x = [float(q) for q in x]
    S = None
    for j, xj in enumerate(x):
        if xj == 0.0 or not math.isfinite(xj):
            continue
        h = REL_STEP * abs(xj)
        xp, xm = list(x), list(x)
        xp[j], xm[j] = xj + h, xj - h
        yp, ym = fn(xp), fn(xm)
        if S is None:
            S = [0.0] * len(yp)
        for i in range(len(yp)):
            S[i] += abs(yp[i] - ym[i]) / (xp[j] - xm[j]) * abs(xj)
    return S


def scales(truth, S, blocks):
    """u (|y|_block + S_i) per output: truth in mpf, blocks the block index of every output."""
    nb = max(blocks) + 1
    n2 = [mpf(0)] * nb
    for y, b in zip(truth, blocks):
        n2[b] = n2[b] + y * y
    return [U * (float(mp.sqrt(n2[b])) + s) for b, s in zip(blocks, S)]


def ratios(y, truth, sc):
    """|y_i - truth_i| / scale_i, the differences taken in mpf; inf where y is not finite."""
    out = []
    for a, t, s in zip(y, truth, sc):
        a = float(a)
        out.append(float(abs(mpf(a) - t) / s) if math.isfinite(a) else math.inf)
    return out


# ---------------------------------------------------------------------------------------------
# drift
# ---------------------------------------------------------------------------------------------
DRIFT_BLOCKS = [0, 0, 0, 1, 1, 1, 2, 3]  # rx ry rz | vx vy vz | r | ir
ECC = (0.0, 0.05, 0.25, 0.55, 0.9, 0.98, 0.995, 1.3)
ANOM = (0.0, 0.04, -0.04, 0.15, -0.15, 0.4, -0.4, 1.0, -1.0, 2.2, math.pi)  # true anomaly: dense near pericentre
DT_P = (1.0 / 224, 1.0 / 112, 1.0 / 56, 1.0 / 32, 1.0 / 12, 0.25, 0.6)


ZAWARE_BAND = ((0.3, 56, 0.1), (0.3, 56, 0.2), (0.4, 80, 0.1), (0.4, 80, 0.2), (0.4, 56, 1.6), (0.5, 112, 0.1), (0.5, 112, 0.2),
               (0.5, 80, 0.4), (0.5, 80, 0.6), (0.5, 80, 1.2), (0.5, 56, 1.8), (0.6, 160, 0.1), (0.6, 160, 0.2), (0.6, 160, 0.3),
               (0.6, 112, 0.4), (0.6, 56, 2.2), (0.7, 224, 0.3), (0.7, 224, 0.6), (0.7, 224, 0.8), (0.7, 224, 1.0), (0.7, 160, 0.5),
               (0.7, 160, 1.8), (0.7, 112, 1.8), (0.7, 80, 2.2), (0.8, 224, 1.8), (0.8, 160, 2.0), (0.8, 80, 2.5), (0.9, 160, 2.5))


def kepler_state(e, f, q, GM, omega):
    """Planar state at true anomaly f of the orbit of eccentricity e and pericentre distance q."""
    p = q * (1.0 + e)
    r = p / (1.0 + e * math.cos(f))
    k = math.sqrt(GM / p)
    return [r * math.cos(f + omega), r * math.sin(f + omega), 0.0,
            -k * (math.sin(f + omega) + e * math.sin(omega)), k * (math.cos(f + omega) + e * math.cos(omega)), 0.0]


def incline(x, a, b):
    """Rotate a state about the x axis by a, then about the y axis by b."""
    out = []
    for v in (x[0:3], x[3:6]):
        y, z = v[1] * math.cos(a) - v[2] * math.sin(a), v[1] * math.sin(a) + v[2] * math.cos(a)
        xx, zz = v[0] * math.cos(b) + z * math.sin(b), -v[0] * math.sin(b) + z * math.cos(b)
        out += [xx, y, zz]
    return out


def drift_items():
    """(x [n][8] = rx ry rz vx vy vz GM dt, n_planar): the planar items first, then inclined copies."""
    items = []
    i = 0
    for e in ECC:
        for f in ANOM:
            for dtp in DT_P:
                for sgn in (1.0, -1.0):
                    i += 1
                    a = 0.6 + 0.9 * ((i * 0.6180339887498949) % 1.0)   # semi-major axis (e < 1)
                    GM = 1.0 + 4e-3 * ((i * 0.7548776662466927) % 1.0)
                    q = a * (1.0 - e) if e < 1.0 else 0.05 + 0.2 * ((i * 0.5698402909980532) % 1.0)
                    # (hyperbolic: the period of the circular orbit at the pericentre distance)
                    P = 2.0 * math.pi * math.sqrt((a if e < 1.0 else q) ** 3 / GM)
                    omega = 0.3 + 2.0 * math.pi * ((i * 0.4142135623730951) % 1.0)
                    items.append(kepler_state(e, f, q, GM, omega) + [GM, sgn * dtp * P])
    # near-parabolic pericentre passages (the orbit of test_near_parabolic_pericentre_reports_the_encounter,
    # e = 0.9775, and closer to the parabola) at steps of half an orbit: the fourth-order guess lands
    # so far outside the series' range that the first Halley step's correction is not finite
    j = 0
    for e in (0.9775328, 0.995, 0.998, 0.9985):
        for f in (0.15, -0.15, 0.4, -0.4, 1.0, -1.0):
            for dtp in (0.45, 0.6):
                j += 1
                a, GM = 1.0225890, 1.0 + 1.5e-3
                P = 2.0 * math.pi * math.sqrt(a ** 3 / GM)
                items.append(kepler_state(e, f, a * (1.0 - e), GM, 0.7 + 0.11 * j) + [GM, (1.0 if j % 3 else -1.0) * dtp * P])
    # the band of (e, steps per orbit, true anomaly) where the cheap acceptance fails and the z-aware
    # form (ACC 1, 2, 4) passes at the shortest series, each with its time reversal
    for e, spo, f in ZAWARE_BAND:
        for sgn in (1.0, -1.0):
            for a, GM in ((0.9, 1.001), (1.3, 1.0032)):
                j += 1
                P = 2.0 * math.pi * math.sqrt(a ** 3 / GM)
                items.append(kepler_state(e, sgn * f, a * (1.0 - e), GM, 0.2 + 0.37 * j) + [GM, sgn * P / spo])
    n_planar = len(items)
    for i in range(0, n_planar, 10):
        x = items[i]
        items.append(incline(x, 0.05 + 1.4 * ((i * 0.6180339887498949) % 1.0), -0.6 + 1.2 * ((i * 0.7548776662466927) % 1.0))
                     + x[6:])
    return np.array(items), n_planar



def drift_fn(x):
    """One Kepler drift by wh_ref.kepler_drift on x's number type: rx ry rz vx vy vz r ir."""
    r, v = list(x[0:3]), list(x[3:6])
    R.kepler_drift(x[6], r, v, x[7], [0, 0])
    rr = R.sqrt(r[0] * r[0] + r[1] * r[1] + r[2] * r[2])
    return r + v + [rr, 1 / rr]


def _problem(fn, X, blocks):
    """Per item: truth (mpf), scales, and the float run's ratios."""
    truth, sc, fr = [], [], []
    with mp.workdps(DPS):
        for x in X:
            xf = [float(q) for q in x]
            t = fn([mpf(q) for q in xf])
            s = scales(t, conditioning(fn, xf), blocks)
            truth.append(t)
            sc.append(s)
            fr.append(ratios(fn(xf), t, s))
    return truth, sc, np.array(fr)


_CACHE = {}


def drift_problem():
    if "drift" not in _CACHE:
        X, n_planar = drift_items()
        truth, sc, fr = _problem(drift_fn, X, DRIFT_BLOCKS)
        _CACHE["drift"] = dict(x=X, n_planar=n_planar, truth=truth, scale=sc, float_ratio=fr)
    return _CACHE["drift"]


def max_ratio(Y, truth, sc, select=None):
    """Largest ratio of outputs Y [n][k] against the truth, per output column, under mp.workdps(DPS)."""
    with mp.workdps(DPS):
        r = np.array([ratios(y, t, s) if (select is None or select[i]) else [0.0] * len(t)
                      for i, (y, t, s) in enumerate(zip(Y, truth, sc))])
    return r


# ---- a float restatement of the drift's solver choice (prediction only: the device's own codes count)
def _series(z, nt):
    a = b = 0.0
    for j in range(nt - 1, -1, -1):
        a = a * z + (-1.0) ** j / math.factorial(2 * j + 2)
        b = b * z + (-1.0) ** j / math.factorial(2 * j + 3)
    return a, b


def _full(z):
    n = 0
    while abs(z) > 0.3 and n < 40:
        z *= 0.25
        n += 1
    C2, C3 = _series(z, 8)
    C1, C0 = 1.0 - z * C3, 1.0 - z * C2
    for _ in range(n):
        z *= 4.0
        C3 = (C2 + C0 * C3) * 0.25
        C2 = C1 * C1 * 0.5
        C1 = 1.0 - z * C3
        C0 = 1.0 - z * C2
    return C0, C1, C2, C3


_TOL = {6: 9.0e-6, 7: 6.2e-6, 8: 4.6e-6}


def _halley(x, nt, beta, r0, eta, zeta, GM, dt):
    x2 = x * x
    z, x3 = beta * x2, x2 * x
    c2, c3 = _series(z, nt)
    G3, G2 = x3 * c3, x2 * c2
    G1, G0 = x - beta * G3, 1.0 - z * c2
    f = GM * G3 + eta * G2 + r0 * G1 - dt
    fp = zeta * G2 + eta * G1 + r0
    fpp = zeta * G1 + eta * G0
    den = fp * fp - 0.5 * f * fpp
    # (the device divides by v_rcp_f64 and one residual correction: not finite for den = 0 or inf)
    q = f * fp / den if den != 0.0 and math.isfinite(den) else math.nan
    return q, z, x3, (G0, G1, G2, G3, f, fp, fpp)


def predict_path(x, nt, kg, acc):
    with np.errstate(all="ignore"):
        return _predict(x, nt, kg, acc)


def _predict(x, nt, kg, acc):
    rx, ry, rz, vx, vy, vz, GM, dt = (float(q) for q in x)
    r0 = math.sqrt(rx * rx + ry * ry + rz * rz)
    ir0 = 1.0 / r0
    v2, eta = vx * vx + vy * vy + vz * vz, rx * vx + ry * vy + rz * vz
    beta = 2.0 * GM * ir0 - v2
    zeta = GM - beta * r0
    u, sg, g = dt * ir0, eta * ir0, GM * ir0
    hs = 0.5 * sg
    T3 = hs * sg + (beta - g) / 6.0
    T4 = sg * (-0.625 * sg * sg + 5.0 / 12.0 * g - 0.375 * beta)
    if kg == 1:
        s2 = sg * sg
        T5 = beta * (9.0 / 120.0 * beta - 19.0 / 120.0 * g + 0.75 * s2) + g * (g / 12.0 - 0.875 * s2) + 0.875 * s2 * s2
        xg = u * (1.0 + u * (-hs + u * (T3 + u * (T4 + u * T5))))
    else:
        xg = u * (1.0 + u * (-hs + u * (T3 + u * T4)))
    Q, z, x3, (G0, G1, G2, G3, f0, fp, fpp) = _halley(xg, nt, beta, r0, eta, zeta, GM, dt)
    if not math.isfinite(Q):
        return NAN_GUESS
    B = STUMPFF_B[nt]
    zok = abs(z) <= B
    if zok and abs(Q) <= _TOL[nt] * abs(xg):
        return FIRST
    if acc in (1, 2, 4):
        if zok and abs(Q * Q * (Q * z)) <= 7.3e-17 * abs(x3):
            return ZAWARE
        if zok and abs(Q) <= 1e-4 * abs(xg):
            f3, f4, d = zeta * G0 - beta * eta * G1, -beta * fpp, -Q
            F = f0 + d * (fp + d * (0.5 * fpp + d * (f3 / 6.0 + d * f4 / 24.0)))
            F1 = fp + d * (fpp + d * (0.5 * f3 + d * f4 / 6.0))
            if abs(F / F1) <= 1e-8 * abs(xg):
                return TAYLOR
    xe = xg
    X1 = xg - Q
    if abs(beta * X1 * X1) <= 0.3:
        xe = X1
        Q, z, x3, _ = _halley(xe, 8, beta, r0, eta, zeta, GM, dt)
        if abs(z) <= 0.3 and abs(Q) <= _TOL[8] * abs(xe):
            return SECOND8
    if abs(beta) * (u * u) > 0.5:
        return SAFE_HARD
    start = xe - Q
    X = start if math.isfinite(start) and xe != xg else xg
    for _ in range(8):
        zi = beta * X * X
        c0, c1, c2, c3 = _full(zi)
        g1, g2, g3 = X * c1, X * X * c2, X * X * X * c3
        ff = r0 * g1 + eta * g2 + GM * g3 - dt
        ffp = r0 * c0 + eta * g1 + GM * g2
        ffpp = eta * c0 + zeta * g1
        den = ffp * ffp - 0.5 * ff * ffpp
        dX = ff * ffp / den if den != 0.0 else math.nan
        if abs((dX * dX) * (dX * zi)) <= 3e-17 * abs(X * X * X):
            return RARE_HALLEY
        X = X - dX
    return SAFE_FALLBACK


def predicted_counts(X, variant):
    nt, mode, d3, kg = variant
    c = [0] * 8
    for x in X:
        c[predict_path(x, nt, kg, acc_of(mode))] += 1
    return c


# ---------------------------------------------------------------------------------------------
# stumpff, recip
# ---------------------------------------------------------------------------------------------
def _frac(i, k):
    return (i * (0.6180339887498949, 0.7548776662466927, 0.5698402909980532, 0.4142135623730951)[k]) % 1.0


def stumpff_items():
    """1536 z in [-40, 40]: a third each in |z| <= 0.1, 0.1 .. 0.3 and 0.3 .. 40, with the edges of
    every range (the series' bounds, the first value the quartering loop takes, its thresholds)."""
    z = [0.0, 1e-300, -1e-300, 1e-8, -1e-8, 0.1, -0.1, 0.3, -0.3, 40.0, -40.0]
    z += [s * math.nextafter(b, d) for s in (1, -1) for b in (0.1, 0.3, 1.2, 4.8, 19.2) for d in (0.0, 50.0)]
    z += [s * b for s in (1, -1) for b in (1.0, 1.2, 4.8, 19.2, 9.869604401089358, 39.47841760435743)]
    i = 0
    while len(z) < 1536:
        i += 1
        sgn = 1.0 if i % 2 else -1.0
        lo, hi = ((0.0, 0.1), (0.1, 0.3), (0.3, 40.0))[i % 3]
        z.append(sgn * (lo + (hi - lo) * _frac(i, 0) ** (2 if i % 3 == 2 else 1)))
    return np.array(z)


def stumpff_problem():
    """z, the truth c0..c3 (mpf), the majorants c_k(-|z|) and the float run's errors over them (in u)."""
    if "stumpff" not in _CACHE:
        z = stumpff_items()
        with mp.workdps(DPS):
            truth = [R.stumpff(mpf(float(q))) for q in z]
            major = [R.stumpff(-abs(mpf(float(q)))) for q in z]
            fl = np.array([[float(abs(mpf(c) - t) / m) / U for c, t, m in zip(R.stumpff(float(q)), tr, mj)]
                           for q, tr, mj in zip(z, truth, major)])
        _CACHE["stumpff"] = dict(z=z, truth=truth, major=major, float_err=fl)
    return _CACHE["stumpff"]


def recip_items():
    """1536 x > 0 over 2^-40 .. 2^40: mantissas at both ends of a binade, at 1.5 and spread between."""
    x = []
    i = 0
    while len(x) < 1536:
        i += 1
        k = i % 81 - 40
        m = (1.0, math.nextafter(1.0, 2.0), math.nextafter(2.0, 1.0), 1.5, 1.0 + _frac(i, 1), 1.0 + _frac(i, 2),
             1.0 + _frac(i, 3), 1.0 + _frac(i, 0))[i % 8]
        x.append(math.ldexp(m, k))
    return np.array(x)


def rel_err_u(y, truth):
    """|y - truth| / |truth| in u, per element (mpf differences)."""
    return np.array([float(abs(mpf(float(a)) - t) / abs(t)) / U if math.isfinite(a) else math.inf for a, t in zip(y, truth)])


def recip_truth(x):
    with mp.workdps(DPS):
        xm = [mpf(float(q)) for q in x]
        return [1 / q for q in xm], [1 / mp.sqrt(q) for q in xm], [1 / (q * mp.sqrt(q)) for q in xm]


# ---------------------------------------------------------------------------------------------
# setup (walker_setup): the walker's Jacobi state at t = 0
# ---------------------------------------------------------------------------------------------
SETUP_W = {1: 100, 2: 50, 3: 40, 4: 40}  # walkers per planet count: several waves, the last partly filled
HILL_FACTOR = 1.3
BENIGN = lambda p: [1e-3, 1.0 + p, 0.0, 0.0, 0.0, 0.0, 0.0]  # walker_setup's substitute for a rejected walker


def setup_items(np_, inclined):
    """(walkers [W][np][7] = m a h k l ix iy, rejected [W]): e up to 0.99 in every quadrant of (h, k),
    |l| up to 1e3, inclinations up to the prior's edge, and prior-rejected walkers among valid ones,
    in a wave's first and last group too."""
    W = SETUP_W[np_]
    out, rej = [], []
    for w in range(W):
        pl = []
        for p in range(np_):
            i = 1 + w * 4 + p + 1000 * np_ + (500 if inclined else 0)
            m = 5.5e-6 * (1e-2 / 5.5e-6) ** _frac(i, 0)
            a = (0.3 + 0.8 * p) * (1.0 + 0.3 * _frac(i, 1))
            e = (0.0, 0.05, 0.3, 0.7, 0.95, 0.99)[(w + p) % 6]
            pom = 2.0 * math.pi * _frac(i, 2)
            lam = (0.3, -2.2, 17.0, -155.0, 1e3, -1e3, 6.2, 0.0)[(w + 3 * p) % 8] + _frac(i, 3)
            # (near e = 1 the iteration from F = lam can wander for more than the 100 steps the kernel,
            # the oracle and the reference give it -- 3 of the 460 walkers first drawn here took 150;
            # that limit is the algorithm's, not the arithmetic's: l moves on until the iteration is direct)
            while newton_steps(e * math.sin(pom), e * math.cos(pom), lam) > NEWTON_MAX:
                lam += 0.37
            mag = (0.0, 0.01, 0.3, 1.0, 1.9, 1.9999)[(w // 2 + p) % 6] if inclined else 0.0
            node = 2.0 * math.pi * _frac(i, 0)
            pl.append([m, a, e * math.sin(pom), e * math.cos(pom), lam, mag * math.cos(node), mag * math.sin(node)])
        bad = w % 7 == 3 or w in (15, 16)
        if bad:
            p = w % np_
            kind = (w // 2) % (6 if inclined else 5)
            if kind == 0:
                pl[p][1] = 0.02           # the prior's edges are outside
            elif kind == 1:
                pl[p][0] = 5e-6
            elif kind == 2:
                pl[p][2], pl[p][3] = 0.9, -0.6
            elif kind == 3:
                pl[p][4] = math.inf
            elif kind == 4:
                pl[p][4] = math.nan
            else:
                pl[p][5], pl[p][6] = 1.8, -1.2
        out.append(pl)
        rej.append(bad)
    return out, rej


SETUP_BLOCK = [0, 0, 0, 1, 1, 1, 2, 3]
NEWTON_MAX = 16


def newton_steps(h, k, lam):
    """Steps of the reference's Newton iteration for the eccentric longitude from F = lam (double)."""
    F = lam
    for it in range(1, 1001):
        sF, cF = math.sin(F), math.cos(F)
        d = (F - k * sF + h * cF - lam) / (1.0 - k * cF - h * sF)
        F -= d
        if abs(d) <= 1e-15 * max(abs(F), 1.0):
            return it
    return 1001


def setup_fn(np_, inclined):
    def fn(x):
        pl = [list(x[7 * p:7 * p + 7]) for p in range(np_)]
        s = R.WH(pl, inclined, HILL_FACTOR)
        out = []
        for i in range(1, np_ + 1):
            r = s.r[i]
            rr = R.sqrt(r[0] * r[0] + r[1] * r[1] + r[2] * r[2])
            out += list(r) + list(s.v[i]) + [rr, 1 / rr]
        return out
    return fn


def setup_problem(np_, inclined):
    """Per walker: the truth of every planet's (rx ry rz vx vy vz r ir), its scales, the float run's
    ratios; GM per planet and dmin2 in mpf; status and the admissible e2w."""
    key = ("setup", np_, inclined)
    if key not in _CACHE:
        walkers, rej = setup_items(np_, inclined)
        eff = [[BENIGN(p) for p in range(np_)] if b else wk for wk, b in zip(walkers, rej)]
        fn = setup_fn(np_, inclined)
        blocks = [4 * p + b for p in range(np_) for b in SETUP_BLOCK]
        truth, sc, fr = _problem(fn, [[q for p in wk for q in p] for wk in eff], blocks)
        GM, dmin2, e2 = [], [], []
        with mp.workdps(DPS):
            for wk, raw in zip(eff, walkers):
                M = [mpf(1)]
                for p in wk:
                    M.append(M[-1] + mpf(p[0]))
                GM.append(M[1:])
                dmin2.append((mpf(HILL_FACTOR) * max(mpf(p[1]) * mp.cbrt(mpf(p[0]) / 3) for p in wk)) ** 2)
                e2.append(e2w_candidates(raw))
        _CACHE[key] = dict(walkers=walkers, rejected=rej, truth=truth, scale=sc, float_ratio=fr, GM=GM, dmin2=dmin2, e2w=e2)
    return _CACHE[key]


def e2w_candidates(walker):
    """max_p (h^2 + k^2) in double as a compiler may contract it: no fma, or either product fused
    (each exactly, from rationals).  Returns (lowest admissible, highest admissible, all values)."""
    from fractions import Fraction as F
    per = []
    for p in walker:
        h, k = p[2], p[3]
        hh, kk = h * h, k * k
        per.append({hh + kk, float(F(h) * F(h) + F(kk)), float(F(hh) + F(k) * F(k))})
    allv = set().union(*per) | {0.0}
    return max(0.0, max(min(c) for c in per)), max(0.0, max(max(c) for c in per)), allv


# ---------------------------------------------------------------------------------------------
# kick
# ---------------------------------------------------------------------------------------------
KICK_W = SETUP_W
KICK_H = 0.5  # (the kick is linear in the step: a long one makes the interaction a larger part of |v|)
EXIT_MARGIN = 1e-8


def _wh_state(np_, r, v, m, dmin2):
    s = object.__new__(R.WH)
    s.np = np_
    s.m = [1] + list(m)
    s.Mi = [1]
    for i in range(1, np_ + 1):
        s.Mi.append(s.Mi[i - 1] + s.m[i])
    s.dmin2 = dmin2
    s.enc = False
    s.r = [None] + [list(q) for q in r]
    s.v = [None] + [list(q) for q in v]
    return s


def pair_r2(np_, r, m):
    """Squared distances of all body pairs from the Jacobi positions (wh_ref.WH.kick's positions)."""
    s = _wh_state(np_, r, [[0 * r[0][0]] * 3] * np_, m, 0.0)
    zero = 0 * r[0][0]
    x, cm = [[zero] * 3], [zero] * 3
    for i in range(1, np_ + 1):
        x.append([s.r[i][c] + cm[c] / s.Mi[i - 1] for c in range(3)])
        cm = [cm[c] + s.m[i] * x[i][c] for c in range(3)]
    return [sum((x[j][c] - x[i][c]) ** 2 for c in range(3)) for i in range(np_ + 1) for j in range(i + 1, np_ + 1)]


def kick_items(np_, inclined):
    """Per walker (r [np][3], v [np][3], m [np], dmin2): mass ratios 5e-6 .. 1e-2; generic, near-aligned
    (the indirect terms cancel) and close configurations; the exit distance none, just inside and just
    outside the closest pair (EXIT_MARGIN relative, so the truth decides the bit)."""
    out = []
    for w in range(KICK_W[np_]):
        i0 = 1 + 5 * w + 2000 * np_ + (700 if inclined else 0)
        geom = w % 3
        th0 = 2.0 * math.pi * _frac(i0, 3)
        r, v, m = [], [], []
        for p in range(np_):
            i = i0 + p
            m.append(5e-6 * 2000.0 ** ((_frac(i, 0) + (0.0, 0.999)[(w // 3 + p) % 2]) % 1.0) if (w + p) % 5 else (5e-6, 1e-2)[p % 2])
            a = (0.5 * 1.6 ** p if geom != 2 else 1.0 + 0.06 * p) * (1.0 + 0.05 * _frac(i, 1))
            th = (2.0 * math.pi * _frac(i, 2), th0 + 2e-3 * p * (1 + w % 4), th0 + 0.02 * p)[geom]
            inc = 0.3 * (_frac(i, 3) - 0.5) if inclined else 0.0
            k = math.sqrt(1.0 / a) * (0.9 + 0.2 * _frac(i, 0))
            r.append([a * math.cos(th), a * math.sin(th) * math.cos(inc), a * math.sin(th) * math.sin(inc)])
            v.append([-k * math.sin(th), k * math.cos(th) * math.cos(inc), k * math.cos(th) * math.sin(inc)])
        r2 = min(pair_r2(np_, r, m))
        dmin2 = (0.0, r2 * (1.0 + EXIT_MARGIN), r2 * (1.0 - EXIT_MARGIN), 0.25 * r2)[w % 4]
        out.append((r, v, m, dmin2))
    return out


def kick_fn(np_, half=False):
    def fn(x):
        n3 = 3 * np_
        r = [x[3 * p:3 * p + 3] for p in range(np_)]
        v = [x[n3 + 3 * p:n3 + 3 * p + 3] for p in range(np_)]
        s = _wh_state(np_, r, v, x[2 * n3:2 * n3 + np_], 0.0)
        s.kick(x[2 * n3 + np_] / 2 if half else x[2 * n3 + np_])
        return [q for p in range(1, np_ + 1) for q in s.v[p]]
    return fn


def kick_problem(np_, inclined):
    """Per walker: the velocities after the full and the half kick (truth, scales, the float run's
    ratios), the encounter verdict and the exit margin in mpf, star_vx and its bound."""
    key = ("kick", np_, inclined)
    if key not in _CACHE:
        items = kick_items(np_, inclined)
        X = [[q for p in r for q in p] + [q for p in v for q in p] + list(m) + [KICK_H] for r, v, m, _ in items]
        blocks = [p for p in range(np_) for _ in range(3)]
        full = _problem(kick_fn(np_), X, blocks)
        half = _problem(kick_fn(np_, True), X, blocks)
        enc, margin, star, star_bound = [], [], [], []
        with mp.workdps(DPS):
            for r, v, m, d2 in items:
                rm, vm, mm = [[mpf(q) for q in p] for p in r], [[mpf(q) for q in p] for p in v], [mpf(q) for q in m]
                r2 = pair_r2(np_, rm, mm)
                enc.append(any(q < mpf(d2) for q in r2))
                margin.append(min(float(abs(q / mpf(d2) - 1)) for q in r2) if d2 > 0.0 else math.inf)
                s = _wh_state(np_, rm, vm, mm, 0.0)
                star.append(s.star_vx())
                star_bound.append((2 * np_ + 3) * U * float(sum(abs(s.m[p] / s.Mi[p] * s.v[p][0]) for p in range(1, np_ + 1))))
        _CACHE[key] = dict(items=items, full=full, half=half, enc=enc, margin=margin, star=star, star_bound=star_bound)
    return _CACHE[key]


NP_D3 = [(n, d) for n in (1, 2, 3, 4) for d in (False, True)]


def measured_constants():
    """What tests/test_step_ref_cpu.py holds the written constants to: MARGIN x the float run's largest ratio."""
    kd = MARGIN * float(drift_problem()["float_ratio"].max())
    ks = MARGIN * max(float(setup_problem(n, d)["float_ratio"].max()) for n, d in NP_D3)
    kk = MARGIN * max(float(kick_problem(n, d)[k][2].max()) for n, d in NP_D3 for k in ("full", "half"))
    sf = max(2.0, MARGIN * float(stumpff_problem()["float_err"].max()))
    return kd, ks, kk, sf
