"""Arbitrary-precision restatement of the plan's discrete likelihood, and of its derivatives.

The model RV that rvm_logl_batch and rvm_logl_derivs evaluate is the Richardson-extrapolated
Wisdom-Holman integration that oracle/rvoracle.c states in double (pal_to_cart, wh_init, wh_kick,
kepler_drift, wh_direction, rvo_whx_rv_seq, rvo_richardson_weights_seq).  This module states the
same algorithm once more, over a number type: every function below runs on Python ``float``, on
``mpmath.mpf`` and on ``HyperDual`` numbers over either.

  * Pal elements -> heliocentric -> Jacobi coordinates; per segment n1 = max(1, ceil(D/dt - 1e-9))
    steps (computed in double, as the oracle and the plan compute it), step h = (sign D / n1) / mult,
    K(h/2) D(h) K(h/2) with the interior half kicks merged; the star's barycentric vx per epoch;
    the Lagrange-at-zero weights.
  * The Kepler step is the mathematical one: Stumpff functions in closed form (cos/sin for z > 1,
    cosh/sinh for z < -1, the power series between), the root of r0 G1 + eta G2 + GM G3 = dt
    iterated to the working precision.  Control flow depends on the parameters only through the
    prior and the encounter test, so the per-epoch RV is a smooth function of the parameters.
  * Two diagnostic counters per level: steps with |beta| (dt/r0)^2 > 0.5 (the kernel's bracketed
    solver) and steps whose converged |beta X^2| > 0.1 (its Stumpff quartering loop).

Truth for the derivative tier (tests/test_gpu_derivs_exact.py) is NOT the hyper-dual class: it is
central differences of the mpf run at 60 digits with steps 1e-15 max(|x_i|, FLOOR_i) (truncation
~1e-30, roundoff 1e-60 / 1e-30), of the per-epoch RV: rv[e], rv_i[e], rv_ij[e] (i >= j).  chi2, the
gradient and the Hessian for any observed RVs follow from those by the reference's sums
(state.py:264-268), so one set of integrations serves several observation vectors.  The hyper-dual
class run on ``float`` is what an independent double-precision implementation of the same
derivatives achieves (the noise floor the kernel is held to); run on ``mpf`` it must reproduce the
finite-difference truth, which checks the class (tests/test_wh_ref_cpu.py).

tests/golden/make_wh_derivs.py writes tests/golden/wh_derivs.json from case_inputs() below.
"""
import json
import math
import os

import numpy as np
from mpmath import mp, mpf

OK, PRIOR, ENCOUNTER, NONFINITE = 0, 1, 2, 3
FLOOR = {0: 1e-4, 1: 1e-2, 2: 1e-2, 3: 1e-2, 4: 1.0, 5: 1e-2, 6: 1e-2}  # m a h k l ix iy (test_gpu_derivs.FLOOR)
TRUTH_DPS = 60
FD_REL = "1e-15"
DIGITS = 30
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "wh_derivs.json")


# ---------------------------------------------------------------------------------------------
# number types
# ---------------------------------------------------------------------------------------------
def _f(name, x):
    return getattr(math, name)(x) if isinstance(x, float) else getattr(mp, name)(x)


class HyperDual:
    """(value, d/dp_i, d/dp_j, d2/dp_i dp_j) over float or mpf."""
    __slots__ = ("v", "a", "b", "ab")

    def __init__(self, v, a=0, b=0, ab=0):
        self.v, self.a, self.b, self.ab = v, a, b, ab

    def chain(self, f, f1, f2):
        return HyperDual(f, f1 * self.a, f1 * self.b, f1 * self.ab + f2 * self.a * self.b)

    def __neg__(self):
        return HyperDual(-self.v, -self.a, -self.b, -self.ab)

    def __add__(self, o):
        if isinstance(o, HyperDual):
            return HyperDual(self.v + o.v, self.a + o.a, self.b + o.b, self.ab + o.ab)
        return HyperDual(self.v + o, self.a, self.b, self.ab)

    __radd__ = __add__

    def __sub__(self, o):
        if isinstance(o, HyperDual):
            return HyperDual(self.v - o.v, self.a - o.a, self.b - o.b, self.ab - o.ab)
        return HyperDual(self.v - o, self.a, self.b, self.ab)

    def __rsub__(self, o):
        return HyperDual(o - self.v, -self.a, -self.b, -self.ab)

    def __mul__(self, o):
        if isinstance(o, HyperDual):
            return HyperDual(self.v * o.v, self.v * o.a + self.a * o.v, self.v * o.b + self.b * o.v,
                             self.v * o.ab + self.a * o.b + self.b * o.a + self.ab * o.v)
        return HyperDual(self.v * o, self.a * o, self.b * o, self.ab * o)

    __rmul__ = __mul__

    def inv(self):
        f = 1 / self.v
        return self.chain(f, -f * f, 2 * f * f * f)

    def __truediv__(self, o):
        if isinstance(o, HyperDual):
            return self * o.inv()
        return HyperDual(self.v / o, self.a / o, self.b / o, self.ab / o)

    def __rtruediv__(self, o):
        return self.inv() * o

    def sqrt(self):
        f = _f("sqrt", self.v)
        return self.chain(f, 1 / (2 * f), -1 / (4 * f * self.v))

    def sin(self):
        s, c = _f("sin", self.v), _f("cos", self.v)
        return self.chain(s, c, -s)

    def cos(self):
        s, c = _f("sin", self.v), _f("cos", self.v)
        return self.chain(c, -s, -c)

    def sinh(self):
        s, c = _f("sinh", self.v), _f("cosh", self.v)
        return self.chain(s, c, s)

    def cosh(self):
        s, c = _f("sinh", self.v), _f("cosh", self.v)
        return self.chain(c, s, c)

    def parts(self):
        return (self.v, self.a, self.b, self.ab)


def val(x):
    return x.v if isinstance(x, HyperDual) else x


def _fn(name):
    def g(x):
        return getattr(x, name)() if isinstance(x, HyperDual) else _f(name, x)
    return g


sqrt, sin, cos, sinh, cosh = (_fn(n) for n in ("sqrt", "sin", "cos", "sinh", "cosh"))


def _eps(x):
    return 2.0 ** -52 if isinstance(val(x), float) else mpf(10) ** (-mp.dps)


def _refine(step, X, inputs):
    """Continue a converged primal Newton iteration X -= step(X) in hyper-dual arithmetic until all
    four parts are stationary (no-op when no input is hyper-dual)."""
    if not any(isinstance(q, HyperDual) for q in inputs):
        return X
    tol = 64 * _eps(X)
    Xh = HyperDual(X)
    for _ in range(10):
        d = step(Xh)
        Xh = Xh - d
        if all(abs(dp) <= tol * abs(xp) for dp, xp in zip(d.parts(), Xh.parts())):
            break
    return Xh


# ---------------------------------------------------------------------------------------------
# the algorithm
# ---------------------------------------------------------------------------------------------
def pal_to_cart(mu, a, lam, k, h, ix, iy, inclined):
    """Pal (2009) elements -> heliocentric position and velocity (rvoracle.c pal_to_cart)."""
    def step(F):
        sF, cF = sin(F), cos(F)
        return (F - k * sF + h * cF - lam) / (1 - k * cF - h * sF)

    lv, kv, hv = val(lam), val(k), val(h)
    tol = 4 * _eps(lv)
    F = lv
    for _ in range(200):
        sF, cF = sin(F), cos(F)
        d = (F - kv * sF + hv * cF - lv) / (1 - kv * cF - hv * sF)
        F = F - d
        if abs(d) <= tol * max(abs(F), 1):
            break
    sF, cF = sin(F), cos(F)
    F = F - (F - kv * sF + hv * cF - lv) / (1 - kv * cF - hv * sF)
    F = _refine(step, F, (lam, k, h))
    sF, cF = sin(F), cos(F)
    beta = 1 / (1 + sqrt(1 - h * h - k * k))
    n = sqrt(mu / (a * a * a))
    r = a * (1 - k * cF - h * sF)
    X = a * ((1 - h * h * beta) * cF + h * k * beta * sF - k)
    Y = a * ((1 - k * k * beta) * sF + h * k * beta * cF - h)
    fac = n * a * a / r
    VX = fac * (h * k * beta * cF - (1 - h * h * beta) * sF)
    VY = fac * ((1 - k * k * beta) * cF - h * k * beta * sF)
    if not inclined:
        return [X, Y, 0 * X], [VX, VY, 0 * VX]
    w2 = 4 - ix * ix - iy * iy
    if val(w2) < 0:
        w2 = -w2
    W = sqrt(w2)
    axx, axy, ayy = 1 - iy * iy / 2, ix * iy / 2, 1 - ix * ix / 2
    return ([axx * X + axy * Y, axy * X + ayy * Y, W * (ix * Y - iy * X) / 2],
            [axx * VX + axy * VY, axy * VX + ayy * VY, W * (ix * VY - iy * VX) / 2])


_COEF = {}


def _coefs(z):
    """1/(2j+2)!, 1/(2j+3)! for the Stumpff series on |z| <= 1, enough terms for z's precision."""
    isf = isinstance(val(z), float)
    key = ("f",) if isf else ("m", mp.dps)
    if key not in _COEF:
        one = 1.0 if isf else mpf(1)
        lim = 1e22 if isf else 10 ** (mp.dps + 6)
        n = 1
        while math.factorial(2 * n + 2) < lim:
            n += 1
        _COEF[key] = ([one / math.factorial(2 * j + 2) for j in range(n + 1)],
                      [one / math.factorial(2 * j + 3) for j in range(n + 1)])
    return _COEF[key]


def stumpff(z):
    """c0..c3 of z in closed form; the series c_k = sum (-z)^j / (2j + k)! where |z| <= 1."""
    zv = val(z)
    if abs(zv) <= 1:
        f2, f3 = _coefs(z)
        c2 = c3 = 0
        for j in range(len(f2) - 1, -1, -1):
            c2 = f2[j] - z * c2
            c3 = f3[j] - z * c3
        return 1 - z * c2, 1 - z * c3, c2, c3
    if zv > 0:
        s = sqrt(z)
        c0, c1 = cos(s), sin(s) / s
    else:
        s = sqrt(-z)
        c0, c1 = cosh(s), sinh(s) / s
    return c0, c1, (1 - c0) / z, (1 - c1) / z


def kepler_root(r0, eta, beta, GM, dt):
    """The root X of r0 G1 + eta G2 + GM G3 = dt (increasing in X), to the working precision:
    bracketed Newton on the primal, then the hyper-dual continuation."""
    def f_fp(X, r0, eta, beta, GM):
        c0, c1, c2, c3 = stumpff(beta * X * X)
        G1, G2, G3 = X * c1, X * X * c2, X * X * X * c3
        return r0 * G1 + eta * G2 + GM * G3 - dt, r0 * c0 + eta * G1 + GM * G2

    p = [val(q) for q in (r0, eta, beta, GM)]
    sgn = 1 if dt >= 0 else -1
    lo, hi = 0 * dt, dt / p[0]
    for _ in range(200):
        if sgn * f_fp(hi, *p)[0] > 0:
            break
        lo, hi = hi, 2 * hi
    X = dt / p[0] - dt * dt * p[1] / (2 * p[0] * p[0] * p[0])
    if not (sgn * (X - lo) > 0 and sgn * (hi - X) > 0):
        X = (lo + hi) / 2
    tol = 4 * _eps(X)
    for _ in range(400):
        f, fp = f_fp(X, *p)
        if sgn * f > 0:
            hi = X
        else:
            lo = X
        Xn = X - f / fp
        if not (sgn * (Xn - lo) >= 0 and sgn * (hi - Xn) >= 0):
            Xn = (lo + hi) / 2
        conv = abs(Xn - X) <= tol * abs(Xn)
        X = Xn
        if conv:
            break
    f, fp = f_fp(X, *p)
    X = X - f / fp

    def step(Xh):
        f, fp = f_fp(Xh, r0, eta, beta, GM)
        return f / fp

    return _refine(step, X, (r0, eta, beta, GM))


def kepler_drift(GM, r, v, dt, cnt):
    r0 = sqrt(r[0] * r[0] + r[1] * r[1] + r[2] * r[2])
    v2 = v[0] * v[0] + v[1] * v[1] + v[2] * v[2]
    eta = r[0] * v[0] + r[1] * v[1] + r[2] * v[2]
    beta = 2 * GM / r0 - v2
    u = dt / val(r0)
    if abs(val(beta)) * u * u > 0.5:
        cnt[0] += 1
    X = kepler_root(r0, eta, beta, GM, dt)
    z = beta * X * X
    if abs(val(z)) > 0.1:
        cnt[1] += 1
    c0, c1, c2, c3 = stumpff(z)
    G1, G2, G3 = X * c1, X * X * c2, X * X * X * c3
    rr = r0 * c0 + eta * G1 + GM * G2
    f, g = 1 - GM * G2 / r0, dt - GM * G3
    fd, gd = -GM * G1 / (rr * r0), 1 - GM * G2 / rr
    for c in range(3):
        r[c], v[c] = f * r[c] + g * v[c], fd * r[c] + gd * v[c]


class WH:
    """Jacobi-coordinate state of one walker (rvoracle.c wh_state, wh_init)."""

    def __init__(self, pl, inclined, hill_factor):
        n = self.np = len(pl)
        self.m = [1] + [p[0] for p in pl]
        self.Mi = [1]
        for i in range(1, n + 1):
            self.Mi.append(self.Mi[i - 1] + self.m[i])
        hill = max(float(val(p[1])) * (float(val(p[0])) / 3.0) ** (1.0 / 3.0) for p in pl)
        self.dmin2 = (hill_factor * hill) ** 2
        self.enc = False
        self.r, self.v = [None], [None]
        zero = 0 * val(pl[0][1])
        sx, sv = [zero] * 3, [zero] * 3
        for i in range(1, n + 1):
            m, a, h, k, l, ix, iy = pl[i - 1]
            x, vv = pal_to_cart(1 + m, a, l, k, h, ix, iy, inclined)
            self.r.append([x[c] - sx[c] / self.Mi[i - 1] for c in range(3)])
            self.v.append([vv[c] - sv[c] / self.Mi[i - 1] for c in range(3)])
            sx = [sx[c] + m * x[c] for c in range(3)]
            sv = [sv[c] + m * vv[c] for c in range(3)]

    def star_vx(self):
        vx = 0
        for i in range(1, self.np + 1):
            vx = vx - (self.m[i] / self.Mi[i]) * self.v[i][0]
        return vx

    def kick(self, h, dry=False):
        n = self.np
        zero = 0 * val(self.r[1][0])
        x = [[zero] * 3]
        cm = [zero] * 3
        for i in range(1, n + 1):
            x.append([self.r[i][c] + cm[c] / self.Mi[i - 1] for c in range(3)])
            cm = [cm[c] + self.m[i] * x[i][c] for c in range(3)]
        acc = [[zero] * 3 for _ in range(n + 1)]
        for i in range(n + 1):
            for j in range(i + 1, n + 1):
                d = [x[j][c] - x[i][c] for c in range(3)]
                r2 = d[0] * d[0] + d[1] * d[1] + d[2] * d[2]
                if val(r2) < self.dmin2:
                    self.enc = True
                ir3 = 1 / (r2 * sqrt(r2))
                for c in range(3):
                    acc[i][c] = acc[i][c] + self.m[j] * ir3 * d[c]
                    acc[j][c] = acc[j][c] - self.m[i] * ir3 * d[c]
        if dry:
            return
        ma = [self.m[0] * acc[0][c] for c in range(3)]
        for i in range(1, n + 1):
            r = self.r[i]
            rj2 = r[0] * r[0] + r[1] * r[1] + r[2] * r[2]
            kep = self.Mi[i] / (rj2 * sqrt(rj2))
            for c in range(3):
                self.v[i][c] = self.v[i][c] + h * (acc[i][c] - ma[c] / self.Mi[i - 1] + kep * r[c])
            ma = [ma[c] + self.m[i] * acc[i][c] for c in range(3)]

    def drift(self, h, cnt):
        for i in range(1, self.np + 1):
            kepler_drift(self.Mi[i], self.r[i], self.v[i], h, cnt)


def _num(like):
    return float if isinstance(val(like), float) else mpf


def wh_direction(pl, inclined, hill_factor, abs_t, sign, dt, sub, cnt):
    """One direction at one level (rvoracle.c wh_direction): (status, rv per epoch of abs_t)."""
    num = _num(pl[0][1])
    s = WH(pl, inclined, hill_factor)
    s.kick(0, dry=True)  # the encounter check before the first step
    if s.enc:
        return ENCOUNTER, None
    rv, tprev = [], 0.0
    for at in abs_t:
        D = at - tprev
        tprev = at
        n1 = max(1, int(math.ceil(D / dt - 1e-9))) if D > 0.0 else 0
        ns = n1 * sub
        if ns > 0:
            h = (num(sign * D) / n1) * (num(1) / sub)
            s.kick(h / 2)
            for j in range(ns):
                s.drift(h, cnt)
                s.kick(h / 2 if j == ns - 1 else h)
        if s.enc:
            return ENCOUNTER, None
        rv.append(s.star_vx())
    return OK, rv


def richardson_weights(mult, num=float):
    x = [num(1) / (m * m) for m in mult]
    w = []
    for k in range(len(mult)):
        wk = num(1)
        for j in range(len(mult)):
            if j != k:
                wk = wk * (x[j] / (x[j] - x[k]))
        w.append(wk)
    return w


def prior_hard(pl, inclined):
    for p in pl:
        m, a, h, k, l, ix, iy = (val(q) for q in p)
        if a <= 0.02 or m <= 5e-6 or h * h + k * k >= 1 or (inclined and ix * ix + iy * iy >= 4):
            return True
    return False


def whx_rv(pl, inclined, hill_factor, t, dt, mult):
    """The kernel's model RV (rvoracle.c rvo_whx_rv_seq): pl [np][7] numbers of one type (m, a, h, k,
    l, ix, iy), t and dt Python floats.  Returns (status, rv [len(t)] in t's order, counters
    [len(mult)][2] = steps with |beta| (dt/r0)^2 > 0.5, steps with |beta X^2| > 0.1)."""
    cnts = [[0, 0] for _ in mult]
    if prior_hard(pl, inclined):
        return PRIOR, None, cnts
    num = _num(pl[0][1])
    w = richardson_weights(mult, num)
    order = [sorted((i for i in range(len(t)) if (t[i] >= 0.0) == fwd), key=lambda i: abs(t[i])) for fwd in (True, False)]
    rv = [0] * len(t)
    status = OK
    for k, sub in enumerate(mult):
        for idx, sign in zip(order, (1.0, -1.0)):
            if not idx:
                continue
            st, out = wh_direction(pl, inclined, hill_factor, [abs(t[i]) for i in idx], sign, dt, sub, cnts[k])
            if st != OK:
                status = st
                break
            for i, o in zip(idx, out):
                rv[i] = rv[i] + w[k] * o
    return status, (rv if status == OK else None), cnts


# ---------------------------------------------------------------------------------------------
# cases (tests/golden/wh_derivs.json)
# ---------------------------------------------------------------------------------------------
def pal_rows(planets):
    return [[float(p.get(k, 0.0)) for k in ("m", "a", "h", "k", "l", "ix", "iy")] for p in planets]


def min_period(pl):
    return min(2.0 * math.pi * math.sqrt(p[1] ** 3 / (1.0 + p[0])) for p in pl)


def to_params(walker, num):
    return [[num(q) for q in p] for p in walker]


def seeded(walker, inclined, num, seeds):
    """walker [np][7] floats -> numbers of type num, kernel rows in seeds {row: (a, b)} hyper-dual"""
    pr = 7 if inclined else 5
    out = to_params(walker, num)
    for row, (a, b) in seeds.items():
        p, q = divmod(row, pr)
        out[p][q] = HyperDual(out[p][q], num(a), num(b), num(0))
    return out


def fd_steps(case, w):
    """Truth's differencing steps: 1e-15 max(|x_i|, FLOOR_i) per row of dir_rows, in mpf."""
    pr = 7 if case["inclined"] else 5
    out = []
    for row in case["dir_rows"]:
        p, q = divmod(row, pr)
        out.append(mpf(FD_REL) * max(abs(mpf(case["walkers"][w][p][q])), mpf(FLOOR[q])))
    return out


def fd_points(case):
    """Stencil of the truth: [(key, {dir index: sign})]: the centre, +-e_i, and the four corners of each i > j."""
    R = len(case["dir_rows"])
    pts = [("0", {})]
    for i in range(R):
        pts += [(f"{i}+", {i: 1}), (f"{i}-", {i: -1})]
    for i in range(R):
        for j in range(i):
            pts += [(f"{i}{a}{j}{b}", {i: 1 if a == "+" else -1, j: 1 if b == "+" else -1}) for a in "+-" for b in "+-"]
    return pts


def eval_point(case, w, shifts, dps=TRUTH_DPS):
    """One mpf run of walker w with dir_rows[i] shifted by shifts[i] steps: (status, rv, counters)."""
    with mp.workdps(dps):
        pr = 7 if case["inclined"] else 5
        pl = to_params(case["walkers"][w], mpf)
        d = fd_steps(case, w)
        for i, s in shifts.items():
            p, q = divmod(case["dir_rows"][i], pr)
            pl[p][q] = pl[p][q] + s * d[i]
        return whx_rv(pl, case["inclined"], case["hill"], case["epochs"], case["dt"], case["levels"])


def truth_from_runs(case, w, runs):
    """runs {key: rv list} -> (rv [E], rv_i [R][E], rv_ij [R(R+1)/2][E], pairs i >= j in the kernel's order)."""
    assert mp.dps >= TRUTH_DPS
    R, E = len(case["dir_rows"]), len(case["epochs"])
    d = fd_steps(case, w)
    f0 = runs["0"]
    rv_i = [[(runs[f"{i}+"][e] - runs[f"{i}-"][e]) / (2 * d[i]) for e in range(E)] for i in range(R)]
    rv_ij = []
    for i in range(R):
        for j in range(i + 1):
            if i == j:
                rv_ij.append([(runs[f"{i}+"][e] - 2 * f0[e] + runs[f"{i}-"][e]) / (d[i] * d[i]) for e in range(E)])
            else:
                rv_ij.append([(runs[f"{i}+{j}+"][e] - runs[f"{i}+{j}-"][e] - runs[f"{i}-{j}+"][e] + runs[f"{i}-{j}-"][e])
                              / (4 * d[i] * d[j]) for e in range(E)])
    return f0, rv_i, rv_ij


def hd_run(case, w, i, j, num=float):
    """One hyper-dual run for the pair of dir_rows (i, j): (status, rv [E] of HyperDual)."""
    ri, rj = case["dir_rows"][i], case["dir_rows"][j]
    seeds = {ri: (1, 1)} if ri == rj else {ri: (1, 0), rj: (0, 1)}
    pl = seeded(case["walkers"][w], case["inclined"], num, seeds)
    st, rv, _ = whx_rv(pl, case["inclined"], case["hill"], case["epochs"], case["dt"], case["levels"])
    return st, rv


def hd_derivs(case, w, num=float):
    """The hyper-dual restatement, a pair per run as the kernel does: (rv, rv_i, rv_ij) like truth_from_runs."""
    R, E = len(case["dir_rows"]), len(case["epochs"])
    rv, rv_i, rv_ij = None, [None] * R, []
    for i in range(R):
        for j in range(i + 1):
            st, out = hd_run(case, w, i, j, num)
            assert st == OK
            rv_ij.append([o.ab for o in out])
            if i == j:
                rv_i[i] = [o.a for o in out]
                rv = [o.v for o in out]
    return rv, rv_i, rv_ij


def _ball(base, W, rel, seed):
    rng = np.random.default_rng(seed)  # test_gpu_logl._ball
    P = np.repeat(np.array(base)[None], W, 0)
    P[:, :, :5] *= 1 + rel * rng.standard_normal((W, len(base), 5))
    return P.tolist()


S2_PLANETS = [{"m": 1.2e-3, "a": 0.88, "h": 0.218, "k": 0.015, "l": 0.3},
              {"m": 2.1e-3, "a": 1.44 + 0.11, "h": 0.16, "k": 0.02, "l": 2.2}]  # conftest.S2_PLANETS
EXTRA_PLANETS = [{"m": 1e-3, "a": 2.6, "h": 0.05, "k": 0.0, "l": 1.0},
                 {"m": 5e-4, "a": 4.1, "h": -0.03, "k": 0.02, "l": 4.0}]  # test_gpu_logl.EXTRA_PLANETS
S2_INCLINED = [dict(S2_PLANETS[0], ix=0.12, iy=-0.05), dict(S2_PLANETS[1], ix=0.04, iy=0.18)]  # test_gpu_logl
ECCENTRIC = [{"m": 1e-3, "a": 1.0, "h": 0.48, "k": 0.36, "l": 0.9}]  # e = 0.6, pericentre (l = 0.927) inside the span


def case_inputs():
    """The cases' inputs {name: dict}: walkers [W][np][7], inclined, levels, dt, epochs, dir_rows, hill."""
    def case(planets, walkers, levels, spo, epochs, dir_rows=None, hill=1.0):
        inclined = any("ix" in p for p in planets)
        walkers = [pal_rows(planets)] if walkers is None else walkers
        rows = list(range((7 if inclined else 5) * len(planets))) if dir_rows is None else dir_rows
        pmin = min_period(pal_rows(planets))  # the nominal planets', as test_gpu_logl._plan
        return dict(walkers=walkers, inclined=inclined, levels=list(levels), spo=spo, dt=pmin / spo,
                    period_hint=pmin, epochs=epochs, dir_rows=rows, hill=hill)

    L4 = (4, 5, 6, 7)
    four = S2_PLANETS + EXTRA_PLANETS
    four = [dict(p, ix=0.03 * (i + 1), iy=-0.02 * i) for i, p in enumerate(four)]
    inc2 = [pal_rows(S2_INCLINED), pal_rows(S2_INCLINED)]
    inc2[1][0][5] = inc2[1][0][6] = 0.0  # walker 2: planet 1 at the zero-inclination point
    return {
        "s2": case(S2_PLANETS, _ball(pal_rows(S2_PLANETS), 2, 1e-3, 0), L4, 8.0, [-5.1, -2.0, 0.0, 1.3, 1.3, 4.7]),
        "t0_only": case(S2_PLANETS, None, L4, 8.0, [0.0, 0.0]),
        "t0_only_inclined": case(S2_INCLINED, None, L4, 8.0, [0.0, 0.0]),
        "eccentric": case(ECCENTRIC, None, (1, 2, 3), 8.0, [-3.0, 2.0, 4.5]),
        "three": case(S2_PLANETS + EXTRA_PLANETS[:1], None, L4, 8.0, [-2.0, 1.0, 3.0]),
        # two rows per planet, scrambled: ix3, a1, l2, m4, iy1, h3, k4, a2
        "four_inclined": case(four, None, L4, 8.0, [-1.5, 2.5], dir_rows=[19, 1, 11, 21, 6, 16, 24, 8]),
        "inclined2": case(S2_INCLINED, inc2, L4, 8.0, [-2.0, 0.0, 3.1]),
        "six_levels": case(S2_PLANETS, None, (4, 5, 6, 7, 8, 9), 6.0, [-1.9, 2.4], dir_rows=[1, 6, 2, 9, 0, 4]),
        "five_levels_inclined": case(S2_INCLINED[:1], None, (1, 2, 3, 4, 5), 12.0, [1.0, 2.2]),
        "one_level": case(S2_PLANETS, None, (1,), 24.0, [-1.0, 2.0], dir_rows=[4, 1]),
    }


STEPLESS = ("t0_only", "t0_only_inclined")
REGENERATED = ("t0_only", "t0_only_inclined", "one_level")  # cheap enough for the CPU test to regenerate


def fmt(x):
    return mp.nstr(x, DIGITS, min_fixed=0, max_fixed=0)


def make_walker_record(case, w, runs, counters):
    """The fixture's record of one walker: truth (decimal strings), branch counters, the float hyper-dual run."""
    rv, rv_i, rv_ij = truth_from_runs(case, w, runs)
    frv, frv_i, frv_ij = hd_derivs(case, w, float)
    return dict(truth=dict(rv=[fmt(x) for x in rv], rv_i=[[fmt(x) for x in r] for r in rv_i],
                           rv_ij=[[fmt(x) for x in r] for r in rv_ij]),
                counters=counters, float_hd=dict(rv=frv, rv_i=frv_i, rv_ij=frv_ij))


def load_fixture():
    with open(FIXTURE) as f:
        return json.load(f)


# ---------------------------------------------------------------------------------------------
# observation vectors and the likelihood's sums (state.py:264-268)
# ---------------------------------------------------------------------------------------------
SIGMA = 1.5e-4


def offset_factor(case_rec):
    """How far the "offset" vector lies from the model, in units of the signal: observed RV =
    (1 - f) x truth.  f = 1 (observed RV = 0) unless the order-2 term then carries too little of the
    Hessian (second_order_share above 0.25 for fewer than half of the entries of some walker); then
    the smallest power of two for which it does.  Cases without a step keep f = 1."""
    E = len(case_rec["epochs"])
    truth = [float(x) for x in case_rec["walkers_out"][0]["truth"]["rv"]]
    f = 1.0
    while not all(t == 0.0 for t in case_rec["epochs"]) and f < 1024.0:
        obs = [(1.0 - f) * x for x in truth]
        if all(np.mean(np.array(second_order_share(r["truth"]["rv"], r["truth"]["rv_i"], r["truth"]["rv_ij"], obs,
                                                   [SIGMA] * E)) > 0.25) >= 0.5 for r in case_rec["walkers_out"]):
            break
        f *= 2.0
    return f


def observation_vectors(case_rec):
    """{"fit": truth RV of walker 0 + a fixed pseudo-random 1-sigma offset, "offset": (1 - f) x that
    truth, f = offset_factor: zeros unless the case needs more (the residual is the whole signal or
    more, so r rv_ij carries a large share of the Hessian)} -> observed RVs."""
    truth = np.array([float(x) for x in case_rec["walkers_out"][0]["truth"]["rv"]])
    rng = np.random.default_rng(20261020)
    return {"fit": (truth + SIGMA * rng.standard_normal(len(truth))).tolist(),
            "offset": ((1.0 - offset_factor(case_rec)) * truth).tolist()}


def assemble(rv, rv_i, rv_ij, obs_rv, sigma, npoints, num=mpf):
    """(logp, grad [R], hess [R][R]) from the per-epoch RV and its derivatives: logp = -chi2/N,
    chi2 = sum r^2/s^2, dchi2_i = sum 2 r rv_i/s^2, d2chi2_ij = sum 2 (rv_i rv_j + r rv_ij)/s^2."""
    R, E = len(rv_i), len(rv)
    rv = [num(x) for x in rv]
    rv_i = [[num(x) for x in r] for r in rv_i]
    rv_ij = [[num(x) for x in r] for r in rv_ij]
    r = [rv[e] - num(obs_rv[e]) for e in range(E)]
    is2 = [1 / (num(sigma[e]) * num(sigma[e])) for e in range(E)]
    n = num(npoints)
    lp = -sum(r[e] * r[e] * is2[e] for e in range(E)) / n
    g = [-sum(2 * r[e] * rv_i[i][e] * is2[e] for e in range(E)) / n for i in range(R)]
    H = [[None] * R for _ in range(R)]
    p = 0
    for i in range(R):
        for j in range(i + 1):
            H[i][j] = H[j][i] = -sum(2 * (rv_i[i][e] * rv_i[j][e] + r[e] * rv_ij[p][e]) * is2[e] for e in range(E)) / n
            p += 1
    return lp, g, H


def second_order_share(rv, rv_i, rv_ij, obs_rv, sigma):
    """Per Hessian entry (i >= j): sum_e |r rv_ij| / s^2 over sum_e (|rv_i rv_j| + |r rv_ij|) / s^2."""
    E, R = len(rv), len(rv_i)
    out, p = [], 0
    for i in range(R):
        for j in range(i + 1):
            a = sum(abs((float(rv[e]) - obs_rv[e]) * float(rv_ij[p][e])) / sigma[e] ** 2 for e in range(E))
            b = sum(abs(float(rv_i[i][e]) * float(rv_i[j][e])) / sigma[e] ** 2 for e in range(E))
            out.append(a / (a + b) if a + b > 0 else 0.0)
            p += 1
    return out


def s2_bad_walkers(case):
    """Two walkers for the status check: a = 0.01 (prior) and planet 2 on planet 1's orbit (encounter at t = 0)."""
    a, b = ([list(p) for p in case["walkers"][0]] for _ in range(2))
    a[0][1] = 0.01
    b[1][:5] = b[0][:5]
    b[1][1] += 0.01
    return [a, b]


def kernel_rows(walkers, inclined):
    """walkers [C][np][7] -> the kernel's parameter matrix [rows][C] (m, a, h, k, l[, ix, iy] per planet)."""
    pr = 7 if inclined else 5
    return np.array([[wk[p][q] for wk in walkers] for p in range(len(walkers[0])) for q in range(pr)])


def problem(case_rec, vec):
    """One case with one observation vector: the plan's observations, per walker the truth's (logp,
    grad, hess) in mpf and the float hyper-dual restatement's scaled errors against it, and the tier's
    bound: FLOOR_FACTOR x the restatement's largest scaled error over all entries (the caller runs
    this under mp.workdps(TRUTH_DPS))."""
    E = len(case_rec["epochs"])
    obs_rv, sigma, npoints = observation_vectors(case_rec)[vec], [SIGMA] * E, float(E)
    truth, floor = [], []
    for rec in case_rec["walkers_out"]:
        t, f = rec["truth"], rec["float_hd"]
        ref = assemble(t["rv"], t["rv_i"], t["rv_ij"], obs_rv, sigma, npoints, mpf)
        lp, g, H = assemble(f["rv"], f["rv_i"], f["rv_ij"], obs_rv, sigma, npoints, float)
        truth.append(ref)
        floor.append(scaled_errors(g, H, ref[1], ref[2]))
    fg, fH = max(f[0] for f in floor), max(f[1] for f in floor)
    return dict(obs_rv=obs_rv, sigma=sigma, npoints=npoints, truth=truth, floor_grad=fg, floor_hess=fH,
                bound=FLOOR_FACTOR * max(fg, fH))


FLOOR_FACTOR = 3.0  # test_gpu_logl.T1_SENS_FACTOR: the project's margin for a second double-precision implementation


def scaled_errors(g, H, g_ref, H_ref):
    """test_gpu_derivs.scaled_errors: gradient |dg_i| / sqrt|H_ii|, Hessian |dH_ij| / sqrt|H_ii H_jj|."""
    R = len(g_ref)  # (the differences are taken in mpf: the truth carries 30 digits)
    s = [mp.sqrt(abs(mpf(H_ref[i][i]))) for i in range(R)]
    eg = max(abs(mpf(float(g[i])) - g_ref[i]) / s[i] for i in range(R))
    eH = max(abs(mpf(float(H[i][j])) - H_ref[i][j]) / (s[i] * s[j]) for i in range(R) for j in range(R))
    return float(eg), float(eH)
