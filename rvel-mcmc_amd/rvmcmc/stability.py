"""Dynamical stability of posterior states, screened on the device (rvm_stability_init / rvm_stability_advance).

    from rvmcmc import stability
    res = stability.screen(state, X, orbits=1e5)       # X [P][S] device tensor of free-parameter vectors
    res.fraction_stable, res.stable, res.e_max, res.da_over_a
    res = recorder.stability(n_samples=1024, years=1e5)   # states drawn from a recorded chain; res.idx

The states are integrated with the likelihood kernel's Wisdom-Holman map far beyond the observations' span, in
blocks of `sample_every` steps; a state ends at the first block end at which a pair has come within the exit
distance (hill_factor x the largest Hill radius), a planet's elements are not finite, or a planet is beyond r_max.
The running extremes of every planet's osculating Jacobi a and e^2 are kept; an unbound orbit is not a status
but shows as a_min <= 0 or e2_max >= 1.  include/rvmcmc.h states the rule; the result does not depend on how the
span is split into launches.
"""
from __future__ import annotations

import dataclasses
import math

import numpy as np

from . import _lib
from ._lib import _torch
from .periodogram import CODE_TIME_PER_DAY

CODE_TIME_PER_YEAR = 365.25 * CODE_TIME_PER_DAY
# Steps per launch: one launch of 1024 two-planet states stays under about a second on the MI355X -- 3.3e5
# steps per second of a wave of 32 such states (scripts/stability_bench.py): 0.8 s
DEFAULT_CHUNK_STEPS = 1 << 18


@dataclasses.dataclass
class StabilityResult:
    """Host arrays over the S screened states ([NP][S] for the per-planet ones)."""
    status: np.ndarray          # [S] RVM_STATUS_OK / PRIOR / ENCOUNTER / NONFINITE / ESCAPE
    steps: np.ndarray           # [S] Wisdom-Holman steps completed
    t_end_years: np.ndarray     # [S] steps x h in years
    stable: np.ndarray          # [S] OK over the whole span
    fraction_stable: float
    a_min: np.ndarray           # [NP][S]
    a_max: np.ndarray
    e_max: np.ndarray           # sqrt of e2_max clipped at 0
    unbound: np.ndarray         # [S] some planet's a_min <= 0 or e2_max >= 1
    da_over_a: np.ndarray       # [NP][S] largest excursion of a relative to its t = 0 value
    h: float                    # step, code time
    n_steps: int                # steps of the whole span
    idx: object = None          # ChainRecorder.stability: the drawn states' indices into chain() (device)
    X: object = None            # return_samples: the free-parameter vectors [P][S] (device)
    params: object = None       # ... the kernel rows [R][S]
    xv: object = None           # ... [6][NP][S]
    ext: object = None          # ... [3][NP][S]
    status_dev: object = None
    steps_dev: object = None


class Screen:
    """The device arrays of one screen and the two launches on them (the ABI, argument for argument)."""

    def __init__(self, params, n_planets, inclined, hill_factor):
        torch = _torch()
        rows = (7 if inclined else 5) * n_planets
        if (not torch.is_tensor(params) or params.dtype != torch.float64 or params.dim() != 2
                or params.shape[0] != rows or params.shape[1] < 1 or not params.is_cuda):
            raise ValueError(f"params must be a float64 device tensor [{rows}][n]")
        self.lib = _lib.load()
        self.params = params.contiguous()
        self.n_planets, self.inclined, self.hill_factor = int(n_planets), int(bool(inclined)), float(hill_factor)
        self.n = n = int(params.shape[1])
        dev = params.device
        self.device = dev
        self.xv = torch.empty((6, n_planets, n), dtype=torch.float64, device=dev)
        self.ext = torch.empty((3, n_planets, n), dtype=torch.float64, device=dev)
        self.status = torch.empty(n, dtype=torch.int32, device=dev)
        self.steps = torch.empty(n, dtype=torch.int64, device=dev)
        self.n_alive = torch.empty(1, dtype=torch.int64, device=dev)

    def init(self):
        with _torch().cuda.device(self.device):
            _lib.check(self.lib.rvm_stability_init(self.n_planets, self.inclined, self.n, self.params.data_ptr(),
                                                   self.hill_factor, self.xv.data_ptr(), self.ext.data_ptr(),
                                                   self.status.data_ptr(), self.steps.data_ptr(),
                                                   _lib.stream_handle()), "rvm_stability_init")
        return self

    def advance(self, h, sample_every, n_blocks, r_max=0.0, count=True):
        """n_blocks blocks of sample_every steps of size h for every state still OK; launches only."""
        with _torch().cuda.device(self.device):
            _lib.check(self.lib.rvm_stability_advance(self.n_planets, self.inclined, self.n, self.params.data_ptr(),
                                                      self.hill_factor, float(h), int(sample_every), int(n_blocks),
                                                      float(r_max), self.xv.data_ptr(), self.ext.data_ptr(),
                                                      self.status.data_ptr(), self.steps.data_ptr(),
                                                      self.n_alive.data_ptr() if count else 0,
                                                      _lib.stream_handle()), "rvm_stability_advance")
        return self


def kepler_periods(K, n_planets, inclined):
    """(P [NP][S], a [NP][S], valid [NP][S]) on the device from kernel rows K: P = 2 pi sqrt(a^3 / (1 + m)); valid
    where a and m are finite and positive."""
    torch = _torch()
    pr = 7 if inclined else 5
    m, a = K[0::pr][:n_planets], K[1::pr][:n_planets]
    valid = torch.isfinite(a) & torch.isfinite(m) & (a > 0) & (m > 0)
    P = 2.0 * math.pi * torch.sqrt(a * a * a / (1.0 + m))
    return P, a, valid


def screen(state, samples, years=None, orbits=1e4, steps_per_orbit=20, sample_every=None, r_max=None,
           hill_factor=None, pmap=None, chunk_steps=None, return_samples=False):
    """StabilityResult of the states samples [P][S] (a device tensor of free-parameter vectors, as
    ChainRecorder.predict(samples=...) takes; pmap, default the state's map, expands them to kernel rows on the
    device).  h = P_min / steps_per_orbit with P_min the shortest Kepler period over all samples and planets (one
    device reduction); the span is orbits x P_min, or `years`; sample_every defaults to steps_per_orbit // 4 (at
    least 1), r_max to 100 x the largest a, hill_factor to the state's.  The host loops rvm_stability_advance in
    launches of chunk_steps steps, reads the count of states still alive after each and stops early at 0."""
    torch = _torch()
    pmap = pmap or state.param_map()
    if not torch.is_tensor(samples) or samples.dtype != torch.float64 or samples.dim() != 2 or not samples.is_cuda:
        raise ValueError("samples must be a float64 device tensor [n_params][S]")
    if steps_per_orbit < 1:
        raise ValueError("steps_per_orbit must be at least 1")
    K = pmap.to_kernel(samples.contiguous()).contiguous()
    hf = state.hillRadiusFactor if hill_factor is None else float(hill_factor)
    with torch.cuda.device(K.device):
        P, a, valid = kepler_periods(K, pmap.n_planets, pmap.inclined)
        inf = torch.full_like(P, float("inf"))
        p_min, a_big = torch.stack([torch.where(valid, P, inf).min(), torch.where(valid, a, -inf).max()]).tolist()
    if not math.isfinite(p_min):
        raise ValueError("no sample has a positive semi-major axis and mass: nothing to set the step from")
    h = p_min / steps_per_orbit
    span = orbits * p_min if years is None else years * CODE_TIME_PER_YEAR
    se = max(1, steps_per_orbit // 4) if sample_every is None else int(sample_every)
    if se < 1:
        raise ValueError("sample_every must be at least 1")
    total_blocks = max(1, math.ceil(span / h / se - 1e-9))
    rm = 100.0 * a_big if r_max is None else float(r_max)
    per = max(1, int(DEFAULT_CHUNK_STEPS if chunk_steps is None else chunk_steps) // se)
    sc = Screen(K, pmap.n_planets, pmap.inclined, hf).init()
    a0 = sc.ext[0].clone()
    left = total_blocks
    while left > 0:
        nb = min(per, left, (2 ** 31 - 1) // se)
        sc.advance(h, se, nb, rm)
        left -= nb
        if int(sc.n_alive.item()) == 0:
            break
    out = result_of(sc, a0, h, total_blocks * se)
    if return_samples:
        out = dataclasses.replace(out, X=samples, params=sc.params, xv=sc.xv, ext=sc.ext, status_dev=sc.status,
                                  steps_dev=sc.steps)
    return out


def result_of(sc, a0, h, n_steps):
    """The host result of a finished Screen; a0 [NP][S]: the t = 0 semi-major axes (ext[0] after init)."""
    status, steps = sc.status.cpu().numpy(), sc.steps.cpu().numpy()
    ext, a0 = sc.ext.cpu().numpy(), a0.cpu().numpy()
    a_min, a_max, e2_max = ext[0], ext[1], ext[2]
    stable = status == _lib.RVM_STATUS_OK
    with np.errstate(invalid="ignore", divide="ignore"):
        e_max = np.sqrt(np.clip(e2_max, 0.0, None))
        da = np.maximum(np.abs(a_max - a0), np.abs(a_min - a0)) / np.abs(a0)
        unbound = np.any((a_min <= 0.0) | (e2_max >= 1.0), axis=0)
    return StabilityResult(status=status, steps=steps, t_end_years=steps * h / CODE_TIME_PER_YEAR, stable=stable,
                           fraction_stable=float(stable.mean()), a_min=a_min, a_max=a_max, e_max=e_max,
                           unbound=unbound, da_over_a=da, h=float(h), n_steps=int(n_steps))
