"""Generalised Lomb-Scargle periodograms on the device (rvm_gls.hip; include/rvmcmc.h states the definition).

Before a fit: which periods are in these velocities?

    pg = periodogram.gls(obs)                  # pg.freq, pg.power, pg.period_days
    pg.period_days[np.argmax(pg.power)]

After it: what is left in the residuals of the posterior's RV curves -- ChainRecorder.residual_periodogram
(rvmcmc/chain.py), which runs the same kernels over the rv_out matrix of the drawn states.

Frequencies are in cycles per code time unit; observations.py's 0.01720 code units per day converts
(period_days, freq_of_period_days).  A grid is (f0, df, n_freq): f_k = f0 + k df, k < n_freq.
"""
from __future__ import annotations

import dataclasses

import numpy as np

from . import _lib
from ._lib import _torch, ptr

CODE_TIME_PER_DAY = 0.01720  # observations.py: days * 0.01720 -> code time


def period_days(freq):
    """Period in days of a frequency in cycles per code time unit."""
    with np.errstate(divide="ignore"):
        return 1.0 / (np.asarray(freq, dtype=np.float64) * CODE_TIME_PER_DAY)


def freq_of_period_days(days):
    """Frequency in cycles per code time unit of a period in days."""
    with np.errstate(divide="ignore"):
        return 1.0 / (np.asarray(days, dtype=np.float64) * CODE_TIME_PER_DAY)


def freq_grid(t, oversample=5, fmax=None):
    """(f0, df, n_freq): df = 1 / (oversample T) over the epochs' span T, f0 = df, up to fmax (default: the
    mean Nyquist frequency N / (2 T))."""
    t = np.asarray(t, dtype=np.float64).ravel()
    if len(t) < 2 or not np.all(np.isfinite(t)):
        raise ValueError("a frequency grid needs at least two finite epochs")
    T = float(t.max() - t.min())
    if not T > 0 or not oversample > 0:
        raise ValueError("the epochs must span a positive time and oversample must be positive")
    df = 1.0 / (oversample * T)
    if fmax is None:
        fmax = len(t) / (2.0 * T)
    n_freq = int(np.floor(fmax / df + 1e-9))
    if n_freq < 1:
        raise ValueError("an empty grid: fmax lies below the first frequency 1 / (oversample T)")
    return df, df, n_freq


@dataclasses.dataclass
class Periodogram:
    """power [F] at freq [F] (cycles per code time unit; period_days the same in days)."""
    freq: np.ndarray
    power: np.ndarray
    period_days: np.ndarray


@dataclasses.dataclass
class PeriodogramBands:
    """The residuals' periodogram over the posterior: bands [n_q][F] are the quantiles q of the power at freq
    over the samples whose evaluation succeeded, n_valid [F] how many those were, data_power [F] the data's own
    periodogram on the same grid (what the model removed is the difference).  With return_samples also the
    device tensors X [P][S], idx [S] (None for the caller's samples), status [S], rv [N][S] as the likelihood
    launch wrote them, and power [F][S]."""
    freq: np.ndarray
    q: np.ndarray
    bands: np.ndarray
    n_valid: np.ndarray
    data_power: np.ndarray
    X: object = None
    idx: object = None
    status: object = None
    rv: object = None
    power: object = None


def _grid(grid, t):
    f0, df, n_freq = freq_grid(t) if grid is None else grid
    f0, df, n_freq = float(f0), float(df), int(n_freq)
    if n_freq < 1:
        raise ValueError("an empty grid: n_freq must be at least 1")
    if not (np.isfinite(f0) and np.isfinite(df)):
        raise ValueError("the grid's f0 and df must be finite")
    return f0, df, n_freq


def series_inputs(t, sigma, float_mean=True):
    """(tau, w) float64 host arrays of an observation set: tau = t - (min + max) / 2, w = (1 / sigma^2) / sum.
    ValueError on what no periodogram can be read from."""
    t = np.ascontiguousarray(np.asarray(t, dtype=np.float64).ravel())
    sigma = np.ascontiguousarray(np.asarray(sigma, dtype=np.float64).ravel())
    need = 4 if float_mean else 3
    if len(t) < need:
        raise ValueError(f"a periodogram {'with' if float_mean else 'without'} a floating mean needs at least "
                         f"{need} epochs, got {len(t)}")
    if len(t) > 2 * _lib.RVM_MAX_EPOCHS_PER_DIRECTION:
        raise ValueError(f"at most {2 * _lib.RVM_MAX_EPOCHS_PER_DIRECTION} epochs per periodogram")
    if len(sigma) != len(t):
        raise ValueError("one error per epoch")
    if not np.all(np.isfinite(t)) or not np.all(np.isfinite(sigma)):
        raise ValueError("epochs and errors must be finite")
    if not np.all(sigma > 0):
        raise ValueError("every error must be > 0")
    iv = 1.0 / (sigma * sigma)
    return t - (t.min() + t.max()) / 2.0, iv / iv.sum()


def upload_series(tau, w, data, device):
    """(tau, w, data) as float64 device tensors [N], the form power_on_device takes them in."""
    torch = _torch()
    return tuple(torch.as_tensor(np.ascontiguousarray(a), device=device) for a in (tau, w, data))


def power_on_device(lib, series, model, n_series, grid, float_mean, device):
    """rvm_gls_power on the current stream: (power [F][S], freq [F]) device tensors.  series: upload_series's
    (tau, w, data); model: None or a contiguous device tensor [N][S]."""
    torch = _torch()
    tau, w, data = series
    f0, df, F = grid
    N, S = int(tau.numel()), int(n_series)
    power = torch.empty((F, S), dtype=torch.float64, device=device)
    freq = torch.empty(F, dtype=torch.float64, device=device)
    ws = _lib.workspace(lib.rvm_gls_workspace_bytes(N, F, S), torch.float64, device, floor=2)
    _lib.check(lib.rvm_gls_power(tau.data_ptr(), w.data_ptr(), N, data.data_ptr(), ptr(model), S, S, f0, df, 0, F,
                                 1 if float_mean else 0, power.data_ptr(), S, freq.data_ptr(), ws.data_ptr(),
                                 _lib.stream_handle()), "rvm_gls_power")
    return power, freq


def gls(obs, grid=None, float_mean=True, device=None):
    """Periodogram of the observed velocities themselves: one series, no model.  grid: (f0, df, n_freq),
    default freq_grid of the epochs.  Synchronises for the [F] results."""
    from . import engine

    t, rv, er = engine.obs_arrays(obs)
    tau, w = series_inputs(t, er, float_mean)
    if not np.all(np.isfinite(rv)):
        raise ValueError("the velocities must be finite")
    grid = _grid(grid, t)
    torch = _torch()
    device = torch.device("cuda" if device is None else device)
    lib = _lib.load()
    with torch.cuda.device(device):
        power, freq = power_on_device(lib, upload_series(tau, w, rv, device), None, 1, grid, float_mean, device)
        power, freq = power[:, 0].cpu().numpy(), freq.cpu().numpy()
    return Periodogram(freq=freq, power=power, period_days=period_days(freq))
