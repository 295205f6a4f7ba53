"""The recorded chain and its convergence read-out, device-resident.

The reference's production workflow (driver.py:86-120 run, :265-333 trim the burn-in, :343-414
autocorrelation times and efficacy) goes through the host every iteration.  Here a ChainRecorder keeps
every `thin`-th step of a sampler in HBM as [n_steps][P][W] float64 (rvm_chain_record: a strided gather
of the sampler's own SoA blocks, one launch per segment), and diagnostics() reads the per-parameter
integrated autocorrelation time, ESS and split-R-hat from it with only a [P][n_lags] array crossing to
the host:

    mean, m2 per column                       rvm_chain_moments
    acov[p][k] = 1/W sum_w sum_t y_t y_t+k    rvm_chain_autocov, for the lags [0, 64), [64, 128),
                                              [128, 256), ... -- each call computes only the new lags
    tau(m) = 2 sum_{k <= m} acov[k]/acov[0] - 1 ;  window = the smallest m with m >= c tau(m)

which is driver.integrated_time's walker-averaged-ACF Sokal window without the full ACF: the search
stops at the first window (a few tau), where the FFT computes all n lags.

    rec = ChainRecorder(sampler, capacity=8000)
    sampler.run_mcmc(8000, rec)
    d = rec.diagnostics(discard=1000)         # d.tau, d.ess, d.rhat, d.long_enough
"""
from __future__ import annotations

import dataclasses

import numpy as np

from . import _lib


def _torch():
    import torch

    return torch


LAG_BLOCK0 = 64  # the first two lag blocks of the window search: [0, 64), [64, 128), then doubling


def lag_blocks(n):
    """The window search's lag ranges [(lo, hi)] over the lags 0 .. n - 1."""
    out, lo, hi = [], 0, LAG_BLOCK0
    while lo < n:
        out.append((lo, min(hi, n)))
        lo, hi = hi, 2 * hi
    return out


class WindowSearch:
    """driver.integrated_time's Sokal window of one parameter, fed the autocovariance block by block
    (same float64 operations in the same order: acov / acov[0], a running sum, 2 sum - 1).  done once
    the window is found, acov[0] <= 0 (tau = nan) or the last lag n - 1 was fed (tau = taus[n - 1])."""

    def __init__(self, n, c=5.0):
        self.n, self.c = int(n), float(c)
        self.done, self.tau, self.window = False, float("nan"), -1
        self._a0, self._sum, self._k = None, 0.0, 0

    def feed(self, acov_block):
        a = np.asarray(acov_block, dtype=np.float64)
        if self.done or len(a) == 0:
            return
        if self._a0 is None:
            self._a0 = a[0]
            if not a[0] > 0:  # (integrated_time: acf[0] <= 0 -> nan)
                self.done = True
                return
        acf = a / self._a0
        sums = np.cumsum(np.concatenate([[self._sum], acf]))[1:] if self._k else np.cumsum(acf)
        taus = 2.0 * sums - 1.0
        inside = np.arange(self._k, self._k + len(a)) < self.c * taus
        if not inside.all():
            i = int(np.argmin(inside))
            self.done, self.tau, self.window = True, float(taus[i]), self._k + i
            return
        self._sum, self._k = sums[-1], self._k + len(a)
        if self._k >= self.n:  # no window: taus[n - 1]
            self.done, self.tau, self.window = True, float(taus[-1]), self.n - 1


@dataclasses.dataclass
class ChainDiagnostics:
    """Per-parameter read-out of the retained steps (numpy [P] arrays).  tau: integrated
    autocorrelation time in recorded steps (multiply by the recorder's thin for iterations); window:
    the Sokal window it was summed to; ess = n_steps n_walkers / tau; rhat: split-R-hat over the
    2 n_walkers half-chains; mean, var: over all retained samples; long_enough: n_steps >= 50 max tau
    (emcee's rule of thumb) with every window found before the last lag -- False when a tau is nan, and
    when the chain is too short for a window (tau is then taus[n_steps - 1], window = n_steps - 1)."""
    tau: np.ndarray
    window: np.ndarray
    ess: np.ndarray
    rhat: np.ndarray
    mean: np.ndarray
    var: np.ndarray
    n_steps: int
    n_walkers: int
    long_enough: bool


class ChainRecorder:
    """Every thin-th step of `sampler` (EnsembleSampler, PTSampler, MhChains, SmalaChains), kept on the
    sampler's device.  capacity: step slots, allocated once -- push() at capacity raises ValueError; the
    buffer never grows and never wraps.  walker_stride: every walker_stride-th walker of each of the
    sampler's segments is recorded (bench.py records 1024 of 4096 this way: the walker-averaged ACF of
    a subset estimates tau as well; ESS then counts the recorded walkers).  lnprob: also keep the
    log-probabilities.  Unpushed slots hold NaN.

    Where the positions live comes from the sampler's _chain_segments(): both halves of the stretch
    ensemble (half 0's walkers first, the order of gather_positions()); for PTSampler the coldest
    temperature, beta = betas[0]; on a sharded EnsembleSampler this rank's own walkers -- each rank
    records and diagnoses its own shard, and combining diagnostics across ranks is out of scope."""

    def __init__(self, sampler, capacity, thin=1, walker_stride=1, lnprob=True):
        torch = _torch()
        capacity, thin, walker_stride = int(capacity), int(thin), int(walker_stride)
        if capacity < 1:
            raise ValueError("capacity must be at least 1")
        if thin < 1:
            raise ValueError("thin must be at least 1")
        if walker_stride < 1:
            raise ValueError("walker_stride must be at least 1")
        if not hasattr(sampler, "_chain_segments"):
            raise TypeError(f"{type(sampler).__name__} has no _chain_segments(): nothing to record from")
        self.sampler = sampler
        self.capacity, self.thin, self.walker_stride = capacity, thin, walker_stride
        self.lib = _lib.load()
        self.device = sampler.device
        segs = sampler._chain_segments()
        self._counts = [len(range(0, s["n"], walker_stride)) for s in segs]
        self.n_params = int(segs[0]["x"].shape[0])
        self.n_walkers = int(sum(self._counts))
        f64 = dict(dtype=torch.float64, device=self.device)
        self._chain = torch.full((capacity, self.n_params, self.n_walkers), float("nan"), **f64)
        self._lnp = torch.full((capacity, self.n_walkers), float("nan"), **f64) if lnprob else None
        self.n = 0          # steps recorded
        self._since = 0     # iterations seen since the last recorded one (observe)
        self._mean = torch.empty((2, self.n_params, self.n_walkers), **f64)
        self._m2 = torch.empty((2, self.n_params, self.n_walkers), **f64)
        self._work = {}     # lag-block length -> (acov [P][L], workspace)

    # ---- recording ---------------------------------------------------------------------------------
    def push(self):
        """Record the sampler's current state into the next slot (launches only, no synchronisation)."""
        torch = _torch()
        if self.n >= self.capacity:
            raise ValueError(f"the chain is full ({self.capacity} steps): a ChainRecorder never grows or wraps")
        segs = self.sampler._chain_segments()
        slot = self._chain[self.n]
        lslot = self._lnp[self.n] if self._lnp is not None else None
        sh = _lib.stream_handle()
        col = 0
        with torch.cuda.device(self.device):
            for s, cnt in zip(segs, self._counts):
                x, lnp = s["x"], s.get("lnp")
                if x.dtype != torch.float64 or x.dim() != 2 or x.stride(1) != 1 or x.shape[0] != self.n_params:
                    raise ValueError("a chain segment must be float64 [n_params][ld] with unit column stride")
                if lslot is not None:
                    if lnp is None:
                        raise ValueError("the sampler has no log-probabilities yet (step() it, or lnprob=False)")
                    if lnp.dtype != torch.float64 or not lnp.is_contiguous() or lnp.numel() < x.shape[1]:
                        raise ValueError("a segment's log-probabilities must be contiguous float64 [ld]")
                ld = x.stride(0) if x.shape[0] > 1 else x.shape[1]  # (a single row's stride means nothing)
                _lib.check(self.lib.rvm_chain_record(self.n_params, cnt, x.data_ptr(), ld, s.get("col0", 0),
                                                     self.walker_stride, slot.data_ptr(), self.n_walkers, col,
                                                     lnp.data_ptr() if lslot is not None else 0,
                                                     lslot.data_ptr() if lslot is not None else 0, sh),
                           "rvm_chain_record")
                col += cnt
        self.n += 1

    def observe(self):
        """One sampler iteration has run: push() on every thin-th call (run_mcmc calls this)."""
        self._since += 1
        if self._since == self.thin:
            self._since = 0
            self.push()

    # ---- the chain ---------------------------------------------------------------------------------
    def chain(self):
        """Device view [n][P][W] of the recorded steps."""
        return self._chain[:self.n]

    def lnprob(self):
        """Device view [n][W] of the recorded log-probabilities."""
        if self._lnp is None:
            raise ValueError("recorded without log-probabilities (lnprob=False)")
        return self._lnp[:self.n]

    def to_numpy(self):
        """The chain on the host in emcee's layout [W][n][P]."""
        return self.chain().permute(2, 0, 1).cpu().numpy()

    # ---- diagnostics -------------------------------------------------------------------------------
    def _moments(self, t0, t1, k):
        _lib.check(self.lib.rvm_chain_moments(self._chain.data_ptr(), self.n_params, self.n_walkers, t0, t1,
                                              self._mean[k].data_ptr(), self._m2[k].data_ptr(), _lib.stream_handle()),
                   "rvm_chain_moments")
        return self._mean[k], self._m2[k]

    def autocov(self, t0, t1, lag0, n_lags, mean):
        """acov [P][n_lags] (device) of the steps [t0, t1) for the lags lag0 .. lag0 + n_lags - 1, around
        `mean` [P][W] (rvm_chain_autocov)."""
        torch = _torch()
        if n_lags not in self._work:
            nbytes = self.lib.rvm_chain_autocov_workspace_bytes(self.n_params, self.n_walkers, n_lags)
            self._work[n_lags] = (torch.empty((self.n_params, n_lags), dtype=torch.float64, device=self.device),
                                  torch.empty(max(nbytes // 8, 1), dtype=torch.float64, device=self.device))
        acov, ws = self._work[n_lags]
        _lib.check(self.lib.rvm_chain_autocov(self._chain.data_ptr(), mean.data_ptr(), self.n_params, self.n_walkers,
                                              t0, t1, lag0, n_lags, acov.data_ptr(), ws.data_ptr(),
                                              _lib.stream_handle()), "rvm_chain_autocov")
        return acov

    def diagnostics(self, discard=0, c=5.0):
        """ChainDiagnostics of the recorded steps [discard, n).  Synchronises: one small [P][n_lags]
        copy per lag block of the window search, and the [P] results."""
        torch = _torch()
        t0, t1 = int(discard), self.n
        if t0 < 0 or t0 >= t1:
            raise ValueError(f"discard must leave at least one of the {self.n} recorded steps")
        n, W, P = t1 - t0, self.n_walkers, self.n_params
        with torch.cuda.device(self.device):
            mean, m2 = self._moments(t0, t1, 0)
            # mean and variance of all n W samples from the columns' moments
            gmean = mean.mean(1)
            dev = mean - gmean[:, None]
            var = (m2.sum(1) + n * (dev * dev).sum(1)) / (n * W - 1) if n * W > 1 else torch.full_like(gmean, float("nan"))
            search = [WindowSearch(n, c) for _ in range(P)]
            for lo, hi in lag_blocks(n):
                block = self.autocov(t0, t1, lo, hi - lo, mean).cpu().numpy()
                for p in range(P):
                    search[p].feed(block[p])
                if all(s.done for s in search):
                    break
            # split-R-hat: the first and the last n // 2 steps of every walker as 2 W chains
            h = n // 2
            if h >= 2:
                ma, qa = self._moments(t0, t0 + h, 0)
                mb, qb = self._moments(t1 - h, t1, 1)
                m = torch.cat([ma, mb], 1)
                within = torch.cat([qa, qb], 1).sum(1) / (2 * W * (h - 1))
                between = h * m.var(1, unbiased=True)
                rhat = torch.sqrt(((h - 1) / h * within + between / h) / within)
            else:
                rhat = torch.full_like(gmean, float("nan"))
            gmean, var, rhat = gmean.cpu().numpy(), var.cpu().numpy(), rhat.cpu().numpy()
        tau = np.array([s.tau for s in search])
        with np.errstate(divide="ignore", invalid="ignore"):
            ess = n * W / tau
        window = np.array([s.window for s in search])
        # (without a window tau is taus[n - 1], which is 0 up to rounding once the walkers' own means are
        # subtracted: such a chain is never long enough, whatever 50 tau says)
        long_enough = bool(n >= 50 * np.max(tau)) and bool(np.all(window < n - 1))
        return ChainDiagnostics(tau=tau, window=window, ess=ess, rhat=rhat, mean=gmean, var=var, n_steps=n,
                                n_walkers=W, long_enough=long_enough)


def run_mcmc(sampler, n_steps, recorder=None):
    """n_steps iterations of sampler.step(), with recorder.observe() after each: every thin-th one is
    recorded.  No host synchronisation beyond step()'s own (its periodic fault check included)."""
    if recorder is not None and recorder.sampler is not sampler:
        raise ValueError("the recorder was built for another sampler")
    for _ in range(int(n_steps)):
        sampler.step()
        if recorder is not None:
            recorder.observe()
    return recorder
