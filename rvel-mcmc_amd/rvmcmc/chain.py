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

What the chain says about the posterior (driver.py:265-333 trims the host chain, draws `Ntrails` states'
RV curves over the data and reports the parameters' distribution) is read from the same buffer
(rvm_summary.hip), again with only the results crossing to the host:

    sm = rec.summary(discard=1000)            # sm.mean, sm.sd, sm.quantiles [P][n_q], sm.cov, sm.corr
    X, idx = rec.draw(1024, discard=1000)     # states of the chain, device tensors
    b = rec.predict(times, n_samples=1024, discard=1000)   # b.bands [n_q][n_times]: the RV curve's band

    quantiles   rvm_rows_quantiles: exact order statistics by a radix select, on the chain in place
                and on the rows of the likelihood launch's rv_out matrix
    cov         rvm_chain_cov around the mean of rvm_chain_moments, rvm_chain_autocov's summation order
    draw        rvm_chain_draw: Philox keyed by (seed, sample, draw_id), with replacement

and what the posterior's fits leave in the data (rvm_gls.hip, rvmcmc/periodogram.py):

    pb = rec.residual_periodogram(n_samples=1024, discard=1000)   # pb.bands [n_q][F] at pb.freq, pb.data_power
"""
from __future__ import annotations

import ctypes as C
import dataclasses

import numpy as np

from . import _lib
from ._lib import _torch, ptr
from .observations import Epochs

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


DEFAULT_Q = (0.025, 0.16, 0.5, 0.84, 0.975)  # the median with the 68% and 95% credible intervals


@dataclasses.dataclass
class ChainSummary:
    """The parameter table of the retained steps (numpy arrays).  keys: the state's get_rawkeys();
    mean, sd [P] and quantiles [P][n_q] (of q) over all n_steps n_walkers samples; cov [P][P] around the
    mean with the n - 1 denominator, sd its diagonal's root, corr = cov / (sd sd') with a unit diagonal."""
    keys: list
    q: np.ndarray
    mean: np.ndarray
    sd: np.ndarray
    quantiles: np.ndarray
    cov: np.ndarray
    corr: np.ndarray
    n_steps: int
    n_walkers: int


@dataclasses.dataclass
class RvBands:
    """The RV curve's credible band: bands [n_q][n_times] are the quantiles q of the model RV at `times`
    over the samples whose evaluation succeeded, n_valid [n_times] how many those were.  With
    return_samples also the device tensors X [P][S] (the samples), idx [S] (where in the chain they were
    drawn; None for the caller's samples), status [S] and rv [n_times][S] as the likelihood launch wrote
    them (columns with status != RVM_STATUS_OK are left out of the bands)."""
    times: np.ndarray
    q: np.ndarray
    bands: np.ndarray
    n_valid: np.ndarray
    X: object = None
    idx: object = None
    status: object = None
    rv: object = None


def _q_array(q):
    q = np.atleast_1d(np.asarray(q, dtype=np.float64)).ravel()
    if not 1 <= len(q) <= _lib.RVM_MAX_QUANTILES or not np.all((q >= 0.0) & (q <= 1.0)):
        raise ValueError(f"q must hold 1 to {_lib.RVM_MAX_QUANTILES} values in [0, 1]")
    return np.ascontiguousarray(q)


def _rows_quantiles(lib, ptr, n_rows, row_stride, n_outer, outer_stride, n_inner, q, device):
    """rvm_rows_quantiles on the current stream: (out [n_rows][n_q], n_valid [n_rows]) device tensors."""
    torch = _torch()
    out = torch.empty((n_rows, len(q)), dtype=torch.float64, device=device)
    n_valid = torch.empty(n_rows, dtype=torch.int64, device=device)
    ws = _lib.workspace(lib.rvm_rows_quantiles_workspace_bytes(n_rows, len(q)), torch.int64, device)
    qc = (C.c_double * len(q))(*q)
    _lib.check(lib.rvm_rows_quantiles(ptr, n_rows, row_stride, n_outer, outer_stride, n_inner, qc, len(q),
                                      out.data_ptr(), n_valid.data_ptr(), ws.data_ptr(), _lib.stream_handle()),
               "rvm_rows_quantiles")
    return out, n_valid


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
        self._epochs = None  # predict(): (the epochs' bytes, their observation set with its cached plan)

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
                                                     ptr(lnp if lslot is not None else None), ptr(lslot), sh),
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
                                  _lib.workspace(nbytes, torch.float64, self.device))
        acov, ws = self._work[n_lags]
        _lib.check(self.lib.rvm_chain_autocov(self._chain.data_ptr(), mean.data_ptr(), self.n_params, self.n_walkers,
                                              t0, t1, lag0, n_lags, acov.data_ptr(), ws.data_ptr(),
                                              _lib.stream_handle()), "rvm_chain_autocov")
        return acov

    def diagnostics(self, discard=0, c=5.0):
        """ChainDiagnostics of the recorded steps [discard, n).  Synchronises: one small [P][n_lags]
        copy per lag block of the window search, and the [P] results."""
        torch = _torch()
        t0, t1 = self._range(discard)
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

    # ---- the posterior -----------------------------------------------------------------------------
    def _range(self, discard):
        t0, t1 = int(discard), self.n
        if t0 < 0 or t0 >= t1:
            raise ValueError(f"discard must leave at least one of the {self.n} recorded steps")
        return t0, t1

    def summary(self, discard=0, q=DEFAULT_Q):
        """ChainSummary of the recorded steps [discard, n): per parameter the mean, the standard deviation
        and the quantiles q (rvm_rows_quantiles over the chain in place), and the parameters' covariance
        around the mean (rvm_chain_cov) with its correlation matrix.  Synchronises: only the [P], [P][n_q]
        and [P][P] results cross to the host."""
        torch = _torch()
        t0, t1 = self._range(discard)
        n, W, P = t1 - t0, self.n_walkers, self.n_params
        q = _q_array(q)
        with torch.cuda.device(self.device):
            mean, _ = self._moments(t0, t1, 0)
            center = mean.mean(1).contiguous()  # (diagnostics()'s mean, the same operations)
            quant, _ = _rows_quantiles(self.lib, self._chain.data_ptr() + 8 * t0 * P * W, P, W, n, P * W, W, q,
                                       self.device)
            cov = torch.empty((P, P), dtype=torch.float64, device=self.device)
            ws = _lib.workspace(self.lib.rvm_chain_cov_workspace_bytes(P, W), torch.float64, self.device)
            _lib.check(self.lib.rvm_chain_cov(self._chain.data_ptr(), P, W, t0, t1, center.data_ptr(), cov.data_ptr(),
                                              ws.data_ptr(), _lib.stream_handle()), "rvm_chain_cov")
            center, quant, cov = center.cpu().numpy(), quant.cpu().numpy(), cov.cpu().numpy()
        with np.errstate(divide="ignore", invalid="ignore"):
            sd = np.sqrt(np.diag(cov))
            corr = cov / (sd[:, None] * sd[None, :])
        corr[np.diag_indices(P)] = np.where(sd > 0, 1.0, np.nan)
        state = getattr(self.sampler, "state", None)
        keys = list(state.get_rawkeys()) if state is not None else [str(p) for p in range(P)]
        return ChainSummary(keys=keys, q=q, mean=center, sd=sd, quantiles=quant, cov=cov, corr=corr, n_steps=n,
                            n_walkers=W)

    def draw(self, n_samples, discard=0, seed=0, draw_id=0):
        """(X [P][S], idx [S]) device tensors: n_samples states of the recorded steps [discard, n), uniform
        with replacement (rvm_chain_draw; Philox keyed by seed, sample and draw_id, so a call repeats);
        idx = step * n_walkers + walker into chain().  Launches only."""
        torch = _torch()
        t0, t1 = self._range(discard)
        S = int(n_samples)
        if S < 1:
            raise ValueError("n_samples must be at least 1")
        X = torch.empty((self.n_params, S), dtype=torch.float64, device=self.device)
        idx = torch.empty(S, dtype=torch.int64, device=self.device)
        with torch.cuda.device(self.device):
            _lib.check(self.lib.rvm_chain_draw(self._chain.data_ptr(), self.n_params, self.n_walkers, t0, t1, S,
                                               int(seed), int(draw_id), 0, X.data_ptr(), idx.data_ptr(),
                                               _lib.stream_handle()), "rvm_chain_draw")
        return X, idx

    def _evaluator(self, with_obs, lacks):
        """(state, obs) of the sampler, what predict() and residual_periodogram() evaluate the RV with: TypeError
        `has no <lacks>` without a state and a parameter map (with_obs: and an observation set, else obs is None)."""
        sampler = self.sampler
        state, obs = getattr(sampler, "state", None), getattr(sampler, "obs", None) if with_obs else None
        if state is None or (with_obs and obs is None) or not hasattr(sampler, "pmap"):
            raise TypeError(f"{type(sampler).__name__} has no {lacks}")
        return state, obs

    def _model_rv(self, state, obs, n_samples, discard, seed, samples):
        """(masked, kept): n_samples states drawn from the steps [discard, n), or the caller's samples [P][S]; one
        likelihood launch with rv_out on obs (the sampler's parameter map and Hill factor).  masked: rv
        [n_epochs][S], NaN in the columns that are not RVM_STATUS_OK; kept: the return_samples fields."""
        torch = _torch()
        X, idx = (samples, None) if samples is not None else self.draw(n_samples, discard, seed)
        if (not torch.is_tensor(X) or X.dtype != torch.float64 or X.dim() != 2 or X.shape[0] != self.n_params
                or X.shape[1] < 1 or X.device != self._chain.device):
            raise ValueError("samples must be a float64 tensor [n_params][S] on the recorder's device")
        X = X.contiguous()
        hf = getattr(self.sampler, "hill_factor", state.hillRadiusFactor)
        with torch.cuda.device(self.device):
            _, status, rv = state.get_logp_batch(obs, X, hill_factor=hf, want_rv=True, pmap=self.sampler.pmap)
            masked = torch.where((status == _lib.RVM_STATUS_OK)[None, :], rv, torch.full_like(rv, float("nan")))
        return masked, dict(X=X, idx=idx, status=status, rv=rv)

    def _bands(self, rows, q):
        """(bands [n_q][n_rows], n_valid [n_rows]) on the host: rvm_rows_quantiles of a device matrix [n_rows][S]."""
        n_rows, S = (int(v) for v in rows.shape)
        with _torch().cuda.device(self.device):
            bands, n_valid = _rows_quantiles(self.lib, rows.data_ptr(), n_rows, S, 1, S, S, q, self.device)
            return np.ascontiguousarray(bands.cpu().numpy().T), n_valid.cpu().numpy()

    def predict(self, times, n_samples=1024, discard=0, q=DEFAULT_Q, seed=0, samples=None, return_samples=False):
        """RvBands: the quantiles q of the model RV at `times` over n_samples states drawn from the recorded
        steps [discard, n) (or over the caller's samples [P][S], a device tensor of free-parameter vectors)
        -- the credible band the reference draws as `Ntrails` ghost curves (driver.py:265-333).  One
        likelihood launch with rv_out on a plan built on `times` (as State.get_rv: the sampler's state,
        parameter map and Hill factor; for PTSampler the cold temperature, which is what is recorded), the
        columns of samples that are not RVM_STATUS_OK masked to NaN, then rvm_rows_quantiles over the
        epochs' rows; n_valid counts the samples behind each epoch.  At most RVM_MAX_EPOCHS_PER_DIRECTION
        epochs with t >= 0 and as many with t < 0 (ValueError beyond).  Synchronises for the [n_q][n_times]
        result."""
        times = np.ascontiguousarray(np.asarray(times, dtype=np.float64).ravel())
        if len(times) < 1 or not np.all(np.isfinite(times)):
            raise ValueError("times must be a non-empty array of finite epochs")
        cap = _lib.RVM_MAX_EPOCHS_PER_DIRECTION
        if int((times >= 0).sum()) > cap or int((times < 0).sum()) > cap:
            raise ValueError(f"at most {cap} epochs with t >= 0 and {cap} with t < 0 per call "
                             f"(RVM_MAX_EPOCHS_PER_DIRECTION)")
        q = _q_array(q)
        state, _ = self._evaluator(False, "state / pmap: nothing to evaluate the RV with")
        key = times.tobytes()
        if self._epochs is None or self._epochs[0] != key:
            self._epochs = (key, Epochs(times))  # (keeps the plan plan_for caches on it)
        masked, kept = self._model_rv(state, self._epochs[1], n_samples, discard, seed, samples)
        bands, n_valid = self._bands(masked, q)
        out = RvBands(times=times, q=q, bands=bands, n_valid=n_valid)
        return dataclasses.replace(out, **kept) if return_samples else out

    def residual_periodogram(self, grid=None, n_samples=1024, discard=0, q=DEFAULT_Q, seed=0, samples=None,
                             float_mean=True, return_samples=False):
        """PeriodogramBands: the quantiles q, per frequency, of the generalised Lomb-Scargle power of the
        residuals (observed RV - model RV) over n_samples states drawn from the recorded steps [discard, n)
        (or over the caller's samples [P][S]) -- what the posterior's fits leave in the data.  One likelihood
        launch with rv_out on the sampler's own observation set (state, parameter map and Hill factor as in
        predict()), the columns that are not RVM_STATUS_OK masked to NaN, rvm_gls_power with that matrix as
        the model, then rvm_rows_quantiles over the [F][S] rows; data_power is the data's own periodogram on
        the same grid.  grid: (f0, df, n_freq), default periodogram.freq_grid of the epochs.  Synchronises
        for the [n_q][F], [F] and [F] results."""
        from . import engine, periodogram

        state, obs = self._evaluator(True, "obs / state / pmap: nothing to take residuals from")
        t, rvobs, er = engine.obs_arrays(obs)
        tau, w = periodogram.series_inputs(t, er, float_mean)
        grid, q = periodogram._grid(grid, t), _q_array(q)
        masked, kept = self._model_rv(state, obs, n_samples, discard, seed, samples)
        S = int(masked.shape[1])
        with _torch().cuda.device(self.device):
            series = periodogram.upload_series(tau, w, rvobs, self.device)
            power, freq = periodogram.power_on_device(self.lib, series, masked.contiguous(), S, grid, float_mean,
                                                      self.device)
            data_power, _ = periodogram.power_on_device(self.lib, series, None, 1, grid, float_mean, self.device)
            bands, n_valid = self._bands(power, q)
            freq, data_power = freq.cpu().numpy(), data_power[:, 0].cpu().numpy()
        out = periodogram.PeriodogramBands(freq=freq, q=q, bands=bands, n_valid=n_valid, data_power=data_power)
        return dataclasses.replace(out, power=power, **kept) if return_samples else out

    def stability(self, n_samples=1024, discard=0, seed=0, samples=None, **screen_kwargs):
        """stability.StabilityResult of n_samples states drawn from the recorded steps [discard, n) (or of the
        caller's samples [P][S]): which of the posterior's states survive an integration far beyond the
        observations' span (stability.screen: years / orbits, steps_per_orbit, sample_every, r_max,
        chunk_steps, return_samples).  The sampler's state, parameter map and Hill factor as in predict(); idx
        [S], the drawn states' indices into chain() (None with the caller's samples), restricts a summary to
        the stable subset.  Synchronises after every launch of chunk_steps steps."""
        from . import stability

        state, _ = self._evaluator(False, "state / pmap: nothing to integrate the states with")
        X, idx = (samples, None) if samples is not None else self.draw(n_samples, discard, seed)
        screen_kwargs.setdefault("hill_factor", getattr(self.sampler, "hill_factor", state.hillRadiusFactor))
        screen_kwargs.setdefault("pmap", self.sampler.pmap)
        return dataclasses.replace(stability.screen(state, X, **screen_kwargs), idx=idx)


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
