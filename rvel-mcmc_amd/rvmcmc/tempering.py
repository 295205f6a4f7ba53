"""Device-resident parallel-tempering ensemble sampler (tempered emcee stretch move).

T ensembles of W walkers run side by side at inverse temperatures 1 = beta_0 > beta_1 > ... > 0
(temperature 0, the coldest, samples the posterior; temperature t samples prior x likelihood^beta_t,
so the hot ensembles cross between modes that the cold one cannot leave -- period aliases, the
two-resonance ambiguity of HD155358-like systems).  emcee 2.2.1, whose EnsembleSampler
ensemble.py restates, ships a PTSampler of this design next to it.

One iteration:

    for half h in (0, 1):                               (all T temperatures in ONE launch each)
        z, j from (u1, u2) ; q = c_j - z (c_j - x)      (c_j: same temperature, other half)
        lnp(q)                                          (ONE rvm_logl_batch of T W/2 walkers)
        lnpdiff = (dim - 1) ln z + beta_t lnp(q) - beta_t lnp(x) ;  accept if lnpdiff > ln u3
    every swap_every iterations, for pairs p = T-2 .. 0 (hottest first), for every walker index w:
        d = (beta_p - beta_p+1) (lnp[p+1][w] - lnp[p][w]) ;  exchange the two walkers if d > ln u

Positions and log-probabilities stay in HBM: each half is SoA [dim][T * W/2] float64 (column
t * W/2 + k), lnp holds the UNtempered log-probabilities.  Random numbers are counter-based Philox
draws keyed by (seed, iteration, stream, item) with item t * W + h * W/2 + k for the stretch
streams -- at T = 1 exactly EnsembleSampler's global walker index, and PTSampler(1, W, ...) then
reproduces EnsembleSampler's unfused path bit for bit -- and p * W + w on stream 7 for the swaps.

With adapt=True the ladder follows the dynamics of Vousden, Farr & Mandel 2016 (ptemcee's default)
after every exchange sweep, on the device (rvm_pt_ladder_update): with A_p the exchanges per walker
of pair p since the previous update and kappa = (lag / (n + lag)) / adaptation_time at update n,

    dS_i = kappa (A_i - A_i+1) ;  T_i+1 - T_i  <-  (T_i+1 - T_i) exp(dS_i)        (T = 1 / beta)

with both end temperatures fixed (beta = 0 is refused, so the hottest one is finite): a pair that
exchanges less than its hotter neighbour moves closer.  An update whose result is not a strictly
decreasing finite ladder is refused and counted (ladder_refusals()).  The adaptation breaks detailed
balance while it runs -- it dies away as lag / n -- so adapt during burn-in, then freeze_ladder().
record_lnprob(True) then accumulates the per-temperature moments of lnp on the device;
mean_lnprob() and log_evidence_ratio() (thermodynamic integration) read them.

The sampler is unfused (propose / likelihood / accept launches): a ladder of T temperatures already
puts T W/2 walkers into every likelihood launch, which is what the fused and speculative launches
of EnsembleSampler were built to achieve for a single ensemble.  Single process only.
"""
from __future__ import annotations

import math

import numpy as np

from . import _lib, engine
from ._lib import _torch, ptr
from .ensemble import check_walker_count


def default_betas(ntemps, dim):
    """Geometric ladder beta_t = r**-t with r = 1 + 2 sqrt(ln 4) / sqrt(dim): the large-dimension
    spacing at which neighbouring temperatures of a dim-dimensional Gaussian target exchange about
    25 % of the time.  emcee's default ladder uses a tabulated ratio below 100 dimensions; no
    equality with emcee's ladder is claimed."""
    ntemps, dim = int(ntemps), int(dim)
    if ntemps < 1:
        raise ValueError("ntemps must be at least 1")
    if dim < 1:
        raise ValueError("dim must be at least 1")
    r = 1.0 + 2.0 * math.sqrt(math.log(4.0)) / math.sqrt(dim)
    return np.array([r ** -t for t in range(ntemps)], dtype=np.float64)


def _positive(v, name):
    v = float(v)
    if not (math.isfinite(v) and v > 0.0):
        raise ValueError(f"{name} must be finite and > 0")
    return v


def check_betas(betas, ntemps):
    """The ladder as float64 [ntemps]: strictly decreasing, 0 < beta <= 1 (beta = 0 would sample the
    hard prior alone, which is improper in a and m)."""
    b = np.array(betas, dtype=np.float64).reshape(-1)
    if len(b) != ntemps:
        raise ValueError(f"betas must have ntemps = {ntemps} entries, got {len(b)}")
    if not np.all(np.isfinite(b)):
        raise ValueError("betas must be finite")
    if np.any(b <= 0.0):
        raise ValueError("every beta must be > 0 (beta = 0 samples the improper hard prior)")
    if np.any(b > 1.0):
        raise ValueError("every beta must be <= 1")
    if np.any(np.diff(b) >= 0.0):
        raise ValueError("betas must be strictly decreasing (temperature 0 is the coldest)")
    return b


def log_evidence_ratio(betas, mean_lnp):
    """(estimate, coarse) of the integral of mean_lnp d(beta) from betas[-1] up to betas[0]: the
    trapezoid rule over all temperatures, and over every second one (0, 2, 4, ..., and the hottest,
    so that both cover the same range)."""
    b, m = np.asarray(betas, dtype=np.float64), np.asarray(mean_lnp, dtype=np.float64)

    def trapezoid(idx):
        s = 0.0
        for i, j in zip(idx[-2::-1], idx[:0:-1]):  # hottest interval first: (colder i, hotter j)
            s = s + (b[i] - b[j]) * (0.5 * (m[i] + m[j]))
        return float(s)

    fine = list(range(len(b)))
    coarse = fine[::2] if fine[-1] % 2 == 0 else fine[::2] + [fine[-1]]
    return trapezoid(fine), trapezoid(coarse)


class PTSampler(engine.DeviceSampler):
    def __init__(self, ntemps, nwalkers, state, obs, betas=None, a=2.0, seed=0, device=None, hill_factor=None,
                 swap_every=1, adapt=False, adaptation_lag=10000, adaptation_time=100):
        # value checks first: nothing below them touches the device
        dim = state.Nvars
        ntemps, nwalkers = int(ntemps), int(nwalkers)
        if ntemps < 1:
            raise ValueError("ntemps must be at least 1")
        check_walker_count(nwalkers, dim)
        self.betas = check_betas(default_betas(ntemps, dim) if betas is None else betas, ntemps)
        if not float(a) > 1.0:
            raise ValueError("the stretch scale a must be > 1")
        if int(swap_every) < 1:
            raise ValueError("swap_every must be at least 1")
        if ntemps * nwalkers > 2 ** 31 - 1:
            raise ValueError("ntemps * nwalkers must fit a 32-bit index")
        self.adaptation_lag = _positive(adaptation_lag, "adaptation_lag")
        self.adaptation_time = _positive(adaptation_time, "adaptation_time")
        self.adapt = bool(adapt)
        torch = _torch()
        if torch.distributed.is_available() and torch.distributed.is_initialized() \
                and torch.distributed.get_world_size() > 1:
            raise RuntimeError("PTSampler runs in a single process (the ladder is not sharded over ranks)")
        self.ntemps, self.k, self.dim = ntemps, nwalkers, dim
        self.halfk = nwalkers // 2
        self.n = ntemps * self.halfk  # columns per half
        self.a = float(a)
        self.seed = int(seed) & ((1 << 64) - 1)
        self.swap_every = int(swap_every)
        self.state, self.obs = state, obs
        self.pmap = state.param_map()
        self.hill_factor = state.hillRadiusFactor if hill_factor is None else float(hill_factor)
        self.device = engine.default_device(device)
        self.lib = _lib.load()
        self.plan = engine.plan_for_state(state, obs, self.n, self.device)
        f64 = dict(dtype=torch.float64, device=self.device)
        i32 = dict(dtype=torch.int32, device=self.device)
        self._betas = torch.as_tensor(self.betas, device=self.device)
        self._q = torch.empty((dim, self.n), **f64)
        self._z = torch.empty(self.n, **f64)
        self._lnp_new = torch.empty(self.n, **f64)
        self._status = torch.empty(self.n, **i32)
        self.naccepted = torch.zeros((2, self.n), **i32)              # [half][t * W/2 + k]
        self.nswapped = torch.zeros((max(ntemps - 1, 0), nwalkers), **i32)  # [pair][w]
        # the ladder's dynamics and the lnp moments (rvm_pt_ladder_update)
        i64 = dict(dtype=torch.int64, device=self.device)
        self._swap_prev = torch.zeros(max(ntemps - 1, 0), **i64)  # the counter rows' totals at the last update
        self._ratios = torch.zeros(max(ntemps - 1, 0), **f64)     # exchanges per walker since the one before
        self._n_refused = torch.zeros(1, **i64)
        self._moments = torch.zeros((ntemps, 2), **f64)           # [t]: sum lnp, sum lnp^2 while recording
        self._work = torch.empty(3 * ntemps - 1, **f64)
        self.nadapt = 0       # ladder updates so far
        self.nrecorded = 0    # iterations in _moments
        self.recording = False
        self.iteration = 0
        self.nswaps = 0  # exchange sweeps so far
        self.nevals = 0
        self.pos = None
        self.lnp = [None, None]

    # ---- layout: [T][W][...] on the host side <-> per-half [...][T * W/2] on the device -----------
    def _split(self, A):
        """[T][W] (+ trailing axes) tensor -> its two halves [T * W/2] (+ trailing axes)."""
        h = self.halfk
        return [A[:, :h].reshape((self.n,) + tuple(A.shape[2:])), A[:, h:].reshape((self.n,) + tuple(A.shape[2:]))]

    def _join(self, halves):
        """Two per-half tensors [T * W/2] (+ trailing axes) -> [T][W] (+ trailing axes)."""
        torch = _torch()
        return torch.cat([x.reshape((self.ntemps, self.halfk) + tuple(x.shape[1:])) for x in halves], 1)

    def set_positions(self, X):
        """X: [T][W][dim] array-like, walker w of temperature t at X[t][w]."""
        torch = _torch()
        Xg = torch.as_tensor(np.asarray(X, dtype=np.float64), device=self.device)
        if tuple(Xg.shape) != (self.ntemps, self.k, self.dim):
            raise ValueError(f"positions must be [{self.ntemps}][{self.k}][{self.dim}]")
        self.pos = [x.t().contiguous() for x in self._split(Xg)]
        self.lnp = [None, None]

    def _logl(self, X, out=None, status=None):
        lp, st, _ = self.plan.logl(self.pmap.to_kernel(X), hill_factor=self.hill_factor, out=out, status=status)
        self.nevals += X.shape[1]
        return lp, st

    def compute_lnprob(self):
        """The log-probabilities of the current positions; a start that is not finite (prior,
        encounter, non-finite or unresolved likelihood) raises: the tempered accept needs a finite
        lnp on its old side."""
        torch = _torch()
        if self.pos is None:
            raise ValueError("set_positions first")
        self.lnp = [self._logl(self.pos[h])[0].clone() for h in (0, 1)]
        for h in (0, 1):
            if not bool(torch.isfinite(self.lnp[h]).all()):
                bad = int((~torch.isfinite(self.lnp[h])).sum())
                self.lnp = [None, None]
                raise ValueError(f"The initial lnprob was not finite for {bad} walker(s) of half {h}.")

    # ---- one iteration ---------------------------------------------------------------------------
    def _dev(self, a, shape):
        """An injected draw array (numpy or tensor, any shape of the right size) on the device."""
        torch = _torch()
        if a is None:
            return None
        t = torch.as_tensor(np.asarray(a, dtype=np.float64) if not torch.is_tensor(a) else a, device=self.device)
        if t.dtype != torch.float64 or t.numel() != int(np.prod(shape)):
            raise ValueError(f"injected draws must be float64 of shape {tuple(shape)}")
        return t.contiguous()

    def half_step(self, half, u12=None, u3=None):
        """Propose, evaluate and accept half `half` of every temperature.  u12 ([2][T][W/2]: u1, u2)
        and u3 ([T][W/2]) replace the Philox draws when given (tests)."""
        X0, c, lnp0 = self.pos[half], self.pos[1 - half], self.lnp[half]
        dp, da = self._dev(u12, (2, self.n)), self._dev(u3, (self.n,))
        sh = _lib.stream_handle()
        _lib.check(self.lib.rvm_pt_stretch_propose(self.dim, self.ntemps, self.halfk, X0.data_ptr(), c.data_ptr(),
                                                   self.a, self.seed, self.iteration, half, ptr(dp),
                                                   self._q.data_ptr(), self._z.data_ptr(), sh),
                   "rvm_pt_stretch_propose")
        self._logl(self._q, out=self._lnp_new, status=self._status)
        _lib.check(self.lib.rvm_pt_stretch_accept(self.dim, self.ntemps, self.halfk, self._betas.data_ptr(),
                                                  X0.data_ptr(), lnp0.data_ptr(), self._q.data_ptr(),
                                                  self._lnp_new.data_ptr(), self._z.data_ptr(), self.seed,
                                                  self.iteration, half, ptr(da), self.naccepted[half].data_ptr(), sh),
                   "rvm_pt_stretch_accept")

    def swap(self, u=None):
        """One exchange sweep over the neighbouring temperature pairs, hottest pair first.
        u ([T-1][W]) replaces the Philox draws when given (tests)."""
        du = self._dev(u, (max(self.ntemps - 1, 0), self.k))
        _lib.check(self.lib.rvm_pt_swap(self.dim, self.ntemps, self.halfk, self._betas.data_ptr(),
                                        self.pos[0].data_ptr(), self.pos[1].data_ptr(), self.lnp[0].data_ptr(),
                                        self.lnp[1].data_ptr(), self.seed, self.iteration, ptr(du),
                                        self.nswapped.data_ptr(), _lib.stream_handle()), "rvm_pt_swap")
        self.nswaps += 1

    def _ladder_update(self, kappa, moments):
        _lib.check(self.lib.rvm_pt_ladder_update(self.ntemps, self.halfk, self.nswapped.data_ptr(),
                                                 self.lnp[0].data_ptr(), self.lnp[1].data_ptr(), kappa,
                                                 self._betas.data_ptr(), self._swap_prev.data_ptr(),
                                                 self._ratios.data_ptr(), self._n_refused.data_ptr(),
                                                 self._moments.data_ptr() if moments else 0, self._work.data_ptr(),
                                                 _lib.stream_handle()), "rvm_pt_ladder_update")

    def adapt_ladder(self):
        """One update of the ladder from the exchanges since the previous one (step() calls this
        after every exchange sweep while adapt is on).  kappa comes from the host's count of
        updates: nothing is read back from the device."""
        kappa = (self.adaptation_lag / (self.nadapt + self.adaptation_lag)) / self.adaptation_time
        self._ladder_update(kappa, False)
        self.nadapt += 1

    def step(self, draws=None):
        """One iteration: both half-steps of every temperature, then (every swap_every iterations)
        the exchange sweep; on the stream the sampler was built on (engine.check_stream).
        draws (tests): a dict of injected uniforms, any of "u1", "u2", "u3" ([2][T][W/2]: per half)
        and "swap" ([T-1][W]); u1 and u2 go together."""
        engine.check_stream(self.plan, "PTSampler.step")
        if self.lnp[0] is None:
            self.compute_lnprob()
        draws = draws or {}
        unknown = set(draws) - {"u1", "u2", "u3", "swap"}
        if unknown:
            raise ValueError(f"unknown injected draws {sorted(unknown)}")
        if ("u1" in draws) != ("u2" in draws):
            raise ValueError("inject u1 and u2 together")
        for half in (0, 1):
            u12 = None
            if "u1" in draws:
                u12 = np.stack([np.asarray(draws["u1"], dtype=np.float64)[half].reshape(-1),
                                np.asarray(draws["u2"], dtype=np.float64)[half].reshape(-1)])
            u3 = np.asarray(draws["u3"], dtype=np.float64)[half] if "u3" in draws else None
            self.half_step(half, u12, u3)
        if (self.iteration + 1) % self.swap_every == 0:
            self.swap(draws.get("swap"))
            if self.adapt:
                self.adapt_ladder()
        if self.recording:
            self._ladder_update(0.0, True)  # kappa = 0: the betas stay bit for bit
            self.nrecorded += 1
        self._end_step()

    def _chain_segments(self):
        """The coldest temperature (beta = betas[0]) for chain.ChainRecorder: the first W/2 columns of
        half 0, then of half 1 -- the walker order of positions()[0]."""
        if self.pos is None:
            raise ValueError("set_positions first")
        return [dict(x=self.pos[h], lnp=self.lnp[h], col0=0, n=self.halfk) for h in (0, 1)]

    # ---- results (host numpy) --------------------------------------------------------------------
    def positions(self):
        """[T][W][dim]"""
        return self._join([p.t() for p in self.pos]).cpu().numpy()

    def lnprob(self):
        """The UNtempered log-probabilities [T][W]."""
        return self._join(self.lnp).cpu().numpy()

    def acceptance_fraction(self):
        """Accepted stretch proposals per iteration, [T][W]."""
        return self._join([self.naccepted[0], self.naccepted[1]]).cpu().numpy() / max(self.iteration, 1)

    def swap_fraction(self):
        """Accepted exchanges per sweep of each neighbouring pair (p, p + 1), [T-1]."""
        return self.nswapped.sum(1).cpu().numpy() / (max(self.nswaps, 1) * self.k)

    # ---- the ladder and the evidence ---------------------------------------------------------------
    def ladder(self):
        """The device's betas [T] (also refreshes the host attribute `betas`)."""
        self.betas = self._betas.cpu().numpy().copy()
        return self.betas.copy()

    def last_swap_ratios(self):
        """Exchanges per walker of each pair between the last two ladder updates, [T-1]."""
        return self._ratios.cpu().numpy()

    def ladder_refusals(self):
        """Updates refused because their result was no strictly decreasing finite ladder."""
        return int(self._n_refused.item())

    def freeze_ladder(self):
        """Turn the adaptation off (the chain satisfies detailed balance from here on)."""
        self.adapt = False
        self.ladder()

    def record_lnprob(self, on=True):
        """While on, every step() adds that iteration's sum of lnp and of lnp^2 per temperature into
        a device accumulator.  The moments belong to one fixed ladder: refused while adapt is on."""
        if on and self.adapt:
            raise ValueError("record_lnprob needs a fixed ladder: freeze_ladder() first")
        if on and self.ntemps < 2:
            raise ValueError("record_lnprob needs at least two temperatures")
        self.recording = bool(on)

    def mean_lnprob(self):
        """(mean [T], std [T]) of the untempered lnp over the walkers and the recorded iterations."""
        if self.nrecorded < 1:
            raise ValueError("nothing recorded: record_lnprob(True), then step()")
        m = self._moments.cpu().numpy()
        n = float(self.nrecorded * self.k)
        mean = m[:, 0] / n
        return mean, np.sqrt(np.maximum(m[:, 1] / n - mean * mean, 0.0))

    def log_evidence_ratio(self):
        """(estimate, coarse): the thermodynamic integral of mean_lnprob over beta from beta_{T-1} up
        to 1 by the trapezoid rule, and the same over every second temperature (emcee's
        discretisation-error estimate is their difference).  This is ln Z(beta = 1) - ln Z(beta_{T-1}),
        NOT an absolute evidence: the hard prior is improper in a and m, so ln Z(0) does not exist
        (which is also why beta = 0 is refused)."""
        return log_evidence_ratio(self.ladder(), self.mean_lnprob()[0])

    # ---- checkpoint / resume ---------------------------------------------------------------------
    def checkpoint(self, path):
        """The whole ladder to an .npz: positions [T][W][dim], lnprob [T][W], the accept and swap
        counters, iteration, seed, stretch scale, the current betas, and the ladder dynamics' and the
        moments' state.  The draws are counter-based (keyed by seed, iteration and walker), so a
        restored sampler continues bit-identically, in mid-adaptation too."""
        np.savez(path, positions=self.positions(), lnprob=self.lnprob(),
                 naccepted=self._join([self.naccepted[0], self.naccepted[1]]).cpu().numpy(),
                 nswapped=self.nswapped.cpu().numpy(), iteration=self.iteration, nswaps=self.nswaps,
                 nevals=self.nevals, seed=np.uint64(self.seed), a=self.a, betas=self.ladder(),
                 swap_every=self.swap_every, swap_totals_prev=self._swap_prev.cpu().numpy(),
                 swap_ratios=self._ratios.cpu().numpy(), nadapt=self.nadapt, n_refused=self.ladder_refusals(),
                 adapt=self.adapt, adaptation_lag=self.adaptation_lag, adaptation_time=self.adaptation_time,
                 lnp_moments=self._moments.cpu().numpy(), nrecorded=self.nrecorded, recording=self.recording)

    def restore(self, path):
        """Load a checkpoint written by checkpoint() (same ntemps, nwalkers and dim)."""
        torch = _torch()
        d = np.load(path)
        if d["positions"].shape != (self.ntemps, self.k, self.dim):
            raise ValueError("checkpoint was written for a different ladder, ensemble size or dimension")
        self.betas = check_betas(d["betas"], self.ntemps)
        self._betas = torch.as_tensor(self.betas, device=self.device)
        self.set_positions(d["positions"])
        self.lnp = [x.contiguous() for x in self._split(torch.as_tensor(d["lnprob"], device=self.device))]
        acc = self._split(torch.as_tensor(d["naccepted"].astype(np.int32), device=self.device))
        self.naccepted = torch.stack(acc).contiguous()
        self.nswapped = torch.as_tensor(d["nswapped"].astype(np.int32), device=self.device).contiguous()
        self.iteration, self.nswaps, self.nevals = int(d["iteration"]), int(d["nswaps"]), int(d["nevals"])
        self.seed, self.a, self.swap_every = int(d["seed"]), float(d["a"]), int(d["swap_every"])
        if "swap_totals_prev" not in d:  # written before the ladder could adapt: nothing more to load
            return
        dev = lambda k: torch.as_tensor(d[k], device=self.device).contiguous()  # noqa: E731
        self._swap_prev, self._ratios, self._moments = dev("swap_totals_prev"), dev("swap_ratios"), dev("lnp_moments")
        self._n_refused = torch.as_tensor([int(d["n_refused"])], dtype=torch.int64, device=self.device)
        self.nadapt, self.nrecorded = int(d["nadapt"]), int(d["nrecorded"])
        self.adapt, self.recording = bool(d["adapt"]), bool(d["recording"])
        self.adaptation_lag, self.adaptation_time = float(d["adaptation_lag"]), float(d["adaptation_time"])
