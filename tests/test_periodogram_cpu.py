"""What rvmcmc/periodogram.py and ChainRecorder.residual_periodogram refuse, and the frequency grid: all decided
on the host before anything reaches a device."""
import numpy as np
import pytest

from rvmcmc import periodogram as PG
from rvmcmc.observations import Observation


def _obs(n, sigma=1e-4, t=None):
    o = Observation()
    t = np.linspace(0.0, 10.0, n) if t is None else np.asarray(t, dtype=np.float64)
    h = len(t) // 2
    o.tb, o.tf = t[:h], t[h:]
    rv = np.sin(np.arange(len(t)))
    o.rvb, o.rvf = rv[:h], rv[h:]
    er = np.full(len(t), sigma) if np.isscalar(sigma) else np.asarray(sigma, dtype=np.float64)
    o.errorb, o.errorf = er[:h], er[h:]
    o.Npoints = n
    return o


def test_freq_grid_and_units():
    t = np.array([3.0, 5.0, 4.0, 13.0])
    f0, df, F = PG.freq_grid(t)
    assert df == 1.0 / (5 * 10.0) and f0 == df and F == 10  # up to N / (2 T) = 0.2
    assert PG.freq_grid(t, oversample=2, fmax=1.0) == (0.05, 0.05, 20)
    obs_t = np.linspace(0.0, 97.3, 122)
    assert PG.freq_grid(obs_t)[2] == 305
    with pytest.raises(ValueError, match="empty grid"):
        PG.freq_grid(t, fmax=0.01)
    with pytest.raises(ValueError):
        PG.freq_grid([1.0, 1.0])
    with pytest.raises(ValueError):
        PG.freq_grid([1.0, np.nan, 2.0])
    days = np.array([1.0, 193.9])
    np.testing.assert_allclose(PG.period_days(PG.freq_of_period_days(days)), days, rtol=1e-15)
    assert PG.freq_of_period_days(1.0) == 1.0 / 0.01720


def test_series_inputs():
    t = np.array([2.0, 4.0, 8.0, 3.0])
    tau, w = PG.series_inputs(t, [1.0, 2.0, 1.0, 2.0])
    np.testing.assert_array_equal(tau, t - 5.0)
    np.testing.assert_array_equal(w, np.array([1.0, 0.25, 1.0, 0.25]) / 2.5)
    assert abs(w.sum() - 1.0) < 1e-15


@pytest.mark.parametrize("call", ["gls", "recorder"])
def test_value_errors(call):
    if call == "gls":
        def run(obs, **kw):
            return PG.gls(obs, **kw)
    else:
        run = _recorder_run()
    with pytest.raises(ValueError, match="at least 4"):
        run(_obs(3))
    with pytest.raises(ValueError, match="at least 3"):
        run(_obs(2), float_mean=False)
    with pytest.raises(ValueError, match="finite"):
        run(_obs(6, t=[0.0, 1.0, np.inf, 3.0, 4.0, 5.0]))
    with pytest.raises(ValueError, match="finite"):
        run(_obs(6, sigma=[1.0, 1.0, np.nan, 1.0, 1.0, 1.0]))
    with pytest.raises(ValueError, match="> 0"):
        run(_obs(6, sigma=[1.0, 1.0, 0.0, 1.0, 1.0, 1.0]))
    with pytest.raises(ValueError, match="> 0"):
        run(_obs(6, sigma=-1.0))
    with pytest.raises(ValueError, match="empty grid"):
        run(_obs(6), grid=(0.1, 0.1, 0))
    with pytest.raises(ValueError, match="finite"):
        run(_obs(6), grid=(np.nan, 0.1, 4))


class _HostSampler:
    """What a ChainRecorder needs of a sampler, in host memory: nothing here can reach a device."""

    def __init__(self, **attrs):
        import torch

        self.device = torch.device("cpu")
        self._x = torch.zeros((2, 4), dtype=torch.float64)
        for k, v in attrs.items():
            setattr(self, k, v)

    def _chain_segments(self):
        return [{"x": self._x, "n": 4}]


def _recorder_run():
    from rvmcmc.chain import ChainRecorder

    def run(obs, **kw):
        rec = ChainRecorder(_HostSampler(obs=obs, state=object(), pmap=object()), capacity=1, lnprob=False)
        return rec.residual_periodogram(n_samples=2, **kw)

    return run


@pytest.mark.parametrize("missing", ["obs", "state", "pmap"])
def test_type_error_without_obs_state_or_pmap(missing):
    from rvmcmc.chain import ChainRecorder

    attrs = dict(obs=_obs(6), state=object(), pmap=object())
    del attrs[missing]
    rec = ChainRecorder(_HostSampler(**attrs), capacity=1, lnprob=False)
    with pytest.raises(TypeError, match="obs / state / pmap"):
        rec.residual_periodogram(n_samples=2)
