"""rvmcmc -- MI355X-native radial-velocity MCMC (the rvel-mcmc hot path on gfx950).

Reference-compatible modules: state, observations, mcmc, driver.  Batched engine: engine,
ensemble, tempering, smala, chain (the recorded chain and its diagnostics), stability (the
posterior's dynamical stability over long spans).  Native code:
librvmcmc.so (HIP kernels + C ABI, include/rvmcmc.h).
"""
from . import _lib  # noqa: F401

__all__ = ["state", "observations", "mcmc", "driver", "engine", "ensemble", "tempering", "smala", "chain",
           "stability"]
