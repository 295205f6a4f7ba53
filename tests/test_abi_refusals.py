"""What the C ABI answers when it refuses a call: return code, rvm_last_error() text, and which check fires first.

tests/golden/abi_refusals.json holds what the library answered when the table below was recorded,
`[entry, case, rc, message]` (the message only where rc != 0):

    python tests/test_abi_refusals.py --record      # on a machine with a HIP device: both halves

Every row fails a check (or takes an early return) before anything is launched or dereferenced on the
device: the device pointers are 16-byte aligned integers that nothing reads.  WITHOUT_PLAN needs no GPU;
WITH_PLAN runs on one adaptive S2 plan of 64 walkers and reaches the checks behind a null plan (the test
runs it in a child process, `--with-plan`, which prints the rows that answer otherwise).
A case is the entry's baseline (valid scalars, non-null pointers) with the named arguments replaced;
the baseline itself is never called.
"""
import ctypes as C
import json
import os
import sys

import pytest
import torch  # noqa: F401  (before librvmcmc.so is loaded: the process then holds one HIP runtime, torch's)
from conftest import GOLDEN, S2_PLANETS, s2_obs_oracle
from support import adaptive_plan, header_prototypes

from rvmcmc import _lib

GOLDEN_FILE = os.path.join(GOLDEN, "abi_refusals.json")
NAN, INF = float("nan"), float("inf")
I64 = 2 ** 63 - 1
MAX_WALKERS = 64

# valid scalars by argument name (an entry's `base` replaces some)
SCALARS = dict(
    n_params=10, n_chains=4, n_walkers=4, n_s0=4, n_s1=4, n_loc=4, n_half=8, s0_begin=0, s1_begin=8, chain_begin=0,
    a=2.0, hill_factor=1.0, seed=1, iteration=2, half=0, n_temps=2, kappa=1.0, step_size=0.1, n_cols=4, t0=0, t1=8,
    src_ld=4, src_col0=0, col_stride=1, dst_ld=4, dst_col0=0, lag0=0, n_lags=2, n_rows=2, row_stride=8, n_outer=2,
    outer_stride=4, n_inner=4, n_q=2, n_samples=3, draw_id=0, rel_step=1e-4, npoints_norm=100.0, alpha=1e6, eps=0.1,
    n_obs=5, n_dirs=2, reset=0, n=_lib.RVM_N_COUNTERS, max_launches=2, max=2, e=0.5, seconds=2.0, on=1,
    max_walkers=MAX_WALKERS)


def _cache(**members):
    """An rvm_smala_cache of dummy device addresses; members=0 leaves one null."""
    c = _lib.SmalaCache(*[0x9000 + 16 * i for i in range(7)])
    for k, v in members.items():
        setattr(c, k, v)
    return c


def _map(n_rows=10, **src):
    """The S2 plan's map (ten rows, row r from free parameter r); src={"3": 10} replaces one source."""
    m = _lib.ParamMapC()
    m.n_rows = n_rows
    for r in range(_lib.RVM_MAX_PARAM_ROWS):
        m.src[r] = r if r < 10 else -1
    for r, k in src.items():
        m.src[int(r)] = k
    return m


def _doubles(*v):
    return (C.c_double * len(v))(*v)


def _rows(*v):
    return (C.c_int32 * len(v))(*v)


def nulls(*names):
    return {"null_" + n: {n: None} for n in names}


def zero(*names):
    return {n + "_zero": {n: 0} for n in names}


def negative(*names):
    return {n + "_negative": {n: -1} for n in names}


def N0(n, **bad):
    """The early return on n == 0, other arguments bad: rc = 0 comes before the checks."""
    return {n + "_is_0": dict({n: 0}, **bad)}


def entry(base=None, *cases):
    rows = {}
    for c in cases:
        assert not set(c) & set(rows), set(c) & set(rows)
        rows.update(c)
    return dict(base or {}, _cases=rows)


NO_MEMBER = {"out": lambda: _cache(ok=0), "cur": lambda: _cache(lp=0), "prop": lambda: _cache(G=0)}


def no_member(*names):
    return {n + "_lacks_a_member": {n: NO_MEMBER[n]()} for n in names}


SMALA_SHAPE = [zero("n_params"), {"n_params_over": {"n_params": _lib.RVM_SMALA_MAX_PARAMS + 1}}, negative("n_chains")]
SMALA_ALL = dict(n_params=0, n_chains=-1, x=None)
PT_SHAPE = [zero("n_params", "n_temps", "n_half")]
CHAIN_SHAPE = [zero("n_params", "n_cols"),
               {"n_params_over": {"n_params": 65535}, "n_cols_over": {"n_cols": 65535 * 256 + 1}}]
WINDOW = [negative("t0"), {"t1_not_after_t0": {"t1": 0}}]
STRETCH_A = {"a_is_1": {"a": 1.0}, "a_nan": {"a": NAN}}
HILL = {"hill_negative": {"hill_factor": -1.0}, "hill_nan": {"hill_factor": NAN}}
HALVES = {"s0_negative": {"s0_begin": -1}, "s0_past_its_half": {"s0_begin": 5}, "s1_in_half_0": {"s1_begin": 7},
          "s1_past_its_half": {"s1_begin": 13}}
PLAN_NULLS = [{"null_plan": {"plan": None}, "null_map": {"plan": 0x7000, "map": None}}]
MAP_ROWS = {"map_rows": {"map": lambda: _map(n_rows=9)}, "map_source": {"map": lambda: _map(**{"3": 10})}}
BAD_MAP = {"map": lambda: _map(n_rows=9, **{"3": 10})}

WITHOUT_PLAN = {
    "rvm_plan_create": entry(
        dict(cfg=lambda: _lib.RvmConfig(2, 0.5, 4, 100.0), t=lambda: _doubles(1.0), rv=lambda: _doubles(1.0),
             sigma=lambda: _doubles(1.0), n_obs=1, out=lambda: C.pointer(C.c_void_p())),
        nulls("cfg", "t", "rv", "sigma", "out"),
        {"no_planets": {"cfg": lambda: _lib.RvmConfig(0, 0.5, 4, 100.0)},
         "too_many_epochs": dict(t=lambda: _doubles(*[0.01 * (i + 1) for i in range(1701)]),
                                 rv=lambda: _doubles(*[1.0] * 1701), sigma=lambda: _doubles(*[1.0] * 1701), n_obs=1701),
         "all": dict(cfg=None, t=None, rv=None, sigma=None, out=None, n_obs=-1, max_walkers=-1)}),
    "rvm_plan_set_certain_reject": entry(None, nulls("plan")),
    "rvm_plan_set_verify_eccentricity": entry(None, nulls("plan"), {"all": dict(plan=None, e=1.0)}),
    "rvm_plan_extension": entry(None, nulls("plan")),
    "rvm_plan_counters": entry(None, nulls("plan"), {"all": dict(plan=None, n=-1)}),
    "rvm_plan_hedge_stats": entry(None, nulls("plan")),
    "rvm_plan_hedge_marks": entry(None, nulls("plan")),
    "rvm_plan_hedge_waits": entry(None, nulls("plan")),
    "rvm_plan_faults": entry(None, nulls("plan")),
    "rvm_plan_time_kernels": entry(None, nulls("plan"), {"all": dict(plan=None, max_launches=-1)}),
    "rvm_plan_kernel_times": entry(None, nulls("plan"), {"max_negative": dict(plan=0x7000, max=-1)}),
    "rvm_plan_set_handoff_timeout": entry(None, nulls("plan"), {"all": dict(plan=None, seconds=0.0)}),
    "rvm_plan_info": entry(None, nulls("plan")),
    "rvm_logl_batch": entry(None, nulls("plan"), {"null_plan_before_n_walkers_is_0": {"plan": None, "n_walkers": 0}},
                            {"all": dict(plan=None, n_walkers=-1, params=None, hill_factor=-1.0)}),
    "rvm_stretch_half_step": entry(None, *PLAN_NULLS, {"null_plan_before_n_s0_is_0": {"plan": None, "n_s0": 0}},
                                   {"all": dict(plan=None, map=None, n_s0=-1, n_params=0, a=1.0, hill_factor=-1.0)}),
    "rvm_stretch_iteration_begin": entry(None, *PLAN_NULLS, {"null_plan_before_n_loc_is_0": {"plan": None, "n_loc": 0}},
                                         {"all": dict(plan=None, map=None, n_loc=-1, n_params=0, s0_begin=-1, a=1.0)}),
    "rvm_mh_step": entry(None, *PLAN_NULLS, {"null_plan_before_n_chains_is_0": {"plan": None, "n_chains": 0}},
                         {"all": dict(plan=None, map=None, n_chains=-1, n_params=0, hill_factor=-1.0)}),
    "rvm_smala_stencil_logl": entry(dict(n_chains=2), *PLAN_NULLS,
                                    {"null_plan_before_n_chains_is_0": {"plan": None, "n_chains": 0}},
                                    {"all": dict(plan=None, map=None, n_chains=-1, n_params=0, hill_factor=-1.0)}),
    "rvm_logl_derivs": entry(dict(dir_rows=lambda: _rows(0, 1)), nulls("plan"),
                             {"null_plan_before_n_chains_is_0": {"plan": None, "n_chains": 0}},
                             {"all": dict(plan=None, n_chains=-1, n_dirs=0, hill_factor=-1.0)}),
    "rvm_stretch_iteration_end": entry(
        None, zero("n_params"), negative("n_loc"), {"n_half_below_n_loc": {"n_half": 3}},
        nulls("x0", "dec", "dec_all", "x1", "lnp1", "c0", "c1", "lnp_spec", "status_spec"), HALVES, STRETCH_A,
        {"all": dict(n_params=0, n_loc=-1, x0=None, s0_begin=-1, s1_begin=0, a=1.0)},
        N0("n_loc", n_params=0, x0=None, s0_begin=-1, a=1.0)),
    "rvm_stretch_propose": entry(
        None, zero("n_params", "n_s1"), negative("n_s0"), nulls("x", "c", "q_out", "z_out"), STRETCH_A,
        {"all": dict(n_params=0, n_s0=-1, x=None, a=1.0)}, N0("n_s0", n_params=0, x=None, a=1.0)),
    "rvm_stretch_accept": entry(
        None, zero("n_params"), negative("n_s0"), nulls("x", "lnp", "q", "lnp_new", "z"),
        {"all": dict(n_params=0, n_s0=-1, x=None)}, N0("n_s0", n_params=0, x=None)),
    "rvm_pt_stretch_propose": entry(
        None, *PT_SHAPE, {"columns_overflow": dict(n_temps=65536, n_half=32768), "half_is_2": {"half": 2}}, STRETCH_A,
        nulls("x", "c", "q_out", "z_out"),
        {"all": dict(n_params=0, n_temps=0, n_half=0, half=2, a=1.0, x=None),
         "all_but_shape": dict(half=2, a=1.0, x=None), "scale_and_null": dict(a=1.0, x=None)}),
    "rvm_pt_stretch_accept": entry(
        None, *PT_SHAPE, {"columns_overflow": dict(n_temps=65536, n_half=32768), "half_is_2": {"half": 2}},
        nulls("betas", "x", "lnp", "q", "lnp_new", "z"),
        {"all": dict(n_params=0, n_temps=0, n_half=0, half=2, betas=None, x=None),
         "all_but_shape": dict(half=2, betas=None, x=None), "both_nulls": dict(betas=None, x=None)}),
    "rvm_pt_swap": entry(
        None, *PT_SHAPE, {"columns_overflow": dict(n_temps=65536, n_half=16384)},
        nulls("betas", "x0", "x1", "lnp0", "lnp1", "swapped"),
        {"all": dict(n_params=0, n_temps=0, n_half=0, betas=None, x0=None), "both_nulls": dict(betas=None, x0=None),
         "one_temperature": dict(n_temps=1, betas=None, x0=None, swapped=None),
         "one_temperature_bad_shape": dict(n_temps=1, n_half=0, betas=None)}),
    "rvm_pt_ladder_update": entry(
        None, zero("n_temps", "n_half"), {"columns_overflow": dict(n_temps=65536, n_half=16384)},
        {"kappa_negative": {"kappa": -1.0}, "kappa_nan": {"kappa": NAN}, "kappa_inf": {"kappa": INF}},
        nulls("swapped", "lnp0", "lnp1", "betas", "swap_totals_prev", "ratios_out", "n_refused", "workspace"),
        {"all": dict(n_temps=0, n_half=0, kappa=-1.0, swapped=None, lnp0=None, betas=None, swap_totals_prev=None,
                     ratios_out=None, n_refused=None, workspace=None),
         "all_nulls": dict(swapped=None, lnp0=None, lnp1=None, betas=None, swap_totals_prev=None, ratios_out=None,
                           n_refused=None, workspace=None),
         "one_temperature": dict(n_temps=1, swapped=None, betas=None, workspace=None),
         "one_temperature_bad_kappa": dict(n_temps=1, kappa=-1.0, swapped=None)}),
    "rvm_chain_record": entry(
        None, *CHAIN_SHAPE, nulls("src", "dst"), zero("col_stride"), negative("src_col0", "dst_col0"),
        {"src_ld_small": {"src_ld": 3}, "src_stride_overflows": {"col_stride": 2 ** 62}, "dst_ld_small": {"dst_ld": 3},
         "dst_col0_overflows": {"dst_col0": I64 - 1}, "lnp_src_alone": {"lnp_dst": None},
         "lnp_dst_alone": {"lnp_src": None},
         "all": dict(n_params=0, n_cols=0, src=None, dst=None, col_stride=0, src_col0=-1, dst_col0=-1, src_ld=0,
                     dst_ld=0, lnp_dst=None),
         "all_but_shape": dict(src=None, dst=None, col_stride=0, src_col0=-1, dst_col0=-1, src_ld=0, dst_ld=0,
                               lnp_dst=None),
         "both_ld_small": dict(src_ld=3, dst_ld=3, lnp_dst=None)}),
    "rvm_chain_moments": entry(
        None, *CHAIN_SHAPE, nulls("chain", "mean_out", "m2_out"), *WINDOW,
        {"all": dict(n_params=0, n_cols=0, chain=None, t0=-1, t1=-2, mean_out=None, m2_out=None),
         "window_and_outputs": dict(t0=-1, t1=-2, mean_out=None, m2_out=None)}),
    "rvm_chain_autocov_workspace_bytes": entry(
        None, zero("n_params", "n_cols", "n_lags"),
        {"n_lags_over": {"n_lags": 2 ** 30 + 1}, "product_over": dict(n_params=65534, n_lags=2 ** 16), "valid": {}}),
    "rvm_chain_autocov": entry(
        None, *CHAIN_SHAPE, nulls("chain", "mean", "acov_out", "workspace"), *WINDOW, negative("lag0"), zero("n_lags"),
        {"n_lags_over": {"n_lags": 2 ** 30 + 1}, "lags_past_the_window": dict(lag0=7, n_lags=2),
         "product_over": dict(n_params=65534, n_lags=2 ** 16, t1=2 ** 20),
         "all": dict(n_params=0, n_cols=0, chain=None, mean=None, t0=-1, t1=-2, lag0=-1, n_lags=0, acov_out=None,
                     workspace=None),
         "lags_and_outputs": dict(lag0=-1, n_lags=0, acov_out=None, workspace=None)}),
    "rvm_rows_quantiles_workspace_bytes": entry(
        None, zero("n_rows", "n_q"), {"n_rows_over": {"n_rows": 65536}, "n_q_over": {"n_q": 17}, "valid": {}}),
    "rvm_rows_quantiles": entry(
        dict(q=lambda: _doubles(0.25, 0.75)), nulls("x", "q", "out", "workspace"),
        zero("n_rows", "n_outer", "n_inner", "n_q"),
        negative("row_stride", "outer_stride"),
        {"n_rows_over": {"n_rows": 65536}, "elements_over": dict(n_outer=2 ** 31, n_inner=2), "n_q_over": {"n_q": 17},
         "q_above_1": {"q": lambda: _doubles(0.25, 1.5)}, "q_nan": {"q": lambda: _doubles(NAN, 0.5)},
         "workspace_misaligned": {"workspace": 0x8004},
         "all": dict(x=None, n_rows=0, row_stride=-1, n_outer=0, outer_stride=-1, n_inner=0, q=None, n_q=0, out=None,
                     workspace=None),
         "q_and_outputs": dict(q=lambda: _doubles(0.25, 1.5), out=None, workspace=0x8004)}),
    "rvm_chain_cov_workspace_bytes": entry(
        None, zero("n_params", "n_cols"),
        {"n_params_over": {"n_params": 16385}, "n_cols_over": {"n_cols": 65535 * 64 + 1}, "valid": {}}),
    "rvm_chain_cov": entry(
        None, zero("n_params", "n_cols"),
        {"n_params_over": {"n_params": 16385}, "n_cols_over": {"n_cols": 65535 * 64 + 1}},
        nulls("chain", "center", "cov_out", "workspace"), *WINDOW,
        {"all": dict(n_params=0, n_cols=0, chain=None, t0=-1, t1=-2, center=None, cov_out=None, workspace=None)}),
    "rvm_chain_draw": entry(
        None, *CHAIN_SHAPE, nulls("chain", "x_out"), *WINDOW, zero("n_samples"),
        {"all": dict(n_params=0, n_cols=0, chain=None, t0=-1, t1=-2, n_samples=0, x_out=None)}),
    "rvm_mh_propose": entry(
        None, zero("n_params"), negative("n_chains"), nulls("x", "scales", "q_out"),
        {"all": dict(n_params=0, n_chains=-1, x=None)}, N0("n_chains", n_params=0, x=None)),
    "rvm_mh_accept": entry(
        None, zero("n_params"), negative("n_chains"), nulls("x", "lnp", "q", "lnp_new"),
        {"all": dict(n_params=0, n_chains=-1, x=None)}, N0("n_chains", n_params=0, x=None)),
    "rvm_fd_params": entry(
        None, zero("n_params", "rel_step"), negative("n_chains"), nulls("x", "floor_", "out"),
        {"rel_step_nan": {"rel_step": NAN}},
        {"all": dict(n_params=0, n_chains=-1, x=None, rel_step=0.0)}, N0("n_chains", n_params=0, x=None)),
    "rvm_logl_derivs_workspace_bytes": entry(None, negative("n_chains", "n_dirs"),
                                             {"valid": dict(n_chains=256, n_dirs=10)}),
}
for _name in ("rvm_smala_derive", "rvm_smala_derive_sides"):
    WITHOUT_PLAN[_name] = entry(
        None, *SMALA_SHAPE, negative("n_obs"),
        nulls("x", "floor_", "lp_stencil", "status_stencil", "rv_stencil", "inv_sigma2", "out"), no_member("out"),
        zero("rel_step", "npoints_norm", "alpha"), {"rel_step_nan": {"rel_step": NAN}, "alpha_nan": {"alpha": NAN}},
        {"all": dict(SMALA_ALL, n_obs=-1, out=None, rel_step=0.0, npoints_norm=0.0, alpha=0.0)},
        N0("n_chains", n_params=0, x=None, out=None))
WITHOUT_PLAN.update({
    "rvm_smala_center_accept": entry(
        None, *SMALA_SHAPE, nulls("x", "x_prop", "lp_center", "status_center", "cur", "prop"), no_member("cur", "prop"),
        {"all": dict(SMALA_ALL, cur=None, prop=None)}, N0("n_chains", n_params=0, x=None, cur=None)),
    "rvm_smala_metric": entry(
        None, *SMALA_SHAPE, nulls("x", "lp", "status", "grad", "hess", "out"), no_member("out"), zero("alpha"),
        {"all": dict(SMALA_ALL, out=None, alpha=0.0)}, N0("n_chains", n_params=0, x=None, out=None)),
    "rvm_smala_derive_accept": entry(
        None, *SMALA_SHAPE, negative("n_obs"),
        nulls("x", "x_prop", "floor_", "lp_stencil", "status_stencil", "rv_stencil", "inv_sigma2", "cur", "prop"),
        no_member("cur", "prop"), zero("rel_step", "npoints_norm", "alpha"),
        {"rel_step_nan": {"rel_step": NAN}, "alpha_nan": {"alpha": NAN}},
        {"all": dict(SMALA_ALL, n_obs=-1, cur=None, prop=None, rel_step=0.0, npoints_norm=0.0, alpha=0.0)},
        N0("n_chains", n_params=0, x=None, cur=None)),
    "rvm_smala_metric_accept": entry(
        None, *SMALA_SHAPE, nulls("x", "x_prop", "lp", "status", "grad", "hess", "cur", "prop"),
        no_member("cur", "prop"),
        zero("alpha"), {"all": dict(SMALA_ALL, cur=None, prop=None, alpha=0.0)},
        N0("n_chains", n_params=0, x=None, cur=None)),
    "rvm_smala_propose": entry(
        None, *SMALA_SHAPE, nulls("x", "x_prop", "cur"), no_member("cur"), {"all": dict(SMALA_ALL, cur=None)},
        N0("n_chains", n_params=0, x=None, cur=None)),
    "rvm_smala_accept": entry(
        None, *SMALA_SHAPE, nulls("x", "x_prop", "cur", "prop"), no_member("cur", "prop"),
        {"all": dict(SMALA_ALL, cur=None, prop=None)}, N0("n_chains", n_params=0, x=None, cur=None)),
})

# the checks behind a null plan (`plan` is the live plan in every row)
WITH_PLAN = {
    "rvm_plan_set_verify_eccentricity": entry(None, {"e_is_1": {"e": 1.0}, "e_nan": {"e": NAN}}),
    "rvm_plan_counters": entry(dict(out=lambda: (C.c_int64 * _lib.RVM_N_COUNTERS)()), negative("n"), nulls("out"),
                               {"all": dict(n=-1, out=None)}),
    "rvm_plan_time_kernels": entry(None, negative("max_launches"), {"max_launches_over": {"max_launches": 4097}}),
    "rvm_plan_kernel_times": entry(None, negative("max")),
    "rvm_plan_set_handoff_timeout": entry(None, zero("seconds"), negative("seconds"),
                                          {"seconds_1e9": {"seconds": 1e9}, "seconds_nan": {"seconds": NAN}}),
    "rvm_logl_batch": entry(
        None, negative("n_walkers"), {"n_walkers_over": {"n_walkers": MAX_WALKERS + 1}},
        nulls("params", "logl_out", "status_out"), HILL,
        {"all": dict(n_walkers=-1, params=None, logl_out=None, status_out=None, hill_factor=NAN),
         "nulls_and_hill": dict(params=None, hill_factor=-1.0)}, N0("n_walkers", params=None, hill_factor=-1.0)),
    "rvm_stretch_half_step": entry(
        None, negative("n_s0"), {"n_s0_over": {"n_s0": MAX_WALKERS + 1}}, zero("n_params", "n_s1"),
        nulls("x", "lnp", "c_aos"), STRETCH_A, HILL, MAP_ROWS,
        {"all": dict(BAD_MAP, n_s0=-1, n_params=0, x=None, a=1.0, hill_factor=-1.0),
         "all_but_n_s0": dict(BAD_MAP, n_params=0, x=None, a=1.0, hill_factor=-1.0),
         "scale_hill_map": dict(BAD_MAP, a=1.0, hill_factor=-1.0), "hill_map": dict(BAD_MAP, hill_factor=-1.0),
         "map_both": dict(BAD_MAP)}, N0("n_s0", n_params=0, x=None, a=1.0, hill_factor=-1.0)),
    "rvm_stretch_iteration_begin": entry(
        None, negative("n_loc"), {"three_n_loc_over": {"n_loc": 22, "n_half": 32, "s1_begin": 32}}, zero("n_params"),
        {"n_half_below_n_loc": {"n_half": 3}},
        nulls("x0", "lnp0", "x1", "c0", "c1", "lnp_spec", "status_spec", "dec"), HALVES, STRETCH_A, HILL, MAP_ROWS,
        {"all": dict(BAD_MAP, n_loc=-1, n_params=0, x0=None, s0_begin=-1, a=1.0, hill_factor=-1.0),
         "all_but_n_loc": dict(BAD_MAP, n_params=0, x0=None, s0_begin=-1, a=1.0, hill_factor=-1.0),
         "ranges_scale_hill_map": dict(BAD_MAP, s0_begin=-1, a=1.0, hill_factor=-1.0),
         "scale_hill_map": dict(BAD_MAP, a=1.0, hill_factor=-1.0), "hill_map": dict(BAD_MAP, hill_factor=-1.0)},
        N0("n_loc", n_params=0, x0=None, s0_begin=-1, a=1.0, hill_factor=-1.0)),
    "rvm_mh_step": entry(
        None, negative("n_chains"), {"n_chains_over": {"n_chains": MAX_WALKERS + 1}}, zero("n_params"),
        nulls("x", "lnp", "scales"), HILL, MAP_ROWS,
        {"all": dict(BAD_MAP, n_chains=-1, n_params=0, x=None, hill_factor=-1.0),
         "all_but_n_chains": dict(BAD_MAP, n_params=0, x=None, hill_factor=-1.0),
         "hill_map": dict(BAD_MAP, hill_factor=-1.0)}, N0("n_chains", n_params=0, x=None, hill_factor=-1.0)),
    "rvm_smala_stencil_logl": entry(
        dict(n_chains=2), zero("n_params", "rel_step"), negative("n_chains"), {"rel_step_nan": {"rel_step": NAN}},
        nulls("x", "floor_", "logl_out", "status_out"), {"stencil_over": {"n_chains": 4}}, HILL, MAP_ROWS,
        {"all": dict(BAD_MAP, n_params=0, n_chains=-1, x=None, rel_step=0.0, hill_factor=-1.0),
         "over_hill_map": dict(BAD_MAP, n_chains=4, hill_factor=-1.0), "hill_map": dict(BAD_MAP, hill_factor=-1.0)},
        N0("n_chains", n_params=0, x=None, hill_factor=-1.0)),
    "rvm_logl_derivs": entry(
        dict(dir_rows=lambda: _rows(0, 1)), negative("n_chains"), zero("n_dirs"),
        {"n_dirs_over": {"n_dirs": 11}}, nulls("dir_rows", "params", "grad_out", "hess_out", "workspace"),
        {"pairs_over": dict(n_chains=2 ** 30 // 55 + 1, n_dirs=10, dir_rows=lambda: _rows(*range(10)))}, HILL,
        {"dir_row_negative": {"dir_rows": lambda: _rows(0, -1)}, "dir_row_over": {"dir_rows": lambda: _rows(0, 10)},
         "dir_rows_repeat": {"dir_rows": lambda: _rows(1, 1)},
         "all": dict(n_chains=-1, n_dirs=0, dir_rows=None, params=None, hill_factor=-1.0),
         "pairs_hill_rows": dict(n_chains=2 ** 30 // 55 + 1, n_dirs=10, dir_rows=lambda: _rows(*[-1] * 10),
                                 hill_factor=-1.0),
         "hill_rows": dict(dir_rows=lambda: _rows(-1, -1), hill_factor=-1.0),
         "row_over_and_repeat": {"dir_rows": lambda: _rows(10, 10)}},
        N0("n_chains", n_dirs=0, params=None, hill_factor=-1.0)),
}


def table_rows(table):
    """(entry, case) of every row, in the table's order."""
    return [(name, case) for name, spec in table.items() for case in spec["_cases"]]


def call(lib, table, name, case, plan=None):
    """One row: (rc, message or None).  Every argument object stays alive until the call returns."""
    spec = table[name]
    protos = header_prototypes()[name][1]
    argtypes = _lib.SIGNATURES[name][1]
    given = dict({k: v for k, v in spec.items() if k != "_cases"}, **spec["_cases"][case])
    args, keep = [], []
    assert set(given) <= {arg for _, arg in protos}, (name, case, set(given) - {arg for _, arg in protos})
    for i, ((ctype, arg), at) in enumerate(zip(protos, argtypes)):
        if arg in given:
            v = given[arg]() if callable(given[arg]) else given[arg]
        elif arg == "plan":
            v = plan
        elif arg == "stream" or (at is not C.c_void_p and at.__name__.startswith("LP_c_")):
            v = None  # the null stream; a nullable host output
        elif arg == "map":
            v = _map()
        elif ctype == "rvm_smala_cache*":
            v = _cache()
        elif at is C.c_void_p:
            v = 0x10000 + 16 * i  # a device address nothing reads
        else:
            v = SCALARS[arg]
        keep.append(v)
        args.append(C.byref(v) if isinstance(v, C.Structure) else v)
    rc = getattr(lib, name)(*args)
    return rc, (lib.rvm_last_error().decode() if rc != 0 and _lib.SIGNATURES[name][0] is C.c_int else None)


def make_plan():
    """The adaptive S2 plan of the second half (engine.LoglPlan; close() it)."""
    from rvmcmc import engine

    plan, _, _ = adaptive_plan(S2_PLANETS, s2_obs_oracle(), MAX_WALKERS, engine.IntegratorConfig().resolve(S2_PLANETS))
    assert plan.resolve_tol > 0.0 and plan.rows == 10
    return plan


def answers(table, plan=None):
    lib = _lib.load()
    return [[name, case, *call(lib, table, name, case, plan)] for name, case in table_rows(table)]


def golden_rows(half):
    with open(GOLDEN_FILE) as f:
        return {(name, case): (rc, msg) for name, case, rc, msg in json.load(f)[half]}


def wrong_rows(half, table, plan=None):
    """[entry, case, (rc, message) got, (rc, message) recorded] of every row that answers otherwise."""
    want = golden_rows(half)
    assert list(want) == table_rows(table)  # (the table and the recording list the same rows)
    lib = _lib.load()
    got = {row: call(lib, table, *row, plan) for row in table_rows(table)}
    return [[*row, got[row], want[row]] for row in got if got[row] != want[row]]


def wrong_rows_with_a_plan():
    plan = make_plan()
    try:
        return wrong_rows("with_plan", WITH_PLAN, plan._h)
    finally:
        plan.close()


def test_refusals_without_a_plan():
    assert wrong_rows("without_plan", WITHOUT_PLAN) == []


@pytest.mark.gpu
def test_refusals_with_a_plan():
    """In a process of its own: tests/test_gpu_a_dist.py must see a suite process that has made no GPU call,
    and this module sorts before it."""
    import subprocess

    p = subprocess.run([sys.executable, os.path.abspath(__file__), "--with-plan"], capture_output=True, text=True)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    assert json.loads(p.stdout.strip().splitlines()[-1]) == []


def test_recorded_rows_are_refusals_or_early_returns():
    """No recorded row got past the checks: -1 with a message, or 0 on the rows that name their early return
    (and the workspace sizes: 0 on bad arguments, the size on the `valid` row)."""
    for half in ("without_plan", "with_plan"):
        for (name, case), (rc, msg) in golden_rows(half).items():
            if name.endswith("_workspace_bytes"):
                assert (rc > 0) == (case == "valid") and msg is None, (name, case, rc)
            elif (case.endswith("_is_0") and not case.startswith("null_plan_before")) or case == "one_temperature":
                assert rc == 0 and msg is None, (name, case, rc, msg)
            else:
                assert rc == -1 and msg, (name, case, rc, msg)


def record():
    plan = make_plan()
    try:
        doc = {"without_plan": answers(WITHOUT_PLAN), "with_plan": answers(WITH_PLAN, plan._h)}
    finally:
        plan.close()
    with open(GOLDEN_FILE, "w") as f:
        f.write("{\n")
        for i, (half, rows) in enumerate(doc.items()):
            body = ",\n".join("  " + json.dumps(r) for r in rows)
            f.write(f' "{half}": [\n{body}\n ]' + ("," if i == 0 else "") + "\n")
        f.write("}\n")
    print(f"{GOLDEN_FILE}: {sum(len(r) for r in doc.values())} rows, "
          f"{len({r[3] for rows in doc.values() for r in rows if r[3]})} distinct messages")


if __name__ == "__main__":
    if sys.argv[1:] == ["--record"]:
        record()
    elif sys.argv[1:] == ["--with-plan"]:  # (the GPU half's child process: the rows that answer otherwise)
        print(json.dumps(wrong_rows_with_a_plan()))
    else:
        sys.exit("usage: python tests/test_abi_refusals.py --record | --with-plan")
