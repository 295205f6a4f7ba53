/*
 * rvmcmc.h -- C ABI of librvmcmc.so, the MI355X (gfx950) radial-velocity MCMC hot path.
 *
 * The reference (MrSwordFish/rvel-mcmc, Python 2 + REBOUND) has no native interface of its own;
 * its hot path is reached through three Python call sites, which this ABI replaces in batch:
 *
 *   reference call site                                   replaced by
 *   ----------------------------------------------------  ----------------------------------------
 *   state.py:103-110  State.get_logp(obs) -> float         rvm_logl_batch (W walkers per call)
 *     (state.py:36-47 setup_sim, :61-73 get_rv,
 *      :89-98 get_chi2, :299-315 priorHard, and
 *      REBOUND sim.add/move_to_com/integrate/Encounter)
 *   mcmc.py:28-35     lnprob(x, e) (emcee callback)         rvm_logl_batch
 *   observations.py:6-69 Observation.{tf,tb,rvf,rvb,       rvm_plan_create (epoch schedule, obs data)
 *     errorf,errorb,Npoints}
 *   mcmc.py:57-65 Ensemble.step -> emcee 2.2.1 stretch     rvm_stretch_propose / rvm_stretch_accept,
 *     move (EnsembleSampler._propose_stretch)                or fused: rvm_stretch_half_step
 *   mcmc.py:89-121 Mh.generate_proposal / Mh.step          rvm_mh_propose / rvm_mh_accept, or fused:
 *                                                            rvm_mh_step
 *   state.py:218-294 get_chi2_d_dd / get_logp_d_dd         rvm_logl_derivs (exact gradient + Hessian,
 *     (REBOUND 1st/2nd-order variational equations)         hyper-dual forward mode)
 *   mcmc.py:144-187 Smala.generate_proposal/step           rvm_fd_params (finite-difference stencil)
 *     mcmc.py:135-139 Smala.softabs,                         + rvm_smala_derive, or rvm_logl_derivs +
 *     mcmc.py:158-162 Smala.transitionProbability              rvm_smala_metric; rvm_smala_propose /
 *                                                              rvm_smala_accept
 *
 * Conventions
 *   - All array pointers passed to launch functions are DEVICE pointers (hipMalloc / torch CUDA
 *     tensors), caller-owned.  Launch functions never allocate, never synchronise, and are
 *     stream-ordered on `stream` (a hipStream_t; NULL = the null stream): everything a launch
 *     enqueues is complete once `stream` is -- including the eager halving pass a plain launch of
 *     32..512 walkers runs on the plan's own side stream, which is forked from `stream` and joined
 *     back into it within the launch -- so inputs may be reused right after `stream` is synchronised.
 *     They are capturable into a hipGraph: no host-side state changes per launch (the launch
 *     generation that tags the kernels' hand-off flags advances on the device) and kernel
 *     attributes are set by rvm_plan_create.  rvm_plan_create is the only call that allocates
 *     (device buffers owned by the plan) and it synchronises once.
 *   - A plan is single-stream: it owns per-launch workspace (the direction-exchange slots and the
 *     level-split hand-off slots, left empty by every completed launch), so launches that use one plan must be
 *     serialised on one stream at a time.  Concurrent launches on two streams need two plans (the
 *     Python layer keys its plan cache by stream, rvmcmc/engine.py).
 *   - Walker parameters are SoA, [n_params][n_walkers] float64, n_params = 5*n_planets with the
 *     canonical per-planet key order  m, a, h, k, l  (the Python layer maps a
 *     State's dict order onto it), or 7*n_planets (m, a, h, k, l, ix, iy) for inclined plans.
 *   - Return code: 0 = success, < 0 = argument / launch error (rvm_last_error() explains).
 *     Per-walker physics outcomes are never errors: they are status codes plus logl = -INFINITY
 *     (the reference raises rebound.Encounter / returns -inf from priorHard; mcmc.py:28-35 maps
 *     every exception to -inf).
 */
#ifndef RVMCMC_H
#define RVMCMC_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RVM_ABI_VERSION 14

/* per-walker status codes (status_out) */
#define RVM_STATUS_OK 0
#define RVM_STATUS_PRIOR 1     /* State.priorHard() true (state.py:299-315) -> logl = -inf        */
#define RVM_STATUS_ENCOUNTER 2 /* pair distance < exit_min_distance (REBOUND Encounter) -> -inf   */
#define RVM_STATUS_NONFINITE 3 /* non-finite chi2 (a main pass that blows up is refined; a halving pass
                                  that blows up ends the walker), or a hand-off that gave up -> -inf */
#define RVM_STATUS_UNRESOLVED 4 /* adaptive resolution: the extrapolation-error estimate still above
                                   rvm_config.resolve_tol after resolve_max refinements -> -inf      */
#define RVM_STATUS_SKIPPED 5    /* rvm_stretch_iteration_begin's status_spec only: a half-1 variant
                                   slot whose partner's first-half decision (already final) rules it
                                   out, not refined by the adaptive resolution; rvm_stretch_iteration_end
                                   never reads it.  logl -inf                                          */
#define RVM_STATUS_ESCAPE 6     /* rvm_stability_advance's status only: a planet's Jacobi |r| beyond
                                   r_max at a block end                                                */

#define RVM_MAX_PLANETS 4
#define RVM_MAX_LEVELS 6
#define RVM_MAX_EPOCHS_PER_DIRECTION 1700 /* epochs with t >= 0, and with t < 0, per plan */
#define RVM_SMALA_MAX_PARAMS 20           /* free parameters per SMALA chain                 */
#define RVM_MAX_QUANTILES 16              /* quantiles per rvm_rows_quantiles call           */
#define RVM_RESOLVE_MAX_LIMIT 12          /* rvm_config.resolve_max                          */

/* Integrator configuration of a plan. */
typedef struct {
    int32_t n_planets;     /* 1..RVM_MAX_PLANETS                                                  */
    double dt;             /* base step in code units (yr/2pi); the segment between two epochs is
                              cut into n = ceil(len/dt) base steps                                 */
    int32_t n_levels;      /* Richardson levels, 1..RVM_MAX_LEVELS                                  */
    double npoints_norm;   /* obs.Npoints: chi2 is divided by this (state.py:98), NOT the epoch count */
    int32_t level_mult[RVM_MAX_LEVELS]; /* level k integrates each segment with n * level_mult[k]
                              steps (distinct, >= 1, at most 64); all zero = harmonic 1, 2, ..., n_levels */
    double period_hint;    /* shortest orbital period the walkers are expected to have (code units):
                              sizes the per-level Stumpff series (performance only, results are
                              exact for any orbit); 0 = longest series on every level              */
    int32_t inclined;      /* 0: coplanar, params [5*n_planets][W] (m, a, h, k, l); 1: inclined,
                              params [7*n_planets][W] (m, a, h, k, l, ix, iy; REBOUND's Pal ix, iy),
                              3-D integration, prior adds ix^2 + iy^2 >= 4 (state.py:311-313)      */
    double resolve_tol;    /* adaptive resolution: bound on a walker's |logL| error as
                              estimated from the extrapolation itself -- the change of chi2/npoints
                              when the coarsest level is dropped -- split evenly over its two
                              directions.  A direction above its half first gets one extra level
                              (the extension, rvm_plan_extension) joined to its stored levels; if
                              that does not settle it, the walker's open directions are integrated
                              again together with every step halved, up to resolve_max times (the
                              reference's IAS15 adapts its step to the orbit; a fixed plan step
                              does not).  The halving passes run in a second kernel on the launch's
                              stream; every launch function of an adaptive plan
                              enqueues both.  <= 0: off                                            */
    int32_t resolve_max;   /* 0..RVM_RESOLVE_MAX_LIMIT halvings; 0 with resolve_tol > 0: flag
                              (UNRESOLVED) only                                                    */
} rvm_config;

typedef struct rvm_plan rvm_plan;

/* Build the epoch schedule for one observation set (host arrays, n_obs epochs in any order and
 * sign; t = 0 is the initial condition).  Allocates device memory and workspace for up to
 * max_walkers walkers per launch -- with four increasing levels and max_walkers large enough for
 * the level-split launch layout (more walker groups than half the CUs) also its hand-off
 * workspace, 16 * max(epochs per direction) * max_walkers + 8 * max_walkers bytes.
 * observations.py:6-69 (tf/tb/rvf/rvb/errorf/errorb). */
int rvm_plan_create(const rvm_config* cfg, const double* t, const double* rv, const double* sigma, int32_t n_obs,
                    int32_t max_walkers, rvm_plan** out);
void rvm_plan_destroy(rvm_plan* plan);
/* schedule introspection: total level-1 steps per direction (fwd, bwd), epochs per direction */
int rvm_plan_info(const rvm_plan* plan, int32_t* steps_fwd, int32_t* steps_bwd, int32_t* epochs_fwd,
                  int32_t* epochs_bwd);
/* The adaptive resolution's extension level of a plan: *ext_mult = its steps per base step
 * (max(level_mult) + 1), or 0 when the plan has none -- resolution off or flag-only, n_levels < 2 or
 * = RVM_MAX_LEVELS, or its stored main-pass values (2 doubles per direction, epoch and walker:
 * 32 * max(epochs per direction) * max_walkers bytes of device memory, written by every launch)
 * above RVM_EXT_MAX_BYTES. */
#define RVM_EXT_MAX_BYTES (4ull << 30)
int rvm_plan_extension(const rvm_plan* plan, int32_t* ext_mult);
/* Eccentricity guard of the adaptive resolution (plans with an extension level): a walker with a
 * planet of eccentricity above e counts as above the bound after the main pass whatever its
 * estimate, so the extension verifies it -- the estimate under-reads on orbits whose pericentre
 * passage is much quicker than the plan's reference orbit.  e <= 0: off (default). */
int rvm_plan_set_verify_eccentricity(rvm_plan* plan, double e);

/* The certain-reject test of the adaptive resolution (on: default).  On fused sampler launches a
 * walker whose accept test fails even at the upper bound on its logL that both directions' lower
 * bounds on chi2 give stops refining and reports that bound (a certain reject).  The bound of an
 * open direction is empirical (chi2 less the change its last stage brought, capped at 100 x its
 * estimate; the measured error / estimate stays <= 57), so on = 0 lets every
 * open walker refine to the plan's tolerance instead.  Replaces nothing in the reference (IAS15
 * integrates every proposal in full, state.py:61-73). */
int rvm_plan_set_certain_reject(rvm_plan* plan, int32_t on);

/* Counters of a plan since its creation or the last reset, read in order on `stream` (the call
 * synchronises that stream; any output pointer may be NULL):
 *   handoff_timeouts  level-split hand-off waits that gave up (rvm_plan_set_handoff_timeout): their
 *                     walkers report RVM_STATUS_NONFINITE, the plan's hand-off workspace is dirty
 *                     and every later level-split launch on the plan reports NONFINITE until reset
 *   nonfinite         walkers finished with RVM_STATUS_NONFINITE (any launch on the plan)
 *   unresolved        walkers finished with RVM_STATUS_UNRESOLVED
 *   refined           walker-direction passes of the adaptive resolution (extension + halvings)
 *   truncated         walker-directions whose refinement stopped because the proposal's accept
 *                     test fails even at the upper bound on its logL both directions give
 *                     (fused sampler launches): such a proposal is rejected and
 *                     reports that upper bound
 * reset != 0: zero the counters and restore the hand-off workspace, after the stream's earlier work.
 * The samplers (rvmcmc) check this and raise on timeouts / non-finite results (mcmc.py:28-35: emcee
 * refuses NaN log-probabilities) rather than treating them as ordinary rejections. */
int rvm_plan_faults(rvm_plan* plan, int32_t reset, int64_t* handoff_timeouts, int64_t* nonfinite,
                    int64_t* unresolved, int64_t* refined, int64_t* truncated, void* stream);
/* All of a plan's counters as an array (the same reset): out[0..4] as rvm_plan_faults, out[5]
 * walker-directions the adaptive resolution settled at their roundoff floor (a halving pass whose
 * estimate no longer fell: the direction keeps its best pass, whose estimate was within
 * RVM_FLOOR_BOUND = 4 x the bound), out[6] speculative variant slots skipped
 * (RVM_STATUS_SKIPPED); entries past RVM_N_COUNTERS read 0. */
#define RVM_N_COUNTERS 7
int rvm_plan_counters(rvm_plan* plan, int32_t reset, int64_t* out, int32_t n, void* stream);
/* Hedged pass 2 (fused stretch launches whose likelihood grid leaves CUs idle run the
 * second halving pass of the walker slots with the quickest pericentre passages beside the likelihood
 * kernel): since the last reset, hedged = walker slots hedged, replayed = pass-2 walker-directions the
 * refinement kernel took from the hedge, missed = pass-2 walker-directions of hedged launches it integrated
 * itself (not hedged, or not complete in time).  Whether a result is ready in time depends on timing:
 * these are kept apart from rvm_plan_counters, whose values do not.  Any pointer may be NULL; all zero on
 * a plan without a hedge (RVM_HEDGE=0).  Synchronises the stream. */
int rvm_plan_hedge_stats(rvm_plan* plan, int32_t reset, int64_t* hedged, int64_t* replayed, int64_t* missed,
                         void* stream);
/* The hedge's early stop (the refinement kernel marks, at its start, the hedge blocks whose
 * group has no walker slot on its work lists, and they stop; RVM_HEDGE_MARK=0 at plan creation: never), since
 * the last reset: marked = (group, direction) marks written, gave_up = hedge blocks that stopped on their mark
 * (a block that had completed before its mark came is not counted, so gave_up <= marked).  Reset semantics
 * and the dependence on timing as rvm_plan_hedge_stats; all zero on a plan without a hedge.  Either pointer
 * may be NULL.  Synchronises the stream. */
int rvm_plan_hedge_marks(rvm_plan* plan, int32_t reset, int64_t* marked, int64_t* gave_up, void* stream);
/* Team A's wait for a running hedge block (after pass 1, when an open walker's hedge block
 * has ranked its slots but not yet stored pass 2, team A polls for it before it hands the pass on to team B, and
 * gives way when team B arrives; RVM_HEDGE_WAIT=0 at plan creation: never), since the last reset: waited = trials
 * that polled, late_hits = polls that ended with the group finished from the hedge's results, gave_way = polls
 * after which team A handed pass 2 on (team B arrived, the group's done word, a block that stopped, the safety
 * bound, or results that did not end every walker); waited = late_hits + gave_way.  Reset semantics and the
 * dependence on timing as rvm_plan_hedge_stats; all zero on a plan without a hedge and in the layouts without
 * teams.  Any pointer may be NULL.  Synchronises the stream. */
int rvm_plan_hedge_waits(rvm_plan* plan, int32_t reset, int64_t* waited, int64_t* late_hits, int64_t* gave_way,
                         void* stream);
/* Kernel timing (benchmarks): the plan's next max_launches likelihood evaluations (any entry point)
 * record HIP events on their stream around the likelihood kernel and around the refinement kernel
 * that follows it (0..4096; 0 stops).  rvm_plan_kernel_times waits for those events and returns
 * each evaluation's two kernel durations in ms (logl_ms[i], refine_ms[i]; either may be NULL; up
 * to max of them, *n_out = how many), then stops timing. */
int rvm_plan_time_kernels(rvm_plan* plan, int32_t max_launches);
int rvm_plan_kernel_times(rvm_plan* plan, float* logl_ms, float* refine_ms, int32_t max, int32_t* n_out);
/* Level-split hand-off waits give up after `seconds` without progress (default 2 s; > 0). */
int rvm_plan_set_handoff_timeout(rvm_plan* plan, double seconds);

/* logl_out[w] = -chi2/npoints_norm or -INF; status_out[w]; rv_out (nullable) = model RV
 * [n_obs][n_walkers] in the plan's input epoch order.  hill_factor = State.hillRadiusFactor
 * as the caller sees it (1.0 inside the reference samplers after deepcopy, state.py:212-213). */
int rvm_logl_batch(const rvm_plan* plan, int32_t n_walkers, const double* params, double hill_factor,
                   double* logl_out, int32_t* status_out, double* rv_out, void* stream);

/* ---- samplers (device-side proposal / accept; counter-based Philox4x32-10 RNG) ------------------
 * Draws are keyed by (seed, iteration, stream_id, global walker index), so results do not depend
 * on how walkers are sharded across ranks.  Every launch takes optional `draws` (device, nullable):
 * when non-NULL the documented uniforms/normals are read from it instead of Philox (tests inject
 * the same draws into the oracle). */

/* emcee 2.2.1 stretch move, half-step (S0 = walkers [s0_begin, s0_begin+n_s0) of the GLOBAL
 * ensemble, complement S1 given as a device array [n_params][n_s1] of positions).
 * propose: z = ((a-1)u1+1)^2/a, j = floor(u2*n_s1), q = c_j - z (c_j - x)
 *   writes q_out [n_params][n_s0] and z_out [n_s0].  draws layout: [2][n_s0] (u1, u2).
 * accept: lnpdiff = (n_params-1) ln z + lnp_new - lnp_old > ln(u3) -> x <- q, lnp <- lnp_new.
 *   x, lnp: [n_params][n_s0], [n_s0] (in place).  accepted: int32 counters [n_s0] (+= 1).
 *   draws layout: [n_s0] (u3). */
int rvm_stretch_propose(int32_t n_params, int32_t n_s0, int64_t s0_begin, const double* x, int32_t n_s1,
                        const double* c, double a, uint64_t seed, uint64_t iteration, uint32_t half,
                        const double* draws, double* q_out, double* z_out, void* stream);
int rvm_stretch_accept(int32_t n_params, int32_t n_s0, int64_t s0_begin, double* x, double* lnp, const double* q,
                       const double* lnp_new, const double* z, uint64_t seed, uint64_t iteration, uint32_t half,
                       const double* draws, int32_t* accepted, void* stream);

/* Mapping of a State's free-parameter vector onto the kernel's parameter rows (rvmcmc.engine.
 * ParamMap): row r (5 or 7 per planet, see Conventions) takes free parameter src[r], or the fixed
 * value base[r] when src[r] < 0 (state.py:26-31 ignore_vars / ignore_params). */
#define RVM_MAX_PARAM_ROWS (7 * RVM_MAX_PLANETS)
typedef struct rvm_param_map {
    int32_t n_rows;
    int32_t src[RVM_MAX_PARAM_ROWS];
    double base[RVM_MAX_PARAM_ROWS];
} rvm_param_map;

/* One whole stretch-move half-step in ONE likelihood launch: the proposal (as
 * rvm_stretch_propose, Philox draws), the walker log-likelihood of the proposals (as
 * rvm_logl_batch on map(q)), and the accept (as rvm_stretch_accept), bit-identical to the
 * three-call sequence.  x: [n_params][n_s0] free parameters (in place), lnp [n_s0] (in place),
 * c_aos: the complement WALKER-MAJOR, [n_s1][n_params] (each c_j one contiguous row: one cache line
 * per gathered walker instead of n_params), n_s0 <= the plan's max_walkers.  x_aos (nullable): a
 * walker-major mirror [n_s0][n_params] of x that accepted proposals are written to as well (the
 * next half-step's c_aos).  lnp_new_out / status_out (nullable): the proposals' logl and status;
 * accepted (nullable): int32 counters += 1. */
int rvm_stretch_half_step(const rvm_plan* plan, const rvm_param_map* map, int32_t n_params, int32_t n_s0,
                          int64_t s0_begin, double* x, double* x_aos, double* lnp, int32_t n_s1, const double* c_aos,
                          double a, uint64_t seed, uint64_t iteration, uint32_t half, double hill_factor,
                          double* lnp_new_out, int32_t* status_out, int32_t* accepted, void* stream);

/* One whole stretch-move ITERATION (both half-steps, mcmc.py:57-65 / emcee 2.2.1 sample()) in one
 * likelihood launch plus one small accept launch, bit-identical to two rvm_stretch_half_step calls.
 * The second half's proposal against partner j depends on j's first-half decision, so begin
 * evaluates it both ways (partner rejected: c0[j]; accepted: its proposal q0(j)) next to the first
 * half's own proposals -- 3 n_loc walker slots in one launch, which keeps a chip that one half-step
 * fills only partly busy (n_loc walkers of each half per rank; the plan needs max_walkers >= 3 n_loc).
 *
 * begin: half 0's proposals against c1, its logl and accepts (x0, lnp0 in place; accepted0 +=);
 *   half 1's proposals x1 against both variants of its partner in c0; logl of all 3 n_loc slots to
 *   lnp_spec / status_spec [3 n_loc] (slot n_loc + v n_loc + k: half 1's walker k, variant v);
 *   half 0's decisions to dec [n_loc] (1 accepted).  c0, c1: both halves walker-major
 *   [n_half][n_params] as at the start of the iteration, global order (on one rank: the walker-major
 *   mirrors); they must not be written before end has run.  s0_begin / s1_begin: global index of
 *   this rank's first walker of half 0 (its index within the half) and of half 1 (n_half + its
 *   index within half 1): the Philox keys.  lnp1 (nullable): half 1's log-probabilities [n_loc] as at the start of
 *   the iteration -- its accept inputs, which lets the adaptive resolution cut a refinement short
 *   on a certain reject (rvm_plan_faults `truncated`); NULL refines half 1's slots fully.
 * end: half 1's accepts with the variant dec_all[j] selects (dec_all: half 0's decisions in
 *   global order, [n_half]; on one rank dec itself); x1, lnp1 in place, x1_aos / x0_aos (nullable)
 *   mirrors updated; lnp_new_out / status_new_out (nullable): the chosen proposals' logl, status. */
int rvm_stretch_iteration_begin(const rvm_plan* plan, const rvm_param_map* map, int32_t n_params, int32_t n_loc,
                                int64_t s0_begin, int64_t s1_begin, double* x0, double* lnp0, const double* x1,
                                const double* lnp1, int32_t n_half, const double* c0, const double* c1, double a,
                                uint64_t seed, uint64_t iteration, double hill_factor, double* lnp_spec,
                                int32_t* status_spec, int32_t* dec, int32_t* accepted0, void* stream);
int rvm_stretch_iteration_end(int32_t n_params, int32_t n_loc, int64_t s0_begin, int64_t s1_begin, const double* x0,
                              double* x0_aos, const int32_t* dec, const int32_t* dec_all, double* x1, double* x1_aos,
                              double* lnp1, int32_t n_half, const double* c0, const double* c1,
                              const double* lnp_spec, const int32_t* status_spec, double a, uint64_t seed,
                              uint64_t iteration, int32_t* accepted1, double* lnp_new_out, int32_t* status_new_out,
                              void* stream);

/* ---- parallel tempering of the stretch-move ensemble ----------------------------------------------
 * n_temps ensembles of W = 2 n_half walkers at inverse temperatures betas[0] > betas[1] > ... > 0
 * (a device array [n_temps]; temperature 0 is the coldest, betas[0] = 1 samples the posterior; the
 * caller validates the values).  Each half h is SoA [n_params][n_temps * n_half], column
 * i = t * n_half + k, with the UNtempered log-probabilities lnp [n_temps * n_half].  The Philox item
 * of walker k of half h at temperature t is g = t * W + h * n_half + k (at n_temps = 1 the global
 * walker index of rvm_stretch_propose / rvm_stretch_accept, whose bits these entries then give).
 * One iteration: propose, rvm_logl_batch of the n_temps * n_half proposals and accept for half 0,
 * the same for half 1, then (every few iterations) the exchange sweep.
 * Argument errors (n_params, n_temps or n_half < 1; n_temps * n_half beyond int32; half > 1; a <= 1;
 * a null required pointer) return < 0 before any HIP call.
 *
 * propose: as rvm_stretch_propose with x this half and c the OTHER half (both [n_params][n_temps *
 *   n_half]): walker (t, k) draws its partner j = floor(u2 * n_half) among its own temperature's
 *   walkers of c, column t * n_half + j.  Stream RNG_STRETCH_PROPOSE | half << 8, item g.  Writes
 *   q_out [n_params][n_temps * n_half], z_out [n_temps * n_half].  draws layout: [2][n_temps * n_half]
 *   (u1, u2).
 * accept: lnpdiff = (n_params-1) ln z + betas[t] * lnp_new - betas[t] * lnp_old > ln(u3)  (evaluated
 *   left to right) -> x <- q, lnp <- lnp_new; a -inf lnp_new is rejected, lnp_old must be finite.
 *   u3: stream RNG_STRETCH_ACCEPT | half << 8, item g.  accepted (nullable): int32 counters
 *   [n_temps * n_half] (+= 1).  draws layout: [n_temps * n_half] (u3).
 * swap: the sweep over the pairs p = n_temps-2 .. 0 (hottest pair first); pair p exchanges walker
 *   w = h * n_half + k of temperature p with walker w of temperature p + 1 when
 *   (betas[p] - betas[p+1]) * (lnp[p+1][w] - lnp[p][w]) > ln(u): their position columns and lnp
 *   values trade places (x0, lnp0: half 0; x1, lnp1: half 1; in place) and swapped[p][w] += 1
 *   (int32 [n_temps-1][W]).  u: the first uniform of stream 7 (RNG_PT_SWAP), item p * W + w.
 *   draws layout: [n_temps-1][W].  One thread carries walker index w through the whole sweep: no
 *   atomics, deterministic.  n_temps = 1 returns 0 without a launch (the array arguments are not read). */
int rvm_pt_stretch_propose(int32_t n_params, int32_t n_temps, int32_t n_half, const double* x, const double* c,
                           double a, uint64_t seed, uint64_t iteration, uint32_t half, const double* draws,
                           double* q_out, double* z_out, void* stream);
int rvm_pt_stretch_accept(int32_t n_params, int32_t n_temps, int32_t n_half, const double* betas, double* x,
                          double* lnp, const double* q, const double* lnp_new, const double* z, uint64_t seed,
                          uint64_t iteration, uint32_t half, const double* draws, int32_t* accepted, void* stream);
int rvm_pt_swap(int32_t n_params, int32_t n_temps, int32_t n_half, const double* betas, double* x0, double* x1,
                double* lnp0, double* lnp1, uint64_t seed, uint64_t iteration, const double* draws,
                int32_t* swapped, void* stream);

/* The ladder's dynamics and the per-temperature log-likelihood moments, after an exchange sweep
 * (ptemcee sampler.py Sampler._get_ladder_adjustment, called from Sampler.sample once per iteration;
 * emcee 2.2.1 ptsampler.py PTSampler.sample stores the per-temperature lnlikelihood that
 * PTSampler.thermodynamic_integration_log_evidence averages).  Two launches on `stream`, no
 * floating-point atomics, the same bits from run to run:
 *   total[p] = sum_w swapped[p][w] (int64) ; count[p] = total[p] - swap_totals_prev[p] ;
 *   swap_totals_prev[p] = total[p] ; ratios_out[p] = (double)count[p] / (double)W        p < n_temps-1
 *   lnp_moments[t][0] += sum_w lnp[t][w] ; lnp_moments[t][1] += sum_w lnp[t][w]^2   (when not null;
 *     w in index order, half 0 first: per-thread strided partials of 256 threads, then a tree)
 *   and, with n_temps >= 3 (both end temperatures stay fixed: beta = 0 is refused, so the hottest
 *   temperature is finite), every expression left to right, A = ratios_out:
 *     dS[i] = kappa * (A[i] - A[i+1]) ; dT[i] = (1/betas[i+1] - 1/betas[i]) * exp(dS[i])   i = 0 .. n_temps-3
 *     acc = 1/betas[0] ; acc = acc + dT[i] ; new[i+1] = 1 / acc
 *   If every dS is 0 (kappa = 0, equal ratios) betas stay bit for bit.  Else if any new beta is not
 *   finite or the new ladder is not strictly decreasing down to the fixed betas[n_temps-1] (the
 *   interior can overshoot it), betas stay and *n_refused += 1.  Else betas[1 .. n_temps-2] = new.
 * swapped: rvm_pt_swap's int32 [n_temps-1][W]; lnp0, lnp1: the halves' lnp [n_temps * n_half];
 * betas [n_temps] in/out; swap_totals_prev int64 [n_temps-1] in/out; ratios_out [n_temps-1];
 * n_refused int64 [1] in/out; lnp_moments [n_temps][2] in/out, may be null (the moment rows are then
 * not launched); workspace: 3 n_temps - 1 words of 8 bytes that carry the totals and this call's
 * moments from the first launch to the second (contents unspecified before and after).  All device
 * arrays.  Argument errors (n_temps or n_half < 1; n_temps * W beyond int32; kappa negative or not
 * finite; a null pointer other than lnp_moments) return < 0 before any HIP call and name the argument
 * in rvm_last_error.  n_temps = 1 returns 0 without a launch (the array arguments are not read). */
int rvm_pt_ladder_update(int32_t n_temps, int32_t n_half, const int32_t* swapped, const double* lnp0,
                         const double* lnp1, double kappa, double* betas, int64_t* swap_totals_prev,
                         double* ratios_out, int64_t* n_refused, double* lnp_moments, void* workspace,
                         void* stream);

/* Gaussian random-walk Metropolis-Hastings (mcmc.py:89-121), n_chains independent chains:
 * propose: q = x + step_size * scales[p] * N(0,1)        draws layout: [n_params][n_chains]
 * accept : exp(lnp_new - lnp_old) > u -> x <- q, lnp <- lnp_new   draws layout: [n_chains] */
int rvm_mh_propose(int32_t n_params, int32_t n_chains, int64_t chain_begin, const double* x, const double* scales,
                   double step_size, uint64_t seed, uint64_t iteration, const double* draws, double* q_out,
                   void* stream);
int rvm_mh_accept(int32_t n_params, int32_t n_chains, int64_t chain_begin, double* x, double* lnp, const double* q,
                  const double* lnp_new, uint64_t seed, uint64_t iteration, const double* draws, int32_t* accepted,
                  void* stream);
/* One whole MH step of n_chains chains (mcmc.py:107-121 for every chain) in ONE likelihood launch:
 * the proposal (as rvm_mh_propose, Philox draws), the walker log-likelihood of map(q) (as
 * rvm_logl_batch) and the accept (as rvm_mh_accept), bit-identical to the three-call sequence.
 * x [n_params][n_chains] and lnp [n_chains] in place; scales [n_params]; n_chains <= the plan's
 * max_walkers.  lnp_new_out / status_out (nullable): the proposals' logl and status; accepted
 * (nullable): int32 counters += 1.  Prior / encounter proposals are rejected through -inf. */
int rvm_mh_step(const rvm_plan* plan, const rvm_param_map* map, int32_t n_params, int32_t n_chains,
                int64_t chain_begin, double* x, double* lnp, const double* scales, double step_size, uint64_t seed,
                uint64_t iteration, double hill_factor, double* lnp_new_out, int32_t* status_out, int32_t* accepted,
                void* stream);

/* Central finite-difference stencil for SMALA's gradient/metric (x: [n_params][n_chains]).
 * out: SoA [n_params][(2P+1) * n_chains]; stencil point s of chain c is walker s*n_chains + c with
 * s = 0: x, s = 1+2p: x + eps_p e_p, s = 2+2p: x - eps_p e_p, eps_p = rel_step*max(|x_p|, floor[p]).
 * One rvm_logl_batch over (2P+1)*n_chains walkers then gives logp, its gradient and (rv_out) the
 * per-epoch RV Jacobian. */
int rvm_fd_params(int32_t n_params, int32_t n_chains, const double* x, double rel_step, const double* floor_,
                  double* out, void* stream);

/* ---- SMALA (mcmc.py:126-187) on device, one thread per chain ---------------------------------
 * Per-chain quantities a SMALA step needs at a point x; all device arrays, C = n_chains,
 * P = n_params (<= RVM_SMALA_MAX_PARAMS), matrices row-major per chain: element (i, j) of chain c
 * at [(i * P + j) * C + c]. */
typedef struct {
    double* lp;      /* [C]       logp(x)                                                          */
    double* grad;    /* [P][C]    central-difference gradient of logp                              */
    double* mu;      /* [P][C]    drift x + eps^2/2 G^-1 grad                  (mcmc.py:150)        */
    double* L;       /* [P*P][C]  Cholesky factor of G^-1, lower                (mcmc.py:149)        */
    double* G;       /* [P*P][C]  SoftAbs metric Q diag(lambda coth(alpha lambda)) Q^T of eig(-H)  */
    double* logdet;  /* [C]       log det G^-1                                                     */
    int32_t* ok;     /* [C]       1: clean stencil and positive-definite metric                    */
} rvm_smala_cache;

/* From one rvm_logl_batch launch over rvm_fd_params' stencil of x (same x, rel_step, floor_;
 * walkers s * C + c, with rv_out): the gradient from the stencil's logp, the Gauss-Newton Hessian
 * H = -(2/npoints) J^T diag(inv_sigma2) J from its per-epoch model RVs (rv_stencil
 * [n_obs][(2P+1) C], rows in the plan's input epoch order; inv_sigma2 [n_obs] in the same order),
 * the SoftAbs metric of -H (cyclic Jacobi eigen-solver), G^-1, its Cholesky factor and the drift.
 * Replaces state.py:253-294 (variational derivatives) + mcmc.py:135-150. */
int rvm_smala_derive(int32_t n_params, int32_t n_chains, int32_t n_obs, const double* x, double rel_step,
                     const double* floor_, const double* lp_stencil, const int32_t* status_stencil,
                     const double* rv_stencil, const double* inv_sigma2, double npoints_norm, double alpha,
                     double eps, const rvm_smala_cache* out, void* stream);
/* The same cache from exact derivatives (rvm_logl_derivs outputs: lp [C], status [C], grad [P][C],
 * hess [P*P][C]): the reference's Hessian (state.py:253-294) instead of the Gauss-Newton one.
 * Chains with status != 0 or non-finite derivatives get ok = 0.  mcmc.py:135-150. */
int rvm_smala_metric(int32_t n_params, int32_t n_chains, const double* x, const double* lp, const int32_t* status,
                     const double* grad, const double* hess, double alpha, double eps, const rvm_smala_cache* out,
                     void* stream);
/* x_prop = mu + eps chol(G^-1) z (x where the cache is not ok); z ~ N(0,1) from Philox keyed by
 * (seed, chain_begin + c, iteration, 5 | p << 8) or from draws [P][C].  mcmc.py:144-153. */
int rvm_smala_propose(int32_t n_params, int32_t n_chains, int64_t chain_begin, const double* x,
                      const rvm_smala_cache* cur, double eps, uint64_t seed, uint64_t iteration,
                      const double* draws, double* x_prop, void* stream);
/* exp(lp* - lp + log q(x | x*) - log q(x* | x)) > u  (u from Philox stream 6 or draws [C]), both
 * caches ok and lp* finite -> x <- x_prop, cur <- prop (per chain), accepted[c] += 1.
 * failures[c] += 1 (nullable) when the proposal's metric failed with a finite logp.
 * mcmc.py:158-187. */
int rvm_smala_accept(int32_t n_params, int32_t n_chains, int64_t chain_begin, double* x, const rvm_smala_cache* cur,
                     const double* x_prop, const rvm_smala_cache* prop, double eps, uint64_t seed,
                     uint64_t iteration, const double* draws, int32_t* accepted, int32_t* failures, void* stream);

/* Fused SMALA step, three launches instead of five (mcmc.py:167-187 for every chain):
 *   rvm_smala_propose                       x* (unchanged)
 *   rvm_smala_stencil_logl                  rvm_fd_params' stencil of x* formed inside ONE likelihood
 *                                           launch (walker s * n_chains + c, as rvm_fd_params; map:
 *                                           free parameters -> kernel rows, as rvm_stretch_half_step)
 *                                           -> logl / status [(2P+1) C], rv_out [n_obs][(2P+1) C]
 *   rvm_smala_derive_accept                 rvm_smala_derive of x* into prop, then rvm_smala_accept,
 *                                           in one kernel (one wave per chain)
 * bit-identical to rvm_fd_params + rvm_logl_batch + rvm_smala_derive + rvm_smala_accept.
 * rvm_smala_metric_accept is the exact-Hessian counterpart (rvm_smala_metric + rvm_smala_accept). */
int rvm_smala_stencil_logl(const rvm_plan* plan, const rvm_param_map* map, int32_t n_params, int32_t n_chains,
                           const double* x, double rel_step, const double* floor_, double hill_factor,
                           double* logl_out, int32_t* status_out, double* rv_out, void* stream);
int rvm_smala_derive_accept(int32_t n_params, int32_t n_chains, int64_t chain_begin, int32_t n_obs, double* x,
                            const double* x_prop, double rel_step, const double* floor_, const double* lp_stencil,
                            const int32_t* status_stencil, const double* rv_stencil, const double* inv_sigma2,
                            double npoints_norm, double alpha, double eps, const rvm_smala_cache* cur,
                            const rvm_smala_cache* prop, uint64_t seed, uint64_t iteration, const double* draws,
                            int32_t* accepted, int32_t* failures, void* stream);
/* The fused step with the centres' logp on a second (adaptive) plan, launched on another stream
 * (mcmc.py:167-187; the reference's logp is IAS15's):
 *   rvm_smala_derive_sides    rvm_smala_derive of x* without the stencil's centre row (its status and
 *                             logp are not read): gradient, Hessian, metric, drift, Cholesky into prop,
 *                             on the stencil's stream while the centres' launch still runs
 *   rvm_smala_center_accept   prop's logp from lp_center, prop ok only if status_center is 0, then
 *                             rvm_smala_accept, once the centres' launch is done
 * bit-identical to copying the centres' logp / status into the stencil's row 0 and calling
 * rvm_smala_derive_accept (the other cache entries do not depend on that row). */
int rvm_smala_derive_sides(int32_t n_params, int32_t n_chains, int32_t n_obs, const double* x, double rel_step,
                           const double* floor_, const double* lp_stencil, const int32_t* status_stencil,
                           const double* rv_stencil, const double* inv_sigma2, double npoints_norm, double alpha,
                           double eps, const rvm_smala_cache* out, void* stream);
int rvm_smala_center_accept(int32_t n_params, int32_t n_chains, int64_t chain_begin, double* x, const double* x_prop,
                            const double* lp_center, const int32_t* status_center, const rvm_smala_cache* cur,
                            const rvm_smala_cache* prop, double eps, uint64_t seed, uint64_t iteration,
                            const double* draws, int32_t* accepted, int32_t* failures, void* stream);
int rvm_smala_metric_accept(int32_t n_params, int32_t n_chains, int64_t chain_begin, double* x, const double* x_prop,
                            const double* lp, const int32_t* status, const double* grad, const double* hess,
                            double alpha, double eps, const rvm_smala_cache* cur, const rvm_smala_cache* prop,
                            uint64_t seed, uint64_t iteration, const double* draws, int32_t* accepted,
                            int32_t* failures, void* stream);

/* ---- exact derivatives (state.py:218-294) ----------------------------------------------------
 * logp, its gradient and its Hessian for n_chains parameter vectors (params: kernel rows
 * [5|7 * n_planets][n_chains], as rvm_logl_batch), differentiated along n_dirs kernel rows
 * dir_rows[0..n_dirs) (host array; the free parameters of the State, in its order):
 *   logl_out [n_chains]            -chi2/npoints_norm (or -INF with status != 0)
 *   grad_out [n_dirs][n_chains]    d logp / d p_i
 *   hess_out [n_dirs*n_dirs][n_chains]  d2 logp / d p_i d p_j, row-major per chain (symmetric)
 *   status_out [n_chains]          as rvm_logl_batch; gradient and Hessian are NaN unless 0
 * The reference integrates REBOUND's order-1 and order-2 variational equations (one variation per
 * parameter, one per pair); here every parameter pair (i >= j) is one hyper-dual integration of the
 * plan's own discrete integrator (same steps, levels and Richardson weights as rvm_logl_batch),
 * so the results are the exact derivatives of that likelihood.  workspace: device buffer of
 * rvm_logl_derivs_workspace_bytes(n_chains, n_dirs) bytes (no allocation inside).  No limit from
 * the plan's max_walkers. */
size_t rvm_logl_derivs_workspace_bytes(int32_t n_chains, int32_t n_dirs);
int rvm_logl_derivs(const rvm_plan* plan, int32_t n_chains, const double* params, int32_t n_dirs,
                    const int32_t* dir_rows, double hill_factor, double* logl_out, double* grad_out, double* hess_out,
                    int32_t* status_out, void* workspace, void* stream);

/* ---- the recorded chain and its autocovariance ---------------------------------------------------
 * Replaces the host side of the reference's production workflow (driver.py:86-120 run loop filling a
 * host chain every iteration; driver.py:265-414 trim, autocorrelation times, efficacy): the chain stays
 * in device memory and only the [n_params][n_lags] autocovariance crosses to the host.
 * A chain buffer is [n_steps][n_params][n_cols] float64 -- one step slot is the SoA block
 * [n_params][n_cols] every sampler holds -- with an optional log-probability buffer [n_steps][n_cols].
 * The conventions above hold for the three launch functions: device pointers, no allocation, no
 * synchronisation, stream-ordered and capturable, no floating-point atomics (the same bits from run to
 * run); argument errors return < 0 before any HIP call and name the argument in rvm_last_error.
 * n_params is 1 .. 65534 and n_cols 1 .. 16776960 (a grid's y and z extents).
 *
 * record: one segment of a sampler's positions src [n_params][src_ld] into one step slot dst
 *   [n_params][dst_ld] (dst points AT the slot): dst[p][dst_col0 + j] = src[p][src_col0 + j col_stride],
 *   j < n_cols; with the nullable pair lnp_src [src_ld] / lnp_dst [dst_ld] (both or neither) also
 *   lnp_dst[dst_col0 + j] = lnp_src[src_col0 + j col_stride].  One launch per segment (the two halves of
 *   the stretch ensemble, the cold temperature's columns of each tempering half, the chains of MH / SMALA).
 * moments, per column (p, w) over the steps [t0, t1), n = t1 - t0, every sum left to right:
 *   mean_out[p][w] = (x[t0] + x[t0+1] + ... + x[t1-1]) / n ;  m2_out[p][w] = sum_t (x[t] - mean)^2
 *   (x - mean rounded, its square rounded, then added: no fused multiply-add).
 * autocov, for the lags k = lag0 .. lag0 + n_lags - 1 (each <= n - 1; n_lags <= 2^30 and
 *   n_params * n_lags within int32):
 *   acov_out[p][k - lag0] = (1/W) sum_w sum_{t = t0}^{t1 - 1 - k} y[t] y[t + k],   W = n_cols,
 *   y = x - mean[p][w] rounded at use, mean [n_params][n_cols] as rvm_chain_moments wrote it.  This is
 *   the unnormalised sum that irfft(f conj f) of the zero-padded y gives (driver.integrated_time).
 *   The order of the sum is fixed:
 *     1. per walker, t ascending in one thread, acc = fma(y[t], y[t + k], acc) from acc = 0;
 *     2. the walkers of a block of 256 (walker block b: w in [256 b, 256 b + 256), absent walkers add
 *        +0) by a binary tree over the 256 slots, slot i += slot i + h for h = 128, 64, ..., 1
 *        (csrc/rvm_block_sum.h block_tree_sum: the one statement of it, for rvm_chain_cov and
 *        rvm_pt_ladder_update's moments as well);
 *     3. the walker blocks in index order, b = 0, 1, ..., in a second small launch, then one division
 *        by W.
 *   workspace: rvm_chain_autocov_workspace_bytes(n_params, n_cols, n_lags) bytes (8 n_params x n_lags
 *   rounded up to a multiple of 16 x ceil(n_cols / 256); 0 on bad arguments) that carry the blocks'
 *   partial sums from the first launch to the second (contents unspecified before and after).
 *   Only the lags asked for are computed: a caller that has lags [0, 64) asks for [64, 128) next. */
int rvm_chain_record(int32_t n_params, int32_t n_cols, const double* src, int64_t src_ld, int64_t src_col0,
                     int64_t col_stride, double* dst, int64_t dst_ld, int64_t dst_col0, const double* lnp_src,
                     double* lnp_dst, void* stream);
int rvm_chain_moments(const double* chain, int32_t n_params, int32_t n_cols, int64_t t0, int64_t t1, double* mean_out,
                      double* m2_out, void* stream);
size_t rvm_chain_autocov_workspace_bytes(int32_t n_params, int32_t n_cols, int32_t n_lags);
int rvm_chain_autocov(const double* chain, const double* mean, int32_t n_params, int32_t n_cols, int64_t t0, int64_t t1,
                      int32_t lag0, int32_t n_lags, double* acov_out, void* workspace, void* stream);

/* ---- posterior summaries of data already in device memory ------------------------------------------
 * What the reference reads off its host chain (driver.py:265-333 return_trimmed_results, :335
 * plot_corners): the parameters' quantiles and covariance, and states drawn from the chain whose RV
 * curves make the credible band.  The conventions of the chain entry points hold for the three launch
 * functions: device pointers (q is a host array, copied into the launch), no allocation, no
 * synchronisation, stream-ordered and capturable, no floating-point atomics, the same bits from run to
 * run; argument errors return < 0 before any HIP call and name the argument in rvm_last_error.  A
 * workspace's contents are unspecified before and after a call.
 *
 * rows_quantiles: exact quantiles of n_rows rows of doubles.  Element (o, i) of row r is
 *   x[r row_stride + o outer_stride + i], o < n_outer, i < n_inner (strides >= 0, in elements;
 *   n_rows 1 .. 65535; n_outer n_inner <= 2^32 - 1, what the 32-bit counters hold).
 *     a parameter of a chain over the steps [t0, t1): x = chain + t0 P W, n_rows = P, row_stride = W,
 *       n_outer = t1 - t0, outer_stride = P W, n_inner = W;
 *     the rows of an rv_out matrix [n_times][S]: n_outer = 1, n_inner = row_stride = S.
 *   q: n_q = 1 .. RVM_MAX_QUANTILES values in [0, 1].  out[r][j], the quantile q[j] of row r, is
 *     NaNs are not counted: m is the number of the row's other values (n_valid_out[r], nullable), and
 *       v[0 .. m-1] those values in ascending order -- +-inf are ordinary values, -0 sorts before +0;
 *     m = 0: NaN;  otherwise h = q (m - 1) (one rounded product), lo = floor(h), g = h - lo,
 *       hi = min(lo + 1, m - 1), and
 *     out = v[lo] if g == 0 or v[hi] == v[lo], else v[lo] + g (v[hi] - v[lo]) (the product rounded, then
 *       the sum: no fused multiply-add) -- numpy's default 'linear' rule up to its last roundings.
 *   The order statistics are exact: a radix select on the order-preserving 64-bit key of a double (all
 *   bits of a negative flipped, the sign bit of the others), eight bits per pass; the row is not sorted
 *   and not modified.  The loads are 16 bytes wide when x is 16-byte aligned and both strides are even.
 *   workspace: rvm_rows_quantiles_workspace_bytes(n_rows, n_q) bytes (0 on bad arguments), 8-byte aligned.
 * chain_cov, over the steps [t0, t1) of a chain [n_steps][n_params][n_cols], n = t1 - t0, W = n_cols:
 *   cov_out[p][q] = (sum_w sum_t y_p y_q) / (double)(n W - 1),  y_p = x[t][p][w] - center[p] rounded at
 *   use, center [n_params] on the device.  The order of the sum is rvm_chain_autocov's: per walker, t
 *   ascending in one thread, acc = fma(y_p, y_q, acc) from acc = 0; the walkers of a block of 256 by the
 *   binary tree (h = 128, 64, ..., 1; absent walkers add +0); the walker blocks in index order in a second
 *   small launch; one division.  p >= q is computed and mirrored, so cov_out is symmetric bit for bit;
 *   n W = 1 gives NaN; n_params <= 16384, n_cols <= 4194240.  workspace:
 *   rvm_chain_cov_workspace_bytes(n_params, n_cols) bytes (8 n_params^2 n_cols, the walkers' own sums
 *   between the two launches; 0 on bad arguments).
 * chain_draw: n_samples states of the steps [t0, t1), with replacement.  Sample s takes (u1, u2) =
 *   uniform2(seed, item = s, iteration = draw_id, stream 8), or draws[0][s], draws[1][s] when draws
 *   [2][n_samples] is given;  t = t0 + min(floor(u1 n), n - 1), w = min(floor(u2 W), W - 1) (the
 *   device's uniform can round to 1.0; below 0 and NaN give index 0);
 *   x_out[p][s] = chain[t][p][w], idx_out[s] = t W + w (nullable). */
size_t rvm_rows_quantiles_workspace_bytes(int32_t n_rows, int32_t n_q);
int rvm_rows_quantiles(const double* x, int32_t n_rows, int64_t row_stride, int64_t n_outer, int64_t outer_stride,
                       int64_t n_inner, const double* q, int32_t n_q, double* out, int64_t* n_valid_out,
                       void* workspace, void* stream);
size_t rvm_chain_cov_workspace_bytes(int32_t n_params, int32_t n_cols);
int rvm_chain_cov(const double* chain, int32_t n_params, int32_t n_cols, int64_t t0, int64_t t1, const double* center,
                  double* cov_out, void* workspace, void* stream);
int rvm_chain_draw(const double* chain, int32_t n_params, int32_t n_cols, int64_t t0, int64_t t1, int32_t n_samples,
                   uint64_t seed, uint64_t draw_id, const double* draws, double* x_out, int64_t* idx_out,
                   void* stream);

/* ---- periodograms of data already in device memory -------------------------------------------------
 * The generalised Lomb-Scargle periodogram (Zechmeister & Kuerster 2009: weights, floating mean) of
 * n_series residual series y_s = data - model[:, s] at the frequencies f_k, over n_obs epochs: which
 * periods are in the velocities, and what a fit left in them.  The conventions of the summary entry
 * points hold: device pointers, no allocation, no synchronisation, stream-ordered and capturable, no
 * floating-point atomics, the same bits from run to run; argument errors return < 0 before any HIP call
 * and name the argument in rvm_last_error; a workspace's contents are unspecified before and after a call.
 *
 *   tau [n_obs]: epochs less a reference time of the caller's.  w [n_obs]: weights that sum to 1 up to
 *   rounding (the caller normalises 1 / sigma^2; used as given).  data [n_obs].  model, nullable:
 *   [n_obs][model_ld], series s in column s -- the layout of rv_out.  power_out[k power_ld + s]: rows are
 *   frequencies, so one rvm_rows_quantiles call over [n_freq][n_series] gives a band per frequency.
 *   freq_out [n_freq], nullable.  cos_out, sin_out [n_freq][n_obs].
 *   Limits: n_obs 1 .. 2 RVM_MAX_EPOCHS_PER_DIRECTION; n_freq >= 1; n_series >= 1; k0 >= 0 and
 *   k0 + n_freq <= 2^53; f0, df finite; model_ld >= n_series when model is given; power_ld >= n_series;
 *   float_mean 0 or 1; workspace 16-byte aligned.
 *
 * The definition is the algorithm: every product and sum below is one IEEE double operation, fma only
 * where it is written, and every sum runs over i ascending in one thread from acc = 0.
 *   1. basis, frequency index k < n_freq and epoch i:  f_k = fma((double)(k0 + k), df, f0);  x = f_k tau_i;
 *      r = x - rint(x) (exact);  (s_ki, c_ki) = sincospi(2 r), the device library's;  freq_out[k] = f_k.
 *      The phase is reduced in cycles before the trigonometry: its only error is the one rounding of x.
 *   2. per frequency:  C = sum fma(w_i, c_i, acc), S likewise (float_mean = 0: C = S = 0);
 *      ct_i = c_i - C, st_i = s_i - S;  u_i = w_i ct_i, v_i = w_i st_i;
 *      CC = sum fma(u_i, ct_i, acc), SS = sum fma(v_i, st_i, acc), CS = sum fma(u_i, st_i, acc).
 *   3. per series:  y_i = data_i - model[i][s] (data_i without a model);  m = sum fma(w_i, y_i, acc)
 *      (float_mean = 0: m = 0);  z_i = y_i - m;  YY = sum fma(w_i z_i, z_i, acc).
 *   4. per (k, s):  YC = sum fma(u_ki, z_is, acc), YS = sum fma(v_ki, z_is, acc);  D = CC SS - CS CS;
 *      p = ((SS YC) YC + (CC YS) YS - (2 (CS YC)) YS) / (YY D), left to right.
 *      Whatever IEEE gives is the result: a NaN column of model gives NaN powers in that column (which
 *      rvm_rows_quantiles does not count), YY = 0 gives NaN.  With a floating mean and n_obs = 3 the fit is
 *      exact and D is rounding noise: the caller keeps n_obs >= 4 (>= 3 without).
 * gls_basis writes step 1.  gls_power fills its table by launching the same kernel, so the public basis is
 * what the power used, and runs the frequencies in chunks (a table of about 64 MiB) that the result does
 * not depend on: a call over [k0, k0 + n_freq) equals the concatenation of calls over its pieces, bit for
 * bit.  workspace: rvm_gls_workspace_bytes(n_obs, n_freq, n_series) bytes (0 on bad arguments): a chunk's
 * u, v table and per-frequency sums, the per-series YY and z. */
int rvm_gls_basis(const double* tau, int32_t n_obs, double f0, double df, int64_t k0, int32_t n_freq, double* cos_out,
                  double* sin_out, double* freq_out, void* stream);
size_t rvm_gls_workspace_bytes(int32_t n_obs, int32_t n_freq, int32_t n_series);
int rvm_gls_power(const double* tau, const double* w, int32_t n_obs, const double* data, const double* model,
                  int64_t model_ld, int32_t n_series, double f0, double df, int64_t k0, int32_t n_freq,
                  int32_t float_mean, double* power_out, int64_t power_ld, double* freq_out, void* workspace,
                  void* stream);

/* ---- dynamical stability of states already in device memory ----------------------------------------
 * Which states of a posterior survive: n states integrated with the likelihood kernel's Wisdom-Holman
 * map over 10^4 .. 10^6 orbits, far beyond the observations' span, with the running extremes of each
 * planet's osculating Jacobi elements.  No plan: there is no observation schedule.  The conventions of the
 * summary entry points hold: device pointers, no allocation, no synchronisation, stream-ordered and
 * capturable, no floating-point atomics, the same bits from run to run; argument errors return < 0
 * before any HIP call and name the argument in rvm_last_error.
 *
 *   n >= 1 states, NP = n_planets (1 .. RVM_MAX_PLANETS), R = 5 NP, or 7 NP when inclined (0 or 1).
 *   params [R][n]     kernel rows, as rvm_logl_batch takes them; read by both calls, never written
 *   xv [6][NP][n]     Jacobi rx ry rz vx vy vz of each planet (rz = vz = 0 for planar states)
 *   ext [3][NP][n]    a_min, a_max, e2_max: the running extremes of the osculating Jacobi elements
 *   status int32 [n]  the state's status code
 *   steps int64 [n]   Wisdom-Holman steps completed when the state ended, or so far
 *   hill_factor >= 0, the same in both calls.  h > 0 and finite, sample_every >= 1, n_blocks >= 1; r_max <= 0
 *   (or NaN) turns the escape test off.  n_alive_out int64 [1], nullable.
 *
 * Elements of planet p from its Jacobi (r, v), GM the interior mass M_p of its coordinate (1 + m_1 + .. + m_p),
 * every operation one IEEE double operation, fma where written:
 *   r2 = fma(rz, rz, fma(ry, ry, rx rx));  |r| = sqrt(r2);  ir = 1 / |r|;
 *   v2 = fma(vz, vz, fma(vy, vy, vx vx));  beta = fma(2 GM, ir, -v2);  a = GM / beta;
 *   hx = fma(ry, vz, -(rz vy)), hy = fma(rz, vx, -(rx vz)), hz = fma(rx, vy, -(ry vx));
 *   h2 = fma(hz, hz, fma(hy, hy, hx hx));  e2 = fma(-(h2 beta), 1 / (GM GM), 1).
 * An unbound orbit is not a status: it shows as a_min <= 0 or e2_max >= 1.
 *
 * stability_init: the likelihood kernel's setup at t = 0 (prior, Pal -> heliocentric -> Jacobi, the Hill exit
 * distance and its check on every pair before the first step).  status = RVM_STATUS_PRIOR or
 * RVM_STATUS_ENCOUNTER exactly as that setup gives them, else RVM_STATUS_OK; xv = the state at t = 0;
 * a_min = a_max = a and e2_max = e2 of it; steps = 0.  A state that is not OK gets NaN in xv and ext.
 *
 * stability_advance: every state whose status is RVM_STATUS_OK runs n_blocks blocks; any other is not
 * written, bit for bit.  A block starts from xv alone -- |r| and 1 / |r| as above, the interaction evaluated
 * at those positions (with its pair test) -- and is sample_every steps of size h of the likelihood kernel's
 * map, K(h/2) [D K]^(sample_every - 1) D K(h/2), with the 8-term Stumpff series and the gated drift.  At its
 * end steps += sample_every, and in this order:
 *   1. a pair came within the exit distance at any kick of the block: RVM_STATUS_ENCOUNTER; xv, ext stay as
 *      at the previous block end;
 *   2. |r|, a or e2 of some planet is not finite: RVM_STATUS_NONFINITE; xv, ext stay likewise;
 *   3. a_min = fmin(a_min, a), a_max = fmax(a_max, a), e2_max = fmax(e2_max, e2); xv = the state;
 *   4. |r| > r_max for some planet: RVM_STATUS_ESCAPE.
 * A state that has ended runs no further block.  Since a block starts from xv alone and the lane constants
 * are rebuilt from params as stability_init built them, the result does not depend on how the blocks are
 * split over calls: n_blocks = a + b equals n_blocks = a, then b, bit for bit; nor on the state's column or
 * its neighbours.  n_alive_out receives the number of states still RVM_STATUS_OK (a second launch, an
 * integer count). */
int rvm_stability_init(int32_t n_planets, int32_t inclined, int32_t n, const double* params, double hill_factor,
                       double* xv, double* ext, int32_t* status, int64_t* steps, void* stream);
int rvm_stability_advance(int32_t n_planets, int32_t inclined, int32_t n, const double* params, double hill_factor,
                          double h, int32_t sample_every, int32_t n_blocks, double r_max, double* xv, double* ext,
                          int32_t* status, int64_t* steps, int64_t* n_alive_out, void* stream);

const char* rvm_last_error(void);
int rvm_abi_version(void);

#ifdef __cplusplus
}
#endif

#endif /* RVMCMC_H */
