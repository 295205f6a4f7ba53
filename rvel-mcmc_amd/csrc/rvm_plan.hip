// rvm_plan.hip -- the plan's lifetime and accessors: rvm_plan_create builds the epoch schedule and the
// DevPlan on the host (rvm_plan_host.cpp), allocates and fills the device blocks, sets up the optional
// side-stream features and the kernels' attributes, once per observation set.
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>

#include "rvm_launch.h"
#include "rvm_plan.h"
#include "rvm_plan_host.h"

using rvm::Entry;
using rvm::fail;
using rvm::hip_fail;

namespace {

template <class T>
T* at(void* block, size_t offset) {
    return reinterpret_cast<T*>(reinterpret_cast<unsigned char*>(block) + offset);
}

// v into the host image of a block at `offset`; returns where it will sit in the device block
template <class T>
const T* put(std::vector<unsigned char>& host, void* block, size_t offset, const std::vector<T>& v) {
    if (!v.empty()) std::memcpy(host.data() + offset, v.data(), v.size() * sizeof(T));
    return at<T>(block, offset);
}

// hipMalloc + fill of an optional workspace; failing is not an error (the plan runs without the feature),
// so the block is released and the runtime's sticky status cleared
bool alloc_filled(void** mem, size_t bytes, int fill) {
    if (hipMalloc(mem, bytes) == hipSuccess && hipMemset(*mem, fill, bytes) == hipSuccess &&
        hipDeviceSynchronize() == hipSuccess)
        return true;
    (void)hipGetLastError();
    if (*mem) (void)hipFree(*mem);
    *mem = nullptr;
    return false;
}

// device layout: per direction [seg_n | obs_idx] int32 and [seg_len | obs_rv | obs_s2] f64, + workspace
int upload_schedule(rvm_plan* plan, const rvm::HostDir dir[2], int32_t max_walkers) {
    const rvm::DmemLayout L = rvm::dmem_layout(dir[0].idx.size(), dir[1].idx.size(), max_walkers);
    hipError_t e = hipMalloc(&plan->dmem, L.bytes);
    if (e != hipSuccess) return hip_fail(e, "rvm_plan_create: hipMalloc");
    std::vector<unsigned char> host(L.bytes, 0);
    rvm::DirSched* S[2] = {&plan->dev.fwd, &plan->dev.bwd};
    for (int dd = 0; dd < 2; dd++) {
        const rvm::HostDir& D = dir[dd];
        S[dd]->n_epochs = (int32_t)D.idx.size();
        S[dd]->n_steps = plan->steps[dd] = (int32_t)D.total_steps;
        S[dd]->split0 = D.split0;
        S[dd]->pre0 = D.pre0;
        S[dd]->split1 = D.split1;
        S[dd]->pre1 = D.pre1;
        S[dd]->seg_h1 = put(host, plan->dmem, L.seg_h1[dd], D.seg_len);
        S[dd]->obs_rv = put(host, plan->dmem, L.obs_rv[dd], D.orv);
        S[dd]->obs_s2 = put(host, plan->dmem, L.obs_s2[dd], D.os2);
        S[dd]->seg_n = put(host, plan->dmem, L.seg_n[dd], D.seg_n);
        S[dd]->obs_idx = put(host, plan->dmem, L.obs_idx[dd], D.idx);
    }
    plan->slots = at<unsigned long long>(plan->dmem, L.slots);
    for (int32_t i = 0; i < max_walkers; i++)  // empty between launches (the kernel restores this)
        at<unsigned long long>(host.data(), L.slots)[i] = 0x7FF4DEADBEEF0001ULL;
    plan->dev.counters = at<unsigned long long>(plan->dmem, L.counters);  // (zeroed)
    plan->max_walkers = max_walkers;
    e = hipMemcpy(plan->dmem, host.data(), L.bytes, hipMemcpyHostToDevice);
    return e == hipSuccess ? 0 : hip_fail(e, "rvm_plan_create: hipMemcpy");
}

int device_cus() {
    int dev = 0, ncu = 0;
    if (hipGetDevice(&dev) != hipSuccess ||
        hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess)
        ncu = 0;
    return ncu;
}

// level-split layout (rvm_logl.hip launch_logl).  Without the workspace launches keep the LDS-coupled layout.
void alloc_level_split(rvm_plan* plan, size_t nf, size_t nb, const rvm::PlanKnobs& K) {
    rvm::DevPlan& P = plan->dev;
    if (!rvm::plan_wants_level_split(P, plan->max_walkers, K)) return;
    const rvm::LvLayout L = rvm::lv_layout(nf, nb, plan->max_walkers);
    // every slot empty (all-ones: the NaN sentinel / -1); the combiners restore this
    if (!alloc_filled(&plan->lvmem, L.bytes, 0xFF)) return;
    P.lv_rv = at<double>(plan->lvmem, L.rv);
    P.lv_enc = at<int32_t>(plan->lvmem, L.enc);
    P.lv_emax = L.emax;
    P.lv_stride = plan->max_walkers;
    plan->lv_bytes = L.bytes;
}

// the extension's room for every launch's main-pass levels (a failed allocation is not an error: the
// plan refines by halving passes alone, ext_mult 0)
void alloc_extension(rvm_plan* plan, size_t nf, size_t nb, const rvm::PlanKnobs& K) {
    rvm::DevPlan& P = plan->dev;
    if (!rvm::plan_wants_extension(P, K)) return;
    const rvm::XLayout L = rvm::x_layout(nf, nb, plan->max_walkers, K.n_teams);
    if (L.bytes > RVM_EXT_MAX_BYTES) return;
    if (hipMalloc(&plan->xmem, L.bytes) != hipSuccess) {
        plan->xmem = nullptr;
        (void)hipGetLastError();  // (clear the runtime's sticky status)
        return;
    }
    rvm::fill_plan_extension(&P);
    P.lvx = at<double>(plan->xmem, L.lvx);
    P.rvp = at<double>(plan->xmem, L.rvp);
    P.rvp2 = K.n_teams >= 2 ? at<double>(plan->xmem, L.rvp2) : nullptr;
    P.lvx_emax = L.emax;
    P.lvx_stride = plan->max_walkers;
}

// the refinement kernel's work lists (rvm_refine.hip): sizes [4] (zero), walkers [3][max_walkers],
// settled directions' chi2 [2][max_walkers], the exchange words; adaptive plans only
int alloc_work_lists(rvm_plan* plan, const rvm::PlanKnobs& K) {
    rvm::DevPlan& P = plan->dev;
    if (P.rmax <= 0) return 0;
    const rvm::RqLayout L = rvm::rq_layout(plan->max_walkers, K.n_teams);
    if (hipMalloc(&plan->rqmem, L.bytes) != hipSuccess || hipMemset(plan->rqmem, 0, L.bytes) != hipSuccess ||
        hipDeviceSynchronize() != hipSuccess) {
        (void)hipGetLastError();
        return fail(-3, "rvm_plan_create: hipMalloc of the refinement work lists failed");
    }
    P.rq_x = K.refine_split ? at<unsigned long long>(plan->rqmem, L.x) : nullptr;
    P.rq_xf = at<unsigned long long>(plan->rqmem, L.xf);
    P.rq_t = K.n_teams >= 2 ? at<unsigned long long>(plan->rqmem, L.t) : nullptr;
    P.rq_tf = at<unsigned long long>(plan->rqmem, L.tf);
    P.rq_c = at<double>(plan->rqmem, L.c);
    P.rq_w = at<int32_t>(plan->rqmem, L.w);
    P.rq_n = at<int32_t>(plan->rqmem, L.n);
    P.gen_dev = at<unsigned long long>(plan->rqmem, L.gen);
    P.rq_mark = at<int32_t>(plan->rqmem, L.mark);  // (zeroed)
    P.depth_w = K.teams_hint ? at<unsigned long long>(plan->rqmem, L.depth) : nullptr;
    P.rq_cap = plan->max_walkers;
    P.rq_xgroups = L.xgroups;
    const unsigned long long gen1 = 1;  // (every flag word starts at generation 0, older than any launch)
    if (hipMemcpy(P.gen_dev, &gen1, sizeof(gen1), hipMemcpyHostToDevice) != hipSuccess) {
        (void)hipGetLastError();
        return fail(-3, "rvm_plan_create: initialising the launch generation failed");
    }
    return 0;
}

// The side stream and its fork / join events, shared by the eager passes and the hedge.  Without them
// the plan runs neither: hedge_groups 0, side null.
void side_drop(rvm_plan* plan) {
    (void)hipGetLastError();
    if (plan->ev_fork) (void)hipEventDestroy(plan->ev_fork);
    if (plan->ev_join) (void)hipEventDestroy(plan->ev_join);
    if (plan->side) (void)hipStreamDestroy(plan->side);
    plan->side = nullptr;
    plan->ev_fork = plan->ev_join = nullptr;
    plan->dev.hedge_groups = 0;
}

bool side_create(rvm_plan* plan) {
    if (hipStreamCreateWithFlags(&plan->side, hipStreamNonBlocking) == hipSuccess &&
        hipEventCreateWithFlags(&plan->ev_fork, hipEventDisableTiming) == hipSuccess &&
        hipEventCreateWithFlags(&plan->ev_join, hipEventDisableTiming) == hipSuccess)
        return true;
    side_drop(plan);
    return false;
}

// Eager halving passes for the plan's plain launches of RVM_EAGER_MIN..RVM_EAGER_MAX walkers
// (SMALA's centres, batched State evaluations): results of passes 1 and 2, a side stream and two
// events -- only for plans that can make such a launch (a one-walker scalar plan never does, and
// its stream would only add to the hardware queues).  Any failure: no eager passes,
// the refinement kernel integrates as usual.
// Hedged pass 2 of fused stretch launches (rvm_refine_impl.h hedge_kernel) shares the side stream and
// the events: RVM_HEDGE=0 turns it off, RVM_HEDGE_GROUPS caps its groups (1 .. RVM_HEDGE_GROUPS_MAX;
// INTEGRATION.md).
void setup_side_features(rvm_plan* plan, const rvm::PlanKnobs& K) {
    rvm::DevPlan& P = plan->dev;
    const int32_t mw = plan->max_walkers;
    const bool refines = P.rmax >= 2 && P.rvp != nullptr && P.gen_dev != nullptr && P.n_levels <= 4 &&
                         mw >= rvm::RVM_EAGER_MIN;
    if (K.hedge_groups > 0 && refines && P.n_cu >= 4) {
        const rvm::HLayout L = rvm::h_layout(P.lvx_emax, mw);
        if (alloc_filled(&plan->hmem, L.bytes, 0)) {
            P.hrv = at<double>(plan->hmem, L.hrv);
            P.hsum = at<double>(plan->hmem, L.hsum);
            P.hslot = at<unsigned long long>(plan->hmem, L.hslot);
            P.htab = at<unsigned long long>(plan->hmem, L.htab);
            P.hw = at<unsigned long long>(plan->hmem, L.hw);
            P.hedge_groups = K.hedge_groups;
            P.hedge_mark = K.hedge_mark;
            P.hedge_wait = K.hedge_wait;
        }
    }
    if (!(refines && K.eager)) {
        // (no eager passes on this plan: the side stream and events for the hedge alone)
        if (P.hedge_groups > 0) (void)side_create(plan);
        return;
    }
    const rvm::ELayout L = rvm::e_layout(P.lvx_emax, P.lvx_stride);
    if (alloc_filled(&plan->emem, L.bytes, 0) && side_create(plan)) {
        P.rve = at<double>(plan->emem, L.rve);
        P.esum = at<double>(plan->emem, L.esum);
        P.eflag = at<unsigned long long>(plan->emem, L.eflag);
        P.eager_max = std::min<int>(mw, rvm::RVM_EAGER_MAX);
        P.eager_passes = K.eager_passes;
    } else {
        side_drop(plan);  // (no side stream: no hedge either)
        if (plan->emem) (void)hipFree(plan->emem);
        plan->emem = nullptr;
    }
}

// kernel attributes (dynamic LDS) set once here, so launches stay capturable; a schedule the
// refinement kernel cannot stage is refused now rather than failing every launch
int prepare_kernels(const rvm::DevPlan& P) {
    const hipError_t pe = rvm::prepare_logl(P);
    if (pe != hipSuccess)
        return fail(-1, pe == hipErrorInvalidConfiguration
                            ? "rvm_plan_create: the epoch schedule does not fit the likelihood kernel's LDS "
                              "(too many epochs in one direction)"
                            : "rvm_plan_create: n_planets has no kernel instantiation");
    if (rvm::prepare_refine(P) != hipSuccess)
        return fail(-1, "rvm_plan_create: the epoch schedule does not fit the refinement kernel's LDS "
                        "(too many epochs in one direction for the adaptive resolution)");
    return 0;
}

// The words of DevPlan::hw from word `first` on into the non-null pointers of `out` (zeros on a plan without
// a hedge), zeroed after the read on request.  Nothing is written when the read fails.
template <int N>
int read_hw_words(const Entry& at, rvm_plan* plan, int first, int32_t reset, void* stream, int64_t* const (&out)[N]) {
    if (!plan) return at.null("plan");
    unsigned long long h[N] = {};
    if (plan->dev.hw != nullptr) {
        hipStream_t st = (hipStream_t)stream;
        unsigned long long* d = plan->dev.hw + first;
        hipError_t e = hipMemcpyAsync(h, d, sizeof(h), hipMemcpyDeviceToHost, st);
        if (e == hipSuccess && reset) e = hipMemsetAsync(d, 0, sizeof(h), st);
        if (e == hipSuccess) e = hipStreamSynchronize(st);
        if (e != hipSuccess) return at.done(e);
    }
    for (int i = 0; i < N; i++)
        if (out[i]) *out[i] = (int64_t)h[i];
    return 0;
}

}  // namespace

extern "C" {

int rvm_plan_create(const rvm_config* cfg, const double* t, const double* rv, const double* sigma, int32_t n_obs,
                    int32_t max_walkers, rvm_plan** out) {
    if (!cfg || !t || !rv || !sigma || !out) return fail(-1, "rvm_plan_create: null argument");
    int mult[RVM_MAX_LEVELS], max_mult = 1;
    if (const char* m = rvm::check_plan_config(cfg, t, rv, sigma, n_obs, max_walkers, mult, &max_mult))
        return fail(-1, m);
    rvm::HostDir dir[2];
    if (const char* m = rvm::build_schedule(cfg, mult, max_mult, t, rv, sigma, n_obs, dir)) return fail(-1, m);
    const size_t nf = dir[0].idx.size(), nb = dir[1].idx.size();
    const rvm::PlanKnobs K = rvm::read_plan_knobs();
    rvm_plan* plan = new rvm_plan();  // (value-initialised: every DevPlan field starts at zero / null)
    int rc = upload_schedule(plan, dir, max_walkers);
    if (rc == 0) {
        rvm::fill_plan_scalars(cfg, mult, n_obs, nf, nb, device_cus(), K, &plan->dev);
        alloc_level_split(plan, nf, nb, K);
        alloc_extension(plan, nf, nb, K);
        rc = alloc_work_lists(plan, K);
    }
    if (rc == 0) {
        setup_side_features(plan, K);
        rc = prepare_kernels(plan->dev);
    }
    if (rc != 0) {
        rvm_plan_destroy(plan);  // (tolerates a partly built plan)
        return rc;
    }
    *out = plan;
    return 0;
}

void rvm_plan_destroy(rvm_plan* plan) {
    if (!plan) return;
    if (plan->side) (void)hipStreamSynchronize(plan->side);
    if (plan->ev_fork) (void)hipEventDestroy(plan->ev_fork);
    if (plan->ev_join) (void)hipEventDestroy(plan->ev_join);
    if (plan->side) (void)hipStreamDestroy(plan->side);
    if (plan->emem) (void)hipFree(plan->emem);
    if (plan->hmem) (void)hipFree(plan->hmem);
    for (hipEvent_t ev : plan->tev) (void)hipEventDestroy(ev);
    if (plan->rqmem) (void)hipFree(plan->rqmem);
    if (plan->lvmem) (void)hipFree(plan->lvmem);
    if (plan->xmem) (void)hipFree(plan->xmem);
    if (plan->dmem) (void)hipFree(plan->dmem);
    delete plan;
}

int rvm_plan_set_certain_reject(rvm_plan* plan, int32_t on) {
    if (!plan) return Entry{"rvm_plan_set_certain_reject"}.null("plan");
    plan->dev.cut = on ? 1 : 0;
    return 0;
}

int rvm_plan_set_verify_eccentricity(rvm_plan* plan, double e) {
    const Entry at{"rvm_plan_set_verify_eccentricity"};
    if (!plan) return at.null("plan");
    if (std::isnan(e) || e >= 1.0) return at.bad("e must be < 1 (<= 0: off)");
    plan->dev.e2_guard = e > 0.0 ? e * e : INFINITY;
    {
        const char* cf = getenv("RVM_CUT_FACTOR");  // (A/B knob: the guard's factor)
        const double ec = 1.0 - (1.0 - e) * (cf ? atof(cf) : rvm::RVM_CUT_ECC_FACTOR);
        const char* cg = getenv("RVM_CUT_GUARD");  // (A/B knob: 0 turns the cut guard off)
        plan->dev.e2_cut = e > 0.0 && !(cg && atoi(cg) == 0) ? ec * ec : INFINITY;
        const char* ck = getenv("RVM_CUT_GUARD_K");  // (A/B knob: past the guard, chi2 - min(k d, 100 est))
        plan->dev.cut_guard_k = ck ? atof(ck) : rvm::RVM_CUT_GUARD_K;
    }
    return 0;
}

int rvm_plan_extension(const rvm_plan* plan, int32_t* ext_mult) {
    if (!plan) return Entry{"rvm_plan_extension"}.null("plan");
    if (ext_mult) *ext_mult = plan->dev.ext_mult;
    return 0;
}

int rvm_plan_counters(rvm_plan* plan, int32_t reset, int64_t* out, int32_t n, void* stream) {
    const Entry at{"rvm_plan_counters"};
    if (!plan) return at.null("plan");
    if (n < 0 || (n > 0 && !out)) return at.bad("bad output array");
    hipStream_t st = (hipStream_t)stream;
    unsigned long long h[RVM_N_COUNTERS] = {};
    hipError_t e = hipMemcpyAsync(h, plan->dev.counters, sizeof(h), hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) return at.done(e);
    for (int i = 0; i < n; i++) out[i] = i < RVM_N_COUNTERS ? (int64_t)h[i] : 0;
    if (reset) {
        // the hand-off slots back to their sentinels (late level-1 stores of a launch that gave up
        // have landed: the stream's earlier work is complete), then the counters
        if (plan->lvmem) e = hipMemsetAsync(plan->lvmem, 0xFF, plan->lv_bytes, st);
        if (e == hipSuccess) e = hipMemsetAsync(plan->dev.counters, 0, sizeof(h), st);
        if (e == hipSuccess) e = hipStreamSynchronize(st);
        if (e != hipSuccess) return hip_fail(e, "rvm_plan_counters: reset");
    }
    return 0;
}

int rvm_plan_hedge_stats(rvm_plan* plan, int32_t reset, int64_t* hedged, int64_t* replayed, int64_t* missed,
                         void* stream) {
    int64_t* const out[] = {hedged, replayed, missed};
    return read_hw_words({"rvm_plan_hedge_stats"}, plan, rvm::RVM_HW_STATS, reset, stream, out);
}

int rvm_plan_hedge_marks(rvm_plan* plan, int32_t reset, int64_t* marked, int64_t* gave_up, void* stream) {
    int64_t* const out[] = {marked, gave_up};
    return read_hw_words({"rvm_plan_hedge_marks"}, plan, rvm::RVM_HW_STATS + 3, reset, stream, out);
}

int rvm_plan_hedge_waits(rvm_plan* plan, int32_t reset, int64_t* waited, int64_t* late_hits, int64_t* gave_way,
                         void* stream) {
    int64_t* const out[] = {waited, late_hits, gave_way};
    return read_hw_words({"rvm_plan_hedge_waits"}, plan, rvm::RVM_HW_WAIT, reset, stream, out);
}

int rvm_plan_faults(rvm_plan* plan, int32_t reset, int64_t* handoff_timeouts, int64_t* nonfinite,
                    int64_t* unresolved, int64_t* refined, int64_t* truncated, void* stream) {
    if (!plan) return Entry{"rvm_plan_faults"}.null("plan");
    int64_t c[RVM_N_COUNTERS] = {};
    const int rc = rvm_plan_counters(plan, reset, c, RVM_N_COUNTERS, stream);
    if (rc != 0) return rc;
    if (handoff_timeouts) *handoff_timeouts = c[0];
    if (nonfinite) *nonfinite = c[1];
    if (unresolved) *unresolved = c[2];
    if (refined) *refined = c[3];
    if (truncated) *truncated = c[4];
    return 0;
}

int rvm_plan_time_kernels(rvm_plan* plan, int32_t max_launches) {
    const Entry at{"rvm_plan_time_kernels"};
    if (!plan) return at.null("plan");
    if (max_launches < 0 || max_launches > 4096) return at.bad("max_launches out of range");
    while ((int32_t)plan->tev.size() < 3 * max_launches) {
        hipEvent_t ev;
        const hipError_t e = hipEventCreate(&ev);
        if (e != hipSuccess) return hip_fail(e, "rvm_plan_time_kernels: hipEventCreate");
        plan->tev.push_back(ev);
    }
    plan->tcap = max_launches;
    plan->tn = 0;
    return 0;
}

int rvm_plan_kernel_times(rvm_plan* plan, float* logl_ms, float* refine_ms, int32_t max, int32_t* n_out) {
    const Entry at{"rvm_plan_kernel_times"};
    if (!plan || max < 0) return at.bad("bad arguments");
    const int n = std::min(plan->tn, max);
    for (int i = 0; i < n; i++) {
        hipError_t e = hipEventSynchronize(plan->tev[3 * i + 2]);
        float a = 0.0f, b = 0.0f;
        if (e == hipSuccess) e = hipEventElapsedTime(&a, plan->tev[3 * i], plan->tev[3 * i + 1]);
        if (e == hipSuccess) e = hipEventElapsedTime(&b, plan->tev[3 * i + 1], plan->tev[3 * i + 2]);
        if (e != hipSuccess) return at.done(e);
        if (logl_ms) logl_ms[i] = a;
        if (refine_ms) refine_ms[i] = b;
    }
    if (n_out) *n_out = n;
    plan->tn = 0;
    plan->tcap = 0;
    return 0;
}

int rvm_plan_set_handoff_timeout(rvm_plan* plan, double seconds) {
    const Entry at{"rvm_plan_set_handoff_timeout"};
    if (!plan) return at.null("plan");
    if (!(seconds > 0.0) || !(seconds < 1e9)) return at.bad("seconds out of range");
    const double ticks = seconds * 1e8;  // 100 MHz real-time counter
    plan->dev.spin_ticks = ticks < 1.0 ? 1ull : (unsigned long long)ticks;
    plan->dev.hedge_wait_ticks = rvm::hedge_wait_bound(plan->dev.spin_ticks);
    return 0;
}

int rvm_plan_info(const rvm_plan* plan, int32_t* sf, int32_t* sb, int32_t* ef, int32_t* eb) {
    if (!plan) return Entry{"rvm_plan_info"}.null("plan");
    if (sf) *sf = plan->steps[0];
    if (sb) *sb = plan->steps[1];
    if (ef) *ef = plan->dev.fwd.n_epochs;
    if (eb) *eb = plan->dev.bwd.n_epochs;
    return 0;
}

}  // extern "C"
