// rvm_plan.h -- the plan object behind the ABI's opaque rvm_plan (built and owned by rvm_plan.hip, launched
// from by rvm_abi.hip run_logl), and the error reporting both files share.
#pragma once
#include <hip/hip_runtime.h>

#include <string>
#include <vector>

#include "rvm_internal.h"

struct rvm_plan {
    rvm::DevPlan dev;
    void* dmem = nullptr;        // one device allocation: schedule + workspace
    void* lvmem = nullptr;       // level-split layout workspace (DevPlan::lv_*), when usable
    size_t lv_bytes = 0;
    void* xmem = nullptr;        // the extension's stored levels (DevPlan::lvx), when the plan has one
    void* rqmem = nullptr;       // the refinement kernel's work lists (DevPlan::rq_*), adaptive plans
    unsigned long long* slots = nullptr;  // [max_walkers] direction meeting slots (rvm_logl.hip)
    int32_t max_walkers = 0;
    int32_t steps[2] = {0, 0};
    // rvm_plan_time_kernels: event triples around the likelihood and refinement kernels of the next
    // `cap` launches (the kernels' own durations on their stream, for the bench's roofline)
    mutable std::vector<hipEvent_t> tev;
    mutable int32_t tcap = 0, tn = 0;
    void* emem = nullptr;                // eager passes' results (DevPlan::rve, esum), small plans
    void* hmem = nullptr;                // hedged pass 2's results and words (DevPlan::hrv ... hw)
    hipStream_t side = nullptr;          // their stream, forked from and joined to the caller's
    hipEvent_t ev_fork = nullptr, ev_join = nullptr;
};

namespace rvm {
// set rvm_last_error's message for this thread and return `code` (rvm_abi.hip)
int fail(int code, const std::string& msg);
int hip_fail(hipError_t e, const char* where);  // code -3, "<where>: <the runtime's message>"

// An entry point's name, said once: its refusals (code -1, "<name>: <text>") and its HIP tail report
// under it.  Nothing here builds a string unless the call fails.
struct Entry {
    const char* name;
    int bad(const char* text) const { return fail(-1, std::string(name) + ": " + text); }
    int null(const char* arg) const { return fail(-1, std::string(name) + ": null " + arg); }
    int done(hipError_t e) const { return e == hipSuccess ? 0 : hip_fail(e, name); }
};
}  // namespace rvm
