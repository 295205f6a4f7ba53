// Host-side sanitizer driver for librvmcmc's C ABI (not part of the library): every entry point's
// argument checks, and rvm_plan_create's host work (epoch split, sort, segment schedule, weights)
// on valid inputs -- the first HIP call then fails on a GPU-less host, which is an error return.
// Built with AddressSanitizer + UBSan on the host side only (`make sanitize-host`), run by
// tests/test_sanitizers.py.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../include/rvmcmc.h"

int main() {
    int fails = 0;
    auto expect = [&](bool ok, const char* what) {
        if (!ok) {
            std::fprintf(stderr, "FAIL %s\n", what);
            fails++;
        }
    };
    expect(rvm_abi_version() == RVM_ABI_VERSION, "abi version");
    rvm_config cfg{};
    cfg.n_planets = 2;
    cfg.dt = 0.65;
    cfg.n_levels = 4;
    cfg.npoints_norm = 100.0;
    const int mult[4] = {4, 5, 6, 7};
    std::memcpy(cfg.level_mult, mult, sizeof(mult));
    cfg.period_hint = 5.2;
    std::vector<double> t, rv, sg;
    for (int i = 0; i < 101; i++) {  // both directions, unsorted, a duplicate epoch
        t.push_back(i % 2 ? -0.6 * i : 0.55 * (100 - i));
        rv.push_back(1e-4 * std::sin(i));
        sg.push_back(1.5e-4);
    }
    t[7] = t[9];
    rvm_plan* plan = nullptr;
    const int rc = rvm_plan_create(&cfg, t.data(), rv.data(), sg.data(), (int)t.size(), 4096, &plan);
    expect(rc == 0 || (rc < 0 && plan == nullptr), "plan_create valid input");
    if (rc == 0) rvm_plan_destroy(plan);
    rvm_config bad = cfg;
    bad.n_levels = 0;
    expect(rvm_plan_create(&bad, t.data(), rv.data(), sg.data(), (int)t.size(), 64, &plan) < 0, "n_levels 0");
    bad = cfg;
    bad.level_mult[1] = 4;
    expect(rvm_plan_create(&bad, t.data(), rv.data(), sg.data(), (int)t.size(), 64, &plan) < 0, "dup multipliers");
    bad = cfg;
    bad.dt = -1.0;
    expect(rvm_plan_create(&bad, t.data(), rv.data(), sg.data(), (int)t.size(), 64, &plan) < 0, "negative dt");
    std::vector<double> tn = t;
    tn[3] = NAN;
    expect(rvm_plan_create(&cfg, tn.data(), rv.data(), sg.data(), (int)t.size(), 64, &plan) < 0, "nan epoch");
    expect(std::strlen(rvm_last_error()) > 0, "last_error");
    expect(rvm_logl_batch(nullptr, 1, nullptr, 1.0, nullptr, nullptr, nullptr, nullptr) < 0, "logl null plan");
    int64_t mk = -1, gu = -1;
    expect(rvm_plan_hedge_marks(nullptr, 0, &mk, &gu, nullptr) < 0 && mk == -1 && gu == -1, "hedge_marks null plan");
    rvm_param_map pm{};
    expect(rvm_stretch_half_step(nullptr, &pm, 10, 1, 0, nullptr, nullptr, nullptr, 1, nullptr, 2.0, 0, 0, 0, 1.0,
                                 nullptr, nullptr, nullptr, nullptr) < 0,
           "half_step null plan");
    expect(rvm_stretch_propose(0, 1, 0, nullptr, 1, nullptr, 2.0, 0, 0, 0, nullptr, nullptr, nullptr, nullptr) < 0,
           "propose bad");
    // parallel tempering: every refusal comes before any HIP call (the int32 bound in 64-bit arithmetic)
    double d1 = 0.5;
    int32_t i1 = 0;
    expect(rvm_pt_stretch_propose(10, 0, 1, &d1, &d1, 2.0, 0, 0, 0, nullptr, &d1, &d1, nullptr) < 0, "pt n_temps 0");
    expect(rvm_pt_stretch_propose(10, 2, 1, &d1, &d1, 1.0, 0, 0, 0, nullptr, &d1, &d1, nullptr) < 0, "pt a = 1");
    expect(rvm_pt_stretch_propose(10, 1 << 16, 1 << 16, &d1, &d1, 2.0, 0, 0, 0, nullptr, &d1, &d1, nullptr) < 0,
           "pt int32 overflow");
    expect(rvm_pt_stretch_accept(10, 2, 1, nullptr, &d1, &d1, &d1, &d1, &d1, 0, 0, 0, nullptr, &i1, nullptr) < 0,
           "pt null betas");
    expect(rvm_pt_stretch_accept(10, 2, 1, &d1, &d1, &d1, &d1, &d1, &d1, 0, 0, 2, nullptr, &i1, nullptr) < 0,
           "pt half 2");
    expect(rvm_pt_swap(10, 2, 0, &d1, &d1, &d1, &d1, &d1, 0, 0, nullptr, &i1, nullptr) < 0, "pt n_half 0");
    expect(rvm_pt_swap(10, 1 << 15, 1 << 15, &d1, &d1, &d1, &d1, &d1, 0, 0, nullptr, &i1, nullptr) < 0,
           "pt swap int32 overflow");
    expect(rvm_pt_swap(10, 1, 4, nullptr, nullptr, nullptr, nullptr, nullptr, 0, 0, nullptr, nullptr, nullptr) == 0,
           "pt swap of one temperature");
    int64_t l1 = 0;
    expect(rvm_pt_ladder_update(3, 1, &i1, &d1, &d1, -1.0, &d1, &l1, &d1, &l1, nullptr, &d1, nullptr) < 0,
           "pt ladder kappa < 0");
    expect(rvm_pt_ladder_update(3, 1, &i1, &d1, &d1, 0.5, &d1, &l1, &d1, &l1, nullptr, nullptr, nullptr) < 0,
           "pt ladder null workspace");
    expect(rvm_pt_ladder_update(1 << 16, 1 << 15, &i1, &d1, &d1, 0.5, &d1, &l1, &d1, &l1, nullptr, &d1, nullptr) < 0,
           "pt ladder int32 overflow");
    expect(rvm_pt_ladder_update(1, 4, nullptr, nullptr, nullptr, 0.5, nullptr, nullptr, nullptr, nullptr, nullptr,
                                nullptr, nullptr) == 0,
           "pt ladder of one temperature");
    // the recorded chain: refusals before any HIP call, the column and lag bounds in 64-bit arithmetic
    expect(rvm_chain_record(2, 4, &d1, 16, 0, INT64_MAX, &d1, 8, 0, nullptr, nullptr, nullptr) < 0,
           "chain record stride overflow");
    expect(rvm_chain_record(2, 4, &d1, 16, 0, 1, &d1, INT64_MAX, INT64_MAX - 1, nullptr, nullptr, nullptr) < 0,
           "chain record dst_col0 overflow");
    expect(rvm_chain_record(2, 4, &d1, 16, 0, 1, &d1, 8, 0, &d1, nullptr, nullptr) < 0, "chain record lone lnp_src");
    expect(rvm_chain_moments(&d1, 2, 4, 5, 5, &d1, &d1, nullptr) < 0, "chain moments empty range");
    expect(rvm_chain_autocov(&d1, &d1, 2, 4, 0, 10, INT32_MAX, 1 << 30, &d1, &d1, nullptr) < 0,
           "chain autocov lag overflow");
    expect(rvm_chain_autocov(&d1, &d1, 65534, 4, 0, INT64_MAX, 0, 1 << 30, &d1, &d1, nullptr) < 0,
           "chain autocov n_params * n_lags");
    expect(rvm_chain_autocov_workspace_bytes(10, 200, 17) == (size_t)8 * 10 * 32, "chain autocov workspace");
    expect(rvm_chain_autocov_workspace_bytes(1, 65535 * 256, 1 << 30) == (size_t)8 * ((size_t)1 << 30) * 65535,
           "chain autocov workspace, largest");
    expect(rvm_chain_autocov_workspace_bytes(65534, 4, 1 << 30) == 0, "chain autocov workspace, refused");
    expect(rvm_mh_accept(0, 1, 0, nullptr, nullptr, nullptr, nullptr, 0, 0, nullptr, nullptr, nullptr) < 0, "mh bad");
    expect(rvm_fd_params(10, 1, nullptr, 1e-6, nullptr, nullptr, nullptr) < 0, "fd bad");
    const int32_t rows[2] = {0, 0};
    expect(rvm_logl_derivs(nullptr, 1, nullptr, 2, rows, 1.0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) < 0,
           "derivs null plan");
    expect(rvm_logl_derivs_workspace_bytes(256, 10) == (size_t)256 * 55 * 2 * 36, "derivs workspace");
    rvm_smala_cache c{};
    expect(rvm_smala_metric(10, 1, nullptr, nullptr, nullptr, nullptr, nullptr, 1.0, 0.5, &c, nullptr) < 0, "metric bad");
    std::printf("host sanitize driver: %d failures\n", fails);
    return fails;
}
