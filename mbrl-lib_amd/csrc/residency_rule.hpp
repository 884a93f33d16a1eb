// residency_rule.hpp -- how many workgroups of a kernel instance one persistent launch may hold, as a pure rule: no HIP in here, the
// co-residency self-test comes in as a callable (residency.hpp runs it on the GPU, tests/residency/rule_harness.cpp stages its outcomes).
#pragma once
#include <algorithm>

namespace hipets {

struct Occ {  // what is known about ONE instance's residency on one device at one dynamic LDS size
    int blocks = 0, api = 0, n_cu = 0;  // workgroups per CU: the estimate in use (1..2), the runtime's own answer (1..2); CUs of the device
    int validated = 0;                  // largest grid whose co-residency the self-test has confirmed
};

// The resident capacity for a call that wants `want` workgroups (0: none -- launch per step).  Candidates, largest first: the estimate,
// the runtime's own answer, one workgroup per CU, each clamped to wg_cap (HIPETS_MAX_WORKGROUPS; 0 = none); the first whose grid (cut to
// `want`) is validated already or passes self_test(grid) wins.  A candidate that is not smaller than its predecessor is skipped, and so
// is a grid that has just failed: a smaller capacity with the same launch size cannot pass.
template <class SelfTest>
int resident_capacity_rule(Occ& oc, const int want, const int wg_cap, SelfTest&& self_test) {
    auto capped = [&](const int c) { return wg_cap ? std::min(c, wg_cap) : c; };
    const int cands[3] = {capped(oc.blocks * oc.n_cu), capped(oc.api * oc.n_cu), capped(oc.n_cu)};
    int cap = 0, failed_g = -1;
    for (int i = 0; i < 3 && cap == 0; ++i) {
        if (i > 0 && cands[i] >= cands[i - 1]) continue;
        const int g = std::min(want, cands[i]);
        if (g == failed_g) continue;
        if (g <= oc.validated || self_test(g)) oc.validated = std::max(oc.validated, g), cap = cands[i];
        else failed_g = g;
    }
    if (cap > 0 && !wg_cap) oc.blocks = cap / oc.n_cu;  // (a capped answer says nothing about the chip)
    return cap;
}

// Given a capacity > 0: does the persistent form pay?  Turns pay off when a CU holds ONE workgroup of this instance (cfg4: 4.51 -> 4.11 ms
// per rollout, cfg4' 16.4 -> 15.0).  Where two are resident, one launch per step lets the hardware deal 1 250 workgroups to 512 slots as
// they free up; fixed turns (3 for some workgroups, 2 for the rest) measured slower there (cfg5: 7.3 vs 6.6 ms).
inline bool persistent_pays(const int logical, const int capacity, const int n_cu) { return logical <= capacity || capacity <= n_cu; }

// The resident-heads instance of a lean fp32 shape (kspec.hpp KSpec::RES) keeps a wave's op heads in registers for the whole launch: right
// only where a launched workgroup serves ONE logical workgroup -- one member -- from the first step to the last.  Asked for
// (resident_heads_wanted) by a DEVICE rollout of `logical` workgroups of R row tiles when the instance exists -- R = 3: one wave per
// SIMD with the whole register file (the R = 4 instance, 13 MFMA units per wave, did not fit the heads next to its accumulators: 40 bytes
// of scratch per lane in the build's report, so it is not instantiated); a model of kResHeadOps ops -- and the call can be one persistent launch with at most one workgroup per CU; kept
// (resident_heads_kept) only if the capacity query then finds all of them co-resident: no turns, no per-step launches.
constexpr int kResHeadOps = 5;
inline bool resident_heads_wanted(const int R, const int n_layers, const int logical, const int n_cu, const int horizon) {
    return R == 3 && n_layers == kResHeadOps && logical >= 1 && logical <= n_cu && horizon > 1;
}
inline bool resident_heads_kept(const bool persistent, const int capacity, const int logical) { return persistent && capacity >= logical; }

}  // namespace hipets
