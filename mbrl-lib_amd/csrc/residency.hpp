// residency.hpp -- host only (rollout.hip): the ONE launcher of every rollout kernel instance and everything that decides whether the
// persistent DEVICE form is safe to run: occupancy estimate, co-residency self-test, table of validated grids, capacity query, choice of
// launch form.  It works on a KernelRec (launch.hpp): hipLaunchKernel takes the kernel's host address, so nothing here is a template
// over the instance.
#pragma once
#include <hip/hip_ext.h>

#include <cstdio>
#include <cstdlib>
#include <iterator>
#include <map>
#include <mutex>
#include <utility>

#include "launch.hpp"
#include "residency_rule.hpp"

namespace hipets {

// start / stop (both or neither) ride on the dispatch packet itself (start / end timestamps of THIS kernel): no extra barrier packets
inline hipError_t enqueue_rollout(const KernelRec& k, int grid, unsigned lds, const ModelDev& md, const RolloutArgs& ra, hipStream_t st, hipEvent_t start, hipEvent_t stop) {
    void* args[2] = {const_cast<ModelDev*>(&md), const_cast<RolloutArgs*>(&ra)};
    if (start) (void)hipExtLaunchKernel(k.fn, dim3(grid), dim3(kThreads), args, lds, st, start, stop, 0);
    else (void)hipLaunchKernel(k.fn, dim3(grid), dim3(kThreads), args, lds, st);
    return hipGetLastError();
}

// HIPETS_MAX_WORKGROUPS=n (tests: several processes sharing one GPU, each leaving room for the others' persistent grids; also a way to
// keep CUs free for another stream): a persistent launch never holds more than n workgroups -- the rest of the batch is served in turns,
// exactly as when the chip itself is the limit.  0: no cap.
inline int max_workgroups() {
    static const int wg_cap = [] { const char* v = std::getenv("HIPETS_MAX_WORKGROUPS"); const int n = v ? std::atoi(v) : 0; return n > 0 ? n : 0; }();
    return wg_cap;
}

// Run f(Occ&) on what is known about k's residency at this dynamic LDS size on the current device, under that device's lock.  One lock
// and one table PER DEVICE: the self-test synchronises a stream, and engines on other devices driven from other host threads must not
// queue behind it; engines on ONE device planning from two host threads serialise here instead of racing between the capacity query and
// the launch that relies on it.  Entries are per (kernel, LDS size): two models / horizons with different LDS sizes keep their own
// (alternating between them costs no new self-test).  Bounded, 32 entries per kernel: a process that walks through many horizons / models
// forgets that kernel's knowledge and re-validates, one launch + one synchronisation.
struct DeviceResidency {
    std::mutex mu;
    std::map<std::pair<const void*, unsigned>, Occ> table;
};
constexpr int kDevSlots = 64, kMaxEntries = 32;
inline DeviceResidency& device_residency(const int dev) {
    static DeviceResidency devices[kDevSlots];  // (ONE set for the process: not inside the template below, which is instantiated per callable)
    return devices[dev >= 0 && dev < kDevSlots ? dev : kDevSlots - 1];
}
template <class F>
hipError_t with_residency(const KernelRec& k, const unsigned lds, const int lds_max, F&& f) {
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    DeviceResidency& d = device_residency(dev);
    std::lock_guard<std::mutex> lock(d.mu);
    auto& table = d.table;
    if (dev >= kDevSlots) table.clear();  // (devices beyond the table share the last slot: never trust another device's entry)
    const auto first = table.lower_bound({k.fn, 0u}), last = table.upper_bound({k.fn, ~0u});
    if (std::distance(first, last) >= kMaxEntries && !table.count({k.fn, lds})) table.erase(first, last);
    Occ& oc = table[{k.fn, lds}];
    if (oc.blocks == 0) {
        int nb = 0;
        hipFuncAttributes fa{};
        if ((e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, k.fn, kThreads, lds)) != hipSuccess) return e;
        if ((e = hipDeviceGetAttribute(&oc.n_cu, hipDeviceAttributeMultiprocessorCount, dev)) != hipSuccess) return e;
        if ((e = hipFuncGetAttributes(&fa, k.fn)) != hipSuccess) return e;
        // the occupancy query prices dynamic LDS against the default 64 KB window, not the 160 KB this kernel opted in to: take the
        // larger of its answer and the count that follows from the register file (512 per lane and SIMD, one wave of every workgroup
        // per SIMD) and the 160 KB of LDS (with a 2 KB margin per workgroup for allocation granularity).  Both are ESTIMATES (no
        // scratch, SGPR or CU-mask terms): the co-residency self-test is what is trusted.
        const int regs = std::max(fa.numRegs, 1);
        const int by_regs = 512 / (((regs + 7) / 8) * 8);
        const int by_lds = (int)((size_t)lds_max / ((size_t)lds + (size_t)fa.sharedSizeBytes + 2048));
        if (std::getenv("HIPETS_DEBUG_OCC")) std::fprintf(stderr, "[hipets] occupancy query %d, regs %d -> %d, lds %u -> %d\n", nb, regs, by_regs, lds, by_lds);
        oc.api = std::clamp(nb, 1, 2);
        oc.blocks = std::clamp(std::max(nb, std::min(by_regs, by_lds)), 1, 2);
        oc.validated = 0;
    }
    return f(oc);
}

// How many workgroups of k may one persistent launch hold, for a call that wants `want` (0: none -- launch per step)?  q: the call's
// arguments with `census` set and the self-test's poll bound.  The self-test of k at grid g is a launch of the kernel itself in census
// mode + ONE stream synchronisation, once per instance, LDS size and grid size (hipets.h documents it; the rule skips it for grids <=
// the validated one); it carries no timing events and is no rollout launch to hipets_timing_read.
inline hipError_t resident_capacity(KernelRec& k, const int want, const unsigned lds, const int lds_max, const ModelDev& md, const RolloutArgs& q, hipStream_t st, int* capacity) {
    const hipError_t e = full_lds_once(k.lds, k.fn, lds_max);
    if (e != hipSuccess) return e;
    auto census_ok = [&](const int g) {
        int seen[2] = {0, 0};
        if (!q.census || hipMemsetAsync(q.census, 0, sizeof(seen), st) != hipSuccess || enqueue_rollout(k, g, lds, md, q, st, nullptr, nullptr) != hipSuccess ||
            hipMemcpyAsync(seen, q.census, sizeof(seen), hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess)
            return false;
        if (std::getenv("HIPETS_DEBUG_OCC")) std::fprintf(stderr, "[hipets] co-residency self-test: grid %d, arrived %d, saw all %d\n", g, seen[0], seen[1]);
        return seen[1] == g;
    };
    return with_residency(k, lds, lds_max, [&](Occ& oc) { return *capacity = resident_capacity_rule(oc, want, max_workgroups(), census_ok), hipSuccess; });
}

// The launch form of a DEVICE rollout whose rows change workgroups every step, `logical` workgroups in all: persistent (ONE launch for the
// horizon, every launched workgroup resident at once, the rest of the batch served in turns) or one launch per step.  How many workgroups
// of this instance can wait for each other?  resident_capacity answers from the occupancy arithmetic AND the self-test; 0 = the self-test
// failed (CUs held by another process, a masked device, an occupancy estimate that does not hold on this ROCm build): *persistent_ok goes
// false -- per-step launches until hipets_set_persistent(e, 1).  With a capacity, persistent_pays (residency_rule.hpp) chooses.
inline hipError_t decide_launch_form(KernelRec& k, const int logical, const unsigned lds, const int lds_max, const int n_cu, const ModelDev& md, const RolloutArgs& ra,
                                     int* census, const long long poll_ticks, hipStream_t st, bool* persistent_ok, bool* persistent, int* capacity_out = nullptr) {
    int capacity = 0;
    RolloutArgs q = ra;
    q.census = census;
    q.poll_ticks = std::max(poll_ticks, 20000000ll);  // the self-test keeps its 0.2 s whatever bound the hand-over polls were given
    const hipError_t e = resident_capacity(k, logical, lds, lds_max, md, q, st, &capacity);
    if (e == hipSuccess && capacity <= 0) *persistent_ok = false;
    *persistent = capacity > 0 && persistent_pays(logical, capacity, n_cu);
    if (capacity_out) *capacity_out = capacity;
    return e;
}

// Launch k.  A persistent launch (ra.exchange set: rollout.hip rollout_impl) is cut to the resident capacity -- the kernel serves the rest of
// the `grid` logical workgroups in turns -- and refused if that grid was never validated; every other launch goes straight out: one
// acquire load in full_lds_once, no lock.
inline hipError_t launch_rollout_kernel(KernelRec& k, int grid, const unsigned lds, const int lds_max, const ModelDev& md, const RolloutArgs& ra, hipStream_t st,
                                        hipEvent_t start, hipEvent_t stop) {
    const hipError_t e = full_lds_once(k.lds, k.fn, lds_max);
    if (e != hipSuccess) return e;
    if (!ra.exchange) return enqueue_rollout(k, grid, lds, md, ra, st, start, stop);
    return with_residency(k, lds, lds_max, [&](Occ& oc) {
        grid = std::min(grid, oc.blocks * oc.n_cu);
        if (max_workgroups()) grid = std::min(grid, max_workgroups());
        if (grid > oc.validated) return hipErrorLaunchFailure;  // the caller skipped the capacity query: never launch an unvalidated persistent grid
        return enqueue_rollout(k, grid, lds, md, ra, st, start, stop);  // under the lock: the grid that was just checked is the grid that goes out
    });
}

}  // namespace hipets
