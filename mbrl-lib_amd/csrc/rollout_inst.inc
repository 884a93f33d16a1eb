// rollout_inst.inc -- body of rollout_r<R>.hip: instantiates rollout_kernel<HIPETS_R, KSpec<...>> -- the generic instances
// (activation fixed to SiLU, or read at run time) and the shape-specialised "lean" instances of the BASELINE configurations --
// and defines the host launcher launch_rollout_r<R> (launch.hpp), which launches the instance launch.hpp pick_rollout_instance names.
// HIPETS_PART splits an R over four translation units, so that no compile job of the build is longer than its largest single kernel
// instance (round 6: the two fully generic instances take 40-60 s each, an R's whole set took 85-140 s as one unit):
//   1  rollout_r<R>.hip       the launcher, the reference-semantics (EXACT / DEVICE) shape-specialised instances, the hidden-static one
//   2  rollout_r<R>_fast.hip  the FAST-mode shape-specialised instances               behind HIPETS_FN(_fast)
//   3  rollout_r<R>_gen.hip   the fully generic instance (activation read at run time) behind HIPETS_FN(_gen)
//   4  rollout_r<R>_gens.hip  the fully generic instance with the SiLU epilogue fixed  behind HIPETS_FN(_gens)
#ifndef HIPETS_PART
#error "define HIPETS_PART (1..4) and HIPETS_R before including rollout_inst.inc"
#endif
#define HIPETS_CAT2_(a, b) a##b
#define HIPETS_CAT2(a, b) HIPETS_CAT2_(a, b)
#define HIPETS_FN(suffix) HIPETS_CAT2(HIPETS_CAT2(launch_rollout_r, HIPETS_R), suffix)
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <atomic>
#include <map>
#include <mutex>
#include <utility>

#include "launch.hpp"
#include "rollout.hpp"

// lean fp32, bf16x3 and bf16 shapes instantiated for this R: the per-R tables of launch.hpp
#define HIPETS_LEAN_SHAPES(X) HIPETS_CAT2(HIPETS_LEAN_SHAPES_R, HIPETS_R)(X)
#define HIPETS_B3_SHAPES(X) HIPETS_CAT2(HIPETS_B3_SHAPES_R, HIPETS_R)(X)
#define HIPETS_BF16_SHAPES(X) HIPETS_CAT2(HIPETS_BF16_SHAPES_R, HIPETS_R)(X)

// The launch mode of this unit's shape-specialised instances and the function that launches them (HIPETS_SPEC_FN), and the launch of
// the instance of a table row that matches the model: the lean fp32 instances run the output layer's accumulators straight into the
// step's tail (KSpec::FUSE = 1).
#if HIPETS_PART == 2
#define HIPETS_LEAN_MODE HIPETS_MODE_FAST
#define HIPETS_SPEC_FN HIPETS_FN(_fast)
#else
#define HIPETS_LEAN_MODE HIPETS_MODE_EXACT
#define HIPETS_SPEC_FN HIPETS_FN(_exact)
#endif
#define HIPETS_TRY_SHAPE(HC, OC, RW, TM, OB) \
    if (lean_shape_is(md, HC, OC, RW, TM, OB)) return launch_one<LeanSpec<HC, OC, RW, TM, OB, HIPETS_LEAN_MODE>>(grid, lds, lds_max, md, ra, st, start, stop);
#define HIPETS_TRY_PREC(PREC, HC, OC, RW, TM)                                                                                 \
    if (b3_shape_is(md, HC, OC, RW, TM))                                                                                      \
        return launch_one<KSpec<HIPETS_ACT_SILU, HC, OC, HIPETS_NORM_F64, HIPETS_OBS_NONE, RW, TM, HIPETS_LEAN_MODE, PREC>>( \
            grid, lds, lds_max, md, ra, st, start, stop);
#define HIPETS_TRY_B3(HC, OC, RW, TM) HIPETS_TRY_PREC(HIPETS_PREC_BF16X3, HC, OC, RW, TM)
#define HIPETS_TRY_BF16(HC, OC, RW, TM) HIPETS_TRY_PREC(HIPETS_PREC_BF16, HC, OC, RW, TM)
#define HIPETS_TRY_HID(HC) \
    if (hid_static_is(md, HC)) return launch_one<KSpec<HIPETS_ACT_SILU, HC>>(grid, lds, lds_max, md, ra, st, start, stop);

namespace hipets {

namespace {
template <class S>
hipError_t launch_one(int grid, unsigned lds, int lds_max, const ModelDev& md, const RolloutArgs& ra, hipStream_t st, hipEvent_t start,
                      hipEvent_t stop) {
    static std::atomic<bool> attr_set[64] = {};  // per device: opt in to the full 160 KB of LDS once (setting it twice is harmless)
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    if (dev < 0 || dev >= 64 || !attr_set[dev].load(std::memory_order_acquire)) {
        e = hipFuncSetAttribute(reinterpret_cast<const void*>(&rollout_kernel<HIPETS_R, S>), hipFuncAttributeMaxDynamicSharedMemorySize, lds_max);
        if (e != hipSuccess) return e;
        if (dev >= 0 && dev < 64) attr_set[dev].store(true, std::memory_order_release);
    }
    if (ra.exchange) {
        // persistent DEVICE form: every launched workgroup must be resident at once (they wait for each other's rows), and as
        // many as fit should be (a second workgroup per CU hides the stalls of the first): `grid` arrives as the number of
        // logical workgroups and is cut to what the chip holds -- the kernel serves the rest in turns (RolloutArgs::n_logical).
        // What is known about THIS instance's residency, per (device, dynamic LDS size): two models / horizons with different LDS
        // sizes keep their own entries (alternating between them costs no new self-test), and engines planning from two host
        // threads serialise here instead of racing between the capacity query and the launch that relies on it.
        struct Occ {
            int blocks = 0, api = 0, n_cu = 0;
            int validated = 0;  // largest grid of THIS instance (at this LDS size) whose co-residency the self-test has confirmed
        };
        // (one lock and one table PER DEVICE: the self-test below synchronises a stream, and engines on other devices driven from
        // other host threads must not queue behind it -- round-4 advice; the table is bounded: a process that walks through many
        // horizons / models forgets the oldest knowledge and re-validates, one launch + one synchronisation)
        constexpr int kDevSlots = 64, kMaxEntries = 32;
        static std::mutex occ_mu[kDevSlots];
        static std::map<unsigned, Occ> occ_cache[kDevSlots];
        const int slot = dev >= 0 && dev < kDevSlots ? dev : kDevSlots - 1;
        std::lock_guard<std::mutex> lock(occ_mu[slot]);
        if (dev >= kDevSlots) occ_cache[slot].clear();  // (devices beyond the table share the last slot: never trust another device's entry)
        if ((int)occ_cache[slot].size() >= kMaxEntries && !occ_cache[slot].count(lds)) occ_cache[slot].clear();
        Occ& oc = occ_cache[slot][lds];
        if (oc.blocks == 0) {
            int nb = 0;
            e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, reinterpret_cast<const void*>(&rollout_kernel<HIPETS_R, S>), kThreads, lds);
            if (e != hipSuccess) return e;
            e = hipDeviceGetAttribute(&oc.n_cu, hipDeviceAttributeMultiprocessorCount, dev);
            if (e != hipSuccess) return e;
            // the occupancy query prices dynamic LDS against the default 64 KB window, not the 160 KB this kernel opted in to:
            // take the larger of its answer and the count that follows from the register file (512 per lane and SIMD, one wave of
            // every workgroup per SIMD) and the 160 KB of LDS (with a 2 KB margin per workgroup for allocation granularity).
            // Both are ESTIMATES (no scratch, SGPR or CU-mask terms): the co-residency self-test below is what is trusted.
            hipFuncAttributes fa{};
            e = hipFuncGetAttributes(&fa, reinterpret_cast<const void*>(&rollout_kernel<HIPETS_R, S>));
            if (e != hipSuccess) return e;
            const int regs = std::max(fa.numRegs, 1);
            const int by_regs = 512 / (((regs + 7) / 8) * 8);
            const int by_lds = (int)((size_t)lds_max / ((size_t)lds + (size_t)fa.sharedSizeBytes + 2048));
            const int own = std::min(by_regs, by_lds);
            if (std::getenv("HIPETS_DEBUG_OCC"))
                std::fprintf(stderr, "[hipets] occupancy query %d, regs %d -> %d, lds %u -> %d\n", nb, regs, by_regs, lds, by_lds);
            oc.api = nb < 1 ? 1 : (nb > 2 ? 2 : nb);
            nb = std::max(nb, own);
            oc.blocks = nb < 1 ? 1 : (nb > 2 ? 2 : nb);
            oc.validated = 0;
        }
        // co-residency self-test of this instance at grid g (a launch of the kernel itself in census mode + ONE stream synchronisation,
        // once per instance, LDS size and grid size -- hipets.h documents it; later launches with grids <= the validated one skip it)
        auto census_ok = [&](const int g) -> bool {
            if (g <= oc.validated) return true;
            if (!ra.census) return false;
            if (hipMemsetAsync(ra.census, 0, 2 * sizeof(int), st) != hipSuccess) return false;
            RolloutArgs c = ra;
            c.capacity_out = nullptr;
            hipLaunchKernelGGL((rollout_kernel<HIPETS_R, S>), dim3(g), dim3(kThreads), lds, st, md, c);
            int seen[2] = {0, 0};
            if (hipGetLastError() != hipSuccess || hipMemcpyAsync(seen, ra.census, sizeof(seen), hipMemcpyDeviceToHost, st) != hipSuccess ||
                hipStreamSynchronize(st) != hipSuccess)
                return false;
            if (std::getenv("HIPETS_DEBUG_OCC")) std::fprintf(stderr, "[hipets] co-residency self-test: grid %d, arrived %d, saw all %d\n", g, seen[0], seen[1]);
            if (seen[1] != g) return false;
            oc.validated = g;
            return true;
        };
        // HIPETS_MAX_WORKGROUPS=n (tests: several processes sharing one GPU, each leaving room for the others' persistent grids; also a
        // way to keep CUs free for another stream): a persistent launch never holds more than n workgroups -- the rest of the batch is
        // served in turns, exactly as when the chip itself is the limit
        static const int wg_cap = [] { const char* v = std::getenv("HIPETS_MAX_WORKGROUPS"); const int n = v ? std::atoi(v) : 0; return n > 0 ? n : 0; }();
        if (ra.capacity_out) {  // query: how many workgroups of this instance may one persistent launch hold (0: none -- launch per step)
            // candidates, largest first: the estimate above, the runtime's own answer, one workgroup per CU; the first whose grid
            // (cut to the `grid` workgroups this call wants) passes the self-test wins
            const int want = grid;
            auto capped = [&](const int c) { return wg_cap ? std::min(c, wg_cap) : c; };
            const int cands[3] = {capped(oc.blocks * oc.n_cu), capped(oc.api * oc.n_cu), capped(oc.n_cu)};
            int cap = 0, failed_g = -1;
            for (int i = 0; i < 3 && cap == 0; ++i) {
                if (i > 0 && cands[i] >= cands[i - 1]) continue;
                const int g = std::min(want, cands[i]);
                if (g == failed_g) continue;  // the same grid just failed: a smaller capacity with the same launch size cannot pass
                if (census_ok(g)) cap = cands[i];
                else failed_g = g;
            }
            if (cap > 0 && !wg_cap) oc.blocks = cap / oc.n_cu;
            *ra.capacity_out = cap;
            return hipSuccess;
        }
        grid = std::min(grid, oc.blocks * oc.n_cu);
        if (wg_cap) grid = std::min(grid, wg_cap);
        if (grid > oc.validated) return hipErrorLaunchFailure;  // the caller skipped the capacity query: never launch an unvalidated persistent grid
        // (launched under the lock: the grid that was just checked is the grid that goes out)
        if (start) hipExtLaunchKernelGGL((rollout_kernel<HIPETS_R, S>), dim3(grid), dim3(kThreads), lds, st, start, stop, 0u, md, ra);
        else hipLaunchKernelGGL((rollout_kernel<HIPETS_R, S>), dim3(grid), dim3(kThreads), lds, st, md, ra);
        return hipGetLastError();
    }
    if (start)  // the events ride on the dispatch packet itself (start / end timestamps of THIS kernel): no extra barrier packets
        hipExtLaunchKernelGGL((rollout_kernel<HIPETS_R, S>), dim3(grid), dim3(kThreads), lds, st, start, stop, 0u, md, ra);
    else
        hipLaunchKernelGGL((rollout_kernel<HIPETS_R, S>), dim3(grid), dim3(kThreads), lds, st, md, ra);
    return hipGetLastError();
}

}  // namespace

// the other translation units of this R
hipError_t HIPETS_FN(_fast)(RolloutInstance pick, int grid, unsigned lds, int lds_max, const ModelDev& md, const RolloutArgs& ra, hipStream_t st,
                            hipEvent_t start, hipEvent_t stop);
hipError_t HIPETS_FN(_gen)(int grid, unsigned lds, int lds_max, const ModelDev& md, const RolloutArgs& ra, hipStream_t st, hipEvent_t start, hipEvent_t stop);
hipError_t HIPETS_FN(_gens)(int grid, unsigned lds, int lds_max, const ModelDev& md, const RolloutArgs& ra, hipStream_t st, hipEvent_t start, hipEvent_t stop);

#if HIPETS_PART == 3
hipError_t HIPETS_FN(_gen)(int grid, unsigned lds, int lds_max, const ModelDev& md, const RolloutArgs& ra, hipStream_t st, hipEvent_t start, hipEvent_t stop) {
    return launch_one<KSpec<-1>>(grid, lds, lds_max, md, ra, st, start, stop);
}
#endif
#if HIPETS_PART == 4
hipError_t HIPETS_FN(_gens)(int grid, unsigned lds, int lds_max, const ModelDev& md, const RolloutArgs& ra, hipStream_t st, hipEvent_t start, hipEvent_t stop) {
    return launch_one<KSpec<HIPETS_ACT_SILU>>(grid, lds, lds_max, md, ra, st, start, stop);  // the PETS default
}
#endif

#if HIPETS_PART <= 2
// the shape-specialised instance that the pick names, in this unit's launch mode: a bf16x3 one, a bf16 one, or a lean fp32 one (KSpec::WIDE or not)
hipError_t HIPETS_SPEC_FN(const RolloutInstance pick, int grid, unsigned lds, int lds_max, const ModelDev& md, const RolloutArgs& ra, hipStream_t st,
                          hipEvent_t start, hipEvent_t stop) {
    if (pick == RolloutInstance::b3) {
        HIPETS_B3_SHAPES(HIPETS_TRY_B3)
    } else if (pick == RolloutInstance::bf16) {
        HIPETS_BF16_SHAPES(HIPETS_TRY_BF16)
    } else {
        HIPETS_LEAN_SHAPES(HIPETS_TRY_SHAPE)
    }
    return hipErrorNotSupported;  // (not reached: the pick found the model's row in this table)
}
#endif

#if HIPETS_PART == 1
hipError_t HIPETS_FN()(int grid, unsigned lds, int lds_max, const ModelDev& md, const RolloutArgs& ra, hipStream_t st, hipEvent_t start,
                            hipEvent_t stop) {
    const RolloutInstance pick = pick_rollout_instance(md, ra, HIPETS_R);
    switch (pick) {
        case RolloutInstance::lean:
        case RolloutInstance::lean_wide:
        case RolloutInstance::b3:
        case RolloutInstance::bf16:
            return (ra.whole_horizon ? HIPETS_FN(_fast) : HIPETS_FN(_exact))(pick, grid, lds, lds_max, md, ra, st, start, stop);
        case RolloutInstance::hidden_static: HIPETS_HID_STATIC_SHAPES(HIPETS_TRY_HID) break;
        case RolloutInstance::generic_silu: return HIPETS_FN(_gens)(grid, lds, lds_max, md, ra, st, start, stop);
        case RolloutInstance::generic: return HIPETS_FN(_gen)(grid, lds, lds_max, md, ra, st, start, stop);
        case RolloutInstance::no_b3:
        case RolloutInstance::no_bf16: return hipErrorNotSupported;          // (hipets.hip launch_rollout reports it)
        case RolloutInstance::no_wide: return hipErrorInvalidConfiguration;  // never run another layout in LDS sized for a WIDE instance
    }
    return hipErrorNotSupported;
}
#endif  // HIPETS_PART == 1

}  // namespace hipets
