// rollout.hpp -- the fused PETS rollout kernel for gfx950 (MI355X).
//
// Replaces, per planning step, the ~55 ATen launches of
//   ModelEnv.evaluate_action_sequences   (mbrl/models/model_env.py:145-191)
//   OneDTransitionRewardModel.sample     (mbrl/models/one_dim_tr_model.py:245-289, :103-116)
//   GaussianMLP._forward_ensemble        (mbrl/models/gaussian_mlp.py:129-216)
//   EnsembleLinearLayer.forward          (mbrl/models/util.py:53-65)
//   Ensemble.sample_1d                   (mbrl/models/model.py:426-473)
//   reward / termination fns             (mbrl/env/reward_fns.py, termination_fns.py)
// with one kernel.  A workgroup (4 waves, one per SIMD) owns R row tiles of 16 rollout rows that
// all use the SAME ensemble member in a given step, keeps their activations in LDS (ping-pong
// [rows][ld] f32 buffers, ld == 8 mod 64 so ds_read_b128 A-fragment reads are conflict free) and
// streams that member's weights from L2 as pre-packed v_mfma_f32_16x16x4_f32 B fragments
// (one coalesced 1 KiB global_load_dwordx4 per 16x16 k-chunk, reused by all R row tiles).
//
//   EXACT mode: one launch per step; rows are gathered through the reference's randperm so that
//               workgroup (member m, chunk) sees exactly rows perm[m*B/M + ...] (bit-for-bit the
//               reference's row->member map); state lives in HBM between launches.
//   FAST  mode: one launch for the whole horizon; workgroup (particle p, candidate group g) owns
//               its rows for all H steps, state stays in LDS, the member is drawn per
//               (workgroup, step) from a balanced schedule, eps comes from Philox.
//
// This file holds the kernel and what only the kernel uses (the hand-over primitives, MinWaves, HIPETS_STAMP).  Its layers:
//   rollout_types.hpp  argument structs          gemm_f32.hpp / gemm_bf16.hpp  the linear ops          kspec.hpp  instance facts, layer dispatch
//   closed_forms.hpp   reward / termination / sampling forms                   rollout_smem.hpp        the LDS layout
#pragma once
#include "closed_forms.hpp"
#include "common.hpp"
#include "gemm_f32.hpp"
#include "kspec.hpp"
#include "rollout_smem.hpp"
#include "rollout_types.hpp"

namespace hipets {

// 16-byte write-through store / load of a PAIR of hand-over granules {value, tag, value, tag} (persistent DEVICE form).  sc1 =
// device scope: the store leaves the XCD's L2, the load never returns a stale L1 line (MI355X_MICROARCH.md: 8-byte sc1 stores
// cost 2.7x the 16-byte ones per byte, and a workgroup's polls queue behind its own stores).  The load is asynchronous:
// pair_wait() is the s_waitcnt, tied to the destination registers so nothing reads them earlier.
// (s_nop 1 behind the store: a VMEM store of more than 8 bytes reads its data registers late, and on gfx940+ a VALU write of one
// of them needs TWO wait states behind it.  The compiler keeps that distance for its own stores; inside an asm statement it does not
// know there is a store.  Round 5: after an unrelated change the next instruction but one rewrote the first data register, and under
// load -- two workgroups per CU -- quads of lanes published a scratch value instead of a state dim, or a corrupt tag that nobody could
// ever match: returns off in the 5th digit, once a time-out.  __graft_entry__.scan_isa_hazards checks the emitted code for it now.)
__device__ __forceinline__ void pair_store(unsigned long long* p, const unsigned v0, const unsigned v1, const unsigned tag) {
    const u32x4g d = {v0, tag, v1, tag};
    asm volatile("global_store_dwordx4 %0, %1, off sc1\n\ts_nop 1" ::"v"(p), "v"(d) : "memory");
}
__device__ __forceinline__ void pair_load_issue(u32x4g& d, const unsigned long long* p) {
    asm volatile("global_load_dwordx4 %0, %1, off sc1" : "=&v"(d) : "v"(p) : "memory");
}
// workgroup barrier for data exchanged through LDS only: waits for this wave's LDS traffic, NOT for global memory operations in flight
// (__syncthreads() also drains vmcnt)
__device__ __forceinline__ void lds_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }
// LDS-DMA of 64 hand-over pairs (one per lane, device-scope loads like pair_load_issue) straight into LDS: lane l's 16 bytes land at
// LDS byte address lds_dst + 16 l (lds_dst wave-uniform), no destination registers.  Counted on vmcnt; the compiler does not know
// (cdna_hip_programming.md: M0 is written and restored inside the statement that reads it; the s_nop is the SALU-write -> M0-read
// state).  Data is visible to a ds_read of the ISSUING wave after its own s_waitcnt vmcnt(0) (MI355X_MICROARCH.md item 7).
__device__ __forceinline__ void pair_dma_issue(const unsigned long long* gsrc, const unsigned lds_dst) {
    unsigned keep;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off sc1\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep) : "v"(gsrc), "s"(lds_dst) : "memory");
}
__device__ __forceinline__ void vmem_drain() { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); }

template <int R, class S> struct MinWaves { static constexpr int value = S::WIDE ? 1 : MinWavesOf<R>::value; };  // (WIDE: the LDS admits one workgroup per CU anyway)

// S = KSpec<...>: the compile-time facts of this instance (generic: only the activation may be fixed; lean: the whole shape).
// Profiling build only (-DHIPETS_STEP_TRACE, profiles/handover_trace.py): wall-clock stamps (100 MHz, chip-wide) of every
// workgroup at four points of every step of the persistent DEVICE form, behind the phase-cycle table of the caller's buffer.
#ifdef HIPETS_STEP_TRACE
#define HIPETS_STAMP(k, step)                                                                                                     \
    do {  /* one record per (launched workgroup, step, turn): stamp_seq = the (step, turn) sequence index of the step loop */     \
        (void)(step);                                                                                                             \
        if (persist && ra.phase_cycles && tid == 0 && n_serve <= 4)                                                                \
            ra.phase_cycles[128 + ((size_t)blockIdx.x * (ra.H * 4) + stamp_seq) * 4 + (k)] = wall_clock64();  /* stride: <= 4 turns per step */ \
    } while (0)
#else
#define HIPETS_STAMP(k, step) do {} while (0)
#endif

template <int R, class S>
__global__ __launch_bounds__(kThreads, (MinWaves<R, S>::value)) void rollout_kernel(const ModelDev md, const RolloutArgs ra) {
    constexpr int ROWS = kTile * R;
    constexpr bool kLean = S::LEAN;
    constexpr bool kB3 = S::PIECES > 0;  // operands as three bf16 pieces (bf16x3) or one (bf16) on the bf16 matrix pipe (lean instances)
    constexpr int kNP = kB3 ? S::PIECES : 1;
    static_assert(!kB3 || kLean, "bf16x3 / bf16 arithmetic exists for the shape-specialised instances");
    // (no cross-layer weight prefetch: the next op's chunk-0 fragments requested behind this op's k loop measured slower -- 56 more live
    // VGPRs and the scalar work between layers outweigh the latency it hides)
    // facts that are template arguments in a lean instance and model / call fields in the generic one
    const int normalizer = S::NORM >= 0 ? S::NORM : md.normalizer;
    const int obs_process = S::OBSP >= 0 ? S::OBSP : md.obs_process;
    const int reward_fn = S::REW >= 0 ? S::REW : md.reward_fn;
    const int term_fn = S::TERM >= 0 ? S::TERM : md.term_fn;
    const int lv_rows = kLean ? 1 : md.lv_rows;
    const bool deterministic = kLean ? false : md.deterministic != 0;
    float* const trace_next_obs = kLean ? nullptr : ra.trace_next_obs;
    float* const trace_rewards = kLean ? nullptr : ra.trace_rewards;
    const int ld_k = S::LD > 0 ? S::LD : md.ld;  // the LDS row stride: a compile-time fact in the shape-specialised fp32 instances
    constexpr bool kWide = S::WIDE;
    const int ld_in = kWide ? md.ld_in : ld_k;    // row stride of the model-input image (buf0 in the WIDE instances, see KSpec)
    extern __shared__ __attribute__((aligned(16))) char smem[];
    RolloutSmem sm;
    {
        // the layout of rollout_smem.hpp, carved.  Its last two sections (rollout_smem.hpp: no kernel has both, nothing follows them)
        // start at the same address and are not sized here: the host's total covers them (rollout_smem_bytes, checked below in debug
        // builds), and their sizes computed here ahead of their real uses moved every rollout kernel's register allocation.
        char* p = smem;
#define HIPETS_CARVE(T, name, bytes)   \
    sm.name = reinterpret_cast<T*>(p); \
    p += (bytes);
        HIPETS_ROLLOUT_SECTIONS(HIPETS_CARVE, ROWS, ld_in, ld_k, md.obs_dim, md.act_dim, md.in_dim, md.lv_rows, md.out_dim, md.out_total, ra.H, false, false)
#undef HIPETS_CARVE
#if HIPETS_DEBUG_BOUNDS
        {   // every section starts inside the launch's dynamic LDS, 16-byte aligned, in layout order; the whole layout fits the launch's size
#define HIPETS_SECTION_START(T, name, bytes) (char*)sm.name,
            const char* const secs[] = {HIPETS_ROLLOUT_SECTION_NAMES(HIPETS_SECTION_START)};
#undef HIPETS_SECTION_START
            for (int i = 0; i < kRolloutSections; ++i) {
                HIPETS_BOUND(secs[i] >= smem && secs[i] <= smem + ra.lds_bytes);
                HIPETS_BOUND(((size_t)(secs[i] - smem) & 15) == 0);
                HIPETS_BOUND(i == 0 || secs[i] >= secs[i - 1]);
            }
            const bool expect = !S::LEAN && md.propagation == HIPETS_PROP_EXPECTATION;
            HIPETS_BOUND(rollout_smem_bytes(ROWS, ld_k, md.obs_dim, md.act_dim, md.in_dim, md.out_dim, md.out_total, ra.H, expect, md.lv_rows, kWide ? ld_in : 0) <= ra.lds_bytes);
            HIPETS_BOUND(md.Kp0 <= (kWide ? md.ld_in : ld_k) && md.obs_in + md.act_dim == md.in_dim && md.in_dim <= md.Kp0);
        }
#endif
    }
    const int tid = threadIdx.x;
    if (ra.census) {
        // Co-residency self-test (launch.hpp / rollout_inst.inc launch_one): the persistent DEVICE form is only correct when every
        // launched workgroup is resident at once, and the occupancy the host computes (API answer, register and LDS arithmetic) is
        // an estimate.  Same kernel, same launch configuration, so the same footprint: if all gridDim.x workgroups can meet here,
        // they can wait for each other's rows.  A workgroup that is not admitted never arrives and the others time out.
        if (tid == 0) {
            __hip_atomic_fetch_add(ra.census, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            const long long t0 = wall_clock64();
            bool all = true;
            while (__hip_atomic_load(ra.census, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < (int)gridDim.x) {
                if (wall_clock64() - t0 > ra.poll_ticks) { all = false; break; }
                __builtin_amdgcn_s_sleep(8);
            }
            if (all) __hip_atomic_fetch_add(ra.census + 1, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        return;
    }
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const bool fast = S::KMODE >= 0 ? S::KMODE == HIPETS_MODE_FAST : ra.whole_horizon != 0;
    const bool expectation = kLean ? false : md.propagation == HIPETS_PROP_EXPECTATION;
    // Modes whose workgroups are bound to a member (EXACT / DEVICE: member = wg / groups): hardware deals block b to XCD b % 8
    // (observed, used for speed only), so the logical workgroup index is taken XCD-major -- XCD x runs a CONTIGUOUS range of
    // logical workgroups, i.e. the workgroups of at most two members, and its 4 MiB L2 streams two members' weights instead of
    // all of them (bf16x3: 0.83 MB per member, all five = 4.2 MB do not fit one L2).  Any bijection is correct.
    int wg = blockIdx.x;
    if (!fast) {
        const int nwg = gridDim.x, x = wg & 7, slot = wg >> 3;
        wg = x * (nwg >> 3) + min(x, nwg & 7) + slot;
    }

    // ---- which rollout rows does this workgroup own; per-dimension constants into LDS -------------
    int domain = 0;
    if (fast) {
        // the B = pop * P rows in ONE run, particle-major (run index g = p * pop + c), dealt ROWS at a time: ceil(ceil(B / 16) / R)
        // workgroups, whatever pop is (until round 5 every particle's pop rows were dealt on their own: cfg4''s second iCEM iteration,
        // pop 805 -> 51 tiles per particle, took 26 x 20 = 520 two-tile workgroups -- a third round on 256 CUs for 8 of them)
        for (int s = tid; s < ROWS; s += kThreads) {
            const int g = wg * ROWS + s;  // (<= 8000 workgroups x 64 rows)
            const int p = g / ra.pop, c = g - p * ra.pop;
            sm.rowid[s] = g < ra.B ? c * ra.P + p : -1;
        }
        if (!expectation) {
            // this workgroup's member slot of every step: the caller's schedule, or drawn here (one keyed bijection of the workgroup
            // indices per step, thread t evaluates step t's: common.hpp fast_member)
            if (ra.schedule) {
                for (int t = tid; t < ra.H; t += kThreads) sm.sched[t] = ra.schedule[(size_t)t * gridDim.x + wg];
            } else {
                const bool fixed = md.propagation == HIPETS_PROP_FIXED_MODEL;
                for (int t = tid; t < ra.H; t += kThreads)
                    sm.sched[t] = fast_member((unsigned)wg, gridDim.x, ra.fm_a, ra.fm_b, md.M, md.iid_members, ra.seed, ra.stream_id, fixed ? 0xFFFFFFFFu : (unsigned)t);
            }
        }
    } else {
        domain = wg / ra.groups;
        const int j0 = (wg % ra.groups) * ROWS;
        const long long* perm = ra.perm ? ra.perm + (long long)ra.t_begin * ra.perm_step : nullptr;
        // unbalanced member maps (BasicEnsemble) pad every member's slots with -1 at the tail: nothing to do here
        if (perm && perm[(long long)domain * ra.rows_per_domain + j0] < 0) return;
        // DEVICE mode: the step's permutation is a keyed bijection evaluated on the fly (common.hpp perm_apply)
        const PermKeys keys0 = ra.exchange ? ra.step_keys[ra.t_begin] : ra.perm_keys;
        for (int s = tid; s < ROWS; s += kThreads) {
            const int j = j0 + s;
            int rid = -1;
            if (j < ra.rows_per_domain) {
                const int jj = domain * ra.rows_per_domain + j;
                rid = perm ? (int)perm[jj] : (ra.perm_n ? (int)perm_apply((unsigned)jj, ra.perm_n, ra.perm_a, ra.perm_b, keys0) : jj);
            }
            sm.rowid[s] = rid;
        }
    }
    // the ensemble member this workgroup runs: its row domain's (reference semantics: slot j -> member j / (B / M)) -- or, for
    // RolloutArgs::fast_members launches (one step of B independent rows, hipets_step in FAST mode), the FAST rule's
    int member_dom = domain;
    if (!fast && ra.fast_members && !expectation)
        member_dom = __builtin_amdgcn_readfirstlane(
            ra.schedule ? ra.schedule[(size_t)ra.t_begin * gridDim.x + wg]
                        : fast_member((unsigned)wg, gridDim.x, ra.fm_a, ra.fm_b, md.M, md.iid_members, ra.seed, ra.stream_id,
                                      md.propagation == HIPETS_PROP_FIXED_MODEL ? 0xFFFFFFFFu : (unsigned)ra.t_begin));
    const bool persist = !fast && ra.exchange != nullptr;  // DEVICE mode in ONE launch: rows are handed over through `exchange`
    // ---- Ragged last turn (round 6; KSpec::WIDE two-tile instances in the turn-based persistent form) -------------------------------
    // A batch of n2 two-tile logical workgroups on G launched ones is served in ceil(n2 / G) turns per step, and a step is as long as
    // its turns: the last turn costs a whole two-tile turn however few rows it holds (cfg4' iCEM, 497 candidates: 315 logical
    // workgroups = 256 + 59 -- the second turn is 23 % full and the rollout takes exactly as long as the 805-candidate one).  When
    // the row tiles left for the last turn fit ONE per launched workgroup, that turn is dealt in one-tile logical workgroups instead
    // -- v >= half_from: (member domain, tile) in domain-major order behind the last full turn -- and runs the R = 1 bodies of the
    // MLP ops on row tile 0 of the same LDS layout (the turn costs 0.69 of a two-tile one).  Which workgroup holds a row never
    // enters the arithmetic (the step's permutation decides the member, every (column tile, row tile) unit sums in the same k
    // order whatever R is): same bits as the two-tile dealing, the per-step launches and the generic kernel (tested).
    constexpr bool kRagged = S::WIDE && R == 2;
    int half_from = 0x7FFFFFFF;     // first one-tile logical workgroup
    int n_logical = ra.n_logical;   // logical workgroups of this launch
    int hf_dom = 0, hf_tile = 0, hf_tpd = 1;  // where the one-tile range starts (member domain, tile in it); tiles per domain
    if constexpr (kRagged) {
        if (persist && ra.ragged_last_turn) {
            const int G = (int)gridDim.x, n2 = ra.n_logical;
            const int turns2 = (n2 + G - 1) / G, full = (turns2 - 1) * G;  // two-tile logical workgroups of the full turns
            if (turns2 >= 2) {
                hf_tpd = (ra.rows_per_domain + kTile - 1) / kTile;
                hf_dom = full / ra.groups;
                hf_tile = 2 * (full - hf_dom * ra.groups);
                const int rem = (hf_tpd - hf_tile) + (n2 / ra.groups - 1 - hf_dom) * hf_tpd;  // row tiles behind the full turns
                if (rem <= G) {
                    half_from = full;
                    n_logical = full + rem;
                }
            }
        }
    }
    // logical workgroup v -> its member domain, first row slot in the domain, rows it holds
    auto logical_rows = [&](const int v, int& dom, int& j0, int& live) __attribute__((always_inline)) {
        if (!kRagged || v < half_from) {
            dom = v / ra.groups;
            j0 = (v - dom * ra.groups) * ROWS;
            live = ROWS;
        } else {
            int w = v - half_from + hf_tile;  // tile index counted from the start of domain hf_dom
            const int dd = w / hf_tpd;
            dom = hf_dom + dd;
            j0 = (w - dd * hf_tpd) * kTile;
            live = kTile;
        }
    };
    const bool poll_every = ra.poll_ticks < 1000;  // bounds below 10 us (tests of the time-out path): look at the clock on every spin, not every 64th
    // hand-over table row = NVP pairs of 8-byte granules: the state dims (padded to an even count), then {running total, flag}.
    // exchange item i = (row slot i / NVP, pair i % NVP): items tid + q * kThreads of a thread are the same every step
    constexpr int kG = 2;  // 16-byte pair loads in flight per thread and round (cfg2: 48 rows x 10 pairs = 480 items, one round)
    const int NVP = (md.obs_dim + 1) / 2 + 1;  // pairs per row
    const int NV = 2 * NVP;                    // granules per row
    const unsigned nvp_magic = (unsigned)(0x100000000ull / (unsigned)NVP) + 1u;  // NVP >= 2
    // The give-up rule of every hand-over poll (true: the caller leaves its loop).  A hand-over takes microseconds; 0.2 s (poll_ticks)
    // without the producer means it is not running at all (the grid is not co-resident: another process or stream holds CUs) -- give up
    // loudly instead of spinning on; a flag that is already up (another workgroup, or an earlier poll, gave up) ends the wait after
    // 64 spins: the results of the launch are void anyway and the host re-runs the call (hipets_check_async_error)
    auto poll_gave_up = [&](const int spins, const long long t_poll) __attribute__((always_inline)) {
        if ((poll_every || (spins & 63) == 63) && (wall_clock64() - t_poll > ra.poll_ticks || *(volatile int*)ra.error_flag)) {
            *ra.error_flag = 1;
            return true;
        }
        return false;
    };
    // sm.pend[s] was set: the row's {running total, flag} pair was late at the collect -- its previous owner published it after ITS
    // output layer / reward phase (normally long arrived).  Poll the row's last pair until its tags are step t's.
    auto fetch_late_total = [&](const int rid, const int t, float& tot, int& trm) __attribute__((always_inline)) {
        const unsigned long long* const src = ra.exchange + (size_t)rid * NV + (NV - 2);
        const unsigned want = ra.tag_base + (unsigned)t;
        const long long t_poll = wall_clock64();
        u32x4g g = {0u, 0u, 0u, 0u};
        for (int spins = 0;; ++spins) {
            pair_load_issue(g, src);
            asm volatile("s_waitcnt vmcnt(0)" : "+v"(g)::"memory");
            if (g[1] == want && g[3] == want) break;
            if (poll_gave_up(spins, t_poll)) break;
            __builtin_amdgcn_s_sleep(8);
        }
        tot = __uint_as_float(g[0]);
        trm = (int)g[2];
    };
    // The masked accumulation that ends a step for row `rid` in slot s (model_env.py:186-188): a terminated row earns nothing more; the
    // running total and flag stay in LDS and are published to the row's next owner (`handover`, tag `tag`) or, on the last step of the
    // persistent form, the total is the row's return
    auto end_step_for_row = [&](const int s, const int rid, float tot, int trm, float r, const bool done, unsigned long long* const handover,
                                const unsigned tag) __attribute__((always_inline)) {
        if (trm) r = 0.f;
        trm = trm | (done ? 1 : 0);
        tot += r;
        sm.term[s] = trm;
        sm.tot[s] = tot;
        if (handover) pair_store(handover + (size_t)rid * NV + (NV - 2), __float_as_uint(tot), (unsigned)trm, tag);
        else if (persist) ra.totals[rid] = tot;  // last step: the row's return
    };
    // rows wider than a few pairs (cfg4: 24 pairs per row, cfg4': 189) are collected in rounds of kGT pairs per thread, each round one
    // round trip to the table (>= 1 us even when the rows are long there: the later turns of a step): 4 / 8 in flight instead of 2
    // cut cfg4''s 12 rounds per turn to 3.  (Only the collect phase holds these registers; the straight form's cfg2 needs one round.)
    // (round 4, step trace of the turn-based form, profiles/turn_trace.py + r4_turn_trace.json: cfg4' spends 9.5 us per turn in its
    // three rounds of 8 and 8.3 us between "my rows arrived" and "input built"; MORE pairs in flight measured SLOWER -- 16 per thread
    // for the WIDE instances: 9.84 -> 10.36 ms per cfg4' rollout (the per-item state of the retry loop pushes the kernel's
    // accumulators into AccVGPR spill space: 98 -> 126), 8 instead of 4 for cfg4: 3.37 -> 3.41 ms -- and HALVING the hand-over
    // traffic changed nothing (9.84 vs 9.89 ms): the phase is bound by round-trip latency and its own bookkeeping, not by bandwidth)
    constexpr int kGT = (kLean && S::OUTC >= 4) ? 4 : kG;  // (KSpec::WIDE instances collect by LDS-DMA: below)
    // Round 6, KSpec::WIDE (cfg4', Humanoid-v4: 189 pairs per row, 6 048 per two-tile workgroup and turn): the rows of a turn are fetched
    // by LDS-DMA -- no destination registers, so ALL of a wave's ~24 KiB are in flight at once (the register path above manages 8 pairs
    // per thread and needs three round trips of ~3 us) -- into the activation buffers, which are idle between two turns, and validated
    // LDS -> LDS by the wave that issued them (dma_collect below).  Every persistent launch of the instance takes the turn-based flow
    // then, also when each workgroup serves one logical workgroup (the straight form's collect writes the input image while it polls:
    // the image IS the staging area here).
    int xs[kG], xv[kG];
#pragma unroll
    for (int q = 0; q < kG; ++q) {
        const int i = tid + q * kThreads;
        xs[q] = i < ROWS * NVP ? i / NVP : -1;
        xv[q] = i < ROWS * NVP ? i - (i / NVP) * NVP : 0;
    }
    if constexpr (kB3) {
        // bf16x3: the k chunks are 32 wide, the column tiles 16: the last chunk of a 13-tile layer ends in 16 columns no epilogue
        // ever writes.  Their weights are zero, but 0 x (whatever bits LDS holds) may be NaN: clear both activation buffers once.
        f32x4* z = reinterpret_cast<f32x4*>(sm.buf0);
        const int n16 = (int)(2 * act_buf_bytes(ROWS, ld_k) / 16);
        for (int i = tid; i < n16; i += kThreads) z[i] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
    // ---- per-dimension constants -> LDS, and the rows' initial state / totals / flags / first actions: EVERY global load of the
    // prologue is issued before the first dependent LDS store, so the whole prologue costs ONE global round trip (the per-step
    // launches of EXACT / DEVICE mode pay it once per step and workgroup; element i of every table is fetched by thread i,
    // tables longer than the workgroup loop on afterwards)
    const int nlv = deterministic ? 0 : lv_rows * md.out_dim;
    const bool norm = normalizer != HIPETS_NORM_NONE;
    double c_nm = 0.0, c_ns = 1.0;
    float c_lo = 0.f, c_hi = 0.f;
    int c_nd = 0, c_lm = 0;
    constexpr int kMetaWords = (int)(sizeof(LayerMeta) / sizeof(int));  // the layer table travels as plain 32-bit words
    const int n_meta = md.n_layers * kMetaWords;                        // (<= 48: one word per thread, no private copy)
    if (norm && tid < md.in_dim) { c_nm = md.norm_mean[tid]; c_ns = md.norm_std[tid]; }
    if (tid < nlv) { c_lo = md.min_lv[tid]; c_hi = md.max_lv[tid]; }
    if (tid < md.obs_dim) c_nd = md.no_delta[tid];
    if (tid < n_meta) c_lm = reinterpret_cast<const int*>(md.layers)[tid];
    auto commit_constants = [&]() __attribute__((always_inline)) {
        if (norm && tid < md.in_dim) { sm.nmean[tid] = c_nm; sm.nstd[tid] = normalizer == HIPETS_NORM_F64 ? 1.0 / c_ns : c_ns; }  // f64: 1 / std, see build_input
        if (tid < nlv) { sm.minlv[tid] = c_lo; sm.maxlv[tid] = c_hi; }
        if (tid < md.obs_dim) sm.nodelta[tid] = c_nd;
        if (tid < n_meta) reinterpret_cast<int*>(sm.lmeta)[tid] = c_lm;
        if (norm)
            for (int i = tid + kThreads; i < md.in_dim; i += kThreads) { sm.nmean[i] = md.norm_mean[i]; sm.nstd[i] = normalizer == HIPETS_NORM_F64 ? 1.0 / md.norm_std[i] : md.norm_std[i]; }
        for (int i = tid + kThreads; i < nlv; i += kThreads) { sm.minlv[i] = md.min_lv[i]; sm.maxlv[i] = md.max_lv[i]; }
        for (int i = tid + kThreads; i < md.obs_dim; i += kThreads) sm.nodelta[i] = md.no_delta[i];
    };
    lds_barrier();  // sm.rowid (and the B3 clear) visible; the constants' loads stay in flight

    // ---- initial state, totals, flags: loads issued in batches of kStage per thread (one round trip, not one per element) ----
    auto load_initial_state = [&]() __attribute__((always_inline)) {
        constexpr int kStage = 4;
        constexpr int kRowStage = (ROWS + kThreads - 1) / kThreads;
        const int n_st = ROWS * md.obs_dim;
        float tot0[kRowStage];
        int term0[kRowStage];
#pragma unroll
        for (int q = 0; q < kRowStage; ++q) {
            const int s = tid + q * kThreads;
            const int rid = s < ROWS ? sm.rowid[s] : -1;
            tot0[q] = (!fast && !persist && rid >= 0) ? ra.totals[rid] : 0.f;
            term0[q] = (!fast && !persist && rid >= 0) ? (int)ra.term[rid] : 0;
        }
        bool first = true;
        for (int base = tid; base < n_st || first; base += kStage * kThreads) {
            float v[kStage];
#pragma unroll
            for (int q = 0; q < kStage; ++q) {
                const int i = base + q * kThreads;
                v[q] = 0.f;
                if (i < n_st) {
                    const int s = i / md.obs_dim, d = i - s * md.obs_dim;
                    const int rid = sm.rowid[s];
                    if (fast) {
                        if (!kLean && ra.pop_env > 0) v[q] = rid >= 0 ? ra.s0[(size_t)((rid / ra.P) / ra.pop_env) * md.obs_dim + d] : 0.f;
                        else v[q] = ra.s0[d];
                    } else if (rid >= 0) {
                        // persistent form: starts from the tiled s0 itself (batched planning: the s0 of the row's environment)
                        if (!persist) v[q] = ra.state[(size_t)rid * md.obs_dim + d];
                        else if (!kLean && ra.pop_env > 0) v[q] = ra.s0[(size_t)((rid / ra.P) / ra.pop_env) * md.obs_dim + d];
                        else v[q] = ra.s0[d];
                    }
                }
            }
            if (first) {  // everything the prologue needs from global memory has been requested: now the dependent stores
                commit_constants();
#pragma unroll
                for (int q = 0; q < kRowStage; ++q) {
                    const int s = tid + q * kThreads;
                    if (s < ROWS) {
                        sm.tot[s] = tot0[q];
                        sm.term[s] = term0[q];
                        sm.lrew[s] = 0.f;
                        sm.pend[s] = 0;
                        sm.pend[ROWS + s] = 0;
                    }
                }
                first = false;
            }
#pragma unroll
            for (int q = 0; q < kStage; ++q) {
                const int i = base + q * kThreads;
                if (i < n_st) sm.state[i] = v[q];
            }
        }
    };

    const int nblk = (md.out_dim + 3) / 4;
    const int Kp0 = md.Kp0;
    Prof prof;
    prof.on = (!kLean || HIPETS_LEAN_PROF) && ra.phase_cycles != nullptr && wg == 0 && lane == 0;
    prof.slot = sm.prof + wave * 16;
    if (prof.on) {
#pragma unroll
        for (int i = 0; i < 15; ++i) prof.slot[i] = 0;
        prof.slot[15] = __builtin_amdgcn_s_getreg((4) | (0 << 6) | (15 << 11));  // where this wave landed (HW_REG_HW_ID: simd [5:4], cu [11:8])
    }
    prof.t = prof.on ? clock64() : 0;

    // the step's actions (model_env.py:179-182: row r uses candidate r // P) come from HBM.  Each thread owns up to
    // kPrefetch (row, action-dim) elements; their addresses are fixed for the whole horizon up to the t * A term, and
    // the loads for step t+1 are issued at the top of step t's sampling phase so their latency hides behind it.
    constexpr int kPrefetch = 4;
    const int n_act = ROWS * md.act_dim;
    long long act_base[kPrefetch];  // element offset of (candidate, t = 0, a); -1 = nothing to fetch
    // (row slot, action dim) of this thread's elements never change; the candidate of a row id (rid / P) by multiply-high with
    // ceil(2^32 / P): exact while rid * P < 2^32 (B * P: 2e5 x 20 at cfg2), else the division itself
    int act_s[kPrefetch], act_a[kPrefetch];
#pragma unroll
    for (int q = 0; q < kPrefetch; ++q) {
        const int i = tid + q * kThreads;
        act_s[q] = i < n_act ? i / md.act_dim : -1;
        act_a[q] = i < n_act ? i - (i / md.act_dim) * md.act_dim : 0;
    }
    const bool magic_ok = ra.P > 1 && (unsigned long long)ra.B * (unsigned)ra.P < 0x100000000ull;  // (P = 1: the constant would be 2^32)
    const unsigned magic_p = (unsigned)(0x100000000ull / (unsigned)max(ra.P, 2)) + 1u;
    const int act_stride = ra.H * md.act_dim;
    // whose rows the action fetch / action columns are for: the slot's current rows -- except in the straight persistent form
    // (below), where the actions of step t + 1 are fetched during step t for the rows the slot will hold THEN
    const int* act_rows = sm.rowid;
    auto compute_act_base = [&]() __attribute__((always_inline)) {  // from act_rows (again whenever the workgroup's rows change)
#pragma unroll
        for (int q = 0; q < kPrefetch; ++q) {
            act_base[q] = -1;
            if (act_s[q] >= 0) {
                const int rid = act_rows[act_s[q]];
                const int cand = magic_ok ? (int)__umulhi((unsigned)rid, magic_p) : rid / ra.P;
                if (rid >= 0) act_base[q] = (long long)cand * act_stride + act_a[q];
            }
        }
    };
    compute_act_base();
    auto fetch_actions_rest = [&](const int t) __attribute__((always_inline)) {  // elements beyond kPrefetch per thread (very wide action spaces)
        float* actn_t = sm.actn + (t & 1) * n_act;
        for (int i = tid + kPrefetch * kThreads; i < n_act; i += kThreads) {
            const int s = i / md.act_dim, a = i % md.act_dim;
            const int rid = act_rows[s];
            actn_t[i] = rid >= 0 ? ra.actions[((size_t)(rid / ra.P) * ra.H + t) * md.act_dim + a] : 0.f;
        }
    };
    auto fetch_actions_issue = [&](const int t, float (&av)[kPrefetch]) {
#pragma unroll
        for (int q = 0; q < kPrefetch; ++q) av[q] = act_base[q] >= 0 ? ra.actions[act_base[q] + (long long)t * md.act_dim] : 0.f;
    };
    auto fetch_actions_commit = [&](const int t, const float (&av)[kPrefetch]) {
        float* actn_t = sm.actn + (t & 1) * n_act;
#pragma unroll
        for (int q = 0; q < kPrefetch; ++q) {
            const int i = tid + q * kThreads;
            if (i < n_act) actn_t[i] = av[q];
        }
        fetch_actions_rest(t);
    };

    // model input of step t: cat(obs_process(obs), act), normalised (one_dim_tr_model.py:103-116), into buf0.
    // One item = (row, 4 consecutive columns): four independent LDS-read -> f64 normalise -> LDS-write chains.
    int kq = Kp0 >> 2;  // column quads per row (the padded input width is a multiple of 16; bf16x3: of 32, set once the layer table is in LDS)
    // The (wave-uniform) normaliser / obs-preprocess switches are resolved ONCE per call into a compile-time variant:
    // with the switches inside, each of the four elements became its own chain of scalar branches and waits.
    // Item -> columns.  The fp32 image stores, inside every 16-wide k chunk, the 4 x 4 block (k-step, lane group) transposed
    // (lds_col): the four columns {16 kk + 4 q + g : q = 0..3} of lane group g sit at the CONSECUTIVE positions 16 kk + 4 g .. + 3.
    // An item is therefore (row, chunk kk, group g) with those four columns (round 4): ONE ds_write_b128 instead of four scattered
    // ds_write_b32, and consecutive threads read consecutive state floats / normaliser doubles (conflict free) where the old item
    // (four CONSECUTIVE columns) read with a stride of four (measured on cfg4', 393 columns x 32 rows: 8.3 us per turn in the step
    // trace, profiles/turn_trace.py).  Same arithmetic per element.  bf16x3 / bf16 images keep consecutive columns (split_x4's layout).
    auto build_input_impl = [&](const int t, float* const dst, auto norm_tag, auto plain_tag) __attribute__((always_inline)) {
        constexpr int NORM = decltype(norm_tag)::value;
        constexpr bool PLAIN = decltype(plain_tag)::value;
        // (shape-specialised instances WITH obs preprocessing keep the old items: their input is narrow, this function runs in their
        // prologue and turn-based flows only, and the R = 2 halfcheetah DEVICE instance -- at the 256-register limit of two waves per
        // SIMD -- spilt one VGPR to scratch with four sinf / cosf-bearing elements held for one store)
        constexpr bool kByGroup = !kB3 && (PLAIN || !kLean);
        const float* actn_t = sm.actn + (t & 1) * n_act;
        if constexpr (kByGroup && PLAIN && NORM != HIPETS_NORM_F32) {
            // Round 5 (step trace of the turn-based DEVICE form, profiles/r5_turn_trace.json: 8.3 us per turn for cfg4''s 32 rows x 400
            // columns = 20 k cycles for 12.5 items per thread): the loop below is a chain of LDS round trips -- row id, then the value
            // (from the state or from the actions, behind a branch), then the two normaliser doubles, element after element.  Here an
            // item's twelve LDS reads are independent of each other (the value's source is a selected ADDRESS, not a branch) and issued
            // together, the (row, quad) of an item follows from the previous item's by addition; same arithmetic per element.
            const int d_s = kThreads / kq, d_c = kThreads - d_s * kq;
            int s = tid / kq, cq = tid - s * kq;
            for (int i = tid; i < ROWS * kq; i += kThreads) {
                const bool valid = sm.rowid[s] >= 0;
                float xv[4];
                double nm[4], ns[4];
                bool inb[4];
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int c = ((cq >> 2) << 4) + 4 * q + (cq & 3);
                    const int cc = min(c, md.in_dim - 1);
                    const float* src = cc < md.obs_in ? sm.state + s * md.obs_dim + cc : actn_t + s * md.act_dim + (cc - md.obs_in);
                    xv[q] = *src;
                    inb[q] = c < md.in_dim;
                    if constexpr (NORM == HIPETS_NORM_F64) { nm[q] = sm.nmean[cc]; ns[q] = sm.nstd[cc]; }
                }
                f32x4 v;
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    float x = xv[q];
                    if constexpr (NORM == HIPETS_NORM_F64) x = (float)(((double)x - nm[q]) * ns[q]);
                    v[q] = (inb[q] && valid) ? x : 0.f;
                }
                HIPETS_BOUND(s >= 0 && s < ROWS && 4 * cq + 3 < ld_in);
                *reinterpret_cast<f32x4*>(dst + s * ld_in + 4 * cq) = v;
                s += d_s;
                cq += d_c;
                if (cq >= kq) { cq -= kq; ++s; }
            }
            return;
        }
        for (int i = tid; i < ROWS * kq; i += kThreads) {
            const int s = i / kq, cq = i % kq;
            const bool valid = sm.rowid[s] >= 0;
            float v[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int c = kByGroup ? ((cq >> 2) << 4) + 4 * q + (cq & 3) : 4 * cq + q;
                const int cc = min(c, md.in_dim - 1);  // clamped index: loads stay in bounds, result masked below
                float x;
                if (cc < md.obs_in) {
                    if constexpr (PLAIN) x = sm.state[s * md.obs_dim + cc];
                    else x = processed_obs(sm.state + s * md.obs_dim, cc, obs_process, kLean ? nullptr : obs_columns(md));  // (the table: read only by HIPETS_OBS_COLUMNS, which a lean instance never is)
                } else {
                    x = actn_t[s * md.act_dim + (cc - md.obs_in)];
                }
                // f64 normaliser: (x - mean) * (1 / std) with the reciprocal formed once per launch in f64.  Against the reference's
                // f64 division the product is off by <= 1.5 ulp OF F64 before the rounding to f32: the f32 value differs (by one
                // f32 ulp) only when the quotient sits within ~2^-29 of a rounding boundary, ~1e-8 of the elements -- far inside
                // T1 -- and the per-element f64 division sequence (~12 f64 instructions) leaves the per-step critical path
                if constexpr (NORM == HIPETS_NORM_F64) x = (float)(((double)x - sm.nmean[cc]) * sm.nstd[cc]);
                else if constexpr (NORM == HIPETS_NORM_F32) x = (x - (float)sm.nmean[cc]) / (float)sm.nstd[cc];
                v[q] = (c < md.in_dim && valid) ? x : 0.f;
            }
            HIPETS_BOUND(s >= 0 && s < ROWS && 4 * cq + 3 < ld_in);
            if constexpr (kB3) {  // three bf16 pieces per value (bf16: the one), in the B-operand layout of wave_gemm_b3
                u32x2 pc[kNP];
                split_x4<kNP>(f32x4{v[0], v[1], v[2], v[3]}, pc);
                char* row = reinterpret_cast<char*>(dst) + (size_t)s * ld_in * 4;
#pragma unroll
                for (int p = 0; p < kNP; ++p) *reinterpret_cast<u32x2*>(row + b3_offset<kNP>(4 * cq, p)) = pc[p];
            } else if constexpr (kByGroup) {  // columns 16 kk + 4 q + g live at positions 16 kk + 4 g + q: item cq = 4 kk + g writes [4 cq, 4 cq + 3]
                *reinterpret_cast<f32x4*>(dst + s * ld_in + 4 * cq) = f32x4{v[0], v[1], v[2], v[3]};
            } else {
#pragma unroll
                for (int q = 0; q < 4; ++q) dst[s * ld_in + lds_col(4 * cq + q)] = v[q];
            }
        }
    };
    // KSpec::WIDE (cfg4': 32 rows x 400 input columns per pass; f64 normaliser, no obs preprocessing -- facts of the shape): the pass
    // by COLUMN.  A thread owns columns tid, tid + 256, ... for every row: its normaliser constants and LDS position are loaded once
    // per column, consecutive lanes read consecutive state floats (no bank conflict) and write the 64 positions of four whole k chunks
    // (lds_col permutes inside a chunk: no conflict either).  The by-group items above read the four columns {16 kk + 4 q + g} per
    // lane: lanes 16 columns apart meet on a bank -- 4-way conflicts on the state reads, 8-way on the f64 constants -- and the pass
    // measured 7-8 us per turn in the step trace (profiles/r6_turn_trace.json: "arrived -> built"), a tenth of a cfg4' turn in BOTH
    // modes.  Same arithmetic per element: same bits.
    int in_rows = ROWS;  // rows of the input image the next MLP pass reads (kTile in a one-tile turn: "ragged last turn" above)
    auto build_input_cols = [&](const int t, float* const dst) __attribute__((always_inline)) {
        const float* actn_t = sm.actn + (t & 1) * n_act;
        constexpr int kU = 8;  // rows per batch: the batch's LDS reads are issued together
        static_assert(ROWS % kU == 0, "row batches");
        for (int c = tid; c < Kp0; c += kThreads) {
            const bool inb = c < md.in_dim;
            const int cc = min(c, md.in_dim - 1);
            const double nm = sm.nmean[cc], ns = sm.nstd[cc];
            const bool from_state = cc < md.obs_in;
            const float* const src = from_state ? sm.state + cc : actn_t + (cc - md.obs_in);
            const int stride = from_state ? md.obs_dim : md.act_dim;
            float* const out = dst + lds_col(c);
            for (int s0_ = 0; s0_ < in_rows; s0_ += kU) {  // (a one-tile turn of the ragged last turn: row tile 0 only)
                float x[kU];
                int rid[kU];
#pragma unroll
                for (int u = 0; u < kU; ++u) {
                    x[u] = src[(s0_ + u) * stride];
                    rid[u] = sm.rowid[s0_ + u];
                }
#pragma unroll
                for (int u = 0; u < kU; ++u) out[(s0_ + u) * ld_in] = (inb && rid[u] >= 0) ? (float)(((double)x[u] - nm) * ns) : 0.f;
            }
        }
    };
    auto build_input = [&](const int t, float* const dst) __attribute__((always_inline)) {
        using T = std::true_type;
        using F = std::false_type;
        if constexpr (kWide) {  // (KSpec static_assert: WIDE instances have the f64 normaliser and no obs preprocessing)
            build_input_cols(t, dst);
            return;
        }
        const bool plain = obs_process == HIPETS_OBS_NONE;
        switch (normalizer) {
            case HIPETS_NORM_F64:
                if (plain) build_input_impl(t, dst, std::integral_constant<int, HIPETS_NORM_F64>{}, T{});
                else build_input_impl(t, dst, std::integral_constant<int, HIPETS_NORM_F64>{}, F{});
                break;
            case HIPETS_NORM_F32:
                if (plain) build_input_impl(t, dst, std::integral_constant<int, HIPETS_NORM_F32>{}, T{});
                else build_input_impl(t, dst, std::integral_constant<int, HIPETS_NORM_F32>{}, F{});
                break;
            default:
                if (plain) build_input_impl(t, dst, std::integral_constant<int, HIPETS_NORM_NONE>{}, T{});
                else build_input_impl(t, dst, std::integral_constant<int, HIPETS_NORM_NONE>{}, F{});
                break;
        }
    };
    // KSpec::FUSE, FAST form: the obs columns of the next step's input are written by the output layer's tail; the remaining
    // columns of the padded input -- the normalised actions of step t and the zero padding up to Kp0 -- come from here, element
    // by element (column obs_in - 1 and column obs_in may share a quad).  Same arithmetic as build_input_impl.
    // This thread's column of those (<= 16 action + padding columns, the usual case): column obs_in + (tid & 15), rows tid / 16 + 16 q --
    // no division, the column's normaliser constants and LDS position fixed for the launch.
    const int bac_c = md.obs_in + (tid & 15);
    const bool bac_fast = S::FUSE && !kWide && Kp0 - md.obs_in <= 16;
    const bool bac_live = bac_fast && bac_c < md.in_dim;  // an action column (else zero padding, or beyond Kp0: nothing to write)
    double bac_nm = 0.0, bac_ns = 0.0;  // read from LDS once the prologue has put the constants there (below)
    const int bac_pos = lds_col(min(bac_c, Kp0 - 1));
    // (fast path: by the waves 1 .. kWaves - 1 only -- the output layer deals its leftover units to wave 0 first, so the others
    // reach the layer's barrier early by at least one unit's k loop and this work disappears in that slack; 12 rows per pass)
    auto build_action_columns = [&](const int t, float* const dst) __attribute__((always_inline)) {
        const float* actn_t = sm.actn + (t & 1) * n_act;
        if (bac_fast) {
            if (wave != 0 && bac_c < Kp0) {
                constexpr int kRowsPerPass = (kThreads - 64) / 16;
                constexpr int kPasses = (ROWS + kRowsPerPass - 1) / kRowsPerPass;
                const int r0 = (tid - 64) >> 4;
                float x[kPasses];
                int rid[kPasses];
#pragma unroll
                for (int q = 0; q < kPasses; ++q) {  // all LDS reads first: one round trip for the thread's rows
                    const int s = r0 + kRowsPerPass * q;
                    rid[q] = s < ROWS ? act_rows[s] : -1;
                    x[q] = (bac_live && s < ROWS) ? actn_t[s * md.act_dim + (bac_c - md.obs_in)] : 0.f;
                }
#pragma unroll
                for (int q = 0; q < kPasses; ++q) {
                    const int s = r0 + kRowsPerPass * q;
                    if (s < ROWS) dst[s * ld_in + bac_pos] = (bac_live && rid[q] >= 0) ? (float)(((double)x[q] - bac_nm) * bac_ns) : 0.f;
                }
            }
            return;
        }
        const int ntc = Kp0 - md.obs_in;
        for (int i = tid; i < ROWS * ntc; i += kThreads) {
            const int s = i / ntc, c = md.obs_in + (i - s * ntc);
            float v = 0.f;
            if (c < md.in_dim && act_rows[s] >= 0) {
                const float x = actn_t[s * md.act_dim + (c - md.obs_in)];
                v = (float)(((double)x - sm.nmean[c]) * sm.nstd[c]);  // KSpec::FUSE instances: f64 normaliser (static_assert in KSpec)
            }
            dst[s * ld_in + lds_col(c)] = v;
        }
    };

    {   // the first step's actions are in flight while the state / totals / flags are fetched: one round trip for all of it
        // (the per-step launches of EXACT / DEVICE mode pay this prologue every step)
        float av[kPrefetch];
        fetch_actions_issue(ra.t_begin, av);
        load_initial_state();
        fetch_actions_commit(ra.t_begin, av);
    }
    __syncthreads();
    if (bac_live) { bac_nm = sm.nmean[bac_c]; bac_ns = sm.nstd[bac_c]; }
    if constexpr (kB3) kq = sm.lmeta[0].Kp32 >> 2;
    build_input(ra.t_begin, sm.buf0);
    __syncthreads();
    prof.mark(0);
    float* step_in = sm.buf0;  // LDS image of the current step's model input (KSpec::FUSE: alternates, see the output layer below)

    // Persistent DEVICE form with more logical workgroups than launched ones: within every step this workgroup serves its
    // logical workgroups in turn (sequence index q = step * n_serve + turn); each turn collects its rows from the hand-over
    // table, runs the step, publishes.  Only a step's first turn can find rows missing (published by other workgroups' last
    // turns of the previous step); the later turns' rows arrived while the earlier ones computed.
    const int n_serve = persist ? (n_logical - wg + (int)gridDim.x - 1) / (int)gridDim.x : 1;
    const int n_seq = (ra.t_end - ra.t_begin) * n_serve;
    int stamp_seq = 0;  // (profiling builds: index of the current (step, turn) for HIPETS_STAMP)
    (void)stamp_seq;
    // Straight persistent form (KSpec::FUSE instances, every launched workgroup serving exactly one logical workgroup, >= 3 hidden
    // layers): see the step loop.  The slot's rows of the current and of the next step live in two LDS arrays that swap roles.
    const bool straight = S::FUSE && !kWide && persist && ra.n_logical == (int)gridDim.x && md.n_layers >= 4;
    int* const rows_a = sm.rowid;
    int* const rows_b = sm.pend + ROWS;
    // fused hopper termination, persistent DEVICE form: per-row "the state this row arrived with is unhealthy" flags, raised by the
    // collecting threads, consumed by the next tail (the fused instances never use sm.lrew: the learned reward stays in registers)
    int* const hop_flags = reinterpret_cast<int*>(sm.lrew);
    // Collect the rows `rows` holds (published by their previous owners in step t_next - 1): every thread polls its (row slot, pair)
    // items as in the general form below, and the thread that receives a pair of state dims also writes them -- normalised exactly
    // like build_input_impl's f64 form -- into the next step's input image: no separate input pass, two barriers less per step.
    auto collect_straight = [&](const int t_next, const int* const rows, float* const dst) __attribute__((always_inline)) {
        const unsigned want = ra.tag_base + (unsigned)t_next;
        for (int base = 0; base < ROWS * NVP; base += kG * kThreads) {
            const unsigned long long* src[kG];
            u32x4g g[kG];
            int gs[kG], gv[kG];
            bool soft[kG], live[kG];
            double nm[kG][2], ns[kG][2];
#pragma unroll
            for (int q = 0; q < kG; ++q) {
                const int i = base + tid + q * kThreads;
                gs[q] = base == 0 ? xs[q] : (i < ROWS * NVP ? i / NVP : -1);
                gv[q] = base == 0 ? xv[q] : (i < ROWS * NVP ? i - (i / NVP) * NVP : 0);
                soft[q] = gv[q] == NVP - 1;
                src[q] = nullptr;
                live[q] = false;
                g[q] = u32x4g{0u, want, 0u, want};
                if (gs[q] >= 0) {
                    const int rid = rows[gs[q]];
                    if (rid >= 0) { src[q] = ra.exchange + (size_t)rid * NV + 2 * gv[q]; live[q] = true; }
                }
                // the normaliser constants of the input columns the pair's two dims feed (ObsMap): requested now, used when the pair has arrived
                const int d = soft[q] ? 0 : 2 * gv[q];
                const int i0 = max(0, min(ObsMap<S::OBSP>::col(d), md.obs_in - 1)), i1 = max(0, min(ObsMap<S::OBSP>::col(d + 1), md.obs_in - 1));
                nm[q][0] = sm.nmean[i0]; nm[q][1] = sm.nmean[i1];
                ns[q][0] = sm.nstd[i0]; ns[q][1] = sm.nstd[i1];
            }
            const long long t_poll = wall_clock64();
            for (int spins = 0;; ++spins) {
                static_assert(kG == 2, "the wait below names the two destinations");
                u32x4g got[kG];
                pair_load_issue(got[0], src[0] ? src[0] : ra.exchange);
                pair_load_issue(got[1], src[1] ? src[1] : ra.exchange);
                asm volatile("s_waitcnt vmcnt(0)" : "+v"(got[0]), "+v"(got[1])::"memory");
                bool ready = true;
#pragma unroll
                for (int q = 0; q < kG; ++q)
                    if (src[q]) {
                        g[q] = got[q];
                        if (got[q][1] == want && got[q][3] == want) src[q] = nullptr;
                        else if (!soft[q]) ready = false;
                    }
                if (ready) break;
                if (poll_gave_up(spins, t_poll)) break;
                __builtin_amdgcn_s_sleep(8);
            }
#pragma unroll
            for (int q = 0; q < kG; ++q)
                if (gs[q] >= 0) {
                    HIPETS_BOUND(gs[q] < ROWS && gv[q] >= 0 && gv[q] < NVP);
                    if (!soft[q]) {
                        using OM = ObsMap<S::OBSP>;
                        const int d = 2 * gv[q];
                        const float v0 = __uint_as_float(g[q][0]), v1 = __uint_as_float(g[q][2]);
                        float x0 = v0, x1 = v1;
                        if constexpr (OM::kTrigDim >= 0) {
                            if (d == OM::kTrigDim || d + 1 == OM::kTrigDim) {  // this thread holds the dim that enters as sin and cos (processed_obs's sinf / cosf)
                                const float tv = d == OM::kTrigDim ? v0 : v1;
                                const float sv = sinf(tv), cv = cosf(tv);
                                if (d == OM::kTrigDim) x0 = sv; else x1 = sv;
                                dst[gs[q] * ld_in + lds_col(OM::kCosCol)] = live[q] ? (float)(((double)cv - sm.nmean[OM::kCosCol]) * sm.nstd[OM::kCosCol]) : 0.f;
                            }
                        }
                        if constexpr (S::TERM == HIPETS_TERM_HOPPER) {
                            if (live[q] && hopper_pair_bad(d, v0, v1, true, d + 1 < md.obs_dim)) hop_flags[gs[q]] = 1;
                        }
                        const int c0 = OM::col(d), c1 = OM::col(d + 1);
                        sm.state[gs[q] * md.obs_dim + d] = v0;
                        if (c0 >= 0) dst[gs[q] * ld_in + lds_col(c0)] = live[q] ? (float)(((double)x0 - nm[q][0]) * ns[q][0]) : 0.f;
                        if (d + 1 < md.obs_dim) {
                            sm.state[gs[q] * md.obs_dim + d + 1] = v1;
                            if (c1 >= 0) dst[gs[q] * ld_in + lds_col(c1)] = live[q] ? (float)(((double)x1 - nm[q][1]) * ns[q][1]) : 0.f;
                        }
                    } else if (src[q]) {
                        sm.pend[gs[q]] = 1;  // not there yet: the next tail fetches the pair
                    } else {
                        sm.tot[gs[q]] = __uint_as_float(g[q][0]);
                        sm.term[gs[q]] = (int)g[q][2];
                    }
                }
        }
        HIPETS_STAMP(2, t_next - 1);  // this thread's rows have arrived
    };
    // ---- KSpec::WIDE: collect the rows `sm.rowid` names (published with tag `want`) by LDS-DMA ---------------------------------------
    // Wave w owns the row slots w, w + kWaves, ... from issue to commit: a row's NVP pairs are CPR = ceil(NVP / 64) chunks of 64 (1 KiB
    // of staging each; slot s, chunk k sits at staging chunk s CPR + k), the row id is wave-uniform, a lane's source is the row's base +
    // its pair -- no division, no per-lane row lookup (the first version dealt chunks of 64 CONSECUTIVE items to the waves and paid an
    // LDS round trip for the row id and a multiply-high per chunk and lane: 12.2 us per collect against the register path's 9.6,
    // profiles/r6_turn_trace.json).  The wave's own s_waitcnt vmcnt(0) is all that orders its ds_reads behind its DMAs (no barrier).  A
    // chunk with a lane whose pair has not been published yet (its tags are an earlier step's) is fetched again; only a step's first
    // turn can see that.  The {running total, flag} pair of a row gets one look per pass and is left to the next tail if late
    // (sm.pend), exactly like the register path.
    auto dma_collect = [&](const unsigned want) __attribute__((always_inline)) {
        // chunks per row: a compile-time fact of the WIDE shapes (47 output column tiles <=> obs 369..376 <=> 186..189 pairs <=> 3 chunks)
        constexpr int CPR = kWide ? (((S::OUTC > 0 ? S::OUTC : 1) * 8 + 1) / 2 + 1 + 63) / 64 : 1;
        constexpr int kRowsPerWave = ROWS / kWaves;
        static_assert(ROWS % kWaves == 0 && kRowsPerWave * CPR <= 32, "row slots are dealt to the waves; one pending bit per (row, chunk)");
        const int n_main = (int)(act_bytes(ROWS, ld_in, ld_k) >> 10);  // chunks that fit buf0 + buf1 (contiguous)
        char* const stage0 = reinterpret_cast<char*>(sm.buf0);
        HIPETS_BOUND(CPR == (NVP + 63) / 64 && (size_t)max(ROWS * CPR - n_main, 0) * 1024 <= stage_extra_bytes(ROWS, ld_in, ld_k, md.obs_dim));
        auto chunk_ptr = [&](const int c) __attribute__((always_inline)) { return c < n_main ? stage0 + ((size_t)c << 10) : sm.stage_x + ((size_t)(c - n_main) << 10); };
        auto lds_of = [&](const int c) __attribute__((always_inline)) { return (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)(size_t)chunk_ptr(c)); };
        unsigned pending = 0;  // bit j CPR + k: chunk k of this wave's j-th row still has a lane waiting
        int rids[kRowsPerWave];
#pragma unroll
        for (int j = 0; j < kRowsPerWave; ++j) rids[j] = sm.rowid[wave + kWaves * j];  // (all of the wave's row ids in one LDS round trip)
#pragma unroll
        for (int j = 0; j < kRowsPerWave; ++j) {
            const int s = wave + kWaves * j;
            const int rid = __builtin_amdgcn_readfirstlane(rids[j]);
            rids[j] = rid;
            if (rid >= 0) {
                const unsigned long long* const row = ra.exchange + (size_t)rid * NV;
#pragma unroll
                for (int k = 0; k < CPR; ++k) {
                    const int v = min(64 * k + lane, NVP - 1);  // (lanes beyond the row's last pair fetch it again and ignore it)
                    pair_dma_issue(row + 2 * v, lds_of(s * CPR + k));
                }
                pending |= ((1u << CPR) - 1u) << (j * CPR);
            } else {  // a row of the padding: zero state, total, flag
                for (int d = lane; d < md.obs_dim; d += 64) sm.state[s * md.obs_dim + d] = 0.f;
                if (lane == 0) { sm.tot[s] = 0.f; sm.term[s] = 0; sm.pend[s] = 0; }
            }
        }
        const long long t_poll = wall_clock64();
        for (int spins = 0; pending; ++spins) {
            vmem_drain();  // this wave's DMAs have landed
            unsigned still = 0;
#pragma unroll
            for (int j = 0; j < kRowsPerWave; ++j) {
                if (!((pending >> (j * CPR)) & ((1u << CPR) - 1u))) continue;  // (wave-uniform) nothing of this row is waiting
                const int s = wave + kWaves * j;
                u32x4g g[CPR];
#pragma unroll
                for (int k = 0; k < CPR; ++k) g[k] = *reinterpret_cast<const u32x4g*>(chunk_ptr(s * CPR + k) + lane * 16);  // the row's chunks in one LDS round trip
#pragma unroll
                for (int k = 0; k < CPR; ++k) {
                    if (!((pending >> (j * CPR + k)) & 1u)) continue;  // (wave-uniform)
                    const int v = 64 * k + lane;
                    const bool mine = v < NVP, soft = v == NVP - 1;
                    const bool ok = g[k][1] == want && g[k][3] == want;
                    HIPETS_BOUND(s < ROWS);
                    if (mine && !soft) {
                        if (ok) {
                            const int d = 2 * v;
                            sm.state[s * md.obs_dim + d] = __uint_as_float(g[k][0]);
                            if (d + 1 < md.obs_dim) sm.state[s * md.obs_dim + d + 1] = __uint_as_float(g[k][2]);
                        }
                    } else if (soft) {
                        if (ok) {
                            sm.tot[s] = __uint_as_float(g[k][0]);
                            sm.term[s] = (int)g[k][2];
                        }
                        sm.pend[s] = ok ? 0 : 1;  // not there yet: the next tail fetches the pair
                    }
                    if (__builtin_amdgcn_ballot_w64(mine && !soft && !ok) != 0) {  // somebody's state pair is still an earlier step's: fetch the chunk again
                        still |= 1u << (j * CPR + k);
                        pair_dma_issue(ra.exchange + (size_t)rids[j] * NV + 2 * min(v, NVP - 1), lds_of(s * CPR + k));
                    }
                }
            }
            pending = still;
            if (!pending) break;
            if (poll_gave_up(spins, t_poll)) {
                vmem_drain();  // nothing of this wave may still be landing in the activation buffers when the flow goes on
                break;
            }
            __builtin_amdgcn_s_sleep(8);
        }
    };
    (void)dma_collect;

    // KSpec::RES: the launch rule (launch.hpp resident_heads_call, rollout.hip) picks this instance for the straight persistent form only.
    // This wave's op heads of its member -- fixed for the launch -- go into AccVGPRs once, here (the layer table is in LDS since the
    // prologue's barrier); every step's ops start from them (gemm_f32.hpp ResHead).
    static_assert(!S::RES || (R == 3 && MinWaves<R, S>::value == 1), "resident op heads: one wave per SIMD (512 registers per lane)");
    ResHeadStore<S::RES> head_store;  // (empty in every other instance)
    ResHead* const heads = head_store.get();
    if constexpr (S::RES) {
        if (!straight || md.n_layers != kResLayers) {  // (never launched like this; a launch that is, fails loudly instead of computing with another form's heads)
            if (tid == 0 && ra.error_flag) *ra.error_flag = 1;
            return;
        }
        res_load_heads<R, S>(heads, md, sm.lmeta, member_dom, wave, lane);
        vmem_drain();
        res_pin_heads<R, S>(heads);
    }
    bool one_tile = false;  // this turn serves a one-tile logical workgroup (kRagged; workgroup-uniform)
    for (int q_seq = 0; q_seq < n_seq; ++q_seq) {
        stamp_seq = q_seq;
        const int t = ra.t_begin + q_seq / n_serve;
        const bool more = t + 1 < ra.t_end;
        const bool has_next = q_seq + 1 < n_seq;  // persistent form: another (step, turn) follows
        const int t_next = ra.t_begin + (q_seq + 1) / n_serve;
        const int v_next = wg + ((q_seq + 1) - ((q_seq + 1) / n_serve) * n_serve) * (int)gridDim.x;  // its logical workgroup
        float av[kPrefetch];
        if (more && !persist) fetch_actions_issue(t + 1, av);  // consumed after the sampling phase: the HBM / L2 latency hides behind the MLP
        unsigned long long* const handover = (more && persist) ? ra.exchange : nullptr;
        const unsigned long long handover_tag = (unsigned long long)(ra.tag_base + (unsigned)t + 1u) << 32;  // tags never repeat across launches
        if constexpr (S::FUSE) {
            // ---- KSpec::FUSE: hidden layers as usual; the OUTPUT layer's accumulators go straight into the step's tail ----------
            const int member = fast ? __builtin_amdgcn_readfirstlane(sm.sched[t]) : member_dom;  // wave-uniform
            float* cur = step_in;
            float* nxt = step_in == sm.buf0 ? sm.buf1 : sm.buf0;
            const int L = md.n_layers;
            const bool write_input = more && !persist && !kWide;  // FAST form: rows stay here, the next step's input is built in place
            const bool wide_fast_next = kWide && more && !persist;  // WIDE: buf0 is the input image AND an activation buffer: the input is built after the step
            // Straight persistent form (every launched workgroup serves ONE logical workgroup): everything of step t + 1 that does
            // not depend on the rows' states is prepared while step t computes -- which rows the slot holds then (the step's keyed
            // permutation, evaluated beside layer 1 by the wave with the lightest GEMM share), their actions (fetched behind layer 2, in LDS before
            // the output layer, their input columns built beside it) -- so that between the output layer and the next step there
            // is only: barrier, wait for the rows, normalise them into the input image as they arrive, barrier.
            const bool prep_next = straight && more;
            int* const rows_nxt = sm.rowid == rows_a ? rows_b : rows_a;
            for (int l = 0; l + 1 < L; ++l) {
                // the raw actions of step t + 1 (requested at the top of the step) go to their LDS buffer now: visible to every
                // thread after this layer's barrier, i.e. when the output layer starts
                prof.mark(12);
                if (l == 1 && prep_next && wave == kWaves - 1) {  // this wave's share of a hidden layer is one unit short: room for the permutation
                    for (int s = lane; s < ROWS; s += 64) {
                        const int j = (wg % ra.groups) * ROWS + s;
                        rows_nxt[s] = j < ra.rows_per_domain
                                          ? (int)perm_apply((unsigned)(domain * ra.rows_per_domain + j), ra.perm_n, ra.perm_a, ra.perm_b, ra.step_keys[t + 1]) : -1;
                    }
                }
                if (l == 2 && prep_next) {  // rows_nxt is visible since layer 1's barrier
                    act_rows = rows_nxt;
                    compute_act_base();
                    fetch_actions_issue(t + 1, av);
                }
                if (l == L - 2 && (write_input || prep_next || wide_fast_next)) fetch_actions_commit(t + 1, av);
                if constexpr (kRagged) {
                    if (one_tile) mlp_layer<1, S>(md, sm.lmeta, l, member, cur, nxt, wave, lane, prof, sm.part);
                    else mlp_layer<R, S>(md, sm.lmeta, l, member, cur, nxt, wave, lane, prof, sm.part);
                } else {
                    mlp_layer<R, S>(md, sm.lmeta, l, member, cur, nxt, wave, lane, prof, sm.part, heads);
                }
                __syncthreads();
                prof.mark(8);
                float* tmp = cur; cur = nxt; nxt = tmp;
            }
            // `nxt` (the output layer's would-be LDS image) is read by nobody while the output layer runs: it receives the next
            // step's model input -- action columns and zero padding from all threads here, the obs columns from the tail lanes
            // (FAST) / from the threads that receive the rows (straight persistent form)
            if (write_input || (prep_next && !kWide)) build_action_columns(t + 1, nxt);
            const float* const actn_t = sm.actn + (t & 1) * n_act;
            const unsigned handover_tg = (unsigned)(handover_tag >> 32);
            // One finished accumulator = column tile c, row tile r of the head-pair pack: this lane (group g, row j) holds
            // {mean d0, mean d0 + 1, logvar d0, logvar d0 + 1} of batch row s = 16 r + j for d0 = 8 c + 2 g.  Same arithmetic, op for
            // op, as the LDS-based phases of the other instances (sample_impl / reward phase / build_input_impl below): the
            // shape-specialised and the generic kernels return the same bits.  BRANCH-FREE on purpose: every lane computes, loads
            // use clamped indices, stores of inactive lanes go to a dump slot -- so the two or three tails of a wave are one
            // basic block and the scheduler overlaps their LDS round trips instead of paying them one after the other.
            auto tail_prep = [&](FusedSlot& q, const int c, const int r) __attribute__((always_inline)) {
                const int s = r * kTile + (lane & 15);
                const int d0 = 8 * c + 2 * (lane >> 4);
                const int dA = min(d0, md.out_dim - 1), dB = min(d0 + 1, md.out_dim - 1);  // clamped: loads stay in bounds
                const int oA = min(d0, md.obs_dim - 1), oB = min(d0 + 1, md.obs_dim - 1);
                q.rid = sm.rowid[s];
                q.mxA = sm.maxlv[dA]; q.mxB = sm.maxlv[dB]; q.mnA = sm.minlv[dA]; q.mnB = sm.minlv[dB];
                q.pA = sm.state[s * md.obs_dim + oA]; q.pB = sm.state[s * md.obs_dim + oB];
                q.ndA = sm.nodelta[oA]; q.ndB = sm.nodelta[oB];
                // the normaliser constants of the input COLUMNS the two dims feed (obs preprocessing moves them: ObsMap)
                using OM = ObsMap<S::OBSP>;
                const int iA = max(0, min(OM::col(d0), md.obs_in - 1)), iB = max(0, min(OM::col(d0 + 1), md.obs_in - 1));
                q.nmA = sm.nmean[iA]; q.nmB = sm.nmean[iB]; q.nsA = sm.nstd[iA]; q.nsB = sm.nstd[iB];
            };
            // The standard normals of two units at once.  A lane's two dims (d0 = 8 c + 2 g, d0 + 1) take HALF of Philox block (row, step,
            // d0 / 4) -- x, y for an even lane group g, z, w for an odd one (exactly rollout_normals4's assignment) -- and the other half
            // belongs to the lane 16 further (g ^ 1: same row, the block's other two dims).  Until round 6 every lane computed the whole
            // block of every unit and dropped half of it (the ten rounds are half of a unit's VALU time).  Now, for a PAIR of units (a, b),
            // the even lane groups compute a's block and the odd ones b's, and each lane fetches the half it lacks from its partner's
            // registers (two ds_bpermute): one block per lane and pair instead of two.  Same blocks, same halves, same Box-Muller: same bits.
            // A group's odd unit out (`two` false) draws as before.  Three instances keep the draw inside tail_unit: the two-tile DEVICE-mode
            // instances with obs preprocessing or a learned reward (pets_halfcheetah, pets_pusher / pets_reacher, pets_mppi_halfcheetah in
            // DEVICE mode) sit at the 256-register limit of two workgroups per CU, and with the pair's exchange they spilt 3-14 registers to
            // scratch memory (the build's resource report; pets_halfcheetah 0.498 -> 0.487 of peak; tests/test_abi.py allows no kernel any).
            constexpr bool kPairDraws = !(MinWaves<R, S>::value == 2 && R == 2 && S::KMODE != HIPETS_MODE_FAST && (S::OBSP != HIPETS_OBS_NONE || S::REW == HIPETS_REW_LEARNED));
            auto unit_draw = [&](const int rid, const int c, float& n0, float& n1) __attribute__((always_inline)) {  // one unit, the whole block per lane
                const int g = lane >> 4;
                const bool odd = (g & 1) != 0;
                const Philox4 r4 = philox4x32_10((uint32_t)rid, (uint32_t)t, (uint32_t)((8 * c + 2 * g) >> 2), (uint32_t)ra.stream_id, (uint32_t)ra.seed,
                                                 (uint32_t)(ra.seed >> 32) ^ (uint32_t)(ra.stream_id >> 32));
                box_muller(odd ? r4.z : r4.x, odd ? r4.w : r4.y, n0, n1);
            };
            auto tail_draw = [&](FusedSlot& qa, FusedSlot& qb, const int ca, const int cb, const bool two) __attribute__((always_inline)) {
#ifndef HIPETS_TIMING_NO_DRAWS
#define HIPETS_TIMING_NO_DRAWS 0  // 1 = TIMING-ONLY builds (results are wrong on purpose): the tail draws nothing -- an upper bound of what moving
#endif                            // the draws off the step's critical path (e.g. into the hand-over wait) could gain; profiles/headline_probe.py
                if constexpr (HIPETS_TIMING_NO_DRAWS) {
                    qa.n0 = 0.37f + 1e-3f * (float)(qa.rid & 7);
                    qa.n1 = -0.81f;
                    qb.n0 = 0.37f + 1e-3f * (float)(qb.rid & 7);
                    qb.n1 = -0.81f;
                    return;
                }
                if constexpr (!kPairDraws) return;  // (drawn by tail_unit)
                const int g = lane >> 4;
                const bool odd = (g & 1) != 0;
                const uint32_t k0 = (uint32_t)ra.seed, k1 = (uint32_t)(ra.seed >> 32) ^ (uint32_t)(ra.stream_id >> 32);
                if (!two) {
                    unit_draw(qa.rid, ca, qa.n0, qa.n1);
                    return;
                }
                const Philox4 r4 = philox4x32_10((uint32_t)(odd ? qb.rid : qa.rid), (uint32_t)t, (uint32_t)((8 * (odd ? cb : ca) + 2 * g) >> 2),
                                                 (uint32_t)ra.stream_id, k0, k1);
                // what the partner lacks of this lane's block: an even lane holds a's block, its (odd) partner wants z, w; an odd lane
                // holds b's block, its (even) partner wants x, y
                const int partner = ((lane ^ 16) & 63) << 2;
                const uint32_t t0 = (uint32_t)__builtin_amdgcn_ds_bpermute(partner, (int)(odd ? r4.x : r4.z));
                const uint32_t t1 = (uint32_t)__builtin_amdgcn_ds_bpermute(partner, (int)(odd ? r4.y : r4.w));
                box_muller(odd ? t0 : r4.x, odd ? t1 : r4.y, qa.n0, qa.n1);  // unit a: (x, y) of a's block on even lanes, (z, w) -- from the partner -- on odd ones
                box_muller(odd ? r4.z : t0, odd ? r4.w : t1, qb.n0, qb.n1);  // unit b: (x, y) of b's block -- from the partner -- on even lanes, (z, w) on odd ones
            };
            auto tail_unit = [&](const FusedSlot& q, const f32x4 a, const int c, const int r) __attribute__((always_inline)) {
                const int g = lane >> 4, j = lane & 15;
                const int s = r * kTile + j;
                const int d0 = 8 * c + 2 * g;
                const int rid = q.rid;
                HIPETS_BOUND(s >= 0 && s < ROWS && r >= 0 && r < R && c >= 0 && 16 * c < 2 * md.out_dim + 16 && rid < ra.B);
                const bool okA = rid >= 0 && d0 < md.obs_dim, okB = rid >= 0 && d0 + 1 < md.obs_dim;
                const float mxA = q.mxA, mxB = q.mxB, mnA = q.mnA, mnB = q.mnB, pA = q.pA, pB = q.pB;
                const bool addA = md.target_is_delta && !q.ndA, addB = md.target_is_delta && !q.ndB;
                const double nmA = q.nmA, nmB = q.nmB, nsA = q.nsA, nsB = q.nsB;
                float n0 = q.n0, n1 = q.n1;  // the two normals of (row, step, dims d0, d0 + 1): tail_draw ...
                if constexpr (!kPairDraws && !HIPETS_TIMING_NO_DRAWS) unit_draw(rid, c, n0, n1);  // ... or drawn here (two workgroups per CU)
                float lvA = a[2], lvB = a[3];
                lvA = mxA - softplus_fast(mxA - lvA);  // gaussian_mlp.py:152
                lvB = mxB - softplus_fast(mxB - lvB);
                lvA = mnA + softplus_fast(lvA - mnA);  // :153
                lvB = mnB + softplus_fast(lvB - mnB);
                const float predA = a[0] + __builtin_amdgcn_sqrtf(exp_hw(lvA)) * n0;  // model.py:471-473
                const float predB = a[1] + __builtin_amdgcn_sqrtf(exp_hw(lvB)) * n1;
                const float vA = predA + (addA ? pA : 0.f);  // one_dim_tr_model.py:281-286 (0 for no_delta dims)
                const float vB = predB + (addB ? pB : 0.f);
                sm.state[okA ? s * md.obs_dim + d0 : (int)(sm.dump - sm.state)] = vA;
                sm.state[okB ? s * md.obs_dim + d0 + 1 : (int)(sm.dump - sm.state) + 1] = vB;
                if (write_input) {  // wave-uniform; build_input_impl's f64 form (the columns ObsMap names: input column d = obs dim d without preprocessing)
                    using OM = ObsMap<S::OBSP>;
                    const int cA = OM::col(d0), cB = OM::col(d0 + 1);
                    float xA = vA, xB = vB;
                    if constexpr (OM::kTrigDim >= 0) {
                        if (c == 0) {  // wave-uniform: the trig dim lives in column tile 0.  Same sinf / cosf as processed_obs: same bits as the generic kernel
                            const bool trigA = d0 == OM::kTrigDim, trigB = d0 + 1 == OM::kTrigDim;
                            const float tv = trigA ? vA : vB;
                            const float sv = sinf(tv), cv = cosf(tv);
                            xA = trigA ? sv : xA;
                            xB = trigB ? sv : xB;
                            const bool okT = (trigA && okA) || (trigB && okB);
                            nxt[okT ? s * ld_k + lds_col(OM::kCosCol) : (int)(sm.dump - nxt) + 1] = (float)(((double)cv - sm.nmean[OM::kCosCol]) * sm.nstd[OM::kCosCol]);
                        }
                    }
                    nxt[(okA && cA >= 0) ? s * ld_k + lds_col(max(cA, 0)) : (int)(sm.dump - nxt) + 2] = (float)(((double)xA - nmA) * nsA);
                    nxt[(okB && cB >= 0) ? s * ld_k + lds_col(max(cB, 0)) : (int)(sm.dump - nxt) + 3] = (float)(((double)xB - nmB) * nsB);
                }
                const unsigned pubA = okA ? __float_as_uint(vA) : 0u, pubB = okB ? __float_as_uint(vB) : 0u;
                // persistent DEVICE form: the row's next owner waits for these values.  Under a real (divergent) predicate: redirecting
                // the inactive lanes' stores to one spare row instead made every workgroup's write-through stores queue on ONE
                // address (measured: 1.375 vs 1.081 ms per cfg2 rollout)
                if (handover && okA) pair_store(handover + (size_t)rid * NV + d0, pubA, pubB, handover_tg);
                // Reward, termination, masked accumulation (model_env.py:124-129, :186-188) by ONE lane per row: closed forms -- the lane
                // that holds dims 0, 1 of the row (dims 2, 3 sit in the next lane group of the same accumulator); learned rewards -- the
                // lane that holds output column obs_dim, whose sampled value IS the reward (one_dim_tr_model.py:287).  (A wave can hold
                // several such units -- one per row tile when the output layer has >= 4 column tiles -- hence here, per unit.)
                constexpr bool kLearnedRew = S::REW == HIPETS_REW_LEARNED;
                constexpr bool kAllDims = S::TERM == HIPETS_TERM_HOPPER;  // every lane judges its own dims; flags through LDS, folded in one step later (KSpec)
                constexpr bool kRewLane = kLearnedRew && (S::TERM == HIPETS_TERM_NONE || kAllDims);  // the reward column's lane keeps the total (else: the lane with dims 0, 1)
                if constexpr (kAllDims) {  // hopper: all dims finite, |dims 1..| < 100, height (dim 0) > 0.7, |angle (dim 1)| < 0.2
                    // (persistent form: the row's next owner judges the dims it receives -- collect phases below)
                    if (!persist && hopper_pair_bad(d0, vA, vB, okA, okB)) sm.pend[(t & 1) * ROWS + s] = 1;  // (every writer stores the same value; read after this step's barrier)
                }
                const int c_rew = kRewLane ? (md.obs_dim >> 3) : 0, g_rew = kRewLane ? ((md.obs_dim & 7) >> 1) : 0;
                if (c == c_rew) {  // wave-uniform
                    float st[4] = {0.f, 0.f, 0.f, 0.f};
                    float lrew = (md.obs_dim & 1) ? predB : predA;  // the learned reward, on the lane that holds output column obs_dim (= sample_impl's sm.lrew[s])
                    if constexpr (!kRewLane) {
                        st[0] = okA ? vA : 0.f;
                        st[1] = okB ? vB : 0.f;
                        st[2] = __uint_as_float((unsigned)__builtin_amdgcn_ds_bpermute(((lane + 16) & 63) << 2, (int)pubA));
                        st[3] = __uint_as_float((unsigned)__builtin_amdgcn_ds_bpermute(((lane + 16) & 63) << 2, (int)pubB));
                        if constexpr (kLearnedRew)  // column obs_dim sits (md.obs_dim & 7) / 2 lane groups further in this accumulator
                            lrew = __uint_as_float((unsigned)__builtin_amdgcn_ds_bpermute(((lane + 16 * ((md.obs_dim & 7) >> 1)) & 63) << 2, (int)__float_as_uint(lrew)));
                    }
                    if (g == g_rew && rid >= 0) {
                        float tot = sm.tot[s];
                        int trm = sm.term[s];
                        if (persist && sm.pend[s]) {  // collected late
                            sm.pend[s] = 0;
                            fetch_late_total(rid, t, tot, trm);
                        }
                        float rwd;
                        if constexpr (kLearnedRew) rwd = lrew;
                        else rwd = reward_eval(st, actn_t + s * md.act_dim, 4, md.act_dim, S::REW, 0.f);
                        bool done = false;
                        if constexpr (kAllDims) {  // `terminated` up to and including step t - 1: that step's flag is complete since its barrier
                            if (persist) {  // raised by the threads that collected this row's state (the state step t - 1 left)
                                trm = trm | hop_flags[s];
                                hop_flags[s] = 0;  // (raised again by the next collect phase: a barrier away)
                            } else {
                                int* const flag = sm.pend + ((t & 1) ^ 1) * ROWS + s;
                                trm = trm | (t > ra.t_begin ? *flag : 0);
                                *flag = 0;  // (raised again in step t + 1 at the earliest: two barriers away)
                            }
                        } else {
                            done = term_eval(st, 4, S::TERM);
                        }
                        end_step_for_row(s, rid, tot, trm, rwd, done, handover, handover_tg);
                    }
                }
            };
            auto tail_finish = [&]() __attribute__((always_inline)) {};
            const auto tail = make_tail(tail_prep, tail_draw, tail_unit, tail_finish);
            prof.mark(12);
            if constexpr (kRagged) {
                if (one_tile) mlp_output_layer_fused<1, S>(md, sm.lmeta, member, cur, wave, lane, prof, tail, sm.part);
                else mlp_output_layer_fused<R, S>(md, sm.lmeta, member, cur, wave, lane, prof, tail, sm.part);
            } else {
                mlp_output_layer_fused<R, S>(md, sm.lmeta, member, cur, wave, lane, prof, tail, sm.part, heads);
            }
            // straight persistent form: what the two sides of this barrier exchange goes through LDS; the tail's write-through
            // hand-over stores need not have been acknowledged (__syncthreads() would wait for that -- about a microsecond --
            // before the first poll for the incoming rows is even issued; this way the two round trips overlap)
            if (prep_next) lds_barrier();
            else __syncthreads();
            prof.mark(8);
            HIPETS_STAMP(0, t);  // the MLP and the step's tail are done
            step_in = kWide ? sm.buf0 : nxt;
            if (wide_fast_next) {  // the tail wrote the new states; the input image of step t + 1 from them (buf0 is free again)
                build_input(t + 1, step_in);
                __syncthreads();
            }
            if (prep_next) {
                HIPETS_STAMP(1, t);
                if (kWide) build_action_columns(t + 1, step_in);  // (not beside the output layer: buf0 may be the buffer it reads)
                collect_straight(t + 1, rows_nxt, step_in);
                sm.rowid = rows_nxt;  // the slot's rows from here on
                __syncthreads();
                HIPETS_STAMP(3, t);
                continue;
            }
            if (persist && has_next) {  // the slot's row in the next turn (the tail above was the last reader of this turn's rowid)
                int nd, nj0, nlive;
                logical_rows(v_next, nd, nj0, nlive);
                if constexpr (kRagged) {
                    one_tile = nlive < ROWS;
                    in_rows = nlive;
                }
                for (int s = tid; s < ROWS; s += kThreads) {
                    const int j = nj0 + s;
                    sm.rowid[s] = (s < nlive && j < ra.rows_per_domain)
                                      ? (int)perm_apply((unsigned)(nd * ra.rows_per_domain + j), ra.perm_n, ra.perm_a, ra.perm_b, ra.step_keys[t_next]) : -1;
                    sm.lrew[s] = 0.f;
                }
                __syncthreads();
            }
        } else {
            const int n_run = expectation ? md.M : 1;
            float* result = nullptr;
            int member = 0;
            for (int mi = 0; mi < n_run; ++mi) {
                if (expectation) member = mi;
                else if (fast) member = __builtin_amdgcn_readfirstlane(sm.sched[t]);  // wave-uniform: weight pointers stay in SGPRs
                else member = member_dom;
                if (mi > 0) {  // expectation: layer 1 overwrote buf0, rebuild the same input for the next member
                    build_input(t, sm.buf0);
                    __syncthreads();
                }
                // ---- the MLP: ping-pong through LDS ------------------------------------------------
                float* cur = sm.buf0;
                float* nxt = sm.buf1;
                for (int l = 0; l < md.n_layers; ++l) {
                    prof.mark(12);
                    if constexpr (kB3) {
                        mlp_layer_b3<R, S>(md, sm.lmeta, l, member, cur, nxt, wave, lane);
                        __syncthreads();
                    } else {
                        mlp_layer<R, S>(md, sm.lmeta, l, member, cur, nxt, wave, lane, prof);
                        __syncthreads();
                    }
                    prof.mark(8);
                    float* tmp = cur; cur = nxt; nxt = tmp;
                }
                result = cur;

                if (expectation) {  // gaussian_mlp.py:213-215: mean over members of mean AND (clamped) logvar
                    for (int i = tid; i < ROWS * md.out_total; i += kThreads) {
                        const int s = i / md.out_total, c = i % md.out_total;
                        float v = result[s * ld_k + c];
                        if (!deterministic && c >= md.out_dim) {
                            const int d = c - md.out_dim;
                            const int bd = (lv_rows > 1 ? member * md.out_dim : 0) + d;
                            const float mx = sm.maxlv[bd], mn = sm.minlv[bd];
                            v = clamp_logvar(v, mn, mx);
                        }
                        sm.expacc[i] = mi == 0 ? v : sm.expacc[i] + v;
                    }
                    __syncthreads();
                }
            }

            // ---- sample, delta, next obs (model.py:458-473, one_dim_tr_model.py:280-288) -----------
            // MODE 0: prediction = mean (deterministic model, or no eps given); 1: injected eps; 2: in-kernel Philox.
            // Wave-uniform switches are hoisted into compile-time variants so the four per-dimension chains
            // (LDS read -> 2 softplus -> exp -> sqrt -> fma) are straight-line code and interleave.
            HIPETS_STAMP(0, t);  // the MLP is done
            auto sample_impl = [&](auto expect_tag, auto mode_tag) __attribute__((always_inline)) {
                constexpr bool EXPECT = decltype(expect_tag)::value;
                constexpr int MODE = decltype(mode_tag)::value;
                const float inv_m = 1.0f / (float)md.M;
                const float* lvmin = sm.minlv + (lv_rows > 1 ? member * md.out_dim : 0);  // this step's member owns the bounds
                const float* lvmax = sm.maxlv + (lv_rows > 1 ? member * md.out_dim : 0);
                for (int item = tid; item < ROWS * nblk; item += kThreads) {
                    const int s = item / nblk, blk = item % nblk;
                    const int rid = sm.rowid[s];
                    HIPETS_BOUND(s < ROWS && rid < ra.B && 4 * blk < md.out_dim + 4 && md.out_total <= ld_k);
                    if (rid < 0) continue;
                    float nrm[4] = {0.f, 0.f, 0.f, 0.f};
                    if constexpr (MODE == 1) {
    #pragma unroll
                        for (int q = 0; q < 4; ++q) {
                            const int d = min(blk * 4 + q, md.out_dim - 1);
                            nrm[q] = ra.eps[((size_t)t * ra.B + rid) * md.out_dim + d];
                        }
                    } else if constexpr (MODE == 2) {
                        rollout_normals4(rid, t, blk, ra.seed, ra.stream_id, nrm);
                    }
                    float pred[4], prev[4];
    #pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        const int d = min(blk * 4 + q, md.out_dim - 1);
                        float mean, lv = 0.f;
                        if constexpr (EXPECT) {
                            mean = sm.expacc[s * md.out_total + d] / (float)md.M;
                            if constexpr (MODE != 0) lv = sm.expacc[s * md.out_total + md.out_dim + d] / (float)md.M;
                        } else {
                            mean = result[s * ld_k + d];
                            if constexpr (MODE != 0) {
                                lv = result[s * ld_k + md.out_dim + d];
                                const float mx = lvmax[d], mn = lvmin[d];
                                lv = clamp_logvar(lv, mn, mx);  // gaussian_mlp.py:152-153
                            }
                        }
                        if constexpr (MODE != 0) pred[q] = mean + __builtin_amdgcn_sqrtf(exp_hw(lv)) * nrm[q];  // model.py:471-473
                        else pred[q] = mean;
                        const int do_ = min(d, md.obs_dim - 1);
                        prev[q] = (md.target_is_delta && !sm.nodelta[do_]) ? sm.state[s * md.obs_dim + do_] : 0.f;
                    }
                    (void)inv_m;
                    unsigned pub[4] = {0u, 0u, 0u, 0u};
    #pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        const int d = blk * 4 + q;
                        if (d < md.obs_dim) {
                            const float nobs = pred[q] + prev[q];  // one_dim_tr_model.py:281-286 (prev = 0 for no_delta dims)
                            sm.state[s * md.obs_dim + d] = nobs;
                            pub[q] = __float_as_uint(nobs);
                            if (trace_next_obs) trace_next_obs[((size_t)t * ra.B + rid) * md.obs_dim + d] = nobs;
                        } else if (d < md.out_dim) {
                            sm.lrew[s] = pred[q];  // learned reward = last output (one_dim_tr_model.py:287)
                        }
                    }
                    // persistent DEVICE form: the row's next owner waits for these values -- on their way before the reward phase
                    if (handover) {
                        const unsigned tg = (unsigned)(handover_tag >> 32);
                        if (blk * 4 < md.obs_dim) pair_store(handover + (size_t)rid * NV + blk * 4, pub[0], pub[1], tg);
                        if (blk * 4 + 2 < md.obs_dim) pair_store(handover + (size_t)rid * NV + blk * 4 + 2, pub[2], pub[3], tg);
                    }
                }
            };
            {
                using T = std::true_type;
                using F = std::false_type;
                // lean instances: stochastic model, in-kernel Philox draws (the host selects them only then)
                const int mode = kLean ? 2 : (deterministic ? 0 : (ra.eps != nullptr ? 1 : (ra.use_philox ? 2 : 0)));
                if (expectation) {
                    if (mode == 0) sample_impl(T{}, std::integral_constant<int, 0>{});
                    else if (mode == 1) sample_impl(T{}, std::integral_constant<int, 1>{});
                    else sample_impl(T{}, std::integral_constant<int, 2>{});
                } else {
                    if (mode == 0) sample_impl(F{}, std::integral_constant<int, 0>{});
                    else if (mode == 1) sample_impl(F{}, std::integral_constant<int, 1>{});
                    else sample_impl(F{}, std::integral_constant<int, 2>{});
                }
            }
            if (more && !persist) fetch_actions_commit(t + 1, av);
            __syncthreads();
            prof.mark(9);

            // ---- reward, termination, masked accumulation (model_env.py:124-129, :186-188) of step t, and, in the
            // same barrier interval, the model input of step t+1 (both only READ the new state) ------------------
            // Persistent DEVICE form: every row changes workgroups now.  Its new state left in the sampling phase; its running
            // total and flag follow from here, and the same thread then evaluates which row the slot holds in step t + 1.
            for (int s = tid; s < ROWS; s += kThreads) {
                const int rid = sm.rowid[s];
                if (rid >= 0) {
                    int so = s;  // (generic instances: the row's state / action addresses are formed here, every step -- as loop invariants they
                    if constexpr (!kLean) asm volatile("" : "+v"(so));  // were carried through the layer loops, where no register is free)
                    const float* st = sm.state + so * md.obs_dim;
                    const float* ac = sm.actn + (t & 1) * ROWS * md.act_dim + so * md.act_dim;
                    float tot = sm.tot[s];
                    int trm = sm.term[s];
                    if (persist && sm.pend[s]) {  // collected late
                        sm.pend[s] = 0;
                        fetch_late_total(rid, t, tot, trm);
                    }
                    const FormTables* forms = kLean ? nullptr : form_tables(md);  // (read only by the parametric forms, which a lean instance never has)
                    if constexpr (!kLean) asm volatile("" : "+s"(forms));  // (likewise: the table address and what is loaded through it stay inside the step)
                    float r = reward_eval(st, ac, md.obs_dim, md.act_dim, reward_fn, sm.lrew[s], forms);
                    const bool done = term_eval(st, md.obs_dim, term_fn, forms);
                    if (reward_fn == HIPETS_REW_TERMS) r = reward_alive_bonus(r, done, forms);
                    if (trace_rewards) trace_rewards[(size_t)t * ra.B + rid] = r;
                    end_step_for_row(s, rid, tot, trm, r, done, handover, (unsigned)(handover_tag >> 32));
                }
                if (persist && has_next) {  // the slot's row in the next turn (only this thread reads rowid[s] between the two barriers around here)
                    const int j = (v_next % ra.groups) * ROWS + s;
                    sm.rowid[s] = j < ra.rows_per_domain
                                      ? (int)perm_apply((unsigned)((v_next / ra.groups) * ra.rows_per_domain + j), ra.perm_n, ra.perm_a, ra.perm_b, ra.step_keys[t_next]) : -1;
                    sm.lrew[s] = 0.f;
                }
            }
            if (more && !persist) build_input(t + 1, sm.buf0);
            __syncthreads();
            prof.mark(10);

        }
        HIPETS_STAMP(1, t);  // sampled, rewarded, published
        if (persist && has_next) {
            // ---- collect the rows of the next turn: 8-byte {value bits, step tag} granules, self-validating ----
            {
                int nj0, nlive;
                logical_rows(v_next, domain, nj0, nlive);
            }
            member_dom = domain;
            compute_act_base();
            float av2[kPrefetch];
            fetch_actions_issue(t_next, av2);  // in flight while the rows arrive
            const unsigned long long tag = (unsigned long long)(ra.tag_base + (unsigned)t_next) << 32;  // published in step t_next - 1
            // (Writing the normalised input columns straight from here, as the straight form does, measured SLOWER in this flow: cfg4'
            // 10.5 vs 9.85 ms per rollout, cfg4 3.44 vs 3.37 -- with 12-24 pairs per thread the f64 work serialises behind every poll
            // round, while the separate pass below spreads it over the workgroup.)
            if (t_next == ra.t_begin) {  // a later turn of the FIRST step: the rows start from s0 (nothing was handed over yet)
                for (int i = tid; i < ROWS * md.obs_dim; i += kThreads) {
                    const int s_ = i / md.obs_dim;
                    const int rid_ = sm.rowid[s_];
                    const size_t env_off = (!kLean && ra.pop_env > 0 && rid_ >= 0) ? (size_t)((rid_ / ra.P) / ra.pop_env) * md.obs_dim : 0;
                    sm.state[i] = rid_ >= 0 ? ra.s0[env_off + (i - s_ * md.obs_dim)] : 0.f;
                }
                for (int s_ = tid; s_ < ROWS; s_ += kThreads) {
                    sm.tot[s_] = 0.f;
                    sm.term[s_] = 0;
                }
            } else if constexpr (kWide) {
                dma_collect((unsigned)(tag >> 32));
            } else
            for (int base = 0; base < ROWS * NVP; base += kGT * kThreads) {
                const unsigned long long* src[kGT];
                u32x4g g[kGT];
                int gs[kGT], gv[kGT];
                bool soft[kGT];  // {running total, flag}: wanted at the NEXT reward phase only -- one look now, the rest there
                const unsigned want = (unsigned)(tag >> 32);
#pragma unroll
                for (int q = 0; q < kGT; ++q) {
                    const int i = base + tid + q * kThreads;
                    // (item -> (row slot, pair) by multiply-high with ceil(2^32 / NVP): exact for i < 2^32 / NVP, and i < 64 * NVP here)
                    const int i_row = (int)__umulhi((unsigned)i, nvp_magic);
                    gs[q] = (base == 0 && q < kG) ? xs[q < kG ? q : 0] : (i < ROWS * NVP ? i_row : -1);
                    gv[q] = (base == 0 && q < kG) ? xv[q < kG ? q : 0] : (i < ROWS * NVP ? i - i_row * NVP : 0);
                    soft[q] = gv[q] == NVP - 1;
                    src[q] = nullptr;
                    g[q] = u32x4g{0u, want, 0u, want};  // rows of the padding: zero state, total, flag
                    if (gs[q] >= 0) {
                        const int rid = sm.rowid[gs[q]];
                        if (rid >= 0) src[q] = ra.exchange + (size_t)rid * NV + 2 * gv[q];
                    }
                }
                const long long t_poll = wall_clock64();  // constant 100 MHz counter
                for (int spins = 0;; ++spins) {
                    // issue, issue, wait as straight-line asm (no branch between a load and its wait: the compiler does not know the
                    // destination registers are still in flight); items with nothing to fetch read the table's first pair and ignore it
                    static_assert(kGT == 2 || kGT == 4, "the wait below names its destinations");
                    u32x4g got[kGT];
#pragma unroll
                    for (int q = 0; q < kGT; ++q) pair_load_issue(got[q], src[q] ? src[q] : ra.exchange);
                    if constexpr (kGT == 2) asm volatile("s_waitcnt vmcnt(0)" : "+v"(got[0]), "+v"(got[1])::"memory");
                    else asm volatile("s_waitcnt vmcnt(0)" : "+v"(got[0]), "+v"(got[1]), "+v"(got[2]), "+v"(got[3])::"memory");
                    bool ready = true;
#pragma unroll
                    for (int q = 0; q < kGT; ++q)
                        if (src[q]) {
                            g[q] = got[q];
                            if (got[q][1] == want && got[q][3] == want) src[q] = nullptr;
                            else if (!soft[q]) ready = false;
                        }
                    if (ready) break;
                    if (poll_gave_up(spins, t_poll)) break;
                    __builtin_amdgcn_s_sleep(8);
                }
#pragma unroll
                for (int q = 0; q < kGT; ++q)
                    if (gs[q] >= 0) {
                        HIPETS_BOUND(gs[q] < ROWS && gv[q] >= 0 && gv[q] < NVP);
                        if (!soft[q]) {
                            const int d = 2 * gv[q];
                            const float v0 = __uint_as_float(g[q][0]), v1 = __uint_as_float(g[q][2]);
                            if constexpr (S::FUSE && S::TERM == HIPETS_TERM_HOPPER) {  // (rows of the padding hold zeros and no row id: never read)
                                if (sm.rowid[gs[q]] >= 0 && hopper_pair_bad(d, v0, v1, true, d + 1 < md.obs_dim)) hop_flags[gs[q]] = 1;
                            }
                            sm.state[gs[q] * md.obs_dim + d] = v0;
                            if (d + 1 < md.obs_dim) sm.state[gs[q] * md.obs_dim + d + 1] = v1;
                        } else if (src[q]) {
                            sm.pend[gs[q]] = 1;  // not there yet: the reward phase fetches the pair
                        } else {
                            sm.tot[gs[q]] = __uint_as_float(g[q][0]);
                            sm.term[gs[q]] = (int)g[q][2];
                        }
                    }
            }
            HIPETS_STAMP(2, t);  // this thread's rows have arrived
            fetch_actions_commit(t_next, av2);
            __syncthreads();
            build_input(t_next, step_in);
            __syncthreads();
            HIPETS_STAMP(3, t);  // the next step's input is built
        }
    }

    // ---- write back -------------------------------------------------------------------------------
    if constexpr (S::FUSE && S::TERM == HIPETS_TERM_HOPPER) {
        // the fused all-dims termination folds step t's per-row flag into `terminated` one step later (tail_unit): the LAST step's
        // flag is still pending here.  It cannot change a return (model_env.py:186-188: the terminating step's reward counts), but
        // sm.term is what the write-back publishes -- one launch per step in DEVICE mode: the next launch starts from it -- so it is
        // completed before anything reads it (complete since the step's barrier)
        if (ra.t_end > ra.t_begin && !persist)
            for (int s = tid; s < ROWS; s += kThreads) sm.term[s] |= sm.pend[((ra.t_end - 1) & 1) * ROWS + s];
    }
    for (int s = tid; s < ROWS; s += kThreads) {
        const int rid = sm.rowid[s];
        if (rid < 0 || persist) continue;  // persistent form: written in the last step's reward phase
        ra.totals[rid] = sm.tot[s];
        if (!fast && !persist) ra.term[rid] = (unsigned char)sm.term[s];
    }
    if (prof.on) {  // flush the phase accumulators of this wave
#pragma unroll
        for (int i = 0; i < 16; ++i) ra.phase_cycles[wave * 16 + i] += prof.slot[i];
    }
    if (!fast && !persist) {
        for (int i = tid; i < ROWS * md.obs_dim; i += kThreads) {
            const int s = i / md.obs_dim, d = i % md.obs_dim;
            const int rid = sm.rowid[s];
            if (rid >= 0) ra.state[(size_t)rid * md.obs_dim + d] = sm.state[i];
        }
    }
}

}  // namespace hipets
