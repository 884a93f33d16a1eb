// engine.hip -- the engine of the C ABI (include/hipets.h): creation and destruction, the thread's error state, stream entry, host
// staging, the engine's switches, launch timing.  gfx950 only; no CPU fallback.  Host code only.
#include <cstdarg>
#include <cstdio>
#include <cstring>

#include "engine.hpp"

namespace hipets {

thread_local std::string g_err;
thread_local int g_err_kind = HIPETS_ERR_NONE;

int fail(const char* fmt, ...) {
    char buf[1024];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    g_err = buf;
    g_err_kind = HIPETS_ERR_INVALID_ARGUMENT;
    return 1;
}

int fail_kind(const int kind, const char* fmt, ...) {
    char buf[1024];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    g_err = buf;
    g_err_kind = kind;
    return 1;
}

int check_reduce(const hipets_engine* e, const int P) {
    if (e->reduce.kind != HIPETS_REDUCE_WORST_K) return 0;
    if (P > kWorstKMaxP) return fail("particle reduction WORST_K: %d particles (max %d)", P, kWorstKMaxP);
    if (e->reduce.k > P) return fail("particle reduction WORST_K: worst_k %d > %d particles", e->reduce.k, P);
    return 0;
}

int stage_h2d(hipets_engine* e, void* dst, const void* src, size_t bytes, hipStream_t st) {
    hipets_engine::HostStage& sl = e->stage[e->stage_next];
    e->stage_next = (e->stage_next + 1) % 4;
    if (sl.used) HCHECK(hipEventSynchronize(sl.done));
    if (bytes > sl.cap) {
        if (sl.p) (void)hipHostFree(sl.p);
        sl.p = nullptr;
        sl.cap = 0;
        HCHECK(hipHostMalloc(&sl.p, bytes < 4096 ? 4096 : bytes, hipHostMallocDefault));
        sl.cap = bytes < 4096 ? 4096 : bytes;
    }
    if (!sl.done) HCHECK(hipEventCreateWithFlags(&sl.done, hipEventDisableTiming));
    std::memcpy(sl.p, src, bytes);
    HCHECK(hipMemcpyAsync(dst, sl.p, bytes, hipMemcpyHostToDevice, st));
    HCHECK(hipEventRecord(sl.done, st));
    sl.used = true;
    return 0;
}

int enter_stream(hipets_engine* e, hipStream_t st) {
    if (!e->last_done) HCHECK(hipEventCreateWithFlags(&e->last_done, hipEventDisableTiming));
    if (e->last_stream_set && e->last_stream != st) HCHECK(hipStreamWaitEvent(st, e->last_done, 0));
    e->last_stream = st;
    e->last_stream_set = true;
    return 0;
}

StreamScope::~StreamScope() {
    static const bool off = std::getenv("HIPETS_NO_STREAM_SCOPE") != nullptr;  // (A/B measurements only)
    if (e && e->last_done && !off) (void)hipEventRecord(e->last_done, st);
}

}  // namespace hipets

using namespace hipets;

extern "C" {

int hipets_abi_version(void) { return HIPETS_ABI_VERSION; }

const char* hipets_last_error(void) { return g_err.c_str(); }

int hipets_last_error_kind(void) { return g_err_kind; }

int hipets_create(int device, hipets_engine** out) {
    if (!out) return fail("null out pointer");
    *out = nullptr;
    int n = 0;
    hipError_t err = hipGetDeviceCount(&n);
    if (err != hipSuccess || n <= 0)
        return fail("no HIP device visible (%s) -- libhipets has no CPU fallback", hipGetErrorString(err));
    if (device < 0 || device >= n) return fail("device %d out of range (%d visible)", device, n);
    HCHECK(hipSetDevice(device));
    hipDeviceProp_t prop;
    HCHECK(hipGetDeviceProperties(&prop, device));
    if (std::string(prop.gcnArchName).rfind("gfx950", 0) != 0)
        return fail("device %d is %s; libhipets is built for gfx950 (MI355X) only", device, prop.gcnArchName);
    auto* e = new hipets_engine();
    e->device = device;
    e->num_cu = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    e->lds_max = prop.sharedMemPerBlockOptin > 0 ? (size_t)prop.sharedMemPerBlockOptin : (size_t)prop.sharedMemPerBlock;
    if (e->lds_max > 160 * 1024) e->lds_max = 160 * 1024;
    // timeout flag of the persistent DEVICE-mode kernel: host memory the device can write, read by the host without a sync
    if (hipHostMalloc(reinterpret_cast<void**>(&e->error_flag), sizeof(int), hipHostMallocMapped) != hipSuccess) e->error_flag = nullptr;
    if (e->error_flag) *e->error_flag = 0;
    const char* np = std::getenv("HIPETS_NO_PERSISTENT");
    e->persistent_ok = e->error_flag != nullptr && !(np && np[0] == '1');
    if (e->census.ensure(2 * sizeof(int))) e->persistent_ok = false;
    *out = e;
    return 0;
}

void hipets_destroy(hipets_engine* e) {
    if (!e) return;
    (void)hipSetDevice(e->device);
    comm_release(e);
    for (DevBuf* b : {&e->w3pack, &e->wpack, &e->bpack, &e->layer_meta, &e->norm_mean, &e->norm_std, &e->min_lv, &e->max_lv, &e->no_delta, &e->members,
                      &e->s0, &e->state, &e->totals, &e->term, &e->exchange, &e->step_keys, &e->plan_keys, &e->mu, &e->disp, &e->population, &e->values,
                      &e->best_value, &e->best_solution, &e->past_action, &e->kept, &e->elite_idx, &e->keep_idx, &e->planet_w, &e->planet_b, &e->planet_member, &e->planet_ops, &e->shard_values, &e->gathered, &e->census, &e->train_slab, &e->train_partial,
                      &e->policy.w, &e->policy.b, &e->compact_counts, &e->sac_ws, &e->sac_one, &e->critic.w, &e->critic.b,
                      &e->ensemble.w, &e->ensemble.b, &e->ensemble.norm, &e->ensemble.lv, &e->ensemble.cols})
        b->release();
    for (auto& ev : e->events) { (void)hipEventDestroy(ev.first); (void)hipEventDestroy(ev.second); }
    for (auto& ev : e->event_pool) { (void)hipEventDestroy(ev.first); (void)hipEventDestroy(ev.second); }
    if (e->error_flag) (void)hipHostFree(e->error_flag);
    if (e->last_done) (void)hipEventDestroy(e->last_done);
    for (auto& sl : e->stage) {
        if (sl.p) (void)hipHostFree(sl.p);
        if (sl.done) (void)hipEventDestroy(sl.done);
    }
    delete e;
}

int hipets_set_plan_mode(hipets_engine* e, int32_t mode) {
    if (!e) return fail("null engine");
    if (mode != HIPETS_MODE_FAST && mode != HIPETS_MODE_DEVICE) return fail("plan mode must be HIPETS_MODE_FAST or HIPETS_MODE_DEVICE");
    e->plan_mode = mode;
    return 0;
}

int hipets_set_particle_reduce(hipets_engine* e, int32_t kind, float kappa, int32_t worst_k) {
    if (!e) return fail("null engine");
    if (kind < HIPETS_REDUCE_MEAN || kind > HIPETS_REDUCE_WORST_K) return fail("unknown particle reduction %d (HIPETS_REDUCE_MEAN .. HIPETS_REDUCE_WORST_K)", kind);
    if (!std::isfinite(kappa)) return fail("particle reduction: kappa must be finite");
    if (kind == HIPETS_REDUCE_WORST_K && worst_k < 1) return fail("particle reduction WORST_K: worst_k %d < 1", worst_k);
    e->reduce.kind = kind;
    e->reduce.kappa = kind == HIPETS_REDUCE_MEAN_STD ? kappa : 0.f;
    e->reduce.k = kind == HIPETS_REDUCE_WORST_K ? worst_k : 0;
    return 0;
}

int hipets_set_persistent(hipets_engine* e, int32_t on) {
    if (!e) return fail("null engine");
    if (on && !e->error_flag) return fail("persistent DEVICE-mode launches need the host-mapped timeout flag, which could not be allocated");
    e->persistent_ok = on != 0;
    return 0;
}

int hipets_set_handover_timeout(hipets_engine* e, double seconds) {
    if (!e) return fail("null engine");
    if (!(seconds >= 0.0) || seconds > 60.0) return fail("hand-over timeout %g s outside [0, 60]", seconds);
    e->poll_ticks = (long long)(seconds * 1.0e8);  // the kernel's wall clock runs at 100 MHz
    return 0;
}

int hipets_check_async_error(hipets_engine* e, int32_t* timed_out) {
    if (!e || !timed_out) return fail("null argument");
    *timed_out = 0;
    if (e->error_flag && *e->error_flag) {
        *e->error_flag = 0;
        e->persistent_ok = false;  // per-step launches from now on (hipets_set_persistent(e, 1) switches back)
        *timed_out = 1;
        g_err_kind = HIPETS_ERR_TIMEOUT;
        g_err = "a persistent DEVICE-mode rollout gave up waiting for rows of another workgroup (its workgroups were not all resident: "
                "another process or stream held CUs); everything computed from that launch on is invalid -- re-run the call.  "
                "Persistent launches are now disabled for this engine.";
    }
    return 0;
}

int hipets_set_plan_trace(hipets_engine* e, const hipets_plan_trace* t) {
    if (!e) return fail("null engine");
    e->has_trace = t != nullptr;
    if (t) e->trace = *t;
    return 0;
}

int hipets_timing_enable(hipets_engine* e, int32_t on) {
    if (!e) return fail("null engine");
    e->timing = on != 0;
    e->timing_stride = on > 1 ? on : 1;
    e->launch_counter = 0;
    return 0;
}

int hipets_timing_read(hipets_engine* e, int64_t* launches, double* total_ms, int32_t reset) {
    if (!e) return fail("null engine");
    HCHECK(hipSetDevice(e->device));
    double tot = 0.0;
    for (auto& ev : e->events) {
        HCHECK(hipEventSynchronize(ev.second));
        float ms = 0.f;
        HCHECK(hipEventElapsedTime(&ms, ev.first, ev.second));
        tot += ms;
    }
    if (launches) *launches = (int64_t)e->events.size();
    if (total_ms) *total_ms = tot;
    if (reset) {
        for (auto& ev : e->events) e->event_pool.push_back(ev);
        e->events.clear();
    }
    return 0;
}

}  // extern "C"
