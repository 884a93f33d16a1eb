// comm.hip -- the communicator of the C ABI (include/hipets.h hipets_comm_*) and the collective of sharded plans.  RCCL through dlopen:
// no link-time dependency, and inside a PyTorch process the already loaded librccl is reused.
#include <dlfcn.h>

#include <cstring>

#include "engine.hpp"

using namespace hipets;

namespace {

struct RcclId { char internal[HIPETS_COMM_ID_BYTES]; };
struct Rccl {
    void* lib = nullptr;
    int (*GetUniqueId)(void*) = nullptr;
    int (*CommInitRank)(void**, int, RcclId /* ncclUniqueId by value */, int) = nullptr;
    int (*CommDestroy)(void*) = nullptr;
    int (*AllGather)(const void*, void*, size_t, int, void*, hipStream_t) = nullptr;
    const char* (*GetErrorString)(int) = nullptr;
    int (*CommCount)(void*, int*) = nullptr;     // optional (hipets_comm_info)
    int (*CommUserRank)(void*, int*) = nullptr;  // optional
};
Rccl g_rccl;

int rccl_load() {
    if (g_rccl.lib) return 0;
    void* lib = nullptr;
    // HIPETS_RCCL_LIB=<path>: load THIS library instead (a site build of RCCL; tests/fake_rccl: a stand-in that implements the
    // five entry points for N processes sharing one GPU, so that the world > 1 path runs on a one-GPU box)
    const char* forced = std::getenv("HIPETS_RCCL_LIB");
    if (forced && forced[0]) {
        lib = dlopen(forced, RTLD_NOW | RTLD_LOCAL);
        if (!lib) return fail_kind(HIPETS_ERR_RUNTIME, "cannot load the RCCL library named by HIPETS_RCCL_LIB (%s): %s", forced, dlerror());
    }
    for (const char* name : {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so"}) {
        if (lib) break;
        lib = dlopen(name, RTLD_NOW | RTLD_GLOBAL);
    }
    if (!lib) return fail_kind(HIPETS_ERR_RUNTIME, "cannot load librccl: %s", dlerror());
    g_rccl.GetUniqueId = reinterpret_cast<int (*)(void*)>(dlsym(lib, "ncclGetUniqueId"));
    g_rccl.CommInitRank = reinterpret_cast<int (*)(void**, int, RcclId, int)>(dlsym(lib, "ncclCommInitRank"));
    g_rccl.CommDestroy = reinterpret_cast<int (*)(void*)>(dlsym(lib, "ncclCommDestroy"));
    g_rccl.AllGather = reinterpret_cast<int (*)(const void*, void*, size_t, int, void*, hipStream_t)>(dlsym(lib, "ncclAllGather"));
    g_rccl.GetErrorString = reinterpret_cast<const char* (*)(int)>(dlsym(lib, "ncclGetErrorString"));
    g_rccl.CommCount = reinterpret_cast<int (*)(void*, int*)>(dlsym(lib, "ncclCommCount"));
    g_rccl.CommUserRank = reinterpret_cast<int (*)(void*, int*)>(dlsym(lib, "ncclCommUserRank"));
    if (!g_rccl.GetUniqueId || !g_rccl.CommInitRank || !g_rccl.CommDestroy || !g_rccl.AllGather) return fail_kind(HIPETS_ERR_RUNTIME, "librccl lacks an expected symbol");
    g_rccl.lib = lib;
    return 0;
}
#define NCHECK(x)                                                                                        \
    do {                                                                                                 \
        const int r_ = (x);                                                                              \
        if (r_ != 0) return fail_kind(HIPETS_ERR_RUNTIME, "RCCL error %d (%s) at %s:%d", r_, g_rccl.GetErrorString ? g_rccl.GetErrorString(r_) : "?", __FILE__, __LINE__); \
    } while (0)

// gathered [world, width] (rank r's shard in row r, padded) -> values [pop]
__global__ void unpad_shards_kernel(const float* gathered, float* values, int pop, int world, int width) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= pop) return;
    const int base = pop / world, extra = pop % world;
    const int split = extra * (base + 1);  // candidates held by the ranks with one more
    const int r = i < split ? i / (base + 1) : extra + (i - split) / base;
    const int lo = r * base + min(r, extra);
    values[i] = gathered[(size_t)r * width + (i - lo)];
}

}  // namespace

namespace hipets {

int comm_all_gather(hipets_engine* e, size_t width, hipStream_t st) {
    NCHECK(g_rccl.AllGather(e->shard_values.p, e->gathered.p, width, 7 /* ncclFloat32 */, e->comm, st));
    return 0;
}

int comm_unpad_shards(hipets_engine* e, int rows, int width, hipStream_t st) {
    hipLaunchKernelGGL(unpad_shards_kernel, dim3((rows + 255) / 256), dim3(256), 0, st, e->gathered.as<float>(), e->values.as<float>(), rows, e->comm_world,
                       width);
    const hipError_t err = hipGetLastError();
    if (err != hipSuccess) return fail_kind(HIPETS_ERR_RUNTIME, "unpad_shards_kernel launch failed: %s", hipGetErrorString(err));
    return 0;
}

void comm_release(hipets_engine* e) {
    if (e->comm && g_rccl.CommDestroy) (void)g_rccl.CommDestroy(e->comm);
}

}  // namespace hipets

extern "C" {

int hipets_comm_unique_id(void* id_out) {
    if (!id_out) return fail("null argument");
    if (rccl_load()) return 1;
    NCHECK(g_rccl.GetUniqueId(id_out));
    return 0;
}

int hipets_comm_init(hipets_engine* e, const void* unique_id, int32_t rank, int32_t world) {
    if (!e || !unique_id) return fail("null argument");
    if (world < 1 || rank < 0 || rank >= world) return fail("bad rank %d / world_size %d", rank, world);
    if (rccl_load()) return 1;
    HCHECK(hipSetDevice(e->device));
    if (e->comm) {
        NCHECK(g_rccl.CommDestroy(e->comm));
        e->comm = nullptr;
    }
    RcclId id;
    std::memcpy(id.internal, unique_id, HIPETS_COMM_ID_BYTES);
    NCHECK(g_rccl.CommInitRank(&e->comm, world, id, rank));
    e->comm_rank = rank;
    e->comm_world = world;
    return 0;
}

int hipets_comm_destroy(hipets_engine* e) {
    if (!e) return fail("null engine");
    if (e->comm) {
        HCHECK(hipSetDevice(e->device));
        NCHECK(g_rccl.CommDestroy(e->comm));
        e->comm = nullptr;
    }
    e->comm_rank = 0;
    e->comm_world = 1;
    return 0;
}

int hipets_comm_info(hipets_engine* e, int32_t* rank, int32_t* world_size) {
    if (!e) return fail("null engine");
    int r = e->comm_rank, w = e->comm_world;
    if (e->comm && g_rccl.CommCount && g_rccl.CommUserRank) {  // what the communicator itself says, not what the caller passed in
        NCHECK(g_rccl.CommCount(e->comm, &w));
        NCHECK(g_rccl.CommUserRank(e->comm, &r));
    }
    if (rank) *rank = r;
    if (world_size) *world_size = w;
    return 0;
}

}  // extern "C"
