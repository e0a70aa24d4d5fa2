// Host-memory double of the few HIP runtime entry points the C-ABI library's HOST half uses -- test infrastructure
// for `make asan` ("-fsanitize=address host build of the C-ABI shim"), never part of the product.
//
// The library's .hip sources are compiled with `hipcc --cuda-host-only -fsanitize=address,undefined` (host code only:
// argument validation, table builders, BatchNorm folding, k4 packing, workspace sizing, launch-strategy selection,
// error-string lifetime) and linked against THIS file instead of libamdhip64: "device" memory is host memory from
// calloc (so AddressSanitizer sees every upload / download the host half performs with its true extent), events are
// counters, and a kernel launch is counted, shown to the launch hook (if one is set) and otherwise ignored -- no
// kernel arithmetic runs here, GPU results are the business of `pytest -m gpu`.  Runs in the GPU-less build container.
// hipMemsetAsync calls are counted too (hipdouble_memset_asyncs: the wipe of the FeCo exchange buffers is one).
// The device the double plays can be resized from the environment, read at every query: HIPDOUBLE_CUS (compute units,
// default 256), HIPDOUBLE_OCCUPANCY (the answer to hipOccupancyMaxActiveBlocksPerMultiprocessor, default 2) and
// HIPDOUBLE_REFUSE_LDS=1 (hipFuncSetAttribute refuses a request for 160 KB or more: a device whose blocks cannot have the whole
// LDS of a gfx950 CU, which the fused AudioNet kernels ask for).
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>

static long g_launches = 0, g_allocs = 0, g_frees = 0, g_bytes = 0, g_memset_asyncs = 0;
static dim3 g_grid, g_block;
static size_t g_shmem = 0;
static hipStream_t g_stream = nullptr;

typedef void (*hipdouble_launch_hook)(const char* mangled_name, dim3 grid, dim3 block, size_t shmem, void** args);
static hipdouble_launch_hook g_hook = nullptr;
// host pointer -> mangled kernel name, as __hipRegisterFunction hands them over (from static constructors: built on first use)
static std::map<const void*, std::string>& kernel_names() {
    static std::map<const void*, std::string> m;
    return m;
}
static int env_int(const char* name, int dflt) {
    const char* e = std::getenv(name);
    return e ? std::atoi(e) : dflt;
}

extern "C" {

long hipdouble_launches() { return g_launches; }
long hipdouble_live_allocs() { return g_allocs - g_frees; }
long hipdouble_memset_asyncs() { return g_memset_asyncs; }
void hipdouble_set_launch_hook(hipdouble_launch_hook hook) { g_hook = hook; }

hipError_t hipGetDeviceCount(int* n) { *n = 1; return hipSuccess; }
hipError_t hipSetDevice(int d) { return d == 0 ? hipSuccess : hipErrorInvalidDevice; }
hipError_t hipGetDevice(int* d) { *d = 0; return hipSuccess; }
hipError_t hipGetDevicePropertiesR0600(hipDeviceProp_t* p, int) {
    std::memset(p, 0, sizeof(*p));
    p->multiProcessorCount = env_int("HIPDOUBLE_CUS", 256);
    p->sharedMemPerBlock = 64 * 1024;
    p->maxSharedMemoryPerMultiProcessor = 160 * 1024;
    std::snprintf(p->name, sizeof(p->name), "host double of gfx950");
    return hipSuccess;
}
hipError_t hipMalloc(void** p, size_t n) {
    *p = std::calloc(1, n ? n : 1);
    ++g_allocs;
    g_bytes += (long)n;
    return *p ? hipSuccess : hipErrorOutOfMemory;
}
hipError_t hipFree(void* p) {
    if (p) ++g_frees;
    std::free(p);
    return hipSuccess;
}
hipError_t hipHostMalloc(void** p, size_t n, unsigned) { return hipMalloc(p, n); }
hipError_t hipHostFree(void* p) { return hipFree(p); }
hipError_t hipHostGetDevicePointer(void** d, void* h, unsigned) { *d = h; return hipSuccess; }
hipError_t hipMemcpy(void* d, const void* s, size_t n, hipMemcpyKind) { std::memmove(d, s, n); return hipSuccess; }
hipError_t hipMemcpyAsync(void* d, const void* s, size_t n, hipMemcpyKind, hipStream_t) { std::memmove(d, s, n); return hipSuccess; }
hipError_t hipMemset(void* d, int v, size_t n) { std::memset(d, v, n); return hipSuccess; }
hipError_t hipMemsetAsync(void* d, int v, size_t n, hipStream_t) { std::memset(d, v, n); ++g_memset_asyncs; return hipSuccess; }
// device globals: the host-only objects keep a host shadow of every __device__ variable; copy to / from that
hipError_t hipMemcpyToSymbol(const void* sym, const void* src, size_t n, size_t off, hipMemcpyKind) {
    std::memmove(const_cast<char*>(static_cast<const char*>(sym)) + off, src, n);
    return hipSuccess;
}
hipError_t hipMemcpyFromSymbol(void* dst, const void* sym, size_t n, size_t off, hipMemcpyKind) {
    std::memmove(dst, static_cast<const char*>(sym) + off, n);
    return hipSuccess;
}
hipError_t hipDeviceSynchronize() { return hipSuccess; }
hipError_t hipStreamSynchronize(hipStream_t) { return hipSuccess; }
hipError_t hipGetLastError() { return hipSuccess; }
const char* hipGetErrorString(hipError_t e) {
    static thread_local char buf[40];
    std::snprintf(buf, sizeof(buf), "hip error %d (host double)", (int)e);
    return e == hipSuccess ? "no error" : buf;
}

struct FakeEvent { long stamp; };
hipError_t hipEventCreate(hipEvent_t* e) { *e = reinterpret_cast<hipEvent_t>(std::calloc(1, sizeof(FakeEvent))); ++g_allocs; return hipSuccess; }
hipError_t hipEventDestroy(hipEvent_t e) { ++g_frees; std::free(e); return hipSuccess; }
hipError_t hipEventRecord(hipEvent_t e, hipStream_t) { reinterpret_cast<FakeEvent*>(e)->stamp = g_launches; return hipSuccess; }
hipError_t hipEventSynchronize(hipEvent_t) { return hipSuccess; }
hipError_t hipEventElapsedTime(float* ms, hipEvent_t a, hipEvent_t b) {
    *ms = 0.001f * (float)(reinterpret_cast<FakeEvent*>(b)->stamp - reinterpret_cast<FakeEvent*>(a)->stamp);
    return hipSuccess;
}

hipError_t hipFuncSetAttribute(const void*, hipFuncAttribute, int value) {
    return value >= 160 * 1024 && env_int("HIPDOUBLE_REFUSE_LDS", 0) ? hipErrorInvalidValue : hipSuccess;
}
hipError_t hipOccupancyMaxActiveBlocksPerMultiprocessor(int* n, const void*, int, size_t) {
    *n = env_int("HIPDOUBLE_OCCUPANCY", 2);
    return hipSuccess;
}

hipError_t __hipPushCallConfiguration(dim3 grid, dim3 block, size_t shmem, hipStream_t s) {
    g_grid = grid; g_block = block; g_shmem = shmem; g_stream = s;
    return hipSuccess;
}
hipError_t __hipPopCallConfiguration(dim3* grid, dim3* block, size_t* shmem, hipStream_t* s) {
    *grid = g_grid; *block = g_block; *shmem = g_shmem; *s = g_stream;
    return hipSuccess;
}
hipError_t hipLaunchKernel(const void* fn, dim3 grid, dim3 block, void** args, size_t shmem, hipStream_t) {
    // what a launch the hardware would refuse looks like: empty or oversized grids / blocks are host-side bugs
    if (grid.x == 0 || grid.y == 0 || grid.z == 0 || block.x * block.y * block.z == 0 || block.x * block.y * block.z > 1024) {
        std::fprintf(stderr, "hip double: invalid launch configuration grid (%u,%u,%u) block (%u,%u,%u)\n", grid.x, grid.y, grid.z,
                     block.x, block.y, block.z);
        std::abort();
    }
    ++g_launches;
    if (g_hook) {
        const auto it = kernel_names().find(fn);
        g_hook(it == kernel_names().end() ? "?" : it->second.c_str(), grid, block, shmem, args);
    }
    return hipSuccess;
}
void** __hipRegisterFatBinary(const void*) { static void* handle[2]; return handle; }
void __hipUnregisterFatBinary(void**) {}
void __hipRegisterFunction(void**, const void* host_fn, char*, const char* device_name, unsigned, void*, void*, void*, void*, int*) {
    kernel_names()[host_fn] = device_name;
}
void __hipRegisterVar(void**, void*, char*, const char*, int, size_t, int, int) {}

}  // extern "C"
