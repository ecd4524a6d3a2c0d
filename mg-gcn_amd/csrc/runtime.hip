// runtime.hip -- device / stream / event / memory entry points of the C ABI.
// Stands in for the reference's per-GPU `context` (src/matrix.hpp:69-158) and the
// cuda_malloc helpers (src/mg_gcn.hpp:74-90).  Thin on purpose: the host layers
// (C++ headers, Python mirror) own all policy.
#include <algorithm>
#include <map>
#include <mutex>
#include <tuple>
#include <vector>

#include "common.h"
#include "scratch_internal.h"

MGGCN_API int mggcn_abi_version(void) { return MGGCN_ABI_VERSION; }

MGGCN_API int mggcn_device_count(void) {
    int n = 0;
    hipError_t st = hipGetDeviceCount(&n);
    if (st != hipSuccess) {  // no driver / no GPU: report zero devices, do not abort
        (void)hipGetLastError();
        return 0;
    }
    return n;
}

MGGCN_API void mggcn_set_device(int device) { MGGCN_CHECK_HIP(hipSetDevice(device)); }

MGGCN_API int mggcn_get_device(void) {
    int d = 0;
    MGGCN_CHECK_HIP(hipGetDevice(&d));
    return d;
}

MGGCN_API void mggcn_device_synchronize(void) { MGGCN_CHECK_HIP(hipDeviceSynchronize()); }

MGGCN_API mggcn_stream_t mggcn_stream_create(int high_priority) {
    int least = 0, greatest = 0;  // numerically: greatest priority is the smaller number
    MGGCN_CHECK_HIP(hipDeviceGetStreamPriorityRange(&least, &greatest));
    hipStream_t s = nullptr;
    MGGCN_CHECK_HIP(hipStreamCreateWithPriority(&s, hipStreamNonBlocking, high_priority ? greatest : least));
    return s;
}

// ---- the reduction scratch (scratch_internal.h) -----------------------------
namespace {
struct scratch_buffer { float *p = nullptr; size_t floats = 0; };
std::mutex g_scratch_mu;
std::map<std::tuple<int, hipStream_t, scratch_kind>, scratch_buffer> g_scratch;     // under g_scratch_mu
}  // namespace

float *stream_scratch(hipStream_t st, scratch_kind kind, size_t floats) {
    int dev = 0;
    MGGCN_CHECK_HIP(hipGetDevice(&dev));
    std::lock_guard<std::mutex> lock(g_scratch_mu);
    scratch_buffer &s = g_scratch[{dev, st, kind}];
    if (s.floats < floats) {
        if (s.p) {
            MGGCN_CHECK_HIP(hipStreamSynchronize(st));                // an earlier kernel may still be summing into it
            MGGCN_CHECK_HIP(hipFree(s.p));
            s.p = nullptr; s.floats = 0;
        }
        MGGCN_CHECK_HIP(hipMalloc(&s.p, floats * sizeof(float)));
        s.floats = floats;
    }
    return s.p;
}

// The scratch belongs to a (device, stream) pair: mggcn_stream_destroy releases it with the stream; a host layer whose
// streams come from elsewhere (torch) calls this when it drops a stream, so that a recycled stream handle never inherits a
// buffer another stream may still be using, and nothing accumulates.
MGGCN_API void mggcn_stream_release_scratch(mggcn_stream_t stream) {
    // by STREAM alone, whatever device is current on the calling thread (a stream handle belongs to one device; a context
    // may be dropped from a thread that has another device current -- the entry must still be found, or a recycled handle
    // inherits the buffer)
    std::vector<std::pair<int, float *>> mine;
    {
        std::lock_guard<std::mutex> lock(g_scratch_mu);
        for (auto it = g_scratch.begin(); it != g_scratch.end();)
            if (std::get<1>(it->first) == as_stream(stream)) { mine.push_back({std::get<0>(it->first), it->second.p}); it = g_scratch.erase(it); }
            else ++it;
    }
    if (mine.empty()) return;
    int prev = 0;
    MGGCN_CHECK_HIP(hipGetDevice(&prev));
    for (const auto &m : mine) {
        MGGCN_CHECK_HIP(hipSetDevice(m.first));
        MGGCN_CHECK_HIP(hipStreamSynchronize(as_stream(stream)));      // nobody may still be summing into it
        MGGCN_CHECK_HIP(hipFree(m.second));
    }
    MGGCN_CHECK_HIP(hipSetDevice(prev));
}

MGGCN_API void mggcn_stream_destroy(mggcn_stream_t stream) {
    if (!stream) return;
    mggcn_stream_release_scratch(stream);
    MGGCN_CHECK_HIP(hipStreamDestroy(as_stream(stream)));
}

MGGCN_API void mggcn_stream_synchronize(mggcn_stream_t stream) {
    MGGCN_CHECK_HIP(hipStreamSynchronize(as_stream(stream)));
}

MGGCN_API mggcn_event_t mggcn_event_create(void) {
    hipEvent_t e = nullptr;
    MGGCN_CHECK_HIP(hipEventCreate(&e));
    return e;
}

MGGCN_API void mggcn_event_destroy(mggcn_event_t event) {
    if (event) MGGCN_CHECK_HIP(hipEventDestroy(reinterpret_cast<hipEvent_t>(event)));
}

MGGCN_API void mggcn_event_record(mggcn_event_t event, mggcn_stream_t stream) {
    MGGCN_CHECK_HIP(hipEventRecord(reinterpret_cast<hipEvent_t>(event), as_stream(stream)));
}

MGGCN_API void mggcn_stream_wait_event(mggcn_stream_t stream, mggcn_event_t event) {
    MGGCN_CHECK_HIP(hipStreamWaitEvent(as_stream(stream), reinterpret_cast<hipEvent_t>(event), 0));
}

MGGCN_API void mggcn_event_synchronize(mggcn_event_t event) {
    MGGCN_CHECK_HIP(hipEventSynchronize(reinterpret_cast<hipEvent_t>(event)));
}

MGGCN_API float mggcn_event_elapsed_ms(mggcn_event_t begin, mggcn_event_t end) {
    float ms = 0.f;
    MGGCN_CHECK_HIP(hipEventElapsedTime(&ms, reinterpret_cast<hipEvent_t>(begin),
                                        reinterpret_cast<hipEvent_t>(end)));
    return ms;
}

MGGCN_API void *mggcn_malloc(size_t bytes) {
    void *p = nullptr;
    if (bytes) MGGCN_CHECK_HIP(hipMalloc(&p, bytes));
    return p;
}

MGGCN_API void mggcn_free(void *device_ptr) {
    if (device_ptr) MGGCN_CHECK_HIP(hipFree(device_ptr));
}

MGGCN_API void *mggcn_malloc_host(size_t bytes) {
    void *p = nullptr;
    if (bytes) MGGCN_CHECK_HIP(hipHostMalloc(&p, bytes, hipHostMallocDefault));
    return p;
}

MGGCN_API void mggcn_free_host(void *host_ptr) {
    if (host_ptr) MGGCN_CHECK_HIP(hipHostFree(host_ptr));
}

MGGCN_API void mggcn_memcpy_h2d(void *dst, const void *src, size_t bytes, mggcn_stream_t stream) {
    if (bytes) MGGCN_CHECK_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, as_stream(stream)));
}

MGGCN_API void mggcn_memcpy_d2h(void *dst, const void *src, size_t bytes, mggcn_stream_t stream) {
    if (bytes) MGGCN_CHECK_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, as_stream(stream)));
}

MGGCN_API void mggcn_memcpy_d2d(void *dst, const void *src, size_t bytes, mggcn_stream_t stream) {
    if (bytes) MGGCN_CHECK_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, as_stream(stream)));
}

namespace {
__global__ __launch_bounds__(256) void zero_words_kernel(uint32_t *__restrict__ p, size_t n) {
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) p[i] = 0u;
}

__global__ __launch_bounds__(256) void occupy_kernel(const volatile uint32_t *stop, unsigned long long max_ticks) {
    // one wave slot per SIMD of whatever CU the block lands on, like a communication kernel's channel; leaves when told to
    // or when the time is up (100 MHz constant clock): every wave reaches one of the two
    // (the flag is looked at every ~50 us: sixty-four waves polling a host-memory word back to back delay every packet the
    // command processor fetches over the same path -- the first version of this stand-in slowed the LAUNCHES it was meant to
    // share the device with by 20 us per workgroup of its own)
    // the clock is read after every sleep (~3.5 us: the kernel also serves as a calibrated delay, rank_epoch_model_r04.py)
    const unsigned long long t0 = __builtin_amdgcn_s_memrealtime();
    for (unsigned it = 1; __builtin_amdgcn_s_memrealtime() - t0 < max_ticks; it++) {
        __builtin_amdgcn_s_sleep(127);
        if ((it & 15u) == 0 && *stop) break;
    }
}
}  // namespace

// Diagnostics (profiles/experiments/coresident_r04.py, never on the product path): n_blocks workgroups of 256 threads that
// do nothing but hold their wave slots until *stop_flag (device memory, or mapped pinned host memory) becomes non-zero or
// max_microseconds have passed -- a stand-in for the channels of a collective kernel that shares the device with the SpMM.
MGGCN_API void mggcn_debug_occupy_cus(mggcn_stream_t stream, uint32_t n_blocks, uint32_t max_microseconds, const uint32_t *stop_flag) {
    if (!n_blocks) return;
    hipLaunchKernelGGL(occupy_kernel, dim3(n_blocks), dim3(256), 0, as_stream(stream), stop_flag, (unsigned long long)max_microseconds * 100ull);
    MGGCN_CHECK_LAUNCH();
}

// Small word-aligned ranges (the loss layer's two scalars, a bias gradient) are zeroed by a kernel of this library, not by
// hipMemsetAsync: the runtime's fill path put a ~100 us bubble between its blit kernel and the next kernel of the stream
// (rocprofv3 kernel trace of an epoch, r02: fillBufferAligned -> softmax_xent 99 us on average, 10 us between ordinary
// kernels).  Works on device memory and on mapped pinned host memory (mggcn_malloc_host) alike.
MGGCN_API void mggcn_memset_zero(void *dst, size_t bytes, mggcn_stream_t stream) {
    if (!bytes) return;
    if (bytes <= (1u << 20) && bytes % 4 == 0 && (reinterpret_cast<uintptr_t>(dst) & 3u) == 0) {
        const size_t n = bytes / 4;
        hipLaunchKernelGGL(zero_words_kernel, dim3((unsigned)std::min<size_t>((n + 255) / 256, 1024)), dim3(256), 0,
                           as_stream(stream), static_cast<uint32_t *>(dst), n);
        MGGCN_CHECK_LAUNCH();
        return;
    }
    MGGCN_CHECK_HIP(hipMemsetAsync(dst, 0, bytes, as_stream(stream)));
}
