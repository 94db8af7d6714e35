// What the C-ABI entry points of libtoricenv share (part of toricenv.hip's translation unit): the last-error text,
// the HIP checks, the device guard, the one way a kernel is launched, the reader of a device error latch and the
// device memory a handle owns.
#pragma once
#include "toricenv.h"

#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>
#include <stdarg.h>
#include <stdio.h>

#include <vector>

#include "kernels.hpp"

namespace {

thread_local char g_err[512] = "";

int fail(int code, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
}

// A failed HIP call is reported through the return code; the runtime's sticky "last error" is cleared so that the
// caller's next launch check (PyTorch's, say) does not trip over it.
#define HIPCHECK(expr)                                                                         \
    do {                                                                                       \
        hipError_t _e = (expr);                                                                \
        if (_e != hipSuccess) {                                                                \
            (void)hipGetLastError();                                                           \
            return fail(TQ_E_HIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), __FILE__, __LINE__); \
        }                                                                                      \
    } while (0)

#define KCHECK() HIPCHECK(hipGetLastError())

int bad_size(int d) { return fail(TQ_E_INVALID, "unsupported lattice size d=%d (odd 3..21)", d); }
// f(D) with the lattice size as a compile-time constant (tq::dispatch_size), so that f launches tq::k_x<D()>
template <class F>
int by_size(int d, F&& f) { return tq::dispatch_size(d, f, bad_size); }

// alignment contract of include/toricenv.h: the kernels use 16-byte vector accesses on these
inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }
#define REQUIRE_ALIGNED16(p, name)                                                        \
    do {                                                                                  \
        if ((p) && !aligned16(p)) return fail(TQ_E_INVALID, "%s must be 16-byte aligned", name); \
    } while (0)

// ---- launches: the arguments are converted to the kernel's parameter types, and the launch is checked.  Inlined by
// force: left to itself the compiler shares one copy between the ten sizes and launches through the kernel pointer.
template <typename... P, typename... A>
__forceinline__ int launch(void (*kernel)(P...), dim3 grid, dim3 block, hipStream_t stream, A&&... args) {
    hipLaunchKernelGGL(kernel, grid, block, 0, stream, static_cast<P>(args)...);
    KCHECK();
    return TQ_OK;
}
// The same with `done` (may be NULL) signalled by the kernel's own dispatch packet when the kernel has finished -- no
// barrier packet behind it, as hipEventRecord would enqueue.  Never on a stream that is being captured.
template <typename... P, typename... A>
__forceinline__ int launch_signal(void (*kernel)(P...), dim3 grid, dim3 block, hipStream_t stream, hipEvent_t done, A&&... args) {
    if (!done) return launch(kernel, grid, block, stream, args...);
    hipExtLaunchKernelGGL(kernel, grid, block, 0, stream, nullptr, done, 0, static_cast<P>(args)...);
    KCHECK();
    return TQ_OK;
}

// the thread-per-item kernels: blocks of BLOCK_1D threads over n items
constexpr int BLOCK_1D = 256;
static_assert(BLOCK_1D == tq::PART_BLOCK, "block_count_partial (scan.hpp) sums the counts of exactly one such block");
inline dim3 grid1(int64_t n) { return dim3((unsigned)((n + BLOCK_1D - 1) / BLOCK_1D)); }
template <typename... P, typename... A>
__forceinline__ int launch_1d(void (*kernel)(P...), int64_t n, hipStream_t stream, A&&... args) {
    return launch(kernel, grid1(n), dim3(BLOCK_1D), stream, args...);
}

// ---- devices
constexpr int MAX_DEVICES = 16;

int current_device(int* dev) {
    HIPCHECK(hipGetDevice(dev));
    if (*dev < 0 || *dev >= MAX_DEVICES) return fail(TQ_E_INVALID, "device %d out of range", *dev);
    return TQ_OK;
}

int valid_device(int device) {                 // of the handle constructors
    int ndev = 0;
    HIPCHECK(hipGetDeviceCount(&ndev));
    if (device < 0 || device >= ndev || device >= MAX_DEVICES)
        return fail(TQ_E_INVALID, "device %d not available (%d HIP devices)", device, ndev);
    return TQ_OK;
}

// Makes the handle's device current for the duration of one entry point and restores the caller's
// device on the way out (PyTorch callers already run under torch.cuda.device(...); C callers must
// not find their current device changed behind their back).
struct DeviceGuard {
    int prev = -1;
    bool switched = false;
    template <class H>
    int enter(const H* h) {
        if (!h) return fail(TQ_E_INVALID, "NULL handle");
        return enter_device(h->device);
    }
    int enter_device(int device) {
        if (int rc = current_device(&prev)) return rc;
        if (prev != device) {
            HIPCHECK(hipSetDevice(device));
            switched = true;
        }
        return TQ_OK;
    }
    ~DeviceGuard() { if (switched) (void)hipSetDevice(prev); }
};

// How an entry point that takes a handle and a `void* stream_` begins: NULL is refused as "NULL <what>", the handle's
// device is current until the entry point returns, and `stream` is the caller's stream.
#define ENTER(h, what)                                            \
    DeviceGuard _guard;                                           \
    if (!(h)) return fail(TQ_E_INVALID, "NULL " what);            \
    if (int _rc = _guard.enter_device((h)->device)) return _rc;   \
    hipStream_t stream = (hipStream_t)stream_

// tq_*_destroy of a handle whose device memory is all in its `mem` (a DeviceBuffers, below): NULL is fine, and a HIP
// error of the frees does not stay behind as the runtime's sticky one.
template <class H>
int destroy_handle(H* h) {
    if (!h) return TQ_OK;
    DeviceGuard guard;
    (void)guard.enter_device(h->device);
    h->mem.release_all();
    (void)hipGetLastError();
    delete h;
    return TQ_OK;
}

// Reads a device error latch (a word of ERR_* bits that kernels OR into) after everything queued on the stream,
// and clears it if it was set.  The caller decodes *flag.
int read_latch(int* device_word, hipStream_t stream, int* flag) {
    *flag = 0;
    HIPCHECK(hipMemcpyAsync(flag, device_word, sizeof(int), hipMemcpyDeviceToHost, stream));
    HIPCHECK(hipStreamSynchronize(stream));
    if (*flag) HIPCHECK(hipMemsetAsync(device_word, 0, sizeof(int), stream));
    return TQ_OK;
}

// The device memory a handle owns.  Buffers come zeroed (on the null stream); the first HIP error sticks and stops
// further allocation; and every buffer is remembered, so that a destructor frees what its constructor -- finished or
// not -- allocated without listing it again.
struct DeviceBuffers {
    std::vector<void*> owned;
    hipError_t err = hipSuccess;
    template <typename T>
    void zeroed(T** p, size_t bytes) {
        void* q = nullptr;
        if (err == hipSuccess) err = hipMalloc(&q, bytes);
        if (err != hipSuccess) return;
        owned.push_back(q);
        *p = static_cast<T*>(q);
        err = hipMemset(q, 0, bytes);
    }
    void release(void* p) {                    // one buffer, ahead of the rest (NULL or not owned: nothing)
        for (void*& o : owned)
            if (o == p) { (void)hipFree(p); o = owned.back(); owned.pop_back(); return; }
    }
    void release_all() {
        for (void* p : owned) (void)hipFree(p);
        owned.clear();
    }
};

}  // namespace
