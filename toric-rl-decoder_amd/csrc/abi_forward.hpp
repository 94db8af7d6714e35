// What the network handles' entry points share (part of toricenv.hip's translation unit): the constructor's frame, the
// argument checks of a forward, its walk over a call's rows in passes of max_rows, the copy of a caller's pointer lists
// and the grid of a convolution whose channels are cut across blockIdx.y.  Plain templates: a family passes its own
// lines as lambdas, and every kernel is still named where launch() (abi_util.hpp) is inlined.
#pragma once
#include <new>

#include "abi_util.hpp"
#include "nn11.hpp"

namespace {
// tq_*_create of a handle H made by `new H()` (every member zero) whose device memory is all in its `mem`.  Refused in
// this order: `out` NULL, net_check() (the family's own `net` argument; no_check where it has none), the lattice size,
// bound_check() (rows, batch, capacity ...), the device.  alloc(h) then finds h->d and h->device set and fills the rest.
inline int no_check() { return TQ_OK; }
template <class H, class NET, class BOUND, class ALLOC>
int create_handle(H** out, const char* what, int d, int device, NET&& net_check, BOUND&& bound_check, ALLOC&& alloc) {
    if (!out) return fail(TQ_E_INVALID, "out is NULL");
    *out = nullptr;
    if (int rc = net_check()) return rc;
    if (!tq::size_ok(d)) return bad_size(d);
    if (int rc = bound_check()) return rc;
    if (int rc = valid_device(device)) return rc;
    DeviceGuard guard;
    if (int rc = guard.enter_device(device)) return rc;
    H* h = new (std::nothrow) H();
    if (!h) return fail(TQ_E_INVALID, "out of host memory");
    h->d = d; h->device = device;
    alloc(h);
    hipError_t e = h->mem.err;
    if (e == hipSuccess) e = hipStreamSynchronize(nullptr);
    if (e != hipSuccess) { destroy_handle(h); return fail(TQ_E_HIP, "%s allocation failed: %s", what, hipGetErrorString(e)); }
    *out = h;
    return TQ_OK;
}
// the bound of the forward handles' max_rows
inline int max_rows_check(int64_t max_rows) {
    if (max_rows <= 0 || max_rows > (int64_t(1) << 24)) return fail(TQ_E_INVALID, "max_rows must be in 1..2^24 (got %lld)", (long long)max_rows);
    return TQ_OK;
}

// what every forward of `family` ("nn11", "nnw", "resnet") refuses before any launch; *done: nothing to do (no rows)
inline int forward_args(const char* family, int loaded, const void* stack, int dtype, int64_t rows, const float* q, bool* done) {
    *done = false;
    if (!loaded) return fail(TQ_E_INVALID, "%s forward before tq_%s_load", family, family);
    if (dtype < TQ_F32 || dtype > TQ_U8) return fail(TQ_E_INVALID, "bad stack dtype %d", dtype);
    if (rows < 0) return fail(TQ_E_INVALID, "negative rows");
    if (rows == 0) { *done = true; return TQ_OK; }
    if (!stack || !q) return fail(TQ_E_INVALID, "stack / q is NULL");
    REQUIRE_ALIGNED16(stack, "stack");
    REQUIRE_ALIGNED16(q, "q");
    return TQ_OK;
}

// The walk of a forward over `rows` perspectives in passes of at most max_rows: pass(D, stack_of_pass, first, n, q_of_pass)
// with the lattice size as a compile-time constant, for the n rows from `first` on.  A pass reads its rows where they lie
// in the stack, 2 d^2 elements of `dtype` each; `gathered`: every pass reads the one stack through a row list, and it is
// the list that the family advances by `first`.
template <class F>
int forward_passes(int d, int64_t max_rows, const void* stack, int dtype, bool gathered, int64_t rows, float* q, F&& pass) {
    const int64_t esize = dtype == TQ_F32 ? 4 : (dtype == TQ_U8 ? 1 : 2);
    const int64_t row_bytes = gathered ? 0 : 2 * (int64_t)d * d * esize;
    return by_size(d, [&](auto D) {
        for (int64_t first = 0; first < rows; first += max_rows) {
            const int64_t n = rows - first < max_rows ? rows - first : max_rows;
            if (int rc = pass(D, static_cast<const void*>(static_cast<const char*>(stack) + first * row_bytes), first, n,
                              q + first * tq::NN11_OUT)) return rc;
        }
        return (int)TQ_OK;
    });
}

// A caller's lists of n device pointers each, weights and biases, into a *Pack's w[] and b[]; a NULL list or entry is refused
inline int pointer_lists(const float* const* weights, const float* const* biases, int n, const float** w, const float** b) {
    if (!weights || !biases) return fail(TQ_E_INVALID, "weights / biases is NULL");
    for (int i = 0; i < n; ++i) {
        if (!weights[i] || !biases[i]) return fail(TQ_E_INVALID, "weights[%d] / biases[%d] is NULL", i, i);
        w[i] = weights[i]; b[i] = biases[i];
    }
    return TQ_OK;
}

// The launch geometry of a convolution over `rows` perspectives at grid side D whose `nt` n-tiles are cut across
// blockIdx.y, CONV_NTB to a workgroup
struct ConvDims { dim3 grid, block; };
template <int D>
ConvDims conv_dims(int64_t rows, int nt) {
    constexpr int G = tq::NN11Geom<D>::G, THREADS = tq::NN11Geom<D>::THREADS;
    return {dim3((unsigned)((rows + G - 1) / G), (unsigned)((nt + tq::CONV_NTB - 1) / tq::CONV_NTB)), dim3(THREADS)};
}
}  // namespace
