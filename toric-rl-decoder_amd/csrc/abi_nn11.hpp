// The NN_11 forward's entry points of include/toricenv.h (part of toricenv.hip's translation unit).
#pragma once
#include <new>

#include "abi_util.hpp"
#include "nn11.hpp"

struct tq_nn11 {                           // made by `new tq_nn11()`: every member starts as zero
    int d, device, loaded;
    int64_t max_rows;
    uint16_t* wimg;                        // the eleven conv layers' bf16 fragment images, back to back
    float* bias;                           // their padded f32 biases, back to back
    float* limg;                           // linear weights f32[3][(d-2)^2][64] (bf16-rounded values)
    float* lbias;                          // f32[3]
    uint16_t* act[2];                      // activation images of one pass, taking turns: max_rows * d^2 * 128 bf16 each
    DeviceBuffers mem;
};

namespace {
#define NHANDLE(h)                                                \
    DeviceGuard _guard;                                           \
    if (!(h)) return fail(TQ_E_INVALID, "NULL nn11 handle");      \
    if (int _rc = _guard.enter_device((h)->device)) return _rc;   \
    hipStream_t stream = (hipStream_t)stream_

template <int D, int KS, int NT, int MODE>
int nn11_conv(const tq_nn11* h, int l, const void* in, int dtype, uint16_t* out, int64_t rows, hipStream_t stream) {
    constexpr int G = tq::NN11Geom<D>::G, THREADS = tq::NN11Geom<D>::THREADS;
    return launch(tq::k_nn11_conv<D, KS, NT, MODE>, dim3((unsigned)((rows + G - 1) / G)), dim3(THREADS), stream, in, dtype,
                  h->wimg + tq::nn11_wimg_offset(l), h->bias + tq::nn11_bias_offset(l), out, rows);
}

// one pass of at most max_rows perspectives: conv1 from the stack, conv2..11 between the two images, the linear layer
template <int D>
int nn11_pass(const tq_nn11* h, const void* stack, int dtype, int64_t rows, float* q, hipStream_t stream) {
    uint16_t* a = h->act[0];
    uint16_t* b = h->act[1];
    if (int rc = nn11_conv<D, 2, 4, tq::NN11_CIRCULAR>(h, 1, stack, dtype, a, rows, stream)) return rc;
    for (int l = 2; l <= tq::NN11_LAYERS; ++l) {
        const int ks = tq::nn11_ksteps(l), nt = tq::nn11_ntiles(l);
        int rc;
        if (l == tq::NN11_LAYERS) rc = nn11_conv<D, 6, 2, tq::NN11_VALID>(h, l, a, 0, b, rows, stream);
        else if (ks == 8 && nt == 4) rc = nn11_conv<D, 8, 4, tq::NN11_ZERO>(h, l, a, 0, b, rows, stream);
        else if (ks == 8 && nt == 3) rc = nn11_conv<D, 8, 3, tq::NN11_ZERO>(h, l, a, 0, b, rows, stream);
        else if (ks == 6 && nt == 3) rc = nn11_conv<D, 6, 3, tq::NN11_ZERO>(h, l, a, 0, b, rows, stream);
        else rc = fail(TQ_E_INVALID, "nn11: no kernel for layer %d (%d k-steps, %d n-tiles)", l, ks, nt);
        if (rc) return rc;
        uint16_t* t = a; a = b; b = t;
    }
    return launch(tq::k_nn11_linear, dim3((unsigned)((rows + 3) / 4)), dim3(256), stream, a, h->limg, h->lbias, q, rows,
                  tq::nn11_out_pixels(D));
}
}  // namespace

extern "C" {

int tq_nn11_destroy(tq_nn11* h) {
    if (!h) return TQ_OK;
    DeviceGuard guard;
    (void)guard.enter_device(h->device);
    h->mem.release_all();
    (void)hipGetLastError();
    delete h;
    return TQ_OK;
}

int tq_nn11_create(tq_nn11** out, int d, int64_t max_rows, int device) {
    if (!out) return fail(TQ_E_INVALID, "out is NULL");
    *out = nullptr;
    if (!tq::size_ok(d)) return bad_size(d);
    if (max_rows <= 0 || max_rows > (int64_t(1) << 24)) return fail(TQ_E_INVALID, "max_rows must be in 1..2^24 (got %lld)", (long long)max_rows);
    if (int rc = valid_device(device)) return rc;
    DeviceGuard guard;
    if (int rc = guard.enter_device(device)) return rc;
    tq_nn11* h = new (std::nothrow) tq_nn11();
    if (!h) return fail(TQ_E_INVALID, "out of host memory");
    h->d = d; h->device = device; h->max_rows = max_rows;
    h->mem.zeroed(&h->wimg, (size_t)tq::nn11_wimg_offset(tq::NN11_LAYERS + 1) * sizeof(uint16_t));
    h->mem.zeroed(&h->bias, (size_t)tq::nn11_bias_offset(tq::NN11_LAYERS + 1) * sizeof(float));
    h->mem.zeroed(&h->limg, (size_t)tq::nn11_lin_elems(d) * sizeof(float));
    h->mem.zeroed(&h->lbias, 16);
    for (int i = 0; i < 2; ++i)
        h->mem.zeroed(&h->act[i], (size_t)max_rows * d * d * tq::NN11_MAX_CP * sizeof(uint16_t));
    hipError_t e = h->mem.err;
    if (e == hipSuccess) e = hipStreamSynchronize(nullptr);
    if (e != hipSuccess) { tq_nn11_destroy(h); return fail(TQ_E_HIP, "nn11 allocation failed: %s", hipGetErrorString(e)); }
    *out = h;
    return TQ_OK;
}

int tq_nn11_load(tq_nn11* h, const float* const* weights, const float* const* biases, void* stream_) {
    NHANDLE(h);
    if (!weights || !biases) return fail(TQ_E_INVALID, "weights / biases is NULL");
    tq::NN11Pack p;
    for (int i = 0; i <= tq::NN11_LAYERS; ++i) {
        if (!weights[i] || !biases[i]) return fail(TQ_E_INVALID, "weights[%d] / biases[%d] is NULL", i, i);
        p.w[i] = weights[i]; p.b[i] = biases[i];
    }
    if (int rc = launch(tq::k_nn11_pack, dim3(64, tq::NN11_LAYERS + 1), dim3(256), stream, p, h->d, h->wimg, h->bias, h->limg,
                        h->lbias)) return rc;
    h->loaded = 1;
    return TQ_OK;
}

int tq_nn11_forward(tq_nn11* h, const void* stack, int dtype, int64_t rows, float* q, void* stream_) {
    NHANDLE(h);
    if (!h->loaded) return fail(TQ_E_INVALID, "nn11 forward before tq_nn11_load");
    if (dtype < TQ_F32 || dtype > TQ_U8) return fail(TQ_E_INVALID, "bad stack dtype %d", dtype);
    if (rows < 0) return fail(TQ_E_INVALID, "negative rows");
    if (rows == 0) return TQ_OK;
    if (!stack || !q) return fail(TQ_E_INVALID, "stack / q is NULL");
    REQUIRE_ALIGNED16(stack, "stack");
    REQUIRE_ALIGNED16(q, "q");
    const int64_t esize = dtype == TQ_F32 ? 4 : (dtype == TQ_U8 ? 1 : 2);
    const int64_t row_bytes = 2 * (int64_t)h->d * h->d * esize;
    return by_size(h->d, [&](auto D) {
        for (int64_t first = 0; first < rows; first += h->max_rows) {
            const int64_t n = rows - first < h->max_rows ? rows - first : h->max_rows;
            if (int rc = nn11_pass<D()>(h, static_cast<const char*>(stack) + first * row_bytes, dtype, n,
                                        q + first * tq::NN11_OUT, stream)) return rc;
        }
        return (int)TQ_OK;
    });
}

}  // extern "C"
