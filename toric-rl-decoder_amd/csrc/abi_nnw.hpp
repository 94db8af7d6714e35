// The wide nets' forward (NN_8, NN_17): the tq_nnw_* entry points of include/toricenv.h (part of toricenv.hip's
// translation unit), after abi_nn11.hpp's conventions.
#pragma once
#include <new>

#include "abi_util.hpp"
#include "nnw.hpp"

struct tq_nnw {                            // made by `new tq_nnw()`: every member starts as zero
    int slot, d, device;                   // slot: tq::nnw_slot(net)
    int64_t max_rows;
    int loaded;
    uint16_t* wimg;                        // the conv layers' bf16 fragment images, back to back
    float* bias;                           // their padded f32 biases, back to back
    float* limg;                           // linear weights f32[3][(d-2)^2][224] (bf16-rounded values)
    float* lbias;                          // f32[3]
    uint16_t* act[2];                      // activation images of one pass, taking turns: max_rows * d^2 * 256 bf16 each
    DeviceBuffers mem;
};

namespace {
// One convolution over `rows` perspectives.  Every k_nnw_conv the library holds is in the list below, by (k-steps,
// n-tiles, mode): the five shapes the two nets need.
template <int D>
int nnw_conv(int mode, int ks, int nt, const void* in, int dtype, const uint16_t* img, const float* bias, uint16_t* out, int64_t rows,
             hipStream_t stream) {
    constexpr int G = tq::NN11Geom<D>::G, THREADS = tq::NN11Geom<D>::THREADS;
    const dim3 grid((unsigned)((rows + G - 1) / G), (unsigned)((nt + tq::CONV_NTB - 1) / tq::CONV_NTB)), block(THREADS);
#define NNW_SHAPE(KS, NT, MODE)                          \
    if (ks == KS && nt == NT && mode == tq::MODE)        \
        return launch(tq::k_nnw_conv<D, KS, NT, tq::MODE>, grid, block, stream, in, dtype, img, bias, out, rows)
    NNW_SHAPE(2, 8, NN11_CIRCULAR);
    NNW_SHAPE(16, 8, NN11_ZERO);
    NNW_SHAPE(16, 7, NN11_ZERO);
    NNW_SHAPE(14, 7, NN11_ZERO);
    NNW_SHAPE(14, 7, NN11_VALID);
#undef NNW_SHAPE
    return fail(TQ_E_INVALID, "nnw: no kernel for layer shape (%d k-steps, %d n-tiles, mode %d)", ks, nt, mode);
}

// The forward of `rows` <= max_rows perspectives: conv l reads the stack (l = 1) or the image conv l - 1 wrote and
// writes act[l & 1]; the linear layer reads the last one and writes q.
template <int D>
int nnw_forward(const tq_nnw* h, const void* stack, int dtype, int64_t rows, float* q, hipStream_t stream) {
    const int s = h->slot, L = tq::nnw_layers(s);
    for (int l = 1; l <= L; ++l) {
        const int cin = tq::nnw_cin(s, l), cout = tq::nnw_cout(s, l);
        if (int rc = nnw_conv<D>(tq::nnw_mode(s, l), tq::conv_ksteps(cin), tq::conv_ntiles(cout), l == 1 ? stack : h->act[(l - 1) & 1],
                                 l == 1 ? dtype : 0, h->wimg + tq::nnw_wimg_offset(s, l), h->bias + tq::nnw_bias_offset(s, l),
                                 h->act[l & 1], rows, stream)) return rc;
    }
    return launch(tq::k_nn_linear<tq::NNW_FEAT_CP>, dim3((unsigned)((rows + 3) / 4)), dim3(256), stream, h->act[L & 1], h->limg, h->lbias, q, rows,
                  tq::nn11_out_pixels(D));
}
}  // namespace

extern "C" {

int tq_nnw_destroy(tq_nnw* h) { return destroy_handle(h); }

int tq_nnw_create(tq_nnw** out, int net, int d, int64_t max_rows, int device) {
    if (!out) return fail(TQ_E_INVALID, "out is NULL");
    *out = nullptr;
    const int s = tq::nnw_slot(net);
    if (s < 0) return fail(TQ_E_INVALID, "net must be TQ_NET_NN8 or TQ_NET_NN17 (got %d)", net);
    if (!tq::size_ok(d)) return bad_size(d);
    if (max_rows <= 0 || max_rows > (int64_t(1) << 24)) return fail(TQ_E_INVALID, "max_rows must be in 1..2^24 (got %lld)", (long long)max_rows);
    if (int rc = valid_device(device)) return rc;
    DeviceGuard guard;
    if (int rc = guard.enter_device(device)) return rc;
    tq_nnw* h = new (std::nothrow) tq_nnw();
    if (!h) return fail(TQ_E_INVALID, "out of host memory");
    h->slot = s; h->d = d; h->device = device; h->max_rows = max_rows;
    const int L = tq::nnw_layers(s);
    h->mem.zeroed(&h->wimg, (size_t)tq::nnw_wimg_offset(s, L + 1) * sizeof(uint16_t));
    h->mem.zeroed(&h->bias, (size_t)tq::nnw_bias_offset(s, L + 1) * sizeof(float));
    h->mem.zeroed(&h->limg, (size_t)tq::nnw_lin_elems(d) * sizeof(float));
    h->mem.zeroed(&h->lbias, 16);
    for (int i = 0; i < 2; ++i)
        h->mem.zeroed(&h->act[i], (size_t)max_rows * d * d * tq::NNW_MAX_CP * sizeof(uint16_t));
    hipError_t e = h->mem.err;
    if (e == hipSuccess) e = hipStreamSynchronize(nullptr);
    if (e != hipSuccess) { tq_nnw_destroy(h); return fail(TQ_E_HIP, "nnw allocation failed: %s", hipGetErrorString(e)); }
    *out = h;
    return TQ_OK;
}

int tq_nnw_load(tq_nnw* h, const float* const* weights, const float* const* biases, void* stream_) {
    ENTER(h, "nnw handle");
    const int L = tq::nnw_layers(h->slot);
    if (!weights || !biases) return fail(TQ_E_INVALID, "weights / biases is NULL");
    tq::NNWPack p = {};
    for (int i = 0; i <= L; ++i) {
        if (!weights[i] || !biases[i]) return fail(TQ_E_INVALID, "weights[%d] / biases[%d] is NULL", i, i);
        p.w[i] = weights[i]; p.b[i] = biases[i];
    }
    if (int rc = launch(tq::k_nnw_pack, dim3(64, L + 1), dim3(256), stream, p, h->slot, h->d, h->wimg, h->bias, h->limg, h->lbias)) return rc;
    h->loaded = 1;
    return TQ_OK;
}

int tq_nnw_forward(tq_nnw* h, const void* stack, int dtype, int64_t rows, float* q, void* stream_) {
    ENTER(h, "nnw handle");
    if (!h->loaded) return fail(TQ_E_INVALID, "nnw forward before tq_nnw_load");
    if (dtype < TQ_F32 || dtype > TQ_U8) return fail(TQ_E_INVALID, "bad stack dtype %d", dtype);
    if (rows < 0) return fail(TQ_E_INVALID, "negative rows");
    if (rows == 0) return TQ_OK;
    if (!stack || !q) return fail(TQ_E_INVALID, "stack / q is NULL");
    REQUIRE_ALIGNED16(stack, "stack");
    REQUIRE_ALIGNED16(q, "q");
    const int64_t esize = dtype == TQ_F32 ? 4 : (dtype == TQ_U8 ? 1 : 2);
    const int64_t row_bytes = 2 * (int64_t)h->d * h->d * esize;
    return by_size(h->d, [&](auto D) {                     // passes of at most max_rows perspectives
        for (int64_t first = 0; first < rows; first += h->max_rows) {
            const int64_t n = rows - first < h->max_rows ? rows - first : h->max_rows;
            if (int rc = nnw_forward<D()>(h, static_cast<const char*>(stack) + first * row_bytes, dtype, n,
                                          q + first * tq::NN11_OUT, stream)) return rc;
        }
        return (int)TQ_OK;
    });
}

}  // extern "C"
