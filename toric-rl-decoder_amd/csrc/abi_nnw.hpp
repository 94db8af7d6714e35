// The wide nets' forward (NN_8, NN_17): the tq_nnw_* entry points of include/toricenv.h (part of toricenv.hip's
// translation unit), over the frame all network handles share (abi_forward.hpp).
#pragma once
#include "abi_forward.hpp"
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
    const auto [grid, block] = conv_dims<D>(rows, nt);
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
    const int s = tq::nnw_slot(net);
    auto net_check = [&] { return s < 0 ? fail(TQ_E_INVALID, "net must be TQ_NET_NN8 or TQ_NET_NN17 (got %d)", net) : (int)TQ_OK; };
    return create_handle(out, "nnw", d, device, net_check, [&] { return max_rows_check(max_rows); }, [&](tq_nnw* h) {
        h->slot = s; h->max_rows = max_rows;
        const int L = tq::nnw_layers(s);
        h->mem.zeroed(&h->wimg, (size_t)tq::nnw_wimg_offset(s, L + 1) * sizeof(uint16_t));
        h->mem.zeroed(&h->bias, (size_t)tq::nnw_bias_offset(s, L + 1) * sizeof(float));
        h->mem.zeroed(&h->limg, (size_t)tq::nnw_lin_elems(d) * sizeof(float));
        h->mem.zeroed(&h->lbias, 16);
        for (int i = 0; i < 2; ++i)
            h->mem.zeroed(&h->act[i], (size_t)max_rows * d * d * tq::NNW_MAX_CP * sizeof(uint16_t));
    });
}

int tq_nnw_load(tq_nnw* h, const float* const* weights, const float* const* biases, void* stream_) {
    ENTER(h, "nnw handle");
    const int L = tq::nnw_layers(h->slot);
    tq::NNWPack p = {};
    if (int rc = pointer_lists(weights, biases, L + 1, p.w, p.b)) return rc;
    if (int rc = launch(tq::k_nnw_pack, dim3(64, L + 1), dim3(256), stream, p, h->slot, h->d, h->wimg, h->bias, h->limg, h->lbias)) return rc;
    h->loaded = 1;
    return TQ_OK;
}

int tq_nnw_forward(tq_nnw* h, const void* stack, int dtype, int64_t rows, float* q, void* stream_) {
    ENTER(h, "nnw handle");
    bool done;
    if (int rc = forward_args("nnw", h->loaded, stack, dtype, rows, q, &done); rc || done) return rc;
    return forward_passes(h->d, h->max_rows, stack, dtype, false, rows, q, [&](auto D, const void* s, int64_t, int64_t n, float* qn) {
        return nnw_forward<D()>(h, s, dtype, n, qn, stream);
    });
}

}  // extern "C"
