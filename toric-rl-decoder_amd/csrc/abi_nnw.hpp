// The wide nets' forward (NN_8, NN_17): the tq_nnw_* entry points of include/toricenv.h (part of toricenv.hip's
// translation unit), over the frame all network handles share (abi_forward.hpp), and what they share with the learner
// step's (abi_nnw_grad.hpp): the packed network on the device, the one launcher of k_nnw_conv and the forward over it.
#pragma once
#include <type_traits>

#include "abi_forward.hpp"
#include "nnw_grad.hpp"

namespace {
// The packed network of one handle.
struct NNWNet {
    int slot, loaded;                      // slot: tq::nnw_slot(net)
    uint16_t* wimg;                        // the conv layers' bf16 fragment images, back to back
    float* bias;                           // their padded f32 biases, back to back
    float* limg;                           // linear weights f32[3][(d-2)^2][224] (bf16-rounded values)
    float* lbias;                          // f32[3]
    uint16_t* dimg;                        // the dgrad fragment images of conv2.., back to back; NULL: forward only

    void alloc(DeviceBuffers& mem, int s, int d, bool with_dgrad) {
        slot = s;
        const int L = tq::nnw_layers(s);
        mem.zeroed(&wimg, (size_t)tq::nnw_wimg_offset(s, L + 1) * sizeof(uint16_t));
        mem.zeroed(&bias, (size_t)tq::nnw_bias_offset(s, L + 1) * sizeof(float));
        mem.zeroed(&limg, (size_t)tq::nnw_lin_elems(d) * sizeof(float));
        mem.zeroed(&lbias, 16);
        if (with_dgrad) mem.zeroed(&dimg, (size_t)tq::nnw_dimg_offset(s, L + 1) * sizeof(uint16_t));
    }
    // torch-layout f32 weights and biases (L + 1 device pointers each) -> the images, on `stream`
    int load(int d, const float* const* weights, const float* const* biases, hipStream_t stream) {
        const int L = tq::nnw_layers(slot);
        tq::NNWPack p = {};
        if (int rc = pointer_lists(weights, biases, L + 1, p.w, p.b)) return rc;
        if (int rc = launch(tq::k_nnw_pack, dim3(64, L + 1), dim3(256), stream, p, slot, d, wimg, bias, limg, lbias)) return rc;
        if (dimg)
            if (int rc = launch(tq::k_nnw_pack_dgrad, dim3(64, L - 1), dim3(256), stream, p, slot, dimg)) return rc;
        loaded = 1;
        return TQ_OK;
    }
};

// One convolution over `rows` perspectives.  Every k_nnw_conv the library holds is in the list below, by (k-steps,
// n-tiles, mode): the five shapes the two nets' forward needs (EPI = ConvBiasRelu, `aux` the padded bias) and the four of
// their dgrad (NN11DgradMask, `aux` the activation image whose sign masks; k-steps of the layer's output channels, n-tiles
// of its input channels).
template <int D, class EPI = tq::ConvBiasRelu>
int nnw_conv(int mode, int ks, int nt, const void* in, int dtype, const uint16_t* img, const typename EPI::Aux* aux, uint16_t* out,
             int64_t rows, hipStream_t stream) {
    const auto [grid, block] = conv_dims<D>(rows, nt);
#define NNW_SHAPE(KS, NT, MODE)                          \
    if (ks == KS && nt == NT && mode == tq::MODE)        \
        return launch(tq::k_nnw_conv<D, KS, NT, tq::MODE, EPI>, grid, block, stream, in, dtype, img, aux, out, rows)
    if constexpr (std::is_same_v<EPI, tq::ConvBiasRelu>) {
        NNW_SHAPE(2, 8, NN11_CIRCULAR);
        NNW_SHAPE(16, 8, NN11_ZERO);
        NNW_SHAPE(16, 7, NN11_ZERO);
        NNW_SHAPE(14, 7, NN11_ZERO);
        NNW_SHAPE(14, 7, NN11_VALID);
    } else {
        NNW_SHAPE(16, 8, NN11_ZERO);
        NNW_SHAPE(14, 8, NN11_ZERO);
        NNW_SHAPE(14, 7, NN11_ZERO);
        NNW_SHAPE(14, 7, NN11_FULL);
    }
#undef NNW_SHAPE
    return fail(TQ_E_INVALID, "nnw: no kernel for layer shape (%d k-steps, %d n-tiles, mode %d, %s)", ks, nt, mode,
                std::is_same_v<EPI, tq::ConvBiasRelu> ? "forward" : "dgrad");
}

// The forward of `rows` perspectives: conv l = 1..L writes its bf16 image to out[l] (conv1 reads the stack, conv l reads
// out[l - 1]), the linear layer reads out[L] and writes q.
template <int D>
int nnw_forward(const NNWNet& net, const void* stack, int dtype, int64_t rows, uint16_t* const* out, float* q, hipStream_t stream) {
    const int s = net.slot, L = tq::nnw_layers(s);
    for (int l = 1; l <= L; ++l) {
        const int cin = tq::nnw_cin(s, l), cout = tq::nnw_cout(s, l);
        if (int rc = nnw_conv<D>(tq::nnw_mode(s, l), tq::conv_ksteps(cin), tq::conv_ntiles(cout), l == 1 ? stack : out[l - 1],
                                 l == 1 ? dtype : 0, net.wimg + tq::nnw_wimg_offset(s, l), net.bias + tq::nnw_bias_offset(s, l),
                                 out[l], rows, stream)) return rc;
    }
    return launch(tq::k_nn_linear<tq::NNW_FEAT_CP>, dim3((unsigned)((rows + 3) / 4)), dim3(256), stream, out[L], net.limg, net.lbias, q, rows,
                  tq::nn11_out_pixels(D));
}

inline int nnw_net_check(int net) {
    return tq::nnw_slot(net) < 0 ? fail(TQ_E_INVALID, "net must be TQ_NET_NN8 or TQ_NET_NN17 (got %d)", net) : (int)TQ_OK;
}
}  // namespace

struct tq_nnw {                            // made by `new tq_nnw()`: every member starts as zero
    int d, device;
    int64_t max_rows;
    NNWNet net;
    uint16_t* act[2];                      // activation images of one pass, taking turns: max_rows * d^2 * 256 bf16 each
    uint16_t* out[tq::NNW_MAX_LAYERS + 1]; // out[l], l = 1..L: the one of the two that layer l writes
    DeviceBuffers mem;
};

extern "C" {

int tq_nnw_destroy(tq_nnw* h) { return destroy_handle(h); }

int tq_nnw_create(tq_nnw** out, int net, int d, int64_t max_rows, int device) {
    return create_handle(out, "nnw", d, device, [&] { return nnw_net_check(net); }, [&] { return max_rows_check(max_rows); }, [&](tq_nnw* h) {
        h->max_rows = max_rows;
        h->net.alloc(h->mem, tq::nnw_slot(net), d, false);
        for (int i = 0; i < 2; ++i)
            h->mem.zeroed(&h->act[i], (size_t)max_rows * d * d * tq::NNW_MAX_CP * sizeof(uint16_t));
        for (int l = 1; l <= tq::NNW_MAX_LAYERS; ++l) h->out[l] = h->act[l & 1];
    });
}

int tq_nnw_load(tq_nnw* h, const float* const* weights, const float* const* biases, void* stream_) {
    ENTER(h, "nnw handle");
    return h->net.load(h->d, weights, biases, stream);
}

int tq_nnw_forward(tq_nnw* h, const void* stack, int dtype, int64_t rows, float* q, void* stream_) {
    ENTER(h, "nnw handle");
    bool done;
    if (int rc = forward_args("nnw", h->net.loaded, stack, dtype, rows, q, &done); rc || done) return rc;
    return forward_passes(h->d, h->max_rows, stack, dtype, false, rows, q, [&](auto D, const void* s, int64_t, int64_t n, float* qn) {
        return nnw_forward<D()>(h->net, s, dtype, n, h->out, qn, stream);
    });
}

}  // extern "C"
