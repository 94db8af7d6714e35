// The wide nets' learner step: the tq_nnw_grad_* entry points of include/toricenv.h (part of toricenv.hip's translation
// unit): slot s of the network table described to the shell all learner-step handles share (abi_grad.hpp, which lists a
// handle's device memory).
#pragma once
#include "abi_grad.hpp"
#include "abi_nnw.hpp"

struct tq_nnw_grad : GradHandle<NNWNet, tq::NNW_MAX_LAYERS> {};

namespace {
struct NNWGradNet {
    static constexpr const char* NAME = "nnw";
    static constexpr int WAVES = tq::NNW_WG_WAVES, CHUNK_ROWS = tq::NNW_WG_CHUNK_ROWS, FEAT_CP = tq::NNW_FEAT_CP, FEAT = tq::NNW_FEAT;
    int s;                                 // tq::nnw_slot(net)
    int layers() const { return tq::nnw_layers(s); }
    int cin(int l) const { return tq::nnw_cin(s, l); }
    int cout(int l) const { return tq::nnw_cout(s, l); }
    int mode(int l) const { return tq::nnw_mode(s, l); }
    int64_t dimg_offset(int l) const { return tq::nnw_dimg_offset(s, l); }
    template <int D>
    int forward(const NNWNet& net, const void* state, int dtype, int64_t n, uint16_t* const* act, float* q, hipStream_t stream) const {
        return nnw_forward<D>(net, state, dtype, n, act, q, stream);
    }
    template <int D>
    int dgrad(int mode, int ks, int nt, const uint16_t* g, const uint16_t* img, const uint16_t* mask, uint16_t* out, int64_t n,
              hipStream_t stream) const {
        return nnw_conv<D, tq::NN11DgradMask>(mode, ks, nt, g, 0, img, mask, out, n, stream);
    }
};
}  // namespace

extern "C" {

int tq_nnw_grad_destroy(tq_nnw_grad* h) { return destroy_handle(h); }

int tq_nnw_grad_create(tq_nnw_grad** out, int net, int d, int max_batch, int device) {
    return grad_create(out, "nnw grad", d, max_batch, device, [&] { return nnw_net_check(net); }, [&](tq_nnw_grad* h) {
        h->net.alloc(h->mem, tq::nnw_slot(net), d, true);
        return NNWGradNet{h->net.slot};
    });
}

int tq_nnw_grad_load(tq_nnw_grad* h, const float* const* weights, const float* const* biases, void* stream_) {
    ENTER(h, "nnw grad handle");
    return h->net.load(h->d, weights, biases, stream);
}

int tq_nnw_grad_step(tq_nnw_grad* h, const void* state, int dtype, int n, const int64_t* actions_idx, const float* y, const float* w,
                     float* q, float* loss, float* const* grad_w, float* const* grad_b, void* stream_) {
    ENTER(h, "nnw grad handle");
    return grad_step(NNWGradNet{h->net.slot}, h, state, dtype, n, actions_idx, y, w, q, loss, grad_w, grad_b, stream);
}

int tq_nnw_grad_check(tq_nnw_grad* h, void* stream_) {
    ENTER(h, "nnw grad handle");
    return grad_check(NNWGradNet{h->net.slot}, h, stream);
}

}  // extern "C"
