// The NN_11 learner step's entry points of include/toricenv.h (part of toricenv.hip's translation unit): NN_11's
// description over the shell all learner-step handles share (abi_grad.hpp).
#pragma once
#include "abi_grad.hpp"
#include "abi_nn11.hpp"

struct tq_nn11_grad : GradHandle<NN11Net, tq::NN11_LAYERS> {};

namespace {
struct NN11GradNet {
    static constexpr const char* NAME = "nn11";
    static constexpr int WAVES = tq::NN11_WG_WAVES, CHUNK_ROWS = tq::NN11_WG_CHUNK_ROWS, FEAT_CP = 64, FEAT = 64;
    int layers() const { return tq::NN11_LAYERS; }
    int cin(int l) const { return tq::nn11_cin(l); }
    int cout(int l) const { return tq::nn11_cout(l); }
    int mode(int l) const { return tq::nn11_mode(l); }
    int64_t dimg_offset(int l) const { return tq::nn11_dimg_offset(l); }
    template <int D>
    int forward(const NN11Net& net, const void* state, int dtype, int64_t n, uint16_t* const* act, float* q, hipStream_t stream) const {
        return nn11_forward<D>(net, state, dtype, n, act, q, stream);
    }
    template <int D>
    int dgrad(int mode, int ks, int nt, const uint16_t* g, const uint16_t* img, const uint16_t* mask, uint16_t* out, int64_t n,
              hipStream_t stream) const {
        return nn11_conv<D, tq::NN11_EPI_MASK>(mode, ks, nt, g, 0, img, mask, out, n, stream);
    }
};
}  // namespace

extern "C" {

int tq_nn11_grad_destroy(tq_nn11_grad* h) { return destroy_handle(h); }

int tq_nn11_grad_create(tq_nn11_grad** out, int d, int max_batch, int device) {
    return grad_create(out, "nn11 grad", d, max_batch, device, no_check, [&](tq_nn11_grad* h) {
        h->net.alloc(h->mem, d, true);
        return NN11GradNet{};
    });
}

int tq_nn11_grad_load(tq_nn11_grad* h, const float* const* weights, const float* const* biases, void* stream_) {
    ENTER(h, "nn11 grad handle");
    return h->net.load(h->d, weights, biases, stream);
}

int tq_nn11_grad_step(tq_nn11_grad* h, const void* state, int dtype, int n, const int64_t* actions_idx, const float* y, const float* w,
                      float* q, float* loss, float* const* grad_w, float* const* grad_b, void* stream_) {
    ENTER(h, "nn11 grad handle");
    return grad_step(NN11GradNet{}, h, state, dtype, n, actions_idx, y, w, q, loss, grad_w, grad_b, stream);
}

int tq_nn11_grad_check(tq_nn11_grad* h, void* stream_) {
    ENTER(h, "nn11 grad handle");
    return grad_check(NN11GradNet{}, h, stream);
}

}  // extern "C"
