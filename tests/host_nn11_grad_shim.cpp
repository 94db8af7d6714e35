// Host-side instantiation of the product's NN_11 learner-step headers (csrc/nn11.hpp, csrc/nn11_grad.hpp), beside
// host_nn11_shim.cpp: torch-layout weights are packed with the headers' own pack routines (forward and dgrad images), and
// the scalar learner step of host_grad_ref.hpp (the forward of host_conv_ref.hpp, a head and a backward) under the numerics
// contract of include/toricenv.h reads the images, the activation and gradient images and the tap -> source pixel maps
// ONLY through the headers' index functions -- what the pack kernels, the MFMA kernels and the head kernel use on the
// device.
// TEST ONLY: built by tests/test_nn11_grad_host.py into a temp dir with g++; it is not a backend of the product.
#include "host_grad_ref.hpp"

using namespace tq;

// weights / biases / grad_w / grad_b: 12 host pointers each in torch layout (conv1..conv11, linear1); stack u8
// [n][2][d][d]; w may be NULL -> q f32 [n][3], loss f32 [n], the 24 gradients (written)
extern "C" int shim_nn11_grad(int d, const float* const* weights, const float* const* biases, const uint8_t* stack, int n,
                              const int64_t* actions, const float* y, const float* w, float* q, float* loss,
                              float* const* grad_w, float* const* grad_b) {
    if (!size_ok(d) || n < 1) return -1;
    grad_host<NN11_MAX_CP>(d, nn11_packed(d, weights, biases), weights, stack, n, actions, y, w, q, loss, grad_w, grad_b);
    return 0;
}

// the dgrad image of layer l = 2..11 from torch's weight, by the header's host pack; -> its element count
extern "C" int64_t shim_nn11_dgrad_image(int l, const float* w, uint16_t* out) {
    if (out) nn11_pack_dgrad_host(l, w, out);
    return nn11_dimg_elems(l);
}
extern "C" int64_t shim_nn11_dimg_of(int l, int ci, int co, int tap) { return nn11_wimg_of(ci, co, tap, nn11_dksteps(l), nn11_dntiles(l)); }
extern "C" int shim_nn11_src_pixel(int mode, int d, int y, int x, int tap) { return nn11_src_pixel(mode, d, y, x, tap); }
extern "C" int shim_nn11_wgrad_persp(int d) { return nn11_wgrad_persp(d); }
// the head on `count` records of a batch of n
extern "C" void shim_nn11_head(int n, int count, const float* qa, const float* y, const float* w, float* loss, float* dq) {
    for (int i = 0; i < count; ++i) {
        const NN11Head h = nn11_head(qa[i], y[i], w ? w[i] : 1.f, n);
        loss[i] = h.loss;
        dq[i] = h.dq;
    }
}
