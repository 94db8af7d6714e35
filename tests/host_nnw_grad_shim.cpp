// Host-side instantiation of the wide nets' learner-step headers (csrc/nnw.hpp, csrc/nnw_grad.hpp), beside
// host_nn11_grad_shim.cpp: torch-layout weights are packed with the headers' own pack routines (forward and dgrad images),
// and the scalar learner step of host_grad_ref.hpp (the forward of host_conv_ref.hpp, NN_11's head and a backward) under
// the numerics contract of include/toricenv.h reads the images, the activation and gradient images and the tap -> source
// pixel maps ONLY through the headers' index functions -- what the pack kernels, the MFMA kernels and the head kernel use
// on the device.
// TEST ONLY: built by tests/test_nnw_grad_host.py into a temp dir with g++; it is not a backend of the product.
#include "host_grad_ref.hpp"
#include "nnw_grad.hpp"

using namespace tq;

// weights / biases / grad_w / grad_b: L + 1 host pointers each in torch layout (conv1..convL, linear1); stack u8
// [n][2][d][d]; w may be NULL -> q f32 [n][3], loss f32 [n], the 2 (L + 1) gradients (written)
extern "C" int shim_nnw_grad(int net_id, int d, const float* const* weights, const float* const* biases, const uint8_t* stack, int n,
                             const int64_t* actions, const float* y, const float* w, float* q, float* loss,
                             float* const* grad_w, float* const* grad_b) {
    const int s = nnw_slot(net_id);
    if (s < 0 || !size_ok(d) || n < 1) return -1;
    const int L = nnw_layers(s);
    std::vector<PlainLayer> layers;
    for (int l = 1; l <= L; ++l) layers.push_back({nnw_cin(s, l), nnw_cout(s, l), nnw_mode(s, l)});
    PackedNet net(layers, weights, biases, nnw_lin_elems(d), nnw_lin_index);
    nnw_pack_linear_host(d, weights[L], net.limg.data());
    grad_host<NNW_MAX_CP>(d, net, weights, stack, n, actions, y, w, q, loss, grad_w, grad_b);
    return 0;
}

// the dgrad image of a layer by its channel counts from torch's weight, by the header's host pack; -> its element count
extern "C" int64_t shim_nnw_dgrad_image(int cin, int cout, const float* w, uint16_t* out) {
    if (out) conv_pack_dgrad_host(cin, cout, w, out);
    return conv_dimg_elems(cin, cout);
}
extern "C" int64_t shim_nnw_dimg_of(int cin, int cout, int ci, int co, int tap) {
    return nn11_wimg_of(ci, co, tap, conv_dksteps(cout), conv_dntiles(cin));
}
extern "C" int64_t shim_nnw_dimg_offset(int net, int l) { return nnw_dimg_offset(nnw_slot(net), l); }
// out[2]: k-steps and n-tiles of layer l's dgrad
extern "C" void shim_nnw_dgrad_shape(int net, int l, int* out) {
    const int s = nnw_slot(net);
    out[0] = conv_dksteps(nnw_cout(s, l)); out[1] = conv_dntiles(nnw_cin(s, l));
}
extern "C" int shim_nnw_wgrad_persp(int d) { return nnw_wgrad_persp(d); }
extern "C" int64_t shim_nnw_wgrad_chunks(int d, int64_t n) { return nnw_wgrad_chunks(d, n); }
extern "C" int64_t shim_nnw_wpart_elems() { return NNW_WPART_ELEMS; }
extern "C" int shim_nnw_layer_pixels(int net, int l, int d) { return nnw_layer_pixels(nnw_slot(net), l, d); }
