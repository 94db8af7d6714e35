// Host-side instantiation of the wide nets' header (csrc/nnw.hpp), beside host_nn11_shim.cpp: the network table, the
// index functions and the host pack routines as the pack kernel and the conv kernel use them, and the scalar forward of
// host_conv_ref.hpp over them.
// TEST ONLY: built by tests/test_nnw_host.py into a temp dir with g++; it is not a backend of the product.
#include "host_conv_ref.hpp"
#include "nnw.hpp"

using namespace tq;

extern "C" int shim_nnw_slot(int net) { return nnw_slot(net); }
extern "C" int shim_nnw_layers(int net) { return nnw_layers(nnw_slot(net)); }
// out[8]: cin, cout, mode, taps, k-steps, n-tiles, bias offset, chunks of layer l = 1..layers
extern "C" void shim_nnw_layer(int net, int l, int* out) {
    const int s = nnw_slot(net), cin = nnw_cin(s, l), cout = nnw_cout(s, l);
    out[0] = cin; out[1] = cout; out[2] = nnw_mode(s, l); out[3] = nnw_taps(cin); out[4] = nnw_ksteps(cin);
    out[5] = nnw_ntiles(cout); out[6] = nnw_bias_offset(s, l); out[7] = nnw_chunks(nnw_ksteps(cin));
}
extern "C" int64_t shim_nnw_wimg_offset(int net, int l) { return nnw_wimg_offset(nnw_slot(net), l); }     // l = layers + 1: the size
extern "C" int shim_nnw_bias_offset(int net, int l) { return nnw_bias_offset(nnw_slot(net), l); }
extern "C" int64_t shim_nnw_wimg_elems(int cin, int cout) { return nnw_wimg_elems(cin, cout); }
extern "C" int64_t shim_nnw_wimg_of(int cout, int k, int tap, int ksteps, int ntiles) { return nn11_wimg_of(cout, k, tap, ksteps, ntiles); }
extern "C" void shim_nnw_wimg_coord(int64_t idx, int ksteps, int ntiles, int* out) {
    const NN11WCoord c = nn11_wimg_coord(idx, ksteps, ntiles);
    out[0] = c.cout; out[1] = c.k; out[2] = c.tap;
}
extern "C" int64_t shim_nnw_lin_elems(int d) { return nnw_lin_elems(d); }
extern "C" int64_t shim_nnw_lin_index(int a, int pixel, int c, int npix) { return nnw_lin_index(a, pixel, c, npix); }
extern "C" void shim_nnw_pack_layer(int cin, int cout, const float* w, const float* b, uint16_t* wimg, float* bias) {
    nnw_pack_layer_host(cin, cout, w, b, wimg, bias);
}
extern "C" void shim_nnw_pack_linear(int d, const float* w, float* limg) { nnw_pack_linear_host(d, w, limg); }

// weights / biases: layers + 1 host pointers each in torch layout; stack u8 [P][2][d][d] -> q f32 [P][3]
extern "C" int shim_nnw_forward(int net, int d, const float* const* weights, const float* const* biases, const uint8_t* stack,
                                int64_t P, float* q) {
    const int s = nnw_slot(net);
    if (s < 0 || !size_ok(d)) return -1;
    const int L = nnw_layers(s), pix = d * d;
    std::vector<PlainLayer> layers;
    for (int l = 1; l <= L; ++l) layers.push_back({nnw_cin(s, l), nnw_cout(s, l), nnw_mode(s, l)});
    PackedNet packed(layers, weights, biases, nnw_lin_elems(d), nnw_lin_index);
    nnw_pack_linear_host(d, weights[L], packed.limg.data());
#pragma omp parallel for schedule(dynamic, 1)
    for (int64_t p = 0; p < P; ++p) {
        std::vector<uint16_t> buf[2] = {std::vector<uint16_t>((size_t)pix * NNW_MAX_CP), std::vector<uint16_t>((size_t)pix * NNW_MAX_CP)};
        uint16_t* act[NNW_MAX_LAYERS + 1];
        for (int l = 0; l <= L; ++l) act[l] = buf[l & 1].data();
        forward_one<NNW_MAX_CP>(d, packed, stack + p * 2 * pix, act, q + p * NN11_OUT);
    }
    return 0;
}
