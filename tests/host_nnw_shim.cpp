// Host-side instantiation of the wide nets' header (csrc/nnw.hpp), beside host_nn11_shim.cpp: the network table, the
// index functions and the host pack routines as the pack kernel and the conv kernel use them, and one scalar forward
// under the numerics contract of include/toricenv.h that reads the packed images ONLY through those index functions.
// TEST ONLY: built by tests/test_nnw_host.py into a temp dir with g++; it is not a backend of the product.
#include <vector>

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

// weights / biases: layers + 1 host pointers each in torch layout; stack u8 [P][2][d][d] -> q f32 [P][3].  Sums within a
// pixel tap by tap, k ascending, then the bias, ReLU and RNE to bf16; the linear layer pixel by pixel, then channel.
extern "C" int shim_nnw_forward(int net, int d, const float* const* weights, const float* const* biases, const uint8_t* stack,
                                int64_t P, float* q) {
    const int s = nnw_slot(net);
    if (s < 0 || !size_ok(d)) return -1;
    const int L = nnw_layers(s), pix = d * d, npix = nn11_out_pixels(d);
    std::vector<std::vector<uint16_t>> img(L + 1);
    std::vector<std::vector<float>> bias(L + 1);
    for (int l = 1; l <= L; ++l) {
        const int cin = nnw_cin(s, l), cout = nnw_cout(s, l);
        img[l].resize(nnw_wimg_elems(cin, cout));
        bias[l].resize(nn11_cpad(cout));
        nnw_pack_layer_host(cin, cout, weights[l - 1], biases[l - 1], img[l].data(), bias[l].data());
    }
    std::vector<float> limg(nnw_lin_elems(d));
    nnw_pack_linear_host(d, weights[L], limg.data());
#pragma omp parallel for schedule(dynamic, 1)
    for (int64_t p = 0; p < P; ++p) {
        std::vector<uint16_t> buf[2] = {std::vector<uint16_t>((size_t)pix * NNW_MAX_CP), std::vector<uint16_t>((size_t)pix * NNW_MAX_CP)};
        float acc[NNW_MAX_CP];
        for (int l = 1; l <= L; ++l) {
            const int cin = nnw_cin(s, l), mode = nnw_mode(s, l), ks = nnw_ksteps(cin), nt = nnw_ntiles(nnw_cout(s, l));
            const int cpo = nt * 32, cpi = ks * 16, od = mode == NN11_VALID ? d - 2 : d, opix = od * od;
            const uint16_t* in = buf[(l - 1) & 1].data();
            uint16_t* out = buf[l & 1].data();
            for (int o = 0; o < opix; ++o) {
                for (int c = 0; c < cpo; ++c) acc[c] = 0.f;
                for (int tap = 0; tap < 9; ++tap) {
                    const int sp = nn11_src_pixel(mode, d, o / od, o % od, tap);
                    if (sp < 0) continue;                               // the zero padding
                    for (int k = 0; k < (l == 1 ? 2 : cpi); ++k) {
                        const float a = l == 1 ? nn11_f32(nn11_bf16((float)stack[p * 2 * pix + k * pix + sp]))
                                               : nn11_f32(in[nn11_act_index(0, sp, k, pix, cpi)]);
                        if (a == 0.f) continue;                         // adds +0: the sum is the same without it
                        for (int c = 0; c < cpo; ++c)
                            acc[c] += a * nn11_f32(img[l][l == 1 ? nn11_wimg_of(c, nn11_k1(k, tap), 0, ks, nt) : nn11_wimg_of(c, k, tap, ks, nt)]);
                    }
                }
                for (int c = 0; c < cpo; ++c) {
                    const float v = acc[c] + bias[l][c];
                    out[nn11_act_index(0, o, c, opix, cpo)] = nn11_bf16(v > 0.f ? v : 0.f);
                }
            }
        }
        const uint16_t* feat = buf[L & 1].data();
        for (int a = 0; a < NN11_OUT; ++a) {
            float sum = 0.f;
            for (int o = 0; o < npix; ++o)
                for (int c = 0; c < NNW_FEAT_CP; ++c)
                    sum += nn11_f32(feat[nn11_act_index(0, o, c, npix, NNW_FEAT_CP)]) * limg[nnw_lin_index(a, o, c, npix)];
            q[p * NN11_OUT + a] = sum + biases[L][a];
        }
    }
    return 0;
}
