// What the two NN_11 host shims (host_nn11_shim.cpp, host_nn11_grad_shim.cpp) share: the network as the product's own
// host pack routines (csrc/nn11.hpp) leave it, and the one scalar forward under the numerics contract of
// include/toricenv.h.  It reads the packed images, the activation images and the tap -> source pixel map ONLY through
// the header's index functions -- what the pack kernel and the MFMA kernels use on the device.
// The order of every sum is part of what the tests pin: within a pixel tap by tap, k ascending, then the bias, ReLU and
// RNE to bf16; the linear layer pixel by pixel, then channel.
// TEST ONLY: it is not a backend of the product.
#pragma once
#include <stdint.h>

#include <vector>

#include "nn11.hpp"

namespace tq {

// element (cout, k, tap) of a packed fragment image, expanded to [tap][k][cp_out] f32
inline std::vector<float> expand(const std::vector<uint16_t>& img, int taps, int ksteps, int ntiles) {
    const int kp = ksteps * 16, cp = ntiles * 32;
    std::vector<float> w((size_t)taps * kp * cp);
    for (int tap = 0; tap < taps; ++tap)
        for (int k = 0; k < kp; ++k)
            for (int c = 0; c < cp; ++c) w[((size_t)tap * kp + k) * cp + c] = nn11_f32(img[nn11_wimg_of(c, k, tap, ksteps, ntiles)]);
    return w;
}

// weights / biases: 12 host pointers each in torch layout (conv1..conv11, linear1)
struct PackedNet {
    std::vector<float> wt[NN11_LAYERS + 1];        // layer l's packed image, expanded: what the kernel finds
    std::vector<float> bias[NN11_LAYERS + 1];      // padded
    std::vector<float> limg;
    const float* lbias;

    PackedNet(int d, const float* const* weights, const float* const* biases) : limg(nn11_lin_elems(d)), lbias(biases[NN11_LAYERS]) {
        for (int l = 1; l <= NN11_LAYERS; ++l) {
            std::vector<uint16_t> img(nn11_wimg_elems(l));
            bias[l].resize(nn11_cpad(nn11_cout(l)));
            nn11_pack_layer_host(l, weights[l - 1], biases[l - 1], img.data(), bias[l].data());
            wt[l] = expand(img, nn11_taps(l), nn11_ksteps(l), nn11_ntiles(l));
        }
        nn11_pack_linear_host(d, weights[NN11_LAYERS], limg.data());
    }
};

// one perspective: stack u8 [2][d][d] -> q[3]; act[l], l = 1..11, receives layer l's bf16 image [pixels(l)][cpad(cout(l))]
// (layer l reads act[l - 1]: two buffers taking turns do when the images are not kept)
inline void forward_one(int d, const PackedNet& net, const uint8_t* stack, uint16_t* const* act, float* q) {
    const int pix = d * d;
    float acc[NN11_MAX_CP];
    for (int l = 1; l <= NN11_LAYERS; ++l) {
        const int mode = nn11_mode(l), cpo = nn11_cpad(nn11_cout(l)), cpi = nn11_cpad(nn11_cin(l));
        const int od = mode == NN11_VALID ? d - 2 : d, opix = od * od;
        const float* W = net.wt[l].data();                              // [tap][k][cpo]
        for (int o = 0; o < opix; ++o) {
            for (int c = 0; c < cpo; ++c) acc[c] = 0.f;
            for (int tap = 0; tap < 9; ++tap) {
                const int sp = nn11_src_pixel(mode, d, o / od, o % od, tap);
                if (sp < 0) continue;                                   // the zero padding
                if (l == 1) {
                    for (int ci = 0; ci < 2; ++ci) {
                        const float a = nn11_f32(nn11_bf16((float)stack[ci * pix + sp]));
                        if (a == 0.f) continue;
                        const float* w = W + (size_t)nn11_k1(ci, tap) * cpo;
                        for (int c = 0; c < cpo; ++c) acc[c] += a * w[c];
                    }
                } else {
                    for (int k = 0; k < cpi; ++k) {
                        const float a = nn11_f32(act[l - 1][nn11_act_index(0, sp, k, pix, cpi)]);
                        if (a == 0.f) continue;                         // adds +0: the sum is the same without it
                        const float* w = W + ((size_t)tap * cpi + k) * cpo;
                        for (int c = 0; c < cpo; ++c) acc[c] += a * w[c];
                    }
                }
            }
            for (int c = 0; c < cpo; ++c) {
                const float v = acc[c] + net.bias[l][c];
                act[l][nn11_act_index(0, o, c, opix, cpo)] = nn11_bf16(v > 0.f ? v : 0.f);
            }
        }
    }
    const int npix = nn11_out_pixels(d);
    for (int a = 0; a < NN11_OUT; ++a) {
        float s = 0.f;
        for (int p = 0; p < npix; ++p)
            for (int c = 0; c < 64; ++c)
                s += nn11_f32(act[NN11_LAYERS][nn11_act_index(0, p, c, npix, 64)]) * net.limg[nn11_lin_index(a, p, c, npix)];
        q[a] = s + net.lbias[a];
    }
}

}  // namespace tq
