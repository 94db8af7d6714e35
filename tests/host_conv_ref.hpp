// What the host shims of the networks (host_nn11_shim.cpp, host_nn11_grad_shim.cpp, host_nnw_shim.cpp,
// host_resnet_shim.cpp) share: one scalar convolution under the numerics contract of include/toricenv.h, the host twin of
// conv_tiles<Shape, ..., Epi> (csrc/conv_tile.hpp), and over it a plain net (conv layers, then one linear layer) as the
// product's own host pack routines (csrc/nn11.hpp) leave it.  They read the packed images, the activation images and the
// tap -> source pixel map ONLY through the headers' index functions -- what the pack kernels and the MFMA kernels use on
// the device.
// The order of every sum is part of what the tests pin, and it is the one the shims had each for itself: within a pixel
// tap by tap, k ascending, a term whose activation is 0 left out; then the epilogue and one RNE to bf16; the linear layer
// pixel by pixel, then channel.
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

// One convolution of one perspective.  W: the expanded image [tap][16 ksteps][32 ntiles]; the input is the bf16 image `in`
// [in_pix][16 ksteps] or, where `stack` is given, the u8 stack [2][in_pix], whose k = nn11_k1(channel, tap) lies in the
// image's one tap; out: [oside^2][32 ntiles] bf16.  src(y, x, tap) -> the source pixel of output pixel (y, x), or -1 for
// the zero padding; epi(sum, channel, element index in out) -> the f32 that is rounded.  MAX_CP: the output channels of
// the caller's widest layer (32 ntiles at most).  It is a template argument and not one bound of 512 for all because the
// NN_11 suites are the long ones and spend their time here: shim_nn11_forward on 1024 perspectives of an integer net at
// d = 13 (g++ -O3 -march=native, 8 threads, three runs each) took 1.27-1.42 s with acc[128] and 1.62-1.79 s with acc[512],
// against 1.31-1.50 s for the forward this one replaced; at d = 7 on 2048, 0.69-0.78 and 1.00-1.04 s against 0.78-0.89 s;
// with a std::vector sized to the layer, d = 13 on 512, 0.91-0.96 s against 0.74-0.82 s.
template <int MAX_CP, typename Src, typename Epi>
inline void conv_host(const float* W, int taps, int ksteps, int ntiles, int oside, int in_pix, const uint8_t* stack, const uint16_t* in,
                      Src src, Epi epi, uint16_t* out) {
    const int cpi = ksteps * 16, cpo = ntiles * 32, opix = oside * oside;
    float acc[MAX_CP];
    // rows of W that hold an inf or a NaN: 0 times such a weight is a NaN, so the term is not left out, not even for
    // the zero padding (torch and the MFMA kernels multiply there as well)
    const int wrows = (stack ? 1 : taps) * cpi;
    std::vector<uint8_t> odd(wrows, 0);
    bool any_odd = false;
    for (int r = 0; r < wrows; ++r) {
        for (int c = 0; c < cpo && !odd[r]; ++c) odd[r] = !(W[(size_t)r * cpo + c] - W[(size_t)r * cpo + c] == 0.f);
        any_odd = any_odd || odd[r];
    }
    for (int o = 0; o < opix; ++o) {
        for (int c = 0; c < cpo; ++c) acc[c] = 0.f;
        for (int tap = 0; tap < taps; ++tap) {
            const int sp = src(o / oside, o % oside, tap);
            if (sp < 0 && !any_odd) continue;                           // the zero padding
            if (stack) {
                for (int ci = 0; ci < 2; ++ci) {
                    const int k = nn11_k1(ci, tap);
                    const float a = sp < 0 ? 0.f : nn11_f32(nn11_bf16((float)stack[ci * in_pix + sp]));
                    if (a == 0.f && !odd[k]) continue;
                    const float* w = W + (size_t)k * cpo;
                    for (int c = 0; c < cpo; ++c) acc[c] += a * w[c];
                }
                continue;
            }
            for (int k = 0; k < cpi; ++k) {
                const float a = sp < 0 ? 0.f : nn11_f32(in[nn11_act_index(0, sp, k, in_pix, cpi)]);
                if (a == 0.f && !odd[tap * cpi + k]) continue;          // adds +0: the sum is the same without it
                const float* w = W + ((size_t)tap * cpi + k) * cpo;
                for (int c = 0; c < cpo; ++c) acc[c] += a * w[c];
            }
        }
        for (int c = 0; c < cpo; ++c) {
            const int64_t at = nn11_act_index(0, o, c, opix, cpo);
            out[at] = nn11_bf16(epi(acc[c], c, at));
        }
    }
}

// A plain net, packed: conv layer l = 1..L by (cin, cout, mode), then the linear layer over feat_cp features per pixel,
// whose image the shim packs and indexes with its family's functions (NN_11: nn11_lin_*, 64; the wide nets: nnw_lin_*, 224).
struct PlainLayer { int cin, cout, mode; };
struct PackedNet {
    std::vector<PlainLayer> layer;                 // [l - 1]
    std::vector<std::vector<float>> wt, bias;      // [l]: the packed image, expanded: what the kernel finds; the padded bias
    std::vector<float> limg;
    int64_t (*lin_index)(int a, int pixel, int c, int npix);
    const float* lbias;

    // weights / biases: L + 1 host pointers each in torch layout (conv1..convL, linear1)
    PackedNet(const std::vector<PlainLayer>& layers, const float* const* weights, const float* const* biases, int64_t lin_elems,
              int64_t (*lin_index_)(int, int, int, int))
        : layer(layers), wt(layers.size() + 1), bias(layers.size() + 1), limg(lin_elems), lin_index(lin_index_), lbias(biases[layers.size()]) {
        for (int l = 1; l <= (int)layer.size(); ++l) {
            const int cin = layer[l - 1].cin, cout = layer[l - 1].cout;
            std::vector<uint16_t> img(conv_wimg_elems(cin, cout, 9));
            bias[l].resize(nn11_cpad(cout));
            conv_pack_layer_host(cin, cout, 9, weights[l - 1], biases[l - 1], img.data(), bias[l].data());
            wt[l] = expand(img, conv_img_taps(cin, 9), conv_ksteps(cin), conv_ntiles(cout));
        }
    }
};

inline PackedNet nn11_packed(int d, const float* const* weights, const float* const* biases) {
    std::vector<PlainLayer> layers;
    for (int l = 1; l <= NN11_LAYERS; ++l) layers.push_back({nn11_cin(l), nn11_cout(l), nn11_mode(l)});
    PackedNet net(layers, weights, biases, nn11_lin_elems(d), nn11_lin_index);
    nn11_pack_linear_host(d, weights[NN11_LAYERS], net.limg.data());
    return net;
}

// one perspective: stack u8 [2][d][d] -> q[3]; act[l], l = 1..L, receives layer l's bf16 image [pixels(l)][cpad(cout(l))]
// (layer l reads act[l - 1]: two buffers taking turns do when the images are not kept)
template <int MAX_CP>
inline void forward_one(int d, const PackedNet& net, const uint8_t* stack, uint16_t* const* act, float* q) {
    const int L = (int)net.layer.size();
    for (int l = 1; l <= L; ++l) {
        const PlainLayer& y = net.layer[l - 1];
        const float* bias = net.bias[l].data();
        conv_host<MAX_CP>(net.wt[l].data(), 9, conv_ksteps(y.cin), conv_ntiles(y.cout), y.mode == NN11_VALID ? d - 2 : d, d * d,
                  l == 1 ? stack : nullptr, act[l - 1],
                  [&](int oy, int ox, int tap) { return nn11_src_pixel(y.mode, d, oy, ox, tap); },
                  [&](float sum, int c, int64_t) { return nn11_relu(sum + bias[c]); }, act[l]);
    }
    const int npix = nn11_out_pixels(d), fcp = nn11_cpad(net.layer[L - 1].cout);
    for (int a = 0; a < NN11_OUT; ++a) {
        float s = 0.f;
        for (int p = 0; p < npix; ++p)
            for (int c = 0; c < fcp; ++c) s += nn11_f32(act[L][nn11_act_index(0, p, c, npix, fcp)]) * net.limg[net.lin_index(a, p, c, npix)];
        q[a] = s + net.lbias[a];
    }
}

}  // namespace tq
