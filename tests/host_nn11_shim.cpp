// Host-side instantiation of the product's NN_11 header (csrc/nn11.hpp), beside host_td_target_shim.cpp: torch-layout
// weights are packed with the header's own pack routines, and a scalar forward under the numerics contract of
// include/toricenv.h reads the packed images, the activation image and the tap -> source pixel map ONLY through the
// header's index functions -- what the pack kernel and the MFMA kernels use on the device.
// TEST ONLY: built by tests/test_nn11_host.py into a temp dir with g++; it is not a backend of the product.
#include <stdint.h>

#include <vector>

#include "nn11.hpp"

using namespace tq;

namespace {
struct Packed {
    std::vector<uint16_t> wimg[NN11_LAYERS + 1];
    std::vector<float> bias[NN11_LAYERS + 1];
    std::vector<float> limg;
};

// one perspective: stack u8 [2][d][d] -> q[3]
void forward_one(int d, const Packed& pk, const std::vector<float>* wt, const uint8_t* stack, const float* lbias, float* q) {
    const int pix = d * d;
    std::vector<uint16_t> cur((size_t)pix * NN11_MAX_CP, 0), nxt((size_t)pix * NN11_MAX_CP, 0);
    std::vector<float> acc(NN11_MAX_CP);
    for (int l = 1; l <= NN11_LAYERS; ++l) {
        const int mode = nn11_mode(l), cpo = nn11_cpad(nn11_cout(l)), cpi = nn11_cpad(nn11_cin(l));
        const int od = mode == NN11_VALID ? d - 2 : d, opix = od * od;
        const float* W = wt[l].data();                                  // [tap][k][cpo], read out of the packed image below
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
                        const float a = nn11_f32(cur[nn11_act_index(0, sp, k, pix, cpi)]);
                        if (a == 0.f) continue;                         // adds +0: the sum is the same without it
                        const float* w = W + ((size_t)tap * cpi + k) * cpo;
                        for (int c = 0; c < cpo; ++c) acc[c] += a * w[c];
                    }
                }
            }
            for (int c = 0; c < cpo; ++c) {
                const float v = acc[c] + pk.bias[l][c];
                nxt[nn11_act_index(0, o, c, opix, cpo)] = nn11_bf16(v > 0.f ? v : 0.f);
            }
        }
        cur.swap(nxt);
    }
    const int npix = nn11_out_pixels(d);
    for (int a = 0; a < NN11_OUT; ++a) {
        float s = 0.f;
        for (int p = 0; p < npix; ++p)
            for (int c = 0; c < 64; ++c) s += nn11_f32(cur[nn11_act_index(0, p, c, npix, 64)]) * pk.limg[nn11_lin_index(a, p, c, npix)];
        q[a] = s + lbias[a];
    }
}
}  // namespace

// weights / biases: 12 host pointers each in torch layout (conv1..conv11, linear1); stack u8 [P][2][d][d] -> q f32 [P][3]
extern "C" int shim_nn11_forward(int d, const float* const* weights, const float* const* biases, const uint8_t* stack,
                                 int64_t P, float* q) {
    if (!size_ok(d)) return -1;
    Packed pk;
    std::vector<float> wt[NN11_LAYERS + 1];
    for (int l = 1; l <= NN11_LAYERS; ++l) {
        pk.wimg[l].resize(nn11_wimg_elems(l));
        pk.bias[l].resize(nn11_cpad(nn11_cout(l)));
        nn11_pack_layer_host(l, weights[l - 1], biases[l - 1], pk.wimg[l].data(), pk.bias[l].data());
        // the layer's weights as the kernel finds them: element (cout, k, tap) of the packed image, through nn11_wimg_of
        const int cpo = nn11_cpad(nn11_cout(l)), kp = nn11_ksteps(l) * 16, taps = nn11_taps(l);
        wt[l].resize((size_t)taps * kp * cpo);
        for (int tap = 0; tap < taps; ++tap)
            for (int k = 0; k < kp; ++k)
                for (int c = 0; c < cpo; ++c)
                    wt[l][((size_t)tap * kp + k) * cpo + c] = nn11_f32(pk.wimg[l][nn11_wimg_of(c, k, tap, nn11_ksteps(l), nn11_ntiles(l))]);
    }
    pk.limg.resize(nn11_lin_elems(d));
    nn11_pack_linear_host(d, weights[NN11_LAYERS], pk.limg.data());
#pragma omp parallel for schedule(dynamic, 4)
    for (int64_t p = 0; p < P; ++p) forward_one(d, pk, wt, stack + p * 2 * d * d, biases[NN11_LAYERS], q + p * NN11_OUT);
    return 0;
}

// perspectives per workgroup of the conv kernels (the tile edge tests/test_gpu_nn11.py aims at)
extern "C" int shim_nn11_group(int d) { return nn11_group(d); }
