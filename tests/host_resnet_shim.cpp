// Host-side instantiation of the ResNets' header (csrc/resnet.hpp), beside host_nnw_shim.cpp: the network table, the
// index functions, the BatchNorm fold and the host pack routines as the pack kernel and the conv kernel use them, and one
// scalar forward under the numerics contract of include/toricenv.h over the scalar convolution of host_conv_ref.hpp.
// TEST ONLY: built by tests/test_resnet_host.py into a temp dir with g++; it is not a backend of the product.
#include "host_conv_ref.hpp"
#include "resnet.hpp"

using namespace tq;

extern "C" int shim_resnet_slot(int net) { return resnet_slot(net); }
extern "C" int shim_resnet_convs(int net) { return resnet_convs(resnet_slot(net)); }
// out[16]: cin, cout, taps, stride, role, stage, block, half_in, half_out, image taps, k-steps, n-tiles, chunks,
// scale/shift offset, reads the stack, has a shortcut conv (of the block, by the table's own predicate)
extern "C" void shim_resnet_conv(int net, int i, int* out) {
    const int s = resnet_slot(net);
    const ResConv c = resnet_conv(s, i);
    const int v[16] = {c.cin, c.cout, c.taps, c.stride, c.role, c.stage, c.block, c.half_in, c.half_out,
                       resnet_img_taps(c.cin, c.taps), resnet_ksteps(c.cin), resnet_ntiles(c.cout), resnet_chunks(resnet_ksteps(c.cin)),
                       resnet_st_offset(s, i), resnet_reads_stack(c.cin) ? 1 : 0,
                       c.stage > 0 && resnet_has_shortcut(c.stage - 1, c.block) ? 1 : 0};
    for (int k = 0; k < 16; ++k) out[k] = v[k];
}
extern "C" int64_t shim_resnet_wimg_offset(int net, int i) { return resnet_wimg_offset(resnet_slot(net), i); }    // i = convs: the size
extern "C" int shim_resnet_st_offset(int net, int i) { return resnet_st_offset(resnet_slot(net), i); }
extern "C" int64_t shim_resnet_wimg_elems(int cin, int cout, int taps) { return resnet_wimg_elems(cin, cout, taps); }
extern "C" int64_t shim_resnet_wimg_of(int cout, int k, int tap, int ksteps, int ntiles) { return nn11_wimg_of(cout, k, tap, ksteps, ntiles); }
extern "C" void shim_resnet_wimg_coord(int64_t idx, int ksteps, int ntiles, int* out) {
    const NN11WCoord c = nn11_wimg_coord(idx, ksteps, ntiles);
    out[0] = c.cout; out[1] = c.k; out[2] = c.tap;
}
extern "C" int shim_resnet_src_pixel(int side, int stride, int taps, int y, int x, int tap) { return resnet_src_pixel(side, stride, taps, y, x, tap); }
extern "C" int shim_resnet_half(int d) { return resnet_half(d); }
extern "C" void shim_resnet_pack_conv(int cin, int cout, int taps, const float* w, const float* const* bn, float eps, uint16_t* wimg,
                                      float* scale, float* shift) {
    resnet_pack_conv_host(cin, cout, taps, w, bn[0], bn[1], bn[2], bn[3], eps, wimg, scale, shift);
}
extern "C" void shim_resnet_pack_linear(const float* w, float* limg) { resnet_pack_linear_host(w, limg); }

namespace {
struct Packed { std::vector<float> wt, scale, shift; };      // one convolution; wt: the packed image, expanded
}

// conv_weights[n], bn[4 n] (gamma, beta, mean, var per convolution), lin_w [3][512], lin_b [3]: host pointers in torch
// layout; stack u8 [P][2][d][d] -> q f32 [P][3].  The block schedule is abi_resnet.hpp's and the head's order of sums is
// k_resnet_head's.
extern "C" int shim_resnet_forward(int net, int d, const float* const* conv_weights, const float* const* bn, const float* lin_w,
                                   const float* lin_b, float eps, const uint8_t* stack, int64_t P, float* q) {
    const int s = resnet_slot(net);
    if (s < 0 || !size_ok(d)) return -1;
    const int n = resnet_convs(s), hs = resnet_half(d), pix = d * d;
    std::vector<Packed> pk(n);
    for (int i = 0; i < n; ++i) {
        const ResConv c = resnet_conv(s, i);
        std::vector<uint16_t> img(conv_wimg_elems(c.cin, c.cout, c.taps));
        pk[i].scale.resize(nn11_cpad(c.cout));
        pk[i].shift.resize(nn11_cpad(c.cout));
        resnet_pack_conv_host(c.cin, c.cout, c.taps, conv_weights[i], bn[4 * i], bn[4 * i + 1], bn[4 * i + 2], bn[4 * i + 3], eps,
                              img.data(), pk[i].scale.data(), pk[i].shift.data());
        pk[i].wt = expand(img, conv_img_taps(c.cin, c.taps), conv_ksteps(c.cin), conv_ntiles(c.cout));
    }
    std::vector<float> limg(resnet_lin_elems());
    resnet_pack_linear_host(lin_w, limg.data());
#pragma omp parallel for schedule(dynamic, 1)
    for (int64_t p = 0; p < P; ++p) {
        std::vector<uint16_t> act[4];
        for (auto& a : act) a.assign((size_t)pix * RESNET_MAX_CP, 0);
        // convolution i: in [side^2][16 ks] (or the u8 stack [2][side][side]) -> out [opix][32 nt]; the epilogue: acc s + t,
        // the residual, the ReLU
        auto run = [&](int i, const uint16_t* in, const uint8_t* st, int epi, const uint16_t* res, uint16_t* out) {
            const ResConv c = resnet_conv(s, i);
            const int side = c.half_in ? hs : d;
            conv_host<RESNET_PLANES[RESNET_STAGES - 1]>(pk[i].wt.data(), c.taps, conv_ksteps(c.cin), conv_ntiles(c.cout), c.stride == 2 ? resnet_half(side) : side,
                      side * side, st, in, [&](int y, int x, int tap) { return resnet_src_pixel(side, c.stride, c.taps, y, x, tap); },
                      [&](float sum, int ch, int64_t at) {
                          float v = sum * pk[i].scale[ch] + pk[i].shift[ch];
                          if (epi == RESNET_EPI_ADD_RELU) v = v + nn11_f32(res[at]);
                          if (epi != RESNET_EPI_NONE) v = nn11_relu(v);
                          return v;
                      }, out);
        };
        run(0, nullptr, stack + p * 2 * pix, RESNET_EPI_RELU, nullptr, act[0].data());
        int x = 0;
        for (int i = 1; i < n;) {
            const bool sc = i + 2 < n && resnet_conv(s, i + 2).role == RESNET_SHORTCUT;
            uint16_t *in = act[x].data(), *mid = act[(x + 1) & 3].data(), *cut = act[(x + 2) & 3].data(), *out = act[(x + 3) & 3].data();
            run(i, in, nullptr, RESNET_EPI_RELU, nullptr, mid);
            if (sc) run(i + 2, in, nullptr, RESNET_EPI_NONE, nullptr, cut);
            run(i + 1, mid, nullptr, RESNET_EPI_ADD_RELU, sc ? cut : in, out);
            x = (x + 3) & 3;
            i += sc ? 3 : 2;
        }
        const uint16_t* feat = act[x].data();
        const int npix = hs * hs;
        // k_resnet_head's order: S[c] over the pixels in pixel order; lane l's partial sum over channels 8 l .. 8 l + 7 in
        // order; the butterfly over the 64 lanes (xor 32, 16, .., 1), read at lane 0
        float S[RESNET_FEAT];
        for (int c = 0; c < RESNET_FEAT; ++c) {
            S[c] = 0.f;
            for (int o = 0; o < npix; ++o) S[c] += nn11_f32(feat[nn11_act_index(0, o, c, npix, RESNET_FEAT)]);
        }
        for (int a = 0; a < NN11_OUT; ++a) {
            float lane[64], next[64];
            for (int l = 0; l < 64; ++l) {
                lane[l] = 0.f;
                for (int j = 0; j < 8; ++j) lane[l] += S[8 * l + j] * limg[a * RESNET_FEAT + 8 * l + j];
            }
            for (int m = 32; m >= 1; m >>= 1) {
                for (int l = 0; l < 64; ++l) next[l] = lane[l] + lane[l ^ m];
                for (int l = 0; l < 64; ++l) lane[l] = next[l];
            }
            q[p * NN11_OUT + a] = lane[0] / (float)npix + lin_b[a];
        }
    }
    return 0;
}
