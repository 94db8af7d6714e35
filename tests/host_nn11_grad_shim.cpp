// Host-side instantiation of the product's NN_11 learner-step headers (csrc/nn11.hpp, csrc/nn11_grad.hpp), beside
// host_nn11_shim.cpp: torch-layout weights are packed with the headers' own pack routines (forward and dgrad images), and
// the scalar forward of host_conv_ref.hpp, a head and a backward (its dgrad: that header's conv_host under the ReLU mask)
// under the numerics contract of include/toricenv.h read the images, the activation and gradient images and the tap ->
// source pixel maps ONLY through the headers' index functions -- what the pack kernels, the MFMA kernels and the head
// kernel use on the device.
// TEST ONLY: built by tests/test_nn11_grad_host.py into a temp dir with g++; it is not a backend of the product.
#include "host_conv_ref.hpp"
#include "nn11_grad.hpp"

using namespace tq;

// weights / biases / grad_w / grad_b: 12 host pointers each in torch layout (conv1..conv11, linear1); stack u8
// [n][2][d][d]; w may be NULL -> q f32 [n][3], loss f32 [n], the 24 gradients (written)
extern "C" int shim_nn11_grad(int d, const float* const* weights, const float* const* biases, const uint8_t* stack, int n,
                              const int64_t* actions, const float* y, const float* w, float* q, float* loss,
                              float* const* grad_w, float* const* grad_b) {
    if (!size_ok(d) || n < 1) return -1;
    constexpr int L = NN11_LAYERS;
    const int pix = d * d, npix = nn11_out_pixels(d);
    const PackedNet net = nn11_packed(d, weights, biases);
    const std::vector<float>& limg = net.limg;
    std::vector<float> dt[L + 1];
    for (int l = 2; l <= L; ++l) {
        std::vector<uint16_t> dimg(nn11_dimg_elems(l));
        nn11_pack_dgrad_host(l, weights[l - 1], dimg.data());
        dt[l] = expand(dimg, 9, nn11_dksteps(l), nn11_dntiles(l));          // [tap'][co][cp of cin]
    }

    // ---- forward, every layer's bf16 image kept: act[l] [n][pixels(l)][cpad(cout(l))]
    std::vector<uint16_t> act[L + 1];
    for (int l = 1; l <= L; ++l) act[l].assign((size_t)n * nn11_layer_pixels(l, d) * nn11_cpad(nn11_cout(l)), 0);
#pragma omp parallel for schedule(dynamic, 1)
    for (int i = 0; i < n; ++i) {
        uint16_t* mine[L + 1] = {nullptr};                                  // record i's part of every image
        for (int l = 1; l <= L; ++l) mine[l] = act[l].data() + nn11_act_index(i, 0, 0, nn11_layer_pixels(l, d), nn11_cpad(nn11_cout(l)));
        forward_one<NN11_MAX_CP>(d, net, stack + (size_t)i * 2 * pix, mine, q + i * NN11_OUT);
    }

    // ---- head
    std::vector<float> dq((size_t)n * NN11_OUT, 0.f);
    for (int i = 0; i < n; ++i) {
        const int64_t a = actions[i];
        loss[i] = 0.f;
        if (a < 0 || a >= NN11_OUT) continue;
        const NN11Head h = nn11_head(q[i * NN11_OUT + a], y[i], w ? w[i] : 1.f, n);
        loss[i] = h.loss;
        dq[i * NN11_OUT + a] = h.dq;
    }

    // ---- the linear layer's gradients and G_11
    for (int a = 0; a < NN11_OUT; ++a) {
        float s = 0.f;
        for (int i = 0; i < n; ++i) s += dq[i * NN11_OUT + a];
        grad_b[L][a] = s;
        for (int p = 0; p < npix; ++p)
            for (int c = 0; c < 64; ++c) {
                float t = 0.f;
                for (int i = 0; i < n; ++i) t += dq[i * NN11_OUT + a] * nn11_f32(act[L][nn11_act_index(i, p, c, npix, 64)]);
                grad_w[L][(size_t)a * 64 * npix + (size_t)c * npix + p] = t;
            }
    }
    std::vector<uint16_t> g((size_t)n * pix * NN11_MAX_CP, 0), gn((size_t)n * pix * NN11_MAX_CP, 0);
    for (int i = 0; i < n; ++i)
        for (int p = 0; p < npix; ++p)
            for (int c = 0; c < 64; ++c) {
                float s = 0.f;
                for (int a = 0; a < NN11_OUT; ++a) s += dq[i * NN11_OUT + a] * limg[nn11_lin_index(a, p, c, npix)];
                const int64_t e = nn11_act_index(i, p, c, npix, 64);
                g[e] = nn11_mask(act[L][e]) ? nn11_bf16(s) : (uint16_t)0;
            }

    // ---- layer by layer: wgrad and bias gradient from G_l, then dgrad to G_{l-1}
    for (int l = L; l >= 1; --l) {
        const int mode = nn11_mode(l), cout = nn11_cout(l), cin = nn11_cin(l), cpo = nn11_cpad(cout), cpi = nn11_cpad(cin);
        const int od = mode == NN11_VALID ? d - 2 : d, opix = od * od;
        float* dw = grad_w[l - 1];
        float* db = grad_b[l - 1];
#pragma omp parallel for schedule(dynamic, 4)
        for (int co = 0; co < cout; ++co) {
            float bs = 0.f;
            for (int64_t e = 0; e < (int64_t)cin * 9; ++e) dw[(int64_t)co * cin * 9 + e] = 0.f;
            for (int i = 0; i < n; ++i)
                for (int o = 0; o < opix; ++o) {
                    const float gv = nn11_f32(g[nn11_act_index(i, o, co, opix, cpo)]);
                    if (gv == 0.f) continue;
                    bs += gv;
                    for (int tap = 0; tap < 9; ++tap) {
                        const int sp = nn11_src_pixel(mode, d, o / od, o % od, tap);
                        if (sp < 0) continue;
                        for (int ci = 0; ci < cin; ++ci) {
                            const float a = l == 1 ? nn11_f32(nn11_bf16((float)stack[((size_t)i * 2 + ci) * pix + sp]))
                                                   : nn11_f32(act[l - 1][nn11_act_index(i, sp, ci, pix, cpi)]);
                            dw[((int64_t)co * cin + ci) * 9 + tap] += gv * a;
                        }
                    }
                }
            db[co] = bs;
        }
        if (l == 1) break;
        const int dmode = l == L ? NN11_FULL : NN11_ZERO;
#pragma omp parallel for schedule(dynamic, 1)
        for (int i = 0; i < n; ++i) {
            const uint16_t* mask = act[l - 1].data() + nn11_act_index(i, 0, 0, pix, cpi);
            conv_host<NN11_MAX_CP>(dt[l].data(), 9, nn11_dksteps(l), nn11_dntiles(l), d, opix, nullptr, g.data() + nn11_act_index(i, 0, 0, opix, cpo),
                      [&](int oy, int ox, int tap) { return nn11_src_pixel(dmode, d, oy, ox, tap); },
                      [&](float sum, int, int64_t at) { return nn11_mask(mask[at]) ? sum : 0.f; }, gn.data() + nn11_act_index(i, 0, 0, pix, cpi));
        }
        g.swap(gn);
    }
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
