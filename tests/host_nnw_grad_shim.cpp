// Host-side instantiation of the wide nets' learner-step headers (csrc/nnw.hpp, csrc/nnw_grad.hpp), beside
// host_nn11_grad_shim.cpp: torch-layout weights are packed with the headers' own pack routines (forward and dgrad images),
// and the scalar forward of host_conv_ref.hpp, NN_11's head and a backward (its dgrad: that header's conv_host under the
// ReLU mask) under the numerics contract of include/toricenv.h read the images, the activation and gradient images and the
// tap -> source pixel maps ONLY through the headers' index functions -- what the pack kernels, the MFMA kernels and the
// head kernel use on the device.
// TEST ONLY: built by tests/test_nnw_grad_host.py into a temp dir with g++; it is not a backend of the product.
#include "host_conv_ref.hpp"
#include "nnw_grad.hpp"

using namespace tq;

// weights / biases / grad_w / grad_b: L + 1 host pointers each in torch layout (conv1..convL, linear1); stack u8
// [n][2][d][d]; w may be NULL -> q f32 [n][3], loss f32 [n], the 2 (L + 1) gradients (written)
extern "C" int shim_nnw_grad(int net_id, int d, const float* const* weights, const float* const* biases, const uint8_t* stack, int n,
                             const int64_t* actions, const float* y, const float* w, float* q, float* loss,
                             float* const* grad_w, float* const* grad_b) {
    const int s = nnw_slot(net_id);
    if (s < 0 || !size_ok(d) || n < 1) return -1;
    const int L = nnw_layers(s), pix = d * d, npix = nn11_out_pixels(d), FC = NNW_FEAT_CP;
    std::vector<PlainLayer> layers;
    for (int l = 1; l <= L; ++l) layers.push_back({nnw_cin(s, l), nnw_cout(s, l), nnw_mode(s, l)});
    PackedNet net(layers, weights, biases, nnw_lin_elems(d), nnw_lin_index);
    nnw_pack_linear_host(d, weights[L], net.limg.data());
    const std::vector<float>& limg = net.limg;
    std::vector<std::vector<float>> dt(L + 1);
    for (int l = 2; l <= L; ++l) {
        const int cin = nnw_cin(s, l), cout = nnw_cout(s, l);
        std::vector<uint16_t> dimg(conv_dimg_elems(cin, cout));
        conv_pack_dgrad_host(cin, cout, weights[l - 1], dimg.data());
        dt[l] = expand(dimg, 9, conv_dksteps(cout), conv_dntiles(cin));     // [tap'][co][cp of cin]
    }

    // ---- forward, every layer's bf16 image kept: act[l] [n][pixels(l)][cpad(cout(l))]
    std::vector<std::vector<uint16_t>> act(L + 1);
    for (int l = 1; l <= L; ++l) act[l].assign((size_t)n * nnw_layer_pixels(s, l, d) * nn11_cpad(nnw_cout(s, l)), 0);
#pragma omp parallel for schedule(dynamic, 1)
    for (int i = 0; i < n; ++i) {
        uint16_t* mine[NNW_MAX_LAYERS + 1] = {nullptr};                     // record i's part of every image
        for (int l = 1; l <= L; ++l)
            mine[l] = act[l].data() + nn11_act_index(i, 0, 0, nnw_layer_pixels(s, l, d), nn11_cpad(nnw_cout(s, l)));
        forward_one<NNW_MAX_CP>(d, net, stack + (size_t)i * 2 * pix, mine, q + i * NN11_OUT);
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

    // ---- the linear layer's gradients and G_L
    for (int a = 0; a < NN11_OUT; ++a) {
        float t0 = 0.f;
        for (int i = 0; i < n; ++i) t0 += dq[i * NN11_OUT + a];
        grad_b[L][a] = t0;
        for (int p = 0; p < npix; ++p)
            for (int c = 0; c < NNW_FEAT; ++c) {
                float t = 0.f;
                for (int i = 0; i < n; ++i) t += dq[i * NN11_OUT + a] * nn11_f32(act[L][nn11_act_index(i, p, c, npix, FC)]);
                grad_w[L][(size_t)a * NNW_FEAT * npix + (size_t)c * npix + p] = t;
            }
    }
    std::vector<uint16_t> g((size_t)n * pix * NNW_MAX_CP, 0), gn((size_t)n * pix * NNW_MAX_CP, 0);
    for (int i = 0; i < n; ++i)
        for (int p = 0; p < npix; ++p)
            for (int c = 0; c < FC; ++c) {
                float t = 0.f;
                for (int a = 0; a < NN11_OUT; ++a) t += dq[i * NN11_OUT + a] * limg[nnw_lin_index(a, p, c, npix)];
                const int64_t e = nn11_act_index(i, p, c, npix, FC);
                g[e] = nn11_mask(act[L][e]) ? nn11_bf16(t) : (uint16_t)0;
            }

    // ---- layer by layer: wgrad and bias gradient from G_l, then dgrad to G_{l-1}
    for (int l = L; l >= 1; --l) {
        const int mode = nnw_mode(s, l), cout = nnw_cout(s, l), cin = nnw_cin(s, l), cpo = nn11_cpad(cout), cpi = nn11_cpad(cin);
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
            conv_host<NNW_MAX_CP>(dt[l].data(), 9, conv_dksteps(cout), conv_dntiles(cin), d, opix, nullptr,
                                  g.data() + nn11_act_index(i, 0, 0, opix, cpo),
                                  [&](int oy, int ox, int tap) { return nn11_src_pixel(dmode, d, oy, ox, tap); },
                                  [&](float sum, int, int64_t at) { return nn11_mask(mask[at]) ? sum : 0.f; },
                                  gn.data() + nn11_act_index(i, 0, 0, pix, cpi));
        }
        g.swap(gn);
    }
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
