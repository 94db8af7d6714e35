// What the host shims of the learner steps (host_nn11_grad_shim.cpp, host_nnw_grad_shim.cpp) share, beside
// host_conv_ref.hpp: the scalar learner step of a plain net under the numerics contract of include/toricenv.h -- that
// header's forward with every layer kept, the head, the linear layer's gradients, G_L, and layer by layer the wgrad and
// the dgrad (its conv_host over the dgrad image, under the ReLU mask).  It reads the packed images, the activation and
// gradient images and the tap -> source pixel maps ONLY through the product headers' index functions -- what the pack
// kernels, the MFMA kernels and the head kernel use on the device.
// The order of every sum is part of what the tests pin: records in index order, then pixels, then taps, then channels.
// TEST ONLY: it is not a backend of the product.
#pragma once
#include "host_conv_ref.hpp"
#include "nn11_grad.hpp"

namespace tq {

// net: the packed forward (its layer list says the net; the last conv's channels are the linear layer's features per
// pixel); weights / grad_w / grad_b: L + 1 host pointers each in torch layout (conv1..convL, linear1); stack u8
// [n][2][d][d]; w may be NULL -> q f32 [n][3], loss f32 [n], the 2 (L + 1) gradients (written).  MAX_CP: the channels of
// the net's widest image.
template <int MAX_CP>
inline void grad_host(int d, const PackedNet& net, const float* const* weights, const uint8_t* stack, int n, const int64_t* actions,
                      const float* y, const float* w, float* q, float* loss, float* const* grad_w, float* const* grad_b) {
    const int L = (int)net.layer.size(), pix = d * d, npix = nn11_out_pixels(d);
    const int feat = net.layer[L - 1].cout, fcp = nn11_cpad(feat);
    auto pixels = [&](int l) { return net.layer[l - 1].mode == NN11_VALID ? npix : pix; };
    auto cpad = [&](int l) { return nn11_cpad(net.layer[l - 1].cout); };
    std::vector<std::vector<float>> dt(L + 1);
    for (int l = 2; l <= L; ++l) {
        const int cin = net.layer[l - 1].cin, cout = net.layer[l - 1].cout;
        std::vector<uint16_t> dimg(conv_dimg_elems(cin, cout));
        conv_pack_dgrad_host(cin, cout, weights[l - 1], dimg.data());
        dt[l] = expand(dimg, 9, conv_dksteps(cout), conv_dntiles(cin));     // [tap'][co][cp of cin]
    }

    // ---- forward, every layer's bf16 image kept: act[l] [n][pixels(l)][cpad(cout(l))]
    std::vector<std::vector<uint16_t>> act(L + 1);
    for (int l = 1; l <= L; ++l) act[l].assign((size_t)n * pixels(l) * cpad(l), 0);
#pragma omp parallel for schedule(dynamic, 1)
    for (int i = 0; i < n; ++i) {
        std::vector<uint16_t*> mine(L + 1, nullptr);                        // record i's part of every image
        for (int l = 1; l <= L; ++l) mine[l] = act[l].data() + nn11_act_index(i, 0, 0, pixels(l), cpad(l));
        forward_one<MAX_CP>(d, net, stack + (size_t)i * 2 * pix, mine.data(), q + i * NN11_OUT);
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
        float s = 0.f;
        for (int i = 0; i < n; ++i) s += dq[i * NN11_OUT + a];
        grad_b[L][a] = s;
        for (int p = 0; p < npix; ++p)
            for (int c = 0; c < feat; ++c) {
                float t = 0.f;
                for (int i = 0; i < n; ++i) t += dq[i * NN11_OUT + a] * nn11_f32(act[L][nn11_act_index(i, p, c, npix, fcp)]);
                grad_w[L][(size_t)a * feat * npix + (size_t)c * npix + p] = t;
            }
    }
    std::vector<uint16_t> g((size_t)n * pix * MAX_CP, 0), gn((size_t)n * pix * MAX_CP, 0);
    for (int i = 0; i < n; ++i)
        for (int p = 0; p < npix; ++p)
            for (int c = 0; c < fcp; ++c) {
                float s = 0.f;
                for (int a = 0; a < NN11_OUT; ++a) s += dq[i * NN11_OUT + a] * net.limg[net.lin_index(a, p, c, npix)];
                const int64_t e = nn11_act_index(i, p, c, npix, fcp);
                g[e] = nn11_mask(act[L][e]) ? nn11_bf16(s) : (uint16_t)0;
            }

    // ---- layer by layer: wgrad and bias gradient from G_l, then dgrad to G_{l-1}
    for (int l = L; l >= 1; --l) {
        const int mode = net.layer[l - 1].mode, cout = net.layer[l - 1].cout, cin = net.layer[l - 1].cin;
        const int cpo = nn11_cpad(cout), cpi = nn11_cpad(cin);
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
            conv_host<MAX_CP>(dt[l].data(), 9, conv_dksteps(cout), conv_dntiles(cin), d, opix, nullptr,
                              g.data() + nn11_act_index(i, 0, 0, opix, cpo),
                              [&](int oy, int ox, int tap) { return nn11_src_pixel(dmode, d, oy, ox, tap); },
                              [&](float sum, int, int64_t at) { return nn11_mask(mask[at]) ? sum : 0.f; },
                              gn.data() + nn11_act_index(i, 0, 0, pix, cpi));
        }
        g.swap(gn);
    }
}

}  // namespace tq
