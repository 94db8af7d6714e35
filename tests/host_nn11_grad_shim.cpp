// Host-side instantiation of the product's NN_11 learner-step headers (csrc/nn11.hpp, csrc/nn11_grad.hpp), beside
// host_nn11_shim.cpp: torch-layout weights are packed with the headers' own pack routines (forward and dgrad images), and
// a scalar forward, head and backward under the numerics contract of include/toricenv.h read the images, the activation
// and gradient images and the tap -> source pixel maps ONLY through the headers' index functions -- what the pack
// kernels, the MFMA kernels and the head kernel use on the device.
// TEST ONLY: built by tests/test_nn11_grad_host.py into a temp dir with g++; it is not a backend of the product.
#include <stdint.h>

#include <vector>

#include "nn11_grad.hpp"

using namespace tq;

namespace {
// element (cout, k, tap) of a packed fragment image, expanded to [tap][k][cp_out] f32
std::vector<float> expand(const std::vector<uint16_t>& img, int taps, int ksteps, int ntiles) {
    const int kp = ksteps * 16, cp = ntiles * 32;
    std::vector<float> w((size_t)taps * kp * cp);
    for (int tap = 0; tap < taps; ++tap)
        for (int k = 0; k < kp; ++k)
            for (int c = 0; c < cp; ++c) w[((size_t)tap * kp + k) * cp + c] = nn11_f32(img[nn11_wimg_of(c, k, tap, ksteps, ntiles)]);
    return w;
}
}  // namespace

// weights / biases / grad_w / grad_b: 12 host pointers each in torch layout (conv1..conv11, linear1); stack u8
// [n][2][d][d]; w may be NULL -> q f32 [n][3], loss f32 [n], the 24 gradients (written)
extern "C" int shim_nn11_grad(int d, const float* const* weights, const float* const* biases, const uint8_t* stack, int n,
                              const int64_t* actions, const float* y, const float* w, float* q, float* loss,
                              float* const* grad_w, float* const* grad_b) {
    if (!size_ok(d) || n < 1) return -1;
    constexpr int L = NN11_LAYERS;
    const int pix = d * d, npix = nn11_out_pixels(d);
    std::vector<float> wt[L + 1], dt[L + 1], bias[L + 1];
    for (int l = 1; l <= L; ++l) {
        std::vector<uint16_t> img(nn11_wimg_elems(l));
        bias[l].resize(nn11_cpad(nn11_cout(l)));
        nn11_pack_layer_host(l, weights[l - 1], biases[l - 1], img.data(), bias[l].data());
        wt[l] = expand(img, nn11_taps(l), nn11_ksteps(l), nn11_ntiles(l));
        if (l >= 2) {
            std::vector<uint16_t> dimg(nn11_dimg_elems(l));
            nn11_pack_dgrad_host(l, weights[l - 1], dimg.data());
            dt[l] = expand(dimg, 9, nn11_dksteps(l), nn11_dntiles(l));      // [tap'][co][cp of cin]
        }
    }
    std::vector<float> limg(nn11_lin_elems(d));
    nn11_pack_linear_host(d, weights[L], limg.data());

    // ---- forward, every layer's bf16 image kept: act[l] [n][pixels(l)][cpad(cout(l))]
    std::vector<uint16_t> act[L + 1];
    for (int l = 1; l <= L; ++l) act[l].assign((size_t)n * nn11_layer_pixels(l, d) * nn11_cpad(nn11_cout(l)), 0);
#pragma omp parallel for schedule(dynamic, 1)
    for (int i = 0; i < n; ++i) {
        std::vector<float> acc(NN11_MAX_CP);
        for (int l = 1; l <= L; ++l) {
            const int mode = nn11_mode(l), cpo = nn11_cpad(nn11_cout(l)), cpi = nn11_cpad(nn11_cin(l));
            const int od = mode == NN11_VALID ? d - 2 : d, opix = od * od;
            for (int o = 0; o < opix; ++o) {
                for (int c = 0; c < cpo; ++c) acc[c] = 0.f;
                for (int tap = 0; tap < 9; ++tap) {
                    const int sp = nn11_src_pixel(mode, d, o / od, o % od, tap);
                    if (sp < 0) continue;
                    if (l == 1) {
                        for (int ci = 0; ci < 2; ++ci) {
                            const float a = nn11_f32(nn11_bf16((float)stack[((size_t)i * 2 + ci) * pix + sp]));
                            if (a == 0.f) continue;
                            const float* ww = wt[1].data() + (size_t)nn11_k1(ci, tap) * cpo;
                            for (int c = 0; c < cpo; ++c) acc[c] += a * ww[c];
                        }
                    } else {
                        for (int k = 0; k < cpi; ++k) {
                            const float a = nn11_f32(act[l - 1][nn11_act_index(i, sp, k, pix, cpi)]);
                            if (a == 0.f) continue;                         // adds +0: the sum is the same without it
                            const float* ww = wt[l].data() + ((size_t)tap * cpi + k) * cpo;
                            for (int c = 0; c < cpo; ++c) acc[c] += a * ww[c];
                        }
                    }
                }
                for (int c = 0; c < cpo; ++c) {
                    const float v = acc[c] + bias[l][c];
                    act[l][nn11_act_index(i, o, c, opix, cpo)] = nn11_bf16(v > 0.f ? v : 0.f);
                }
            }
        }
        for (int a = 0; a < NN11_OUT; ++a) {
            float s = 0.f;
            for (int p = 0; p < npix; ++p)
                for (int c = 0; c < 64; ++c) s += nn11_f32(act[L][nn11_act_index(i, p, c, npix, 64)]) * limg[nn11_lin_index(a, p, c, npix)];
            q[i * NN11_OUT + a] = s + biases[L][a];
        }
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
            std::vector<float> acc(NN11_MAX_CP);
            for (int o = 0; o < pix; ++o) {
                for (int c = 0; c < cpi; ++c) acc[c] = 0.f;
                for (int tap = 0; tap < 9; ++tap) {
                    const int sp = nn11_src_pixel(dmode, d, o / d, o % d, tap);
                    if (sp < 0) continue;
                    for (int k = 0; k < cpo; ++k) {
                        const float gv = nn11_f32(g[nn11_act_index(i, sp, k, opix, cpo)]);
                        if (gv == 0.f) continue;
                        const float* ww = dt[l].data() + ((size_t)tap * cpo + k) * cpi;
                        for (int c = 0; c < cpi; ++c) acc[c] += gv * ww[c];
                    }
                }
                for (int c = 0; c < cpi; ++c) {
                    const int64_t e = nn11_act_index(i, o, c, pix, cpi);
                    gn[e] = nn11_mask(act[l - 1][e]) ? nn11_bf16(acc[c]) : (uint16_t)0;
                }
            }
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
