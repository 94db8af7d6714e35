// NN_11's optimizer step (src/Learner_mp.py:81-84: Adam or RMSprop, lr 0.00025, torch's defaults for the rest): the
// update of the f32 master parameters and of the optimizer state from the gradients tq_nn11_grad_step wrote, and, from
// the same registers, the re-pack of the bf16 forward image, the dgrad image, the padded biases and the linear image --
// one launch, and no tq_nn11_grad_load after it.  Contract text: include/toricenv.h; design: DESIGN.md 3.8.
//
// Numerics contract.  Per element, all in f32, every operation rounded once in the order the parentheses give, never
// contracted (the build passes -ffp-contract=off on both sides); sqrt and / are IEEE correctly rounded and subnormals
// are kept.  On the device that is hipcc's DEFAULT for f32 (correctly rounded divide and sqrt, no flush to zero on
// gfx950): the contract relies on that default, and the build must not pass a flag that changes it.  NaN and Inf
// propagate as IEEE has it, nothing is clamped.
//   scalars   computed on the host in double, exactly as Python does, each cast to f32 once (nn11_opt_consts); t is the
//             1-based count of this update
//   Adam      c1 = (float)(1 - b1), c2 = (float)b2, c3 = (float)(1 - b2), cb = (float)sqrt(1 - b2^t), ce = (float)eps,
//             cs = (float)(-(lr / (1 - b1^t)))
//               m' = m + c1 * (g - m)
//               v' = (v * c2) + ((c3 * g) * g)
//               den = (sqrt(v') / cb) + ce
//               p' = p + cs * (m' / den)
//   RMSprop   (momentum 0, not centered)  ca = (float)alpha, c3 = (float)(1 - alpha), ce, cs = (float)(-lr)
//               s' = (s * ca) + ((c3 * g) * g)
//               p' = p + cs * (g / (sqrt(s') + ce))
// These are the expressions of torch's single-tensor Adam and RMSprop (weight_decay 0, no amsgrad, no maximize).  Torch
// itself has no one answer in bits (its CPU loops are vectorised and fused; foreach and fused variants differ again), so
// the lines above are the definition and torch is an accuracy reference only.
//
// Destinations.  The thread that owns a torch-layout element scatters bf16(p') to the element's places in the images:
// the exact inverses of nn11_wimg_value, nn11_dimg_value and nn11_lin_value (tests/test_nn11_opt_host.py scatters every
// element of every layer and compares with the host packs byte for byte).  Padding elements are never written: they
// stay the zeros that create and load left.
#pragma once
#include <math.h>

#include "nn11.hpp"

namespace tq {

enum { NN11_OPT_ADAM = 0, NN11_OPT_RMSPROP = 1 };          // TQ_OPT_ADAM, TQ_OPT_RMSPROP of include/toricenv.h

struct NN11OptConsts { int kind; float c1, c2, c3, cb, ce, cs, ca; };     // what a kind does not use is 0

// NULL, or what is wrong with the arguments (outside the contract).  Only what the kind uses is looked at.
inline const char* nn11_opt_bad_args(int kind, double lr, double beta1, double beta2, double eps, double alpha, int64_t step) {
    if (kind != NN11_OPT_ADAM && kind != NN11_OPT_RMSPROP) return "kind must be TQ_OPT_ADAM or TQ_OPT_RMSPROP";
    if (!(lr >= 0.0)) return "lr must be >= 0";
    if (!(eps >= 0.0)) return "eps must be >= 0";
    if (kind == NN11_OPT_ADAM && !(beta1 >= 0.0 && beta1 < 1.0)) return "beta1 must be in [0, 1)";
    if (kind == NN11_OPT_ADAM && !(beta2 >= 0.0 && beta2 < 1.0)) return "beta2 must be in [0, 1)";
    if (kind == NN11_OPT_RMSPROP && !(alpha >= 0.0 && alpha < 1.0)) return "alpha must be in [0, 1)";
    if (step < 1) return "step is the 1-based count of this update: it must be >= 1";
    return nullptr;
}

// the scalars of update number `step`, in double as Python computes them (b ** t is C's pow), each cast to f32 once
inline NN11OptConsts nn11_opt_consts(int kind, double lr, double beta1, double beta2, double eps, double alpha, int64_t step) {
    NN11OptConsts c = {kind, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    c.ce = (float)eps;
    if (kind == NN11_OPT_ADAM) {
        const double t = (double)step;
        c.c1 = (float)(1.0 - beta1);
        c.c2 = (float)beta2;
        c.c3 = (float)(1.0 - beta2);
        c.cb = (float)sqrt(1.0 - pow(beta2, t));
        c.cs = (float)(-(lr / (1.0 - pow(beta1, t))));
    } else {
        c.ca = (float)alpha;
        c.c3 = (float)(1.0 - alpha);
        c.cs = (float)(-lr);
    }
    return c;
}

// ---- one element's update, as the contract writes it
struct NN11OptElem { float p, m, v; };                      // RMSprop: v is the square average, m is not used
TQ_HD NN11OptElem nn11_adam(float p, float g, float m, float v, const NN11OptConsts& c) {
    NN11OptElem r;
    r.m = m + c.c1 * (g - m);
    r.v = (v * c.c2) + ((c.c3 * g) * g);
    const float den = (sqrtf(r.v) / c.cb) + c.ce;
    r.p = p + c.cs * (r.m / den);
    return r;
}
TQ_HD NN11OptElem nn11_rmsprop(float p, float g, float s, const NN11OptConsts& c) {
    NN11OptElem r;
    r.m = 0.f;
    r.v = (s * c.ca) + ((c.c3 * g) * g);
    r.p = p + c.cs * (g / (sqrtf(r.v) + c.ce));
    return r;
}

// ---- where element e of a torch-layout tensor goes
// conv l's weight [cout][cin][3][3], e = (co * cin + ci) * 9 + tap -> its element of the layer's forward image.  conv1's
// image has one tap whose k runs over (input channel, 3x3 tap): k = ci * 9 + tap (nn11_k1), which is e - 18 co.
TQ_HD int64_t nn11_opt_wimg_dest(int l, int64_t e) {
    const int cin = nn11_cin(l), tap = (int)(e % 9), ci = (int)(e / 9 % cin), co = (int)(e / 9 / cin);
    if (l == 1) return nn11_wimg_of(co, nn11_k1(ci, tap), 0, nn11_ksteps(1), nn11_ntiles(1));
    return nn11_wimg_of(co, ci, tap, nn11_ksteps(l), nn11_ntiles(l));
}
// ... and, l = 2..11, of the layer's dgrad image: the channel roles swapped, tap 8 - tap
TQ_HD int64_t nn11_opt_dimg_dest(int l, int64_t e) {
    const int cin = nn11_cin(l), tap = (int)(e % 9), ci = (int)(e / 9 % cin), co = (int)(e / 9 / cin);
    return nn11_wimg_of(ci, co, 8 - tap, nn11_dksteps(l), nn11_dntiles(l));
}
// linear1's weight [3][64 npix] with features in (channel, y, x) order, e = a * 64 npix + c * npix + pixel
TQ_HD int64_t nn11_opt_lin_dest(int64_t e, int npix) {
    const int pixel = (int)(e % npix), c = (int)(e / npix % 64), a = (int)(e / npix / 64);
    return nn11_lin_index(a, pixel, c, npix);
}
TQ_HD int64_t nn11_opt_weight_elems(int l, int d) {         // l = 1..11 the convs, 12 the linear layer
    return l <= NN11_LAYERS ? (int64_t)nn11_cout(l) * nn11_cin(l) * 9 : (int64_t)NN11_OUT * 64 * nn11_out_pixels(d);
}
TQ_HD int nn11_opt_bias_elems(int l) { return l <= NN11_LAYERS ? nn11_cout(l) : NN11_OUT; }

// ---- host-side scatter of one layer (what k_nn11_opt's stores do with the values p'), for the header's unit test
inline void nn11_opt_scatter_host(int l, int d, const float* w, const float* b, uint16_t* wimg, uint16_t* dimg, float* bias, float* limg,
                                  float* lbias) {
    const int64_t n = nn11_opt_weight_elems(l, d);
    for (int64_t e = 0; e < n; ++e) {
        if (l <= NN11_LAYERS) {
            wimg[nn11_opt_wimg_dest(l, e)] = nn11_bf16(w[e]);
            if (l >= 2) dimg[nn11_opt_dimg_dest(l, e)] = nn11_bf16(w[e]);
        } else limg[nn11_opt_lin_dest(e, nn11_out_pixels(d))] = nn11_f32(nn11_bf16(w[e]));
    }
    for (int c = 0; c < nn11_opt_bias_elems(l); ++c) (l <= NN11_LAYERS ? bias : lbias)[c] = b[c];
}

#if defined(__HIPCC__)
// the 12 layers' masters, gradients and state: [0] the weights, [1] the biases; m is not read by RMSprop
struct NN11Opt {
    float* p[2][NN11_LAYERS + 1];
    const float* g[2][NN11_LAYERS + 1];
    float* m[2][NN11_LAYERS + 1];
    float* v[2][NN11_LAYERS + 1];
};

// One tensor of n elements: the thread of index i (of `stride`) updates elements in place and hands each p' to put(e, p').
// 16-byte accesses over the whole groups of four when every pointer is 16-byte aligned, scalar ones over the tail (and
// over everything otherwise): which path an element takes does not change its bits.
template <int KIND, class Put>
__device__ __forceinline__ void nn11_opt_tensor(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m, float* __restrict__ v,
                                                int64_t n, const NN11OptConsts& c, int64_t i, int64_t stride, Put&& put) {
    const uintptr_t bits = reinterpret_cast<uintptr_t>(p) | reinterpret_cast<uintptr_t>(g) | reinterpret_cast<uintptr_t>(v) |
                           (KIND == NN11_OPT_ADAM ? reinterpret_cast<uintptr_t>(m) : 0);
    const int64_t n4 = (bits & 15u) ? 0 : n / 4;
    for (int64_t t = i; t < n4; t += stride) {
        const float4 P = reinterpret_cast<const float4*>(p)[t], G = reinterpret_cast<const float4*>(g)[t];
        const float4 V = reinterpret_cast<const float4*>(v)[t];
        const float4 M = KIND == NN11_OPT_ADAM ? reinterpret_cast<const float4*>(m)[t] : make_float4(0.f, 0.f, 0.f, 0.f);
        const float pp[4] = {P.x, P.y, P.z, P.w}, gg[4] = {G.x, G.y, G.z, G.w}, vv[4] = {V.x, V.y, V.z, V.w}, mm[4] = {M.x, M.y, M.z, M.w};
        NN11OptElem r[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) r[j] = KIND == NN11_OPT_ADAM ? nn11_adam(pp[j], gg[j], mm[j], vv[j], c) : nn11_rmsprop(pp[j], gg[j], vv[j], c);
        reinterpret_cast<float4*>(p)[t] = make_float4(r[0].p, r[1].p, r[2].p, r[3].p);
        reinterpret_cast<float4*>(v)[t] = make_float4(r[0].v, r[1].v, r[2].v, r[3].v);
        if (KIND == NN11_OPT_ADAM) reinterpret_cast<float4*>(m)[t] = make_float4(r[0].m, r[1].m, r[2].m, r[3].m);
#pragma unroll
        for (int j = 0; j < 4; ++j) put(4 * t + j, r[j].p);
    }
    for (int64_t e = 4 * n4 + i; e < n; e += stride) {
        const NN11OptElem r = KIND == NN11_OPT_ADAM ? nn11_adam(p[e], g[e], m[e], v[e], c) : nn11_rmsprop(p[e], g[e], v[e], c);
        p[e] = r.p;
        v[e] = r.v;
        if (KIND == NN11_OPT_ADAM) m[e] = r.m;
        put(e, r.p);
    }
}

// One block row (blockIdx.y) per layer, as k_nn11_pack has: y = 0..10 conv l = y + 1, y = 11 the linear layer.  Threads
// run over the torch-layout elements of the layer's weight, then of its bias; the owner of an element stores p' and the
// state in place and bf16(p') (the linear layer: that value as f32; a bias: p' itself) where the forward and the
// backward read it.  No atomics, and no thread reads what another one writes.
template <int KIND>
__global__ __launch_bounds__(256) void k_nn11_opt(NN11Opt o, NN11OptConsts c, int d, uint16_t* __restrict__ wimg, uint16_t* __restrict__ dimg,
                                                  float* __restrict__ bias, float* __restrict__ limg, float* __restrict__ lbias) {
    const int y = (int)blockIdx.y, l = y + 1;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x, i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t nw = nn11_opt_weight_elems(l, d);
    const int nb = nn11_opt_bias_elems(l);
    if (l <= NN11_LAYERS) {
        uint16_t* img = wimg + nn11_wimg_offset(l);
        uint16_t* dim = dimg + nn11_dimg_offset(l);                          // l = 1: not used
        float* bl = bias + nn11_bias_offset(l);
        nn11_opt_tensor<KIND>(o.p[0][y], o.g[0][y], o.m[0][y], o.v[0][y], nw, c, i, stride, [&](int64_t e, float pn) {
            const uint16_t h = nn11_bf16(pn);
            img[nn11_opt_wimg_dest(l, e)] = h;
            if (l >= 2) dim[nn11_opt_dimg_dest(l, e)] = h;
        });
        nn11_opt_tensor<KIND>(o.p[1][y], o.g[1][y], o.m[1][y], o.v[1][y], nb, c, i, stride, [&](int64_t e, float pn) { bl[e] = pn; });
    } else {
        const int npix = nn11_out_pixels(d);
        nn11_opt_tensor<KIND>(o.p[0][y], o.g[0][y], o.m[0][y], o.v[0][y], nw, c, i, stride,
                              [&](int64_t e, float pn) { limg[nn11_opt_lin_dest(e, npix)] = nn11_f32(nn11_bf16(pn)); });
        nn11_opt_tensor<KIND>(o.p[1][y], o.g[1][y], o.m[1][y], o.v[1][y], nb, c, i, stride, [&](int64_t e, float pn) { lbias[e] = pn; });
    }
}
#endif  // __HIPCC__

}  // namespace tq
