// Host-side instantiation of the product's NN_11 optimizer header (csrc/nn11_opt.hpp), beside host_nn11_grad_shim.cpp:
// the update functions and nn11_opt_consts as k_nn11_opt and the entry point use them, the argument check, and the
// scatter of torch-layout elements through the header's destination functions next to the header's own host packs.
// TEST ONLY: built by tests/test_nn11_opt_host.py into a temp dir with g++; it is not a backend of the product.
#include <stdint.h>

#include "nn11_opt.hpp"

using namespace tq;

// out[7]: c1, c2, c3, cb, ce, cs, ca
extern "C" void shim_nn11_opt_consts(int kind, double lr, double b1, double b2, double eps, double alpha, int64_t step, float* out) {
    const NN11OptConsts c = nn11_opt_consts(kind, lr, b1, b2, eps, alpha, step);
    out[0] = c.c1; out[1] = c.c2; out[2] = c.c3; out[3] = c.cb; out[4] = c.ce; out[5] = c.cs; out[6] = c.ca;
}

extern "C" int shim_nn11_opt_bad_args(int kind, double lr, double b1, double b2, double eps, double alpha, int64_t step) {
    return nn11_opt_bad_args(kind, lr, b1, b2, eps, alpha, step) != nullptr;
}

// n elements in place; m may be NULL for RMSprop
extern "C" void shim_nn11_opt_update(int kind, double lr, double b1, double b2, double eps, double alpha, int64_t step, int64_t n,
                                     float* p, const float* g, float* m, float* v) {
    const NN11OptConsts c = nn11_opt_consts(kind, lr, b1, b2, eps, alpha, step);
    for (int64_t e = 0; e < n; ++e) {
        const NN11OptElem r = kind == NN11_OPT_ADAM ? nn11_adam(p[e], g[e], m[e], v[e], c) : nn11_rmsprop(p[e], g[e], v[e], c);
        p[e] = r.p;
        v[e] = r.v;
        if (kind == NN11_OPT_ADAM) m[e] = r.m;
    }
}

// sizes[0..3]: elements of layer l's forward image, dgrad image (0 for l = 1 and 12), padded bias, linear image
extern "C" void shim_nn11_opt_sizes(int l, int d, int64_t* sizes) {
    const bool conv = l <= NN11_LAYERS;
    sizes[0] = conv ? nn11_wimg_elems(l) : 0;
    sizes[1] = conv && l >= 2 ? nn11_dimg_elems(l) : 0;
    sizes[2] = conv ? nn11_cpad(nn11_cout(l)) : NN11_OUT;
    sizes[3] = conv ? 0 : nn11_lin_elems(d);
}
// layer l = 1..12 from torch's weight and bias: which = 0 the header's host packs, 1 the optimizer's scatter.  Both write
// into the caller's buffers of shim_nn11_opt_sizes' sizes (bias: the layer's padded bias or the linear layer's 3).
extern "C" void shim_nn11_opt_images(int which, int l, int d, const float* w, const float* b, uint16_t* wimg, uint16_t* dimg, float* bias,
                                     float* limg) {
    if (which) { nn11_opt_scatter_host(l, d, w, b, wimg, dimg, bias, limg, bias); return; }
    if (l <= NN11_LAYERS) {
        nn11_pack_layer_host(l, w, b, wimg, bias);
        if (l >= 2) nn11_pack_dgrad_host(l, w, dimg);
    } else {
        nn11_pack_linear_host(d, w, limg);
        for (int a = 0; a < NN11_OUT; ++a) bias[a] = b[a];
    }
}
