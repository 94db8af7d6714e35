// The NN_11 optimizer step's entry point of include/toricenv.h (part of toricenv.hip's translation unit).
#pragma once
#include "abi_nn11_grad.hpp"
#include "nn11_opt.hpp"

static_assert(TQ_OPT_ADAM == tq::NN11_OPT_ADAM && TQ_OPT_RMSPROP == tq::NN11_OPT_RMSPROP, "toricenv.h and nn11_opt.hpp name the same kinds");

extern "C" {

int tq_nn11_grad_opt_step(tq_nn11_grad* h, int kind, double lr, double beta1, double beta2, double eps, double alpha, int64_t step,
                          float* const* weights, float* const* biases, const float* const* grad_w, const float* const* grad_b,
                          float* const* m_w, float* const* m_b, float* const* v_w, float* const* v_b, void* stream_) {
    ENTER(h, "nn11 grad handle");
    if (!h->net.loaded) return fail(TQ_E_INVALID, "nn11 optimizer step before tq_nn11_grad_load");
    if (const char* bad = tq::nn11_opt_bad_args(kind, lr, beta1, beta2, eps, alpha, step)) return fail(TQ_E_INVALID, "nn11 optimizer step: %s", bad);
    const bool adam = kind == TQ_OPT_ADAM;
    if (!weights || !biases || !grad_w || !grad_b || !v_w || !v_b) return fail(TQ_E_INVALID, "weights / biases / grad_w / grad_b / v_w / v_b is NULL");
    if (adam && (!m_w || !m_b)) return fail(TQ_E_INVALID, "m_w / m_b is NULL (Adam's exp_avg)");
    tq::NN11Opt o;
    for (int i = 0; i <= tq::NN11_LAYERS; ++i) {
        if (!weights[i] || !biases[i] || !grad_w[i] || !grad_b[i] || !v_w[i] || !v_b[i] || (adam && (!m_w[i] || !m_b[i])))
            return fail(TQ_E_INVALID, "a pointer of layer %d (weights / biases / grad / state) is NULL", i);
        o.p[0][i] = weights[i]; o.p[1][i] = biases[i];
        o.g[0][i] = grad_w[i]; o.g[1][i] = grad_b[i];
        o.m[0][i] = adam ? m_w[i] : nullptr; o.m[1][i] = adam ? m_b[i] : nullptr;
        o.v[0][i] = v_w[i]; o.v[1][i] = v_b[i];
    }
    const tq::NN11OptConsts c = tq::nn11_opt_consts(kind, lr, beta1, beta2, eps, alpha, step);
    // 144 blocks of 256 threads take the largest weight (128 x 128 x 9) in one pass of 16-byte groups
    const dim3 grid(144, tq::NN11_LAYERS + 1), block(256);
    const NN11Net& net = h->net;
    if (adam) return launch(tq::k_nn11_opt<tq::NN11_OPT_ADAM>, grid, block, stream, o, c, h->d, net.wimg, net.dimg, net.bias, net.limg, net.lbias);
    return launch(tq::k_nn11_opt<tq::NN11_OPT_RMSPROP>, grid, block, stream, o, c, h->d, net.wimg, net.dimg, net.bias, net.limg, net.lbias);
}

}  // extern "C"
