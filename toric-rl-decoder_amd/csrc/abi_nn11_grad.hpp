// The NN_11 learner step's entry points of include/toricenv.h (part of toricenv.hip's translation unit).
#pragma once
#include "abi_nn11.hpp"

struct tq_nn11_grad {                      // made by `new tq_nn11_grad()`: every member starts as zero
    int d, device, max_batch;
    NN11Net net;                           // as tq_nn11's, with the dgrad images
    uint16_t* act[tq::NN11_LAYERS + 1];    // act[l], l = 1..11: layer l's bf16 output, max_batch * pixels(l) * cpad(cout(l))
    uint16_t* g[2];                        // gradient images taking turns: max_batch * d^2 * 128 bf16 each
    float* q;                              // f32[max_batch][3], used when the caller passes no q
    float* dq;                             // f32[max_batch][3]
    float* wpart;                          // wgrad partial images, one of NN11_WPART_ELEMS f32 per chunk of records
    float* bpart;                          // bias partials f32[chunks][128]
    float* lpart;                          // linear partials f32[slices][3][64 (d-2)^2]
    int* latch;
    DeviceBuffers mem;
};

namespace {
// G_l (in `g`) -> the gradient of layer l - 1's pre-activation (in `out`), l = 2..11: the convolution over layer l's dgrad
// image, masked by the sign of act[l - 1]
template <int D>
int nn11g_dgrad(const tq_nn11_grad* h, int l, const uint16_t* g, uint16_t* out, int64_t n, hipStream_t stream) {
    return nn11_conv<D, tq::NN11_EPI_MASK>(l == tq::NN11_LAYERS ? tq::NN11_FULL : tq::NN11_ZERO, tq::nn11_dksteps(l), tq::nn11_dntiles(l),
                                           g, 0, h->net.dimg + tq::nn11_dimg_offset(l), h->act[l - 1], out, n, stream);
}

// dW_l and db_l from G_l (in `g`) and layer l's input, l = 1..11
int nn11g_wgrad(const tq_nn11_grad* h, int l, const uint16_t* g, const void* stack, int dtype, int64_t n, float* dw, float* db,
                hipStream_t stream) {
    const int d = h->d, chunks = (int)tq::nn11_wgrad_chunks(d, n);
    const int cout = tq::nn11_cout(l), cpo = tq::nn11_cpad(cout);
    if (l == 1) {
        if (int rc = launch(tq::k_nn11_wgrad1, dim3(chunks), dim3(256), stream, g, stack, dtype, h->wpart, h->bpart, n, d)) return rc;
        return launch_1d(tq::k_nn11_wreduce<tq::NN11_MAX_CP>, (int64_t)cout * 18 + cout, stream, h->wpart, h->bpart, chunks, 1, cout, 18, cpo, 18, dw, db);
    }
    const int cin = tq::nn11_cin(l), cpi = tq::nn11_cpad(cin);
    int rc;
    if (cpi == 128) rc = launch(tq::k_nn11_wgrad<4>, dim3(chunks, 9), dim3(256), stream, g, h->act[l - 1], h->wpart, h->bpart, n, d,
                                tq::nn11_mode(l), cpo / 32);
    else if (cpi == 96) rc = launch(tq::k_nn11_wgrad<3>, dim3(chunks, 9), dim3(256), stream, g, h->act[l - 1], h->wpart, h->bpart, n, d,
                                    tq::nn11_mode(l), cpo / 32);
    else rc = fail(TQ_E_INVALID, "nn11 grad: no wgrad kernel for layer %d (%d padded input channels)", l, cpi);
    if (rc) return rc;
    return launch_1d(tq::k_nn11_wreduce<tq::NN11_MAX_CP>, (int64_t)9 * cout * cin + cout, stream, h->wpart, h->bpart, chunks, 9, cout, cin, cpo, cpi, dw, db);
}

template <int D>
int nn11g_step(const tq_nn11_grad* h, const void* state, int dtype, int n, const int64_t* actions, const float* y, const float* w,
               float* q, float* loss, float* const* gw, float* const* gb, hipStream_t stream) {
    constexpr int L = tq::NN11_LAYERS, NPIX = tq::NN11Geom<D>::OPIX, F = NPIX * 64;
    if (int rc = nn11_forward<D>(h->net, state, dtype, n, h->act, q, stream)) return rc;      // every layer's output kept
    if (int rc = launch_1d(tq::k_nn11_head, n, stream, q, actions, y, w, n, loss, h->dq, h->latch)) return rc;
    if (int rc = launch(tq::k_nn11_dblin, dim3(1), dim3(256), stream, h->dq, n, gb[L])) return rc;
    uint16_t* g = h->g[0];
    uint16_t* o = h->g[1];
    if (int rc = launch_1d(tq::k_nn11_g11<64>, (int64_t)n * F, stream, h->dq, h->net.limg, h->act[L], g, n, NPIX)) return rc;
    const int slices = (n + tq::NN11_LIN_SLICE - 1) / tq::NN11_LIN_SLICE;
    if (int rc = launch(tq::k_nn11_lin_part<64>, dim3((F + 255) / 256, slices), dim3(256), stream, h->dq, h->act[L], h->lpart, n, NPIX)) return rc;
    if (int rc = launch_1d(tq::k_nn11_lin_reduce<64, 64>, (int64_t)tq::NN11_OUT * F, stream, h->lpart, slices, NPIX, gw[L])) return rc;
    for (int l = L; l >= 1; --l) {
        if (int rc = nn11g_wgrad(h, l, g, state, dtype, n, gw[l - 1], gb[l - 1], stream)) return rc;
        if (l == 1) break;
        if (int rc = nn11g_dgrad<D>(h, l, g, o, n, stream)) return rc;
        uint16_t* t = g; g = o; o = t;
    }
    return TQ_OK;
}
}  // namespace

extern "C" {

int tq_nn11_grad_destroy(tq_nn11_grad* h) { return destroy_handle(h); }

int tq_nn11_grad_create(tq_nn11_grad** out, int d, int max_batch, int device) {
    auto batch_check = [&] {
        return max_batch < 1 || max_batch > 4096 ? fail(TQ_E_INVALID, "max_batch must be in 1..4096 (got %d)", max_batch) : (int)TQ_OK;
    };
    return create_handle(out, "nn11 grad", d, device, no_check, batch_check, [&](tq_nn11_grad* h) {
        h->max_batch = max_batch;
        constexpr int L = tq::NN11_LAYERS;
        const size_t n = (size_t)max_batch;
        h->net.alloc(h->mem, d, true);
        for (int l = 1; l <= L; ++l)
            h->mem.zeroed(&h->act[l], n * tq::nn11_layer_pixels(l, d) * tq::nn11_cpad(tq::nn11_cout(l)) * sizeof(uint16_t));
        for (int i = 0; i < 2; ++i) h->mem.zeroed(&h->g[i], n * d * d * tq::NN11_MAX_CP * sizeof(uint16_t));
        h->mem.zeroed(&h->q, n * tq::NN11_OUT * sizeof(float));
        h->mem.zeroed(&h->dq, n * tq::NN11_OUT * sizeof(float));
        const size_t chunks = (size_t)tq::nn11_wgrad_chunks(d, max_batch);
        h->mem.zeroed(&h->wpart, chunks * tq::NN11_WPART_ELEMS * sizeof(float));
        h->mem.zeroed(&h->bpart, chunks * tq::NN11_MAX_CP * sizeof(float));
        const size_t slices = (n + tq::NN11_LIN_SLICE - 1) / tq::NN11_LIN_SLICE;
        h->mem.zeroed(&h->lpart, slices * (size_t)tq::nn11_lin_elems(d) * sizeof(float));
        h->mem.zeroed(&h->latch, 16);
    });
}

int tq_nn11_grad_load(tq_nn11_grad* h, const float* const* weights, const float* const* biases, void* stream_) {
    ENTER(h, "nn11 grad handle");
    return h->net.load(h->d, weights, biases, stream);
}

int tq_nn11_grad_step(tq_nn11_grad* h, const void* state, int dtype, int n, const int64_t* actions_idx, const float* y, const float* w,
                      float* q, float* loss, float* const* grad_w, float* const* grad_b, void* stream_) {
    ENTER(h, "nn11 grad handle");
    if (!h->net.loaded) return fail(TQ_E_INVALID, "nn11 grad step before tq_nn11_grad_load");
    if (dtype < TQ_F32 || dtype > TQ_U8) return fail(TQ_E_INVALID, "bad state dtype %d", dtype);
    if (n <= 0 || n > h->max_batch) return fail(TQ_E_INVALID, "n must be in 1..max_batch = %d (got %d)", h->max_batch, n);
    if (!state || !actions_idx || !y || !loss) return fail(TQ_E_INVALID, "state / actions_idx / y / loss is NULL");
    if (!grad_w || !grad_b) return fail(TQ_E_INVALID, "grad_w / grad_b is NULL");
    for (int i = 0; i <= tq::NN11_LAYERS; ++i)
        if (!grad_w[i] || !grad_b[i]) return fail(TQ_E_INVALID, "grad_w[%d] / grad_b[%d] is NULL", i, i);
    REQUIRE_ALIGNED16(state, "state");
    return by_size(h->d, [&](auto D) {
        return nn11g_step<D()>(h, state, dtype, n, actions_idx, y, w, q ? q : h->q, loss, grad_w, grad_b, stream);
    });
}

int tq_nn11_grad_check(tq_nn11_grad* h, void* stream_) {
    ENTER(h, "nn11 grad handle");
    int flag = 0;
    if (int rc = read_latch(h->latch, stream, &flag)) return rc;
    if (flag & tq::NN11_ERR_ACTION) return fail(TQ_E_ACTION, "nn11 grad step: an actions_idx outside 0..2 was given");
    return TQ_OK;
}

}  // extern "C"
