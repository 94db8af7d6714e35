// What the learner-step handles' entry points share (part of toricenv.hip's translation unit), beside abi_forward.hpp: the
// scratch of a handle and its allocation, the step -- head, linear gradients, G_L, then wgrad and dgrad layer by layer
// with two gradient images taking turns -- the wgrad launcher, the argument checks of *_grad_step and the latch check.
// Plain templates over a family description F, a small struct passed by value (NN11GradNet in abi_nn11_grad.hpp,
// NNWGradNet in abi_nnw_grad.hpp):
//   F::NAME                      the prefix of the refusal texts and of the entry points' names: "nn11", "nnw"
//   F::WAVES, F::CHUNK_ROWS      of the family's wgrad kernels; its widest image has 32 WAVES channels
//   F::FEAT_CP, F::FEAT          the last conv's padded and real channels: the linear layer's features per pixel
//   layers(), cin(l), cout(l), mode(l), dimg_offset(l)          conv layer l = 1..layers() and where its dgrad image lies
//   forward<D>(net, state, dtype, n, act, q, stream)            the family's forward, every layer's image kept in act[l]
//   dgrad<D>(mode, ksteps, ntiles, g, img, mask, out, n, stream)    its conv launcher with the dgrad epilogue
// Every kernel is still named where launch() (abi_util.hpp) is inlined.
// Device memory of a handle for steps of up to B = max_batch records at size d, beside the packed network and its dgrad
// images (cp = channels rounded up to 32, W = 32 WAVES, p = conv_wgrad_persp(CHUNK_ROWS, d), bf16 = 2 bytes):
//   activations   sum over l = 1..L of B * pixels(l) * cp(cout(l)) bf16      (pixels: (d-2)^2 for l = L, else d^2)
//   gradients     2 * B * d^2 * W bf16
//   partials      ceil(B / p) * (9 * W * W + W) f32  +  ceil(B / 64) * 3 * FEAT_CP (d-2)^2 f32
//   q, dq         2 * B * 3 f32
#pragma once
#include "abi_forward.hpp"
#include "nn11_grad.hpp"

namespace {
// A family's handle type derives from this (tq_nn11_grad, tq_nnw_grad: distinct C types).  Made by `new H()`: every
// member starts as zero.  NET: the family's packed network (NN11Net, NNWNet); MAXL: its layer count, at most.
template <class NET, int MAXL>
struct GradHandle {
    int d, device, max_batch;
    NET net;                               // as the forward handle's, with the dgrad images
    uint16_t* act[MAXL + 1];               // act[l], l = 1..L: layer l's bf16 output, max_batch * pixels(l) * cpad(cout(l))
    uint16_t* g[2];                        // gradient images taking turns: max_batch * d^2 * 32 WAVES bf16 each
    float* q;                              // f32[max_batch][3], used when the caller passes no q
    float* dq;                             // f32[max_batch][3]
    float* wpart;                          // wgrad partial images, one of 9 (32 WAVES)^2 f32 per chunk of records
    float* bpart;                          // bias partials f32[chunks][32 WAVES]
    float* lpart;                          // linear partials f32[slices][3][FEAT_CP (d-2)^2]
    int* latch;
    DeviceBuffers mem;
};

template <class F>
int grad_chunks(int d, int64_t n) { const int p = tq::conv_wgrad_persp(F::CHUNK_ROWS, d); return (int)((n + p - 1) / p); }

// tq_*_grad_create: create_handle's refusals with the bound of max_batch; net_alloc(h) allocates the family's packed
// network (first, as ever) and returns its description, over which the scratch is sized
template <class H, class NET, class ALLOC>
int grad_create(H** out, const char* what, int d, int max_batch, int device, NET&& net_check, ALLOC&& net_alloc) {
    auto batch_check = [&] {
        return max_batch < 1 || max_batch > 4096 ? fail(TQ_E_INVALID, "max_batch must be in 1..4096 (got %d)", max_batch) : (int)TQ_OK;
    };
    return create_handle(out, what, d, device, net_check, batch_check, [&](H* h) {
        h->max_batch = max_batch;
        const auto f = net_alloc(h);
        using F = decltype(f);
        constexpr size_t W = 32 * F::WAVES;
        const int L = f.layers();
        const size_t n = (size_t)max_batch, npix = (size_t)tq::nn11_out_pixels(d);
        for (int l = 1; l <= L; ++l)
            h->mem.zeroed(&h->act[l], n * (l == L ? npix : (size_t)d * d) * tq::nn11_cpad(f.cout(l)) * sizeof(uint16_t));
        for (int i = 0; i < 2; ++i) h->mem.zeroed(&h->g[i], n * d * d * W * sizeof(uint16_t));
        h->mem.zeroed(&h->q, n * tq::NN11_OUT * sizeof(float));
        h->mem.zeroed(&h->dq, n * tq::NN11_OUT * sizeof(float));
        const size_t chunks = (size_t)grad_chunks<F>(d, max_batch);
        h->mem.zeroed(&h->wpart, chunks * 9 * W * W * sizeof(float));
        h->mem.zeroed(&h->bpart, chunks * W * sizeof(float));
        const size_t slices = (n + tq::NN11_LIN_SLICE - 1) / tq::NN11_LIN_SLICE;
        h->mem.zeroed(&h->lpart, slices * tq::NN11_OUT * npix * F::FEAT_CP * sizeof(float));
        h->mem.zeroed(&h->latch, 16);
    });
}

// dW_l and db_l from G_l (in `g`) and layer l's input, l = 1..L.  The library holds the wgrad kernels of a family's two
// widest inputs: WAVES and WAVES - 1 tiles of 32 channels.
template <class F, class H>
int grad_wgrad(const F& f, const H* h, int l, const uint16_t* g, const void* stack, int dtype, int64_t n, float* dw, float* db,
               hipStream_t stream) {
    constexpr int W = F::WAVES, R = F::CHUNK_ROWS, MAX_CP = 32 * W;
    const int d = h->d, chunks = grad_chunks<F>(d, n);
    const int cout = f.cout(l), cpo = tq::nn11_cpad(cout);
    if (l == 1) {
        if (cpo != MAX_CP) return fail(TQ_E_INVALID, "%s grad: no conv1 wgrad kernel for %d padded output channels", F::NAME, cpo);
        if (int rc = launch(tq::k_conv_wgrad1<MAX_CP, R>, dim3(chunks), dim3(2 * MAX_CP), stream, g, stack, dtype, h->wpart, h->bpart, n, d)) return rc;
        return launch_1d(tq::k_nn11_wreduce<MAX_CP>, (int64_t)cout * 18 + cout, stream, h->wpart, h->bpart, chunks, 1, cout, 18, cpo, 18, dw, db);
    }
    const int cin = f.cin(l), cpi = tq::nn11_cpad(cin), mt = cpo / 32;
    const dim3 grid(chunks, 9), block(W * 64);
    int rc;
    if (mt > W) rc = fail(TQ_E_INVALID, "%s grad: no wgrad kernel for layer %d (%d padded output channels)", F::NAME, l, cpo);
    else if (cpi == 32 * W) rc = launch(tq::k_conv_wgrad<W, W, R>, grid, block, stream, g, h->act[l - 1], h->wpart, h->bpart, n, d, f.mode(l), mt);
    else if (cpi == 32 * (W - 1)) rc = launch(tq::k_conv_wgrad<W - 1, W, R>, grid, block, stream, g, h->act[l - 1], h->wpart, h->bpart, n, d, f.mode(l), mt);
    else rc = fail(TQ_E_INVALID, "%s grad: no wgrad kernel for layer %d (%d padded input channels)", F::NAME, l, cpi);
    if (rc) return rc;
    return launch_1d(tq::k_nn11_wreduce<MAX_CP>, (int64_t)9 * cout * cin + cout, stream, h->wpart, h->bpart, chunks, 9, cout, cin, cpo, cpi, dw, db);
}

template <int D, class F, class H>
int grad_step_at(const F& f, const H* h, const void* state, int dtype, int n, const int64_t* actions, const float* y, const float* w,
                 float* q, float* loss, float* const* gw, float* const* gb, hipStream_t stream) {
    constexpr int NPIX = tq::NN11Geom<D>::OPIX, CP = F::FEAT_CP, FEATS = NPIX * CP;
    const int L = f.layers();
    if (int rc = f.template forward<D>(h->net, state, dtype, n, h->act, q, stream)) return rc;      // every layer's output kept
    if (int rc = launch_1d(tq::k_nn11_head, n, stream, q, actions, y, w, n, loss, h->dq, h->latch)) return rc;
    if (int rc = launch(tq::k_nn11_dblin, dim3(1), dim3(256), stream, h->dq, n, gb[L])) return rc;
    uint16_t* g = h->g[0];
    uint16_t* o = h->g[1];
    if (int rc = launch_1d(tq::k_nn11_g11<CP>, (int64_t)n * FEATS, stream, h->dq, h->net.limg, h->act[L], g, n, NPIX)) return rc;
    const int slices = (n + tq::NN11_LIN_SLICE - 1) / tq::NN11_LIN_SLICE;
    if (int rc = launch(tq::k_nn11_lin_part<CP>, dim3((FEATS + 255) / 256, slices), dim3(256), stream, h->dq, h->act[L], h->lpart, n, NPIX)) return rc;
    if (int rc = launch_1d(tq::k_nn11_lin_reduce<CP, F::FEAT>, (int64_t)tq::NN11_OUT * FEATS, stream, h->lpart, slices, NPIX, gw[L])) return rc;
    for (int l = L; l >= 1; --l) {
        if (int rc = grad_wgrad(f, h, l, g, state, dtype, n, gw[l - 1], gb[l - 1], stream)) return rc;
        if (l == 1) break;
        // G_l (in `g`) -> the gradient of layer l - 1's pre-activation (in `o`): the convolution over layer l's dgrad image,
        // masked by the sign of act[l - 1]
        if (int rc = f.template dgrad<D>(l == L ? tq::NN11_FULL : tq::NN11_ZERO, tq::conv_dksteps(f.cout(l)), tq::conv_dntiles(f.cin(l)), g,
                                         h->net.dimg + f.dimg_offset(l), h->act[l - 1], o, n, stream)) return rc;
        uint16_t* t = g; g = o; o = t;
    }
    return TQ_OK;
}

// tq_*_grad_step after ENTER: what is refused before any launch, in this order, then the step at the handle's size
template <class F, class H>
int grad_step(const F& f, const H* h, const void* state, int dtype, int n, const int64_t* actions_idx, const float* y, const float* w,
              float* q, float* loss, float* const* grad_w, float* const* grad_b, hipStream_t stream) {
    if (!h->net.loaded) return fail(TQ_E_INVALID, "%s grad step before tq_%s_grad_load", F::NAME, F::NAME);
    if (dtype < TQ_F32 || dtype > TQ_U8) return fail(TQ_E_INVALID, "bad state dtype %d", dtype);
    if (n <= 0 || n > h->max_batch) return fail(TQ_E_INVALID, "n must be in 1..max_batch = %d (got %d)", h->max_batch, n);
    if (!state || !actions_idx || !y || !loss) return fail(TQ_E_INVALID, "state / actions_idx / y / loss is NULL");
    if (!grad_w || !grad_b) return fail(TQ_E_INVALID, "grad_w / grad_b is NULL");
    for (int i = 0; i <= f.layers(); ++i)
        if (!grad_w[i] || !grad_b[i]) return fail(TQ_E_INVALID, "grad_w[%d] / grad_b[%d] is NULL", i, i);
    REQUIRE_ALIGNED16(state, "state");
    return by_size(h->d, [&](auto D) {
        return grad_step_at<D()>(f, h, state, dtype, n, actions_idx, y, w, q ? q : h->q, loss, grad_w, grad_b, stream);
    });
}

// tq_*_grad_check after ENTER
template <class F, class H>
int grad_check(const F&, const H* h, hipStream_t stream) {
    int flag = 0;
    if (int rc = read_latch(h->latch, stream, &flag)) return rc;
    if (flag & tq::NN11_ERR_ACTION) return fail(TQ_E_ACTION, "%s grad step: an actions_idx outside 0..2 was given", F::NAME);
    return TQ_OK;
}
}  // namespace
