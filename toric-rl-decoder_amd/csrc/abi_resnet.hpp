// The BasicBlock ResNets' forward (ResNet18, ResNet34; eval-mode BatchNorm): the tq_resnet_* entry points of
// include/toricenv.h (part of toricenv.hip's translation unit), over the frame all network handles share
// (abi_forward.hpp).
#pragma once
#include "abi_forward.hpp"
#include "resnet.hpp"

struct tq_resnet {                         // made by `new tq_resnet()`: every member starts as zero
    int slot, d, device;                   // slot: tq::resnet_slot(net)
    int64_t max_rows;
    int loaded;
    uint16_t* wimg;                        // the convolutions' bf16 fragment images, back to back
    float* scale;                          // their padded f32 BatchNorm scales, back to back
    float* shift;                          // ... and shifts, at the same offsets
    float* limg;                           // linear weights f32[3][512] (bf16-rounded values)
    float* lbias;                          // f32[3]
    uint16_t* act[4];                      // activation images of one pass: a block's input, mid image, shortcut image and
    DeviceBuffers mem;                     // output are live at once; max_rows * d^2 * 256 bf16 each
};

namespace {
struct ResConvArgs {
    const void* in; int dtype; const uint16_t* img; const float* scale; const float* shift; int epi; const uint16_t* res; uint16_t* out;
    int64_t rows;
};

// One convolution over the full grid of side D.  Every k_resnet_conv<D, ...> the library holds is in the list below, by
// (k-steps, n-tiles, taps, stride): the ten shapes the two nets need at the full grid.
template <int D>
int resnet_conv_full(const tq::ResConv& c, const ResConvArgs& a, hipStream_t stream) {
    const int ks = tq::conv_ksteps(c.cin), nt = tq::conv_ntiles(c.cout);
    const auto [grid, block] = conv_dims<D>(a.rows, nt);
#define RESNET_SHAPE(KS, NT, TAPS, STRIDE, STACK)                                                                           \
    if (ks == KS && nt == NT && c.taps == TAPS && c.stride == STRIDE && tq::conv_reads_stack(c.cin) == STACK)               \
        return launch(tq::k_resnet_conv<D, KS, NT, TAPS, STRIDE, STACK>, grid, block, stream, a.in, a.dtype, a.img, a.scale, a.shift, \
                      a.epi, a.res, a.out, a.rows)
    RESNET_SHAPE(2, 2, 9, 1, true);
    RESNET_SHAPE(4, 2, 9, 1, false);
    RESNET_SHAPE(4, 4, 9, 1, false);
    RESNET_SHAPE(4, 4, 1, 1, false);
    RESNET_SHAPE(8, 4, 9, 1, false);
    RESNET_SHAPE(8, 8, 9, 1, false);
    RESNET_SHAPE(8, 8, 1, 1, false);
    RESNET_SHAPE(16, 8, 9, 1, false);
    RESNET_SHAPE(16, 16, 9, 2, false);
    RESNET_SHAPE(16, 16, 1, 2, false);
#undef RESNET_SHAPE
    return fail(TQ_E_INVALID, "resnet: no kernel for convolution shape (%d k-steps, %d n-tiles, %d taps, stride %d)", ks, nt, c.taps, c.stride);
}

// One convolution over the half grid of side HS: 512 -> 512 is the only shape there.
template <int HS>
int resnet_conv_half(const tq::ResConv& c, const ResConvArgs& a, hipStream_t stream) {
    if (c.cin != 512 || c.cout != 512 || c.taps != 9 || c.stride != 1)
        return fail(TQ_E_INVALID, "resnet: no half-grid kernel for %d -> %d, %d taps, stride %d", c.cin, c.cout, c.taps, c.stride);
    const auto [grid, block] = conv_dims<HS>(a.rows, 16);
    return launch(tq::k_resnet_conv<HS, 32, 16, 9, 1, false>, grid, block, stream, a.in, a.dtype, a.img, a.scale, a.shift, a.epi, a.res,
                  a.out, a.rows);
}

// The forward of `rows` <= max_rows perspectives.  The stem writes act[0]; a block whose input is act[x] writes its mid
// image to act[x + 1], its shortcut convolution's image (if it has one) to act[x + 2] and its output to act[x + 3]
// (indices mod 4), which is the next block's input; the head reads the last one and writes q.
template <int D>
int resnet_forward(const tq_resnet* h, const void* stack, int dtype, int64_t rows, float* q, hipStream_t stream) {
    constexpr int HS = (D + 1) / 2;
    const int s = h->slot, n = tq::resnet_convs(s);
    auto run = [&](int i, const void* in, int dt, int epi, const uint16_t* res, uint16_t* out) {
        const tq::ResConv c = tq::resnet_conv(s, i);
        const int o = tq::resnet_st_offset(s, i);
        const ResConvArgs a = {in, dt, h->wimg + tq::resnet_wimg_offset(s, i), h->scale + o, h->shift + o, epi, res, out, rows};
        return c.half_in ? resnet_conv_half<HS>(c, a, stream) : resnet_conv_full<D>(c, a, stream);
    };
    if (int rc = run(0, stack, dtype, tq::RESNET_EPI_RELU, nullptr, h->act[0])) return rc;
    int x = 0;
    for (int i = 1; i < n;) {
        const bool sc = i + 2 < n && tq::resnet_conv(s, i + 2).role == tq::RESNET_SHORTCUT;
        uint16_t *in = h->act[x], *mid = h->act[(x + 1) & 3], *cut = h->act[(x + 2) & 3], *out = h->act[(x + 3) & 3];
        if (int rc = run(i, in, 0, tq::RESNET_EPI_RELU, nullptr, mid)) return rc;
        if (sc)
            if (int rc = run(i + 2, in, 0, tq::RESNET_EPI_NONE, nullptr, cut)) return rc;
        if (int rc = run(i + 1, mid, 0, tq::RESNET_EPI_ADD_RELU, sc ? cut : in, out)) return rc;
        x = (x + 3) & 3;
        i += sc ? 3 : 2;
    }
    return launch(tq::k_resnet_head, dim3((unsigned)((rows + 3) / 4)), dim3(256), stream, h->act[x], h->limg, h->lbias, q, rows, HS * HS);
}
}  // namespace

extern "C" {

int tq_resnet_destroy(tq_resnet* h) { return destroy_handle(h); }

int tq_resnet_create(tq_resnet** out, int net, int d, int64_t max_rows, int device) {
    const int s = tq::resnet_slot(net);
    auto net_check = [&] { return s < 0 ? fail(TQ_E_INVALID, "net must be TQ_NET_RESNET18 or TQ_NET_RESNET34 (got %d)", net) : (int)TQ_OK; };
    return create_handle(out, "resnet", d, device, net_check, [&] { return max_rows_check(max_rows); }, [&](tq_resnet* h) {
        h->slot = s; h->max_rows = max_rows;
        const int n = tq::resnet_convs(s);
        h->mem.zeroed(&h->wimg, (size_t)tq::resnet_wimg_offset(s, n) * sizeof(uint16_t));
        h->mem.zeroed(&h->scale, (size_t)tq::resnet_st_offset(s, n) * sizeof(float));
        h->mem.zeroed(&h->shift, (size_t)tq::resnet_st_offset(s, n) * sizeof(float));
        h->mem.zeroed(&h->limg, (size_t)tq::resnet_lin_elems() * sizeof(float));
        h->mem.zeroed(&h->lbias, 16);
        for (int i = 0; i < 4; ++i)
            h->mem.zeroed(&h->act[i], (size_t)max_rows * d * d * tq::RESNET_MAX_CP * sizeof(uint16_t));
    });
}

int tq_resnet_load(tq_resnet* h, const float* const* conv_weights, const float* const* bn_params, const float* lin_w, const float* lin_b,
                   double eps, void* stream_) {
    ENTER(h, "resnet handle");
    const int n = tq::resnet_convs(h->slot);
    if (!conv_weights || !bn_params || !lin_w || !lin_b) return fail(TQ_E_INVALID, "conv_weights / bn_params / lin_w / lin_b is NULL");
    if (!(eps > 0.0)) return fail(TQ_E_INVALID, "eps must be positive (got %g)", eps);
    tq::ResNetPack p = {};
    for (int i = 0; i < n; ++i) {
        if (!conv_weights[i]) return fail(TQ_E_INVALID, "conv_weights[%d] is NULL", i);
        p.w[i] = conv_weights[i];
        for (int k = 0; k < 4; ++k) {
            if (!bn_params[4 * i + k]) return fail(TQ_E_INVALID, "bn_params[%d] is NULL", 4 * i + k);
            p.bn[i][k] = bn_params[4 * i + k];
        }
    }
    p.lw = lin_w; p.lb = lin_b;
    if (int rc = launch(tq::k_resnet_pack, dim3(64, n + 1), dim3(256), stream, p, h->slot, (float)eps, h->wimg, h->scale, h->shift, h->limg,
                        h->lbias)) return rc;
    h->loaded = 1;
    return TQ_OK;
}

int tq_resnet_forward(tq_resnet* h, const void* stack, int dtype, int64_t rows, float* q, void* stream_) {
    ENTER(h, "resnet handle");
    bool done;
    if (int rc = forward_args("resnet", h->loaded, stack, dtype, rows, q, &done); rc || done) return rc;
    return forward_passes(h->d, h->max_rows, stack, dtype, false, rows, q, [&](auto D, const void* s, int64_t, int64_t n, float* qn) {
        return resnet_forward<D()>(h, s, dtype, n, qn, stream);
    });
}

}  // extern "C"
