// The BasicBlock ResNets' forward (ResNet18, ResNet34; eval-mode BatchNorm): the tq_resnet_* entry points of
// include/toricenv.h (part of toricenv.hip's translation unit), after abi_nnw.hpp's conventions.
#pragma once
#include <new>

#include "abi_util.hpp"
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
    constexpr int G = tq::NN11Geom<D>::G, THREADS = tq::NN11Geom<D>::THREADS;
    const int ks = tq::conv_ksteps(c.cin), nt = tq::conv_ntiles(c.cout);
    const dim3 grid((unsigned)((a.rows + G - 1) / G), (unsigned)((nt + tq::CONV_NTB - 1) / tq::CONV_NTB)), block(THREADS);
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
    constexpr int G = tq::NN11Geom<HS>::G, THREADS = tq::NN11Geom<HS>::THREADS;
    if (c.cin != 512 || c.cout != 512 || c.taps != 9 || c.stride != 1)
        return fail(TQ_E_INVALID, "resnet: no half-grid kernel for %d -> %d, %d taps, stride %d", c.cin, c.cout, c.taps, c.stride);
    const dim3 grid((unsigned)((a.rows + G - 1) / G), 4), block(THREADS);
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
    if (!out) return fail(TQ_E_INVALID, "out is NULL");
    *out = nullptr;
    const int s = tq::resnet_slot(net);
    if (s < 0) return fail(TQ_E_INVALID, "net must be TQ_NET_RESNET18 or TQ_NET_RESNET34 (got %d)", net);
    if (!tq::size_ok(d)) return bad_size(d);
    if (max_rows <= 0 || max_rows > (int64_t(1) << 24)) return fail(TQ_E_INVALID, "max_rows must be in 1..2^24 (got %lld)", (long long)max_rows);
    if (int rc = valid_device(device)) return rc;
    DeviceGuard guard;
    if (int rc = guard.enter_device(device)) return rc;
    tq_resnet* h = new (std::nothrow) tq_resnet();
    if (!h) return fail(TQ_E_INVALID, "out of host memory");
    h->slot = s; h->d = d; h->device = device; h->max_rows = max_rows;
    const int n = tq::resnet_convs(s);
    h->mem.zeroed(&h->wimg, (size_t)tq::resnet_wimg_offset(s, n) * sizeof(uint16_t));
    h->mem.zeroed(&h->scale, (size_t)tq::resnet_st_offset(s, n) * sizeof(float));
    h->mem.zeroed(&h->shift, (size_t)tq::resnet_st_offset(s, n) * sizeof(float));
    h->mem.zeroed(&h->limg, (size_t)tq::resnet_lin_elems() * sizeof(float));
    h->mem.zeroed(&h->lbias, 16);
    for (int i = 0; i < 4; ++i)
        h->mem.zeroed(&h->act[i], (size_t)max_rows * d * d * tq::RESNET_MAX_CP * sizeof(uint16_t));
    hipError_t e = h->mem.err;
    if (e == hipSuccess) e = hipStreamSynchronize(nullptr);
    if (e != hipSuccess) { tq_resnet_destroy(h); return fail(TQ_E_HIP, "resnet allocation failed: %s", hipGetErrorString(e)); }
    *out = h;
    return TQ_OK;
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
    if (!h->loaded) return fail(TQ_E_INVALID, "resnet forward before tq_resnet_load");
    if (dtype < TQ_F32 || dtype > TQ_U8) return fail(TQ_E_INVALID, "bad stack dtype %d", dtype);
    if (rows < 0) return fail(TQ_E_INVALID, "negative rows");
    if (rows == 0) return TQ_OK;
    if (!stack || !q) return fail(TQ_E_INVALID, "stack / q is NULL");
    REQUIRE_ALIGNED16(stack, "stack");
    REQUIRE_ALIGNED16(q, "q");
    const int64_t esize = dtype == TQ_F32 ? 4 : (dtype == TQ_U8 ? 1 : 2);
    const int64_t row_bytes = 2 * (int64_t)h->d * h->d * esize;
    return by_size(h->d, [&](auto D) {                     // passes of at most max_rows perspectives
        for (int64_t first = 0; first < rows; first += h->max_rows) {
            const int64_t n = rows - first < h->max_rows ? rows - first : h->max_rows;
            if (int rc = resnet_forward<D()>(h, static_cast<const char*>(stack) + first * row_bytes, dtype, n,
                                             q + first * tq::NN11_OUT, stream)) return rc;
        }
        return (int)TQ_OK;
    });
}

}  // extern "C"
