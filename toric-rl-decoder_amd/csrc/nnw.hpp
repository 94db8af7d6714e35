// Forward pass of the reference's two wide Q-networks (src/nn/torch/NN.py:47-133): NN_8, eight conv3x3 + ReLU, and
// NN_17, twenty of them despite its name, both with up to 256 channels, the paddings of NN_11 (circular pad before the
// unpadded first conv, zero padding 1 in the middle, the last conv unpadded) and Linear(200 (d-2)^2, 3).  Implicit-GEMM
// convolutions on v_mfma_f32_32x32x16_bf16 under NN_11's numerics contract (include/toricenv.h), with
// NN_11's images, fragment order, tile geometry, shape policy and epilogue (nn11.hpp) over the shared tile body
// (conv_tile.hpp): what differs is how a layer is cut.
//   - Output channels are cut across blockIdx.y: a workgroup computes at most CONV_NTB = 4 n-tiles (128 channels), so a
//     wavefront's accumulators stay at the MW x 4 x 16 = 128 registers of NN_11's 128 -> 128 layer.
//   - Input channels come in more than one chunk of conv_tiles: 16 k-steps as 8 + 8, 14 as 7 + 7.  The LDS tile is
//     never larger than NN_11's own.
// The order of a sum is (chunk, tap, k-step) and depends on (net, layer, d) alone; no atomics.
//
// The network table is host+device, and a layer's index arithmetic is nn11.hpp's conv_* functions by channel counts: the
// pack kernel, the conv kernel and a g++ build of this header (tests/host_nnw_shim.cpp) share them.
#pragma once
#include "nn11.hpp"

namespace tq {

constexpr int NNW_NETS = 2;                   // slot 0: NN_8 (TQ_NET_NN8), slot 1: NN_17 (TQ_NET_NN17)
constexpr int NNW_MAX_LAYERS = 20;
constexpr int NNW_LAYERS[NNW_NETS] = {8, 20};
constexpr int NNW_CH[NNW_NETS][NNW_MAX_LAYERS + 1] = {
    {2, 256, 256, 240, 224, 220, 215, 205, 200},
    {2, 256, 256, 251, 250, 240, 240, 235, 233, 233, 229, 225, 223, 220, 220, 220, 215, 214, 205, 204, 200}};
constexpr int NNW_MAX_CP = 256;               // channels of the widest activation image
constexpr int NNW_FEAT = 200, NNW_FEAT_CP = 224;        // the last conv's channels: the linear layer's features per pixel

inline int nnw_slot(int net) { return net == 8 ? 0 : (net == 17 ? 1 : -1); }        // TQ_NET_NN8 / TQ_NET_NN17 -> slot
// slot s, layer l = 1..nnw_layers(s)
TQ_HD int nnw_layers(int s) { return NNW_LAYERS[s]; }
TQ_HD int nnw_cin(int s, int l) { return NNW_CH[s][l - 1]; }
TQ_HD int nnw_cout(int s, int l) { return NNW_CH[s][l]; }
TQ_HD int nnw_mode(int s, int l) { return l == 1 ? NN11_CIRCULAR : (l == NNW_LAYERS[s] ? NN11_VALID : NN11_ZERO); }

// ---- one layer by its channel counts: one-line calls into nn11.hpp's conv_* functions, as NN_11's by-layer functions
// are.  The names stay because the host shim (tests/host_nnw_shim.cpp) uses them.
TQ_HD int nnw_taps(int cin) { return conv_img_taps(cin, 9); }
TQ_HD int nnw_ksteps(int cin) { return conv_ksteps(cin); }
TQ_HD int nnw_ntiles(int cout) { return conv_ntiles(cout); }
TQ_HD int nnw_chunks(int ksteps) { return conv_chunks(ksteps); }
TQ_HD int64_t nnw_wimg_elems(int cin, int cout) { return conv_wimg_elems(cin, cout, 9); }

// ---- where a layer lies in the handle's one weight image and one padded bias array (l = layers + 1: their sizes)
TQ_HD int64_t nnw_wimg_offset(int s, int l) {
    int64_t o = 0;
    for (int i = 1; i < l; ++i) o += conv_wimg_elems(nnw_cin(s, i), nnw_cout(s, i), 9);
    return o;
}
TQ_HD int nnw_bias_offset(int s, int l) {
    int o = 0;
    for (int i = 1; i < l; ++i) o += nn11_cpad(nnw_cout(s, i));
    return o;
}

// ---- linear image f32 [a][pixel][224] (bf16-rounded values, 0 in channels 200..223) <- torch [a][c * npix + pixel]
TQ_HD int64_t nnw_lin_elems(int d) { return (int64_t)NN11_OUT * nn11_out_pixels(d) * NNW_FEAT_CP; }
TQ_HD int64_t nnw_lin_index(int a, int pixel, int c, int npix) { return ((int64_t)a * npix + pixel) * NNW_FEAT_CP + c; }
TQ_HD float nnw_lin_value(int64_t idx, int npix, const float* w) {
    const int c = (int)(idx % NNW_FEAT_CP);
    const int pixel = (int)((idx / NNW_FEAT_CP) % npix), a = (int)((idx / NNW_FEAT_CP) / npix);
    if (c >= NNW_FEAT) return 0.f;
    return nn11_f32(nn11_bf16(w[(int64_t)a * NNW_FEAT * npix + (int64_t)c * npix + pixel]));
}

// ---- host-side pack (what k_nnw_pack does on the device), for the header's unit test
inline void nnw_pack_layer_host(int cin, int cout, const float* w, const float* b, uint16_t* wimg, float* bias) {
    conv_pack_layer_host(cin, cout, 9, w, b, wimg, bias);
}
inline void nnw_pack_linear_host(int d, const float* w, float* limg) {
    const int64_t n = nnw_lin_elems(d);
    for (int64_t i = 0; i < n; ++i) limg[i] = nnw_lin_value(i, nn11_out_pixels(d), w);
}

#if defined(__HIPCC__)
// ======================================================================================================= device side
struct NNWPack { const float* w[NNW_MAX_LAYERS + 1]; const float* b[NNW_MAX_LAYERS + 1]; };

// one block row (blockIdx.y) per layer of slot s: y < layers: conv l = y + 1 (image, then its padded bias); y = layers:
// the linear layer
__global__ __launch_bounds__(256) void k_nnw_pack(NNWPack p, int s, int d, uint16_t* wimg, float* bias, float* limg, float* lbias) {
    const int l = (int)blockIdx.y + 1, L = nnw_layers(s);
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (l <= L) {
        const int cin = nnw_cin(s, l), cout = nnw_cout(s, l);
        const int64_t n = conv_wimg_elems(cin, cout, 9);
        uint16_t* img = wimg + nnw_wimg_offset(s, l);
        for (int64_t e = i; e < n; e += stride) img[e] = nn11_bf16(conv_wimg_value(cin, cout, 9, e, p.w[l - 1]));
        if (i < nn11_cpad(cout)) bias[nnw_bias_offset(s, l) + i] = i < cout ? p.b[l - 1][i] : 0.f;
    } else {
        const int64_t n = nnw_lin_elems(d);
        for (int64_t e = i; e < n; e += stride) limg[e] = nnw_lin_value(e, nn11_out_pixels(d), p.w[L]);
        if (i < NN11_OUT) lbias[i] = p.b[L][i];
    }
}

// One conv3x3 layer of a wide net.  KS: k-steps of 16 input channels per tap (the stack layer: 2 steps over its 18 k
// values), NT: tiles of 32 output channels, MODE: where a tap's source pixel lies.  `in`: the previous layer's activation
// image [P][d^2][16 KS] (MODE != CIRCULAR; (d-2)^2 pixels for NN11_FULL) or the perspective stack [P][2][d][d] of element
// type `dtype`; `out`: this layer's image [P][pixels][32 NT] ((d-2)^2 pixels for NN11_VALID).
// EPI says what becomes of the sums (nn11.hpp).  ConvBiasRelu, the forward: `aux` is the layer's padded f32 bias.
// NN11DgradMask, the backward's dgrad over a dgrad image (nnw_grad.hpp): `aux` is the bf16 activation image of `out`'s
// shape, whose sign masks.
// Grid: (ceil(P / G), ceil(NT / CONV_NTB)) workgroups of NN11Geom<D>::THREADS threads: workgroup (x, y) computes the
// n-tiles 4 y .. of the perspectives G x ..
template <int D, int KS, int NT, int MODE, class EPI = ConvBiasRelu>
__global__ __launch_bounds__(NN11Geom<D>::THREADS) void k_nnw_conv(const void* __restrict__ in, int dtype, const uint16_t* __restrict__ wimg,
                                                  const typename EPI::Aux* __restrict__ aux, uint16_t* __restrict__ out, int64_t P) {
    using Shape = NN11Shape<D, MODE>;
    __shared__ __attribute__((aligned(16))) unsigned char lds[conv_lds_bytes<Shape, KS>()];
    constexpr int REM = NT % CONV_NTB;                                      // n-tiles of the last block row, if fewer
    const int n0 = (int)blockIdx.y * CONV_NTB;
    if constexpr (REM != 0) {
        if (n0 + CONV_NTB > NT) {                                           // uniform over the workgroup
            conv_tiles<Shape, KS, NT, REM>(lds, n0, in, dtype, wimg, out, P, EPI{aux});
            return;
        }
    }
    conv_tiles<Shape, KS, NT, CONV_NTB>(lds, n0, in, dtype, wimg, out, P, EPI{aux});
}
#endif  // __HIPCC__

}  // namespace tq
