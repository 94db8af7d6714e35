// Forward pass of the Q-network NN_11 (src/nn/torch/NN.py:10-45, src/nn/torch/util.py:21-26): 11 conv3x3 + ReLU
// (circular pad before the unpadded conv1, zero padding 1 in conv2..10, unpadded conv11) and one linear layer, as
// implicit-GEMM convolutions on v_mfma_f32_32x32x16_bf16.
//
// Numerics contract (include/toricenv.h): conv and linear weights are rounded once to bf16 (RNE) when
// they are packed, biases stay f32; a stack element is converted to bf16 (exact for 0/1); a conv layer accumulates
// bf16 x bf16 products in f32, adds the f32 bias, applies ReLU in f32 and rounds to bf16 (RNE); the linear layer
// accumulates in f32, adds its f32 bias and stores f32.  No atomics: the same call gives the same bits.
//
// Images.  The index functions below are host+device and shared by the pack kernels, the conv kernels and a g++ build of
// this header (tests/host_nn11_shim.cpp), like lattice.hpp / td_target.hpp:
//   activation  [perspective][pixel][CP] bf16, channels last, CP = channels rounded up to 32; padded channels hold 0
//               (their weights and biases are 0).
//   weights     per layer, bf16, in MFMA fragment order: fragment (tap, kstep, ntile) is 64 lanes x 8 elements = 1 KiB,
//               lane l element j = W[cout = 32 ntile + (l & 31)][k = 16 kstep + 8 (l >> 5) + j][tap]: one 16-byte load
//               per lane.  conv1 has one "tap" whose k runs over (input channel, 3x3 tap) = 18 values padded to 32.
//   linear      f32 [3][pixel][64] holding bf16-rounded values, repacked from torch's (channel, y, x) feature order.
// The weight fragment is the MFMA's A operand (rows = output channels), the activation fragment its B operand (columns
// = pixels), so an accumulator lane holds 4 x 4 consecutive output channels of one pixel: 8-byte channels-last stores.
#pragma once
#include <stdint.h>
#include <string.h>

#include "lattice.hpp"

namespace tq {

constexpr int NN11_LAYERS = 11;
constexpr int NN11_CH[NN11_LAYERS + 1] = {2, 128, 128, 120, 111, 104, 103, 90, 80, 73, 71, 64};
constexpr int NN11_OUT = 3;                 // Q-values per perspective
constexpr int NN11_MAX_CP = 128;

enum { NN11_CIRCULAR = 0, NN11_ZERO = 1, NN11_VALID = 2, NN11_FULL = 3 };   // NN11_FULL: the backward of NN11_VALID
enum { NN11_EPI_BIAS_RELU = 0, NN11_EPI_MASK = 1 };                       // what k_nn11_conv does with its sums

TQ_HD int nn11_cpad(int c) { return (c + 31) & ~31; }

// ---- one convolution by its channel counts and taps (9, or 1 for a 1x1), for every net of the library.  The one whose
// input has 2 channels reads the stack: its weight image has one "tap" whose k runs over (input channel, 3x3 tap).
constexpr int CONV_NTB = 4;                   // n-tiles of one workgroup where a layer is cut across blockIdx.y
constexpr int CONV_CHUNK_KS = 8;              // k-steps of one staged chunk, at most
TQ_HD bool conv_reads_stack(int cin) { return cin == 2; }
TQ_HD int conv_img_taps(int cin, int taps) { return conv_reads_stack(cin) ? 1 : taps; }    // taps of the weight image
TQ_HD int conv_kdim(int cin) { return conv_reads_stack(cin) ? 18 : cin; }                  // k values per image tap
TQ_HD int conv_ksteps(int cin) { return conv_reads_stack(cin) ? 2 : nn11_cpad(cin) / 16; }
TQ_HD int conv_ntiles(int cout) { return nn11_cpad(cout) / 32; }
TQ_HD constexpr int conv_chunks(int ksteps) { return (ksteps + CONV_CHUNK_KS - 1) / CONV_CHUNK_KS; }    // equal chunks
TQ_HD int64_t conv_wimg_elems(int cin, int cout, int taps) {
    return (int64_t)conv_img_taps(cin, taps) * conv_ksteps(cin) * conv_ntiles(cout) * 512;
}

// layer l = 1..11
TQ_HD int nn11_cin(int l) { return NN11_CH[l - 1]; }
TQ_HD int nn11_cout(int l) { return NN11_CH[l]; }
TQ_HD int nn11_mode(int l) { return l == 1 ? NN11_CIRCULAR : (l == NN11_LAYERS ? NN11_VALID : NN11_ZERO); }
TQ_HD int nn11_taps(int l) { return conv_img_taps(nn11_cin(l), 9); }
TQ_HD int nn11_kdim(int l) { return conv_kdim(nn11_cin(l)); }
TQ_HD int nn11_ksteps(int l) { return conv_ksteps(nn11_cin(l)); }
TQ_HD int nn11_ntiles(int l) { return conv_ntiles(nn11_cout(l)); }
TQ_HD int64_t nn11_wimg_elems(int l) { return conv_wimg_elems(nn11_cin(l), nn11_cout(l), 9); }
TQ_HD int64_t nn11_wimg_offset(int l) {            // first element of layer l in the handle's one weight image
    int64_t o = 0;
    for (int i = 1; i < l; ++i) o += nn11_wimg_elems(i);
    return o;
}
TQ_HD int nn11_bias_offset(int l) {                // first f32 of layer l in the padded bias array (then the linear's 3)
    int o = 0;
    for (int i = 1; i < l; ++i) o += nn11_cpad(nn11_cout(i));
    return o;
}
TQ_HD int nn11_out_pixels(int d) { return (d - 2) * (d - 2); }
TQ_HD int64_t nn11_lin_elems(int d) { return (int64_t)NN11_OUT * nn11_out_pixels(d) * 64; }

// ---- bf16, round to nearest even; beyond the rounding boundary +-inf; a NaN stays a NaN (its quiet bit is set, so
// that the rounding's carry cannot turn it into +-0 or inf)
TQ_HD uint16_t nn11_bf16(float f) {
    uint32_t u;
#if defined(__HIP_DEVICE_COMPILE__)
    u = __float_as_uint(f);
#else
    memcpy(&u, &f, 4);
#endif
    // one select, no early return: a branch here is not if-converted, and the conv epilogue calls this per output
    const uint32_t rne = u + (0x7fffu + ((u >> 16) & 1u)), nan = u | 0x00400000u;
    return (uint16_t)((f != f ? nan : rne) >> 16);
}
TQ_HD float nn11_f32(uint16_t b) {
    const uint32_t u = (uint32_t)b << 16;
#if defined(__HIP_DEVICE_COMPILE__)
    return __uint_as_float(u);
#else
    float f;
    memcpy(&f, &u, 4);
    return f;
#endif
}

// relu as torch has it: +0 for x <= 0, x otherwise, so that a NaN stays (fmaxf would drop it)
TQ_HD float nn11_relu(float x) { return x <= 0.f ? 0.f : x; }

// the ReLU mask of the backward pass, torch's threshold_backward: the gradient passes unless the stored bf16
// activation is <= 0.  The forward stores +0, a positive value or a NaN (either sign), and a NaN lets it through.
TQ_HD bool nn11_mask(uint16_t a) { return (a & 0x7fffu) > 0x7f80u || (a != 0 && !(a & 0x8000u)); }

// ---- weight image of one layer: element <-> (cout, k, tap)
TQ_HD int64_t nn11_wimg_index(int tap, int kstep, int ntile, int lane, int j, int ksteps, int ntiles) {
    return ((((int64_t)tap * ksteps + kstep) * ntiles + ntile) * 64 + lane) * 8 + j;
}
TQ_HD int64_t nn11_wimg_of(int cout, int k, int tap, int ksteps, int ntiles) {
    return nn11_wimg_index(tap, k >> 4, cout >> 5, (cout & 31) | (((k >> 3) & 1) << 5), k & 7, ksteps, ntiles);
}
struct NN11WCoord { int cout, k, tap; };
TQ_HD NN11WCoord nn11_wimg_coord(int64_t idx, int ksteps, int ntiles) {
    const int j = (int)(idx & 7), lane = (int)((idx >> 3) & 63);
    int64_t f = idx >> 9;
    const int ntile = (int)(f % ntiles); f /= ntiles;
    const int kstep = (int)(f % ksteps);
    const int tap = (int)(f / ksteps);
    return NN11WCoord{32 * ntile + (lane & 31), 16 * kstep + 8 * (lane >> 5) + j, tap};
}
// conv1's k: (input channel, 3x3 tap), 18 values
TQ_HD int nn11_k1(int cin, int tap) { return cin * 9 + tap; }
// the value (before rounding) of image element idx from the torch weight [cout][cin][3][3] or [cout][cin][1][1]; 0 in
// the padding
TQ_HD float conv_wimg_value(int cin, int cout, int taps, int64_t idx, const float* w) {
    const NN11WCoord c = nn11_wimg_coord(idx, conv_ksteps(cin), conv_ntiles(cout));
    if (c.cout >= cout || c.k >= conv_kdim(cin)) return 0.f;
    if (conv_reads_stack(cin)) return w[(int64_t)c.cout * 18 + c.k];    // [cout][cin][ky][kx] with k = nn11_k1(cin, tap)
    if (taps == 1) return w[(int64_t)c.cout * cin + c.k];
    return w[((int64_t)c.cout * cin + c.k) * 9 + c.tap];
}
TQ_HD float nn11_wimg_value(int l, int64_t idx, const float* w) { return conv_wimg_value(nn11_cin(l), nn11_cout(l), 9, idx, w); }
// host-side pack of one convolution by its channel counts, for the unit tests: the weight image; with it the padded bias
inline void conv_pack_image_host(int cin, int cout, int taps, const float* w, uint16_t* wimg) {
    const int64_t n = conv_wimg_elems(cin, cout, taps);
    for (int64_t i = 0; i < n; ++i) wimg[i] = nn11_bf16(conv_wimg_value(cin, cout, taps, i, w));
}
inline void conv_pack_layer_host(int cin, int cout, int taps, const float* w, const float* b, uint16_t* wimg, float* bias) {
    conv_pack_image_host(cin, cout, taps, w, wimg);
    const int cp = nn11_cpad(cout);
    for (int c = 0; c < cp; ++c) bias[c] = c < cout ? b[c] : 0.f;
}

// ---- dgrad weight image of one 3x3 layer by its channel counts: the image of the convolution that takes G_l (cout
// channels) to the gradient of the layer's input (cin channels).  The forward's fragment order with the two channel counts
// in each other's place and the taps flipped: element (cout' = ci, k = co, tap') = W[co][ci][8 - tap'].
TQ_HD int conv_dksteps(int cout) { return nn11_cpad(cout) / 16; }
TQ_HD int conv_dntiles(int cin) { return nn11_cpad(cin) / 32; }
TQ_HD int64_t conv_dimg_elems(int cin, int cout) { return (int64_t)9 * conv_dksteps(cout) * conv_dntiles(cin) * 512; }
TQ_HD float conv_dimg_value(int cin, int cout, int64_t idx, const float* w) {
    const NN11WCoord c = nn11_wimg_coord(idx, conv_dksteps(cout), conv_dntiles(cin));      // .cout: ci, .k: co
    if (c.cout >= cin || c.k >= cout) return 0.f;
    return w[((int64_t)c.k * cin + c.cout) * 9 + (8 - c.tap)];
}
inline void conv_pack_dgrad_host(int cin, int cout, const float* w, uint16_t* dimg) {
    const int64_t n = conv_dimg_elems(cin, cout);
    for (int64_t i = 0; i < n; ++i) dimg[i] = nn11_bf16(conv_dimg_value(cin, cout, i, w));
}
// layer l = 2..11
TQ_HD int nn11_dksteps(int l) { return conv_dksteps(nn11_cout(l)); }
TQ_HD int nn11_dntiles(int l) { return conv_dntiles(nn11_cin(l)); }
TQ_HD int64_t nn11_dimg_elems(int l) { return conv_dimg_elems(nn11_cin(l), nn11_cout(l)); }
TQ_HD int64_t nn11_dimg_offset(int l) {            // first element of layer l = 2..12 in the handle's one dgrad image
    int64_t o = 0;
    for (int i = 2; i < l; ++i) o += nn11_dimg_elems(i);
    return o;
}
TQ_HD float nn11_dimg_value(int l, int64_t idx, const float* w) { return conv_dimg_value(nn11_cin(l), nn11_cout(l), idx, w); }

// ---- linear image [a][pixel][64] <- torch [a][c * npix + pixel]
TQ_HD int64_t nn11_lin_index(int a, int pixel, int c, int npix) { return ((int64_t)a * npix + pixel) * 64 + c; }
TQ_HD float nn11_lin_value(int64_t idx, int npix, const float* w) {
    const int c = (int)(idx & 63);
    const int pixel = (int)((idx >> 6) % npix), a = (int)((idx >> 6) / npix);
    return nn11_f32(nn11_bf16(w[(int64_t)a * 64 * npix + (int64_t)c * npix + pixel]));
}

// ---- activation image
TQ_HD int64_t nn11_act_index(int64_t persp, int pixel, int c, int npix, int cp) { return (persp * npix + pixel) * cp + c; }

// ---- tap -> source pixel.  (y, x): the OUTPUT pixel in its own grid (d x d; (d-2) x (d-2) for NN11_VALID); tap =
// 3 ky + kx.  -> pixel index in the d x d input grid, or -1 for the zero padding.  NN11_FULL is the transpose of
// NN11_VALID (a full correlation): the output grid is d x d, the input grid (d-2) x (d-2), and the source of tap
// (ky, kx) is (y + ky - 2, x + kx - 2) where that lies inside it.
TQ_HD int nn11_src_pixel(int mode, int d, int y, int x, int tap) {
    int sy = y + tap / 3 - 1, sx = x + tap % 3 - 1;
    if (mode == NN11_FULL) {
        sy -= 1; sx -= 1;
        return (sy < 0 || sy >= d - 2 || sx < 0 || sx >= d - 2) ? -1 : sy * (d - 2) + sx;
    }
    if (mode == NN11_VALID) { sy += 1; sx += 1; }
    else if (mode == NN11_CIRCULAR) {
        sy = sy < 0 ? sy + d : (sy >= d ? sy - d : sy);
        sx = sx < 0 ? sx + d : (sx >= d ? sx - d : sx);
    } else if (sy < 0 || sy >= d || sx < 0 || sx >= d) return -1;
    return sy * d + sx;
}

// ---- tile geometry of one workgroup: G whole perspectives, G d^2 rows in MT tiles of 32 (the MFMA's N), NW waves
// with MW tiles each.
template <int D>
struct NN11Geom {
    static constexpr int PIX = D * D;
    static constexpr int OPIX = (D - 2) * (D - 2);
    static constexpr int G = 256 / PIX > 0 ? 256 / PIX : 1;
    static constexpr int ROWS = G * PIX;
    static constexpr int MT = (ROWS + 31) / 32;
    static constexpr int NW = MT > 8 ? 8 : 4;            // wavefronts: at most two tiles each, so that the accumulators
    static constexpr int MW = (MT + NW - 1) / NW;        // (MW x 4 x 16 registers) leave room for the fragments
    static constexpr int THREADS = NW * 64;
    static constexpr int ZROW = MT * 32;                 // the zero row of the LDS tile
    static constexpr int LROWS = MT * 32 + 1;
};
inline int nn11_group(int d) { const int g = 256 / (d * d); return g > 0 ? g : 1; }

// ---- host-side pack (what k_nn11_pack does on the device), for the header's unit test
inline void nn11_pack_layer_host(int l, const float* w, const float* b, uint16_t* wimg, float* bias) {
    conv_pack_layer_host(nn11_cin(l), nn11_cout(l), 9, w, b, wimg, bias);
}
inline void nn11_pack_dgrad_host(int l, const float* w, uint16_t* dimg) {       // l = 2..11
    conv_pack_dgrad_host(nn11_cin(l), nn11_cout(l), w, dimg);
}
inline void nn11_pack_linear_host(int d, const float* w, float* limg) {
    const int64_t n = nn11_lin_elems(d);
    for (int64_t i = 0; i < n; ++i) limg[i] = nn11_lin_value(i, nn11_out_pixels(d), w);
}

#if defined(__HIPCC__)
// ======================================================================================================= device side
typedef __bf16 nn11_bf16x8 __attribute__((ext_vector_type(8)));
typedef float nn11_f32x16 __attribute__((ext_vector_type(16)));

struct NN11Pack { const float* w[NN11_LAYERS + 1]; const float* b[NN11_LAYERS + 1]; };

// The one more argument of a gathering k_nn11_conv: the row list.
constexpr int NN11_ERR_INDEX = 1;                         // the forward handle's latch: a row index outside the stack was seen
struct NN11Rows { const int32_t* rows; int64_t stack_rows; int* latch; };
__device__ __forceinline__ const NN11Rows& nn11_rows_arg(const NN11Rows& g) { return g; }

// one block row (blockIdx.y) per layer: y = 0..10 conv l = y + 1 (image, then its padded bias); y = 11 the linear layer
__global__ __launch_bounds__(256) void k_nn11_pack(NN11Pack p, int d, uint16_t* wimg, float* bias, float* limg, float* lbias) {
    const int l = (int)blockIdx.y + 1;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (l <= NN11_LAYERS) {
        const int64_t n = nn11_wimg_elems(l);
        uint16_t* img = wimg + nn11_wimg_offset(l);
        for (int64_t e = i; e < n; e += stride) img[e] = nn11_bf16(nn11_wimg_value(l, e, p.w[l - 1]));
        const int cp = nn11_cpad(nn11_cout(l));
        if (i < cp) bias[nn11_bias_offset(l) + i] = i < nn11_cout(l) ? p.b[l - 1][i] : 0.f;
    } else {
        const int64_t n = nn11_lin_elems(d);
        for (int64_t e = i; e < n; e += stride) limg[e] = nn11_lin_value(e, nn11_out_pixels(d), p.w[NN11_LAYERS]);
        if (i < NN11_OUT) lbias[i] = p.b[NN11_LAYERS][i];
    }
}

__device__ __forceinline__ uint16_t nn11_stack_bf16(const void* stack, int dtype, int64_t i) {
    switch (dtype) {
        case 0: return nn11_bf16(static_cast<const float*>(stack)[i]);
        case 1: return nn11_bf16(__half2float(static_cast<const __half*>(stack)[i]));
        case 2: return static_cast<const uint16_t*>(stack)[i];
        default: return nn11_bf16((float)static_cast<const uint8_t*>(stack)[i]);
    }
}

}  // namespace tq
#define TQ_NN11_DEVICE_DECLARATIONS                       // NN11Geom, NN11Rows, nn11_stack_bf16, conv_chunks, ... are declared
#include "conv_tile.hpp"                                  // conv_tiles, the one tile body, over the declarations above
namespace tq {

// NN_11's and the wide nets' shape policy (conv_tile.hpp): a 3x3 of stride 1 on the d x d grid, MODE as nn11_src_pixel's.
template <int D, int MODE>
struct NN11Shape {
    static constexpr int SIDE = D, OSIDE = MODE == NN11_VALID ? D - 2 : D;
    static constexpr int NPIX_IN = MODE == NN11_FULL ? (D - 2) * (D - 2) : D * D, NPIX_OUT = OSIDE * OSIDE;
    static constexpr int TAPS = 9, STACK = MODE == NN11_CIRCULAR ? CONV_STACK_CIRCULAR : CONV_NO_STACK;
    TQ_HD static int src(int y, int x, int tap) { return nn11_src_pixel(MODE, D, y, x, tap); }
};

// The forward's epilogue, NN_11's and the wide nets': relu(sum + bias) over the layer's padded f32 bias.
struct ConvBiasRelu {
    using Aux = float;                                    // what a kernel's `aux` argument points to
    const float* bias;
    __device__ __forceinline__ float4 operator()(const float4& a, int c0, int64_t) const {
        const float4 b = *reinterpret_cast<const float4*>(bias + c0);
        return make_float4(nn11_relu(a.x + b.x), nn11_relu(a.y + b.y), nn11_relu(a.z + b.z), nn11_relu(a.w + b.w));
    }
};
// The dgrad's: the sum where nn11_mask passes the bf16 activation of `out`'s shape (> 0 or a NaN), else 0.
struct NN11DgradMask {
    using Aux = uint16_t;
    const uint16_t* act;
    __device__ __forceinline__ float4 operator()(const float4& a, int, int64_t at) const {
        const uint2 m = *reinterpret_cast<const uint2*>(act + at);
        return make_float4(nn11_mask((uint16_t)m.x) ? a.x : 0.f, nn11_mask((uint16_t)(m.x >> 16)) ? a.y : 0.f,
                           nn11_mask((uint16_t)m.y) ? a.z : 0.f, nn11_mask((uint16_t)(m.y >> 16)) ? a.w : 0.f);
    }
};

// One conv3x3 layer of NN_11, all n-tiles in one workgroup.  KS: k-steps of 16 input channels per tap (conv1: 2 steps
// over its 18 k values), NT: tiles of 32 output channels, MODE: where a tap's source pixel lies.  `in`: the previous
// layer's activation image (MODE != CIRCULAR; (d-2)^2 pixels for NN11_FULL) or the perspective stack [P][2][d][d] of
// element type `dtype`; `out`: this layer's activation image ((d-2)^2 pixels for NN11_VALID).  Grid: ceil(P / G)
// workgroups of NN11Geom<D>::THREADS threads.
// EPI says what becomes of the sums.  NN11_EPI_BIAS_RELU (the forward): `aux` is the layer's padded f32 bias;
// out = bf16(relu(sum + bias)).  NN11_EPI_MASK (the backward's dgrad over a dgrad image): `aux` is the bf16 activation
// image of `out`'s shape; out = bf16(sum where the activation is > 0, else 0).
// GATHER (conv1 only; ROWS is then NN11Rows, one more argument, and empty otherwise, so that the kernels without it keep
// their argument list): the row list of conv_tiles.
template <int D, int KS, int NT, int MODE, int EPI = NN11_EPI_BIAS_RELU, bool GATHER = false, typename... ROWS>
__global__ __launch_bounds__(NN11Geom<D>::THREADS) void k_nn11_conv(const void* __restrict__ in, int dtype, const uint16_t* __restrict__ wimg,
                                                   const void* __restrict__ aux, uint16_t* __restrict__ out, int64_t P, ROWS... rows_arg) {
    static_assert(!GATHER || MODE == NN11_CIRCULAR, "only conv1 reads the stack");
    static_assert(sizeof...(ROWS) == (GATHER ? 1 : 0), "a gathering conv takes one NN11Rows, the others nothing");
    using Shape = NN11Shape<D, MODE>;
    __shared__ __attribute__((aligned(16))) unsigned char lds[conv_lds_bytes<Shape, KS>()];
    if constexpr (EPI == NN11_EPI_BIAS_RELU)
        conv_tiles<Shape, KS, NT, NT>(lds, 0, in, dtype, wimg, out, P, ConvBiasRelu{static_cast<const float*>(aux)}, rows_arg...);
    else
        conv_tiles<Shape, KS, NT, NT>(lds, 0, in, dtype, wimg, out, P, NN11DgradMask{static_cast<const uint16_t*>(aux)}, rows_arg...);
}

// The linear layer of NN_11 (FEAT_CP = 64) and of the wide nets (224): one wavefront per perspective over the last
// conv's image [P][npix][FEAT_CP] and the linear image f32 [3][npix][FEAT_CP]; f32 sums in a fixed order (lane-strided
// partial sums over 16-byte chunks of 8 features, then a butterfly over the 64 lanes), + bias, f32 out.
template <int FEAT_CP>
__global__ __launch_bounds__(256) void k_nn_linear(const uint16_t* __restrict__ act, const float* __restrict__ limg,
                                                   const float* __restrict__ lbias, float* __restrict__ q, int64_t P, int npix) {
    const int lane = threadIdx.x & 63;
    const int64_t p = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (p >= P) return;
    const int chunks = npix * (FEAT_CP / 8);
    const uint4* a = reinterpret_cast<const uint4*>(act + p * npix * FEAT_CP);
    float s[NN11_OUT] = {0.f, 0.f, 0.f};
    for (int c = lane; c < chunks; c += 64) {
        const uint4 v = a[c];
        const uint32_t wd[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const float x = nn11_f32((uint16_t)(wd[j >> 1] >> (16 * (j & 1))));
#pragma unroll
            for (int o = 0; o < NN11_OUT; ++o) s[o] += x * limg[((int64_t)o * npix * FEAT_CP) + c * 8 + j];
        }
    }
#pragma unroll
    for (int o = 0; o < NN11_OUT; ++o) {
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) s[o] += __shfl_xor(s[o], m);
        if (lane == 0) q[p * NN11_OUT + o] = s[o] + lbias[o];
    }
}
#endif  // __HIPCC__

}  // namespace tq
