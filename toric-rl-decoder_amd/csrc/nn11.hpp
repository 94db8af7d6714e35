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
// layer l = 1..11
TQ_HD int nn11_cin(int l) { return NN11_CH[l - 1]; }
TQ_HD int nn11_cout(int l) { return NN11_CH[l]; }
TQ_HD int nn11_mode(int l) { return l == 1 ? NN11_CIRCULAR : (l == NN11_LAYERS ? NN11_VALID : NN11_ZERO); }
TQ_HD int nn11_taps(int l) { return l == 1 ? 1 : 9; }                                  // taps of the weight image
TQ_HD int nn11_kdim(int l) { return l == 1 ? 18 : nn11_cin(l); }                       // k values per image tap
TQ_HD int nn11_ksteps(int l) { return l == 1 ? 2 : nn11_cpad(nn11_cin(l)) / 16; }
TQ_HD int nn11_ntiles(int l) { return nn11_cpad(nn11_cout(l)) / 32; }
TQ_HD int64_t nn11_wimg_elems(int l) { return (int64_t)nn11_taps(l) * nn11_ksteps(l) * nn11_ntiles(l) * 512; }
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

// ---- bf16, round to nearest even (finite inputs; NaN is not produced by this network's arithmetic on finite weights)
TQ_HD uint16_t nn11_bf16(float f) {
    uint32_t u;
#if defined(__HIP_DEVICE_COMPILE__)
    u = __float_as_uint(f);
#else
    memcpy(&u, &f, 4);
#endif
    u += 0x7fffu + ((u >> 16) & 1u);
    return (uint16_t)(u >> 16);
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

// the ReLU mask of the backward pass: a stored bf16 activation is > 0 (activations are never negative or NaN)
TQ_HD bool nn11_mask(uint16_t a) { return a != 0 && !(a & 0x8000u); }

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
// the value (before rounding) of image element idx of layer l from the torch weight [cout][cin][3][3]; 0 in the padding
TQ_HD float nn11_wimg_value(int l, int64_t idx, const float* w) {
    const NN11WCoord c = nn11_wimg_coord(idx, nn11_ksteps(l), nn11_ntiles(l));
    if (c.cout >= nn11_cout(l) || c.k >= nn11_kdim(l)) return 0.f;
    if (l == 1) return w[(int64_t)c.cout * 18 + c.k];                   // [cout][cin][ky][kx] with k = cin * 9 + tap
    return w[((int64_t)c.cout * nn11_cin(l) + c.k) * 9 + c.tap];
}

// ---- dgrad weight image of layer l = 2..11: the image of the convolution that takes G_l (cout(l) channels) to the
// gradient of layer l - 1's output (cin(l) channels).  Same fragment order with the two channel counts in each other's
// place and the taps flipped: element (cout' = ci, k = co, tap') = W_l[co][ci][8 - tap'].
TQ_HD int nn11_dksteps(int l) { return nn11_cpad(nn11_cout(l)) / 16; }
TQ_HD int nn11_dntiles(int l) { return nn11_cpad(nn11_cin(l)) / 32; }
TQ_HD int64_t nn11_dimg_elems(int l) { return (int64_t)9 * nn11_dksteps(l) * nn11_dntiles(l) * 512; }
TQ_HD int64_t nn11_dimg_offset(int l) {            // first element of layer l = 2..12 in the handle's one dgrad image
    int64_t o = 0;
    for (int i = 2; i < l; ++i) o += nn11_dimg_elems(i);
    return o;
}
TQ_HD float nn11_dimg_value(int l, int64_t idx, const float* w) {
    const NN11WCoord c = nn11_wimg_coord(idx, nn11_dksteps(l), nn11_dntiles(l));       // .cout: ci, .k: co
    if (c.cout >= nn11_cin(l) || c.k >= nn11_cout(l)) return 0.f;
    return w[((int64_t)c.k * nn11_cin(l) + c.cout) * 9 + (8 - c.tap)];
}

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
    const int64_t n = nn11_wimg_elems(l);
    for (int64_t i = 0; i < n; ++i) wimg[i] = nn11_bf16(nn11_wimg_value(l, i, w));
    const int cp = nn11_cpad(nn11_cout(l));
    for (int c = 0; c < cp; ++c) bias[c] = c < nn11_cout(l) ? b[c] : 0.f;
}
inline void nn11_pack_dgrad_host(int l, const float* w, uint16_t* dimg) {       // l = 2..11
    const int64_t n = nn11_dimg_elems(l);
    for (int64_t i = 0; i < n; ++i) dimg[i] = nn11_bf16(nn11_dimg_value(l, i, w));
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

// One conv3x3 + bias + ReLU layer.  KS: k-steps of 16 input channels per tap (conv1: 2 steps over its 18 k values),
// NT: tiles of 32 output channels, MODE: where a tap's source pixel lies.  `in`: the previous layer's activation image
// (MODE != CIRCULAR) or the perspective stack [P][2][d][d] of element type `dtype`; `out`: this layer's activation image
// ((d-2)^2 pixels for NN11_VALID).  Grid: ceil(P / G) workgroups of NN11Geom<D>::THREADS threads.
// EPI says what becomes of the sums.  NN11_EPI_BIAS_RELU (the forward): `aux` is the layer's padded f32 bias;
// out = bf16(relu(sum + bias)).  NN11_EPI_MASK (the backward's dgrad over a dgrad image; NN11_FULL reads a (d-2)^2
// image): `aux` is the bf16 activation image of `out`'s shape; out = bf16(sum where the activation is > 0, else 0).
// GATHER (conv1 only; ROWS is then NN11Rows, one more argument `g`, and empty otherwise, so that the kernels without it
// keep their argument list): perspective i of the call is row g.rows[i] of the stack `in` -- any list, unsorted, with
// repeats.  An index outside [0, g.stack_rows) stages zeros, reads nothing and sets NN11_ERR_INDEX in g.latch.
template <int D, int KS, int NT, int MODE, int EPI = NN11_EPI_BIAS_RELU, bool GATHER = false, typename... ROWS>
__global__ __launch_bounds__(NN11Geom<D>::THREADS) void k_nn11_conv(const void* __restrict__ in, int dtype, const uint16_t* __restrict__ wimg,
                                                   const void* __restrict__ aux, uint16_t* __restrict__ out, int64_t P, ROWS... rows_arg) {
    static_assert(!GATHER || MODE == NN11_CIRCULAR, "only conv1 reads the stack");
    static_assert(sizeof...(ROWS) == (GATHER ? 1 : 0), "a gathering conv takes one NN11Rows, the others nothing");
    using Ge = NN11Geom<D>;
    constexpr int PIX = Ge::PIX, G = Ge::G, MW = Ge::MW, NW = Ge::NW, THREADS = Ge::THREADS;
    constexpr int NPIX_OUT = MODE == NN11_VALID ? Ge::OPIX : PIX;
    constexpr int OD = MODE == NN11_VALID ? D - 2 : D;                      // side of the output grid
    constexpr int ROWS_OUT = G * NPIX_OUT;
    constexpr int NPIX_IN = MODE == NN11_FULL ? Ge::OPIX : PIX;             // pixels of one perspective in `in`
    constexpr int CINP = KS * 16, COUTP = NT * 32;
    // LDS: the workgroup's input rows, channels last, 16 bytes of padding per row (consecutive rows start in different
    // banks: the 16-byte fragment reads of 8 neighbouring pixels are conflict-free); conv1 stages its G x 2 x d^2 stack
    // elements as bf16 instead.
    constexpr int PITCH = CINP * 2 + 16;
    constexpr int LDS_BYTES = MODE == NN11_CIRCULAR ? ((G * 2 * PIX * 2 + 15) & ~15) : Ge::LROWS * PITCH;
    __shared__ __attribute__((aligned(16))) unsigned char lds[LDS_BYTES];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t persp0 = (int64_t)blockIdx.x * G;
    const int np = (int)(P - persp0 < G ? P - persp0 : G);                  // perspectives of this workgroup

    if constexpr (MODE == NN11_CIRCULAR) {
        uint16_t* s = reinterpret_cast<uint16_t*>(lds);
        if constexpr (GATHER) {
            const NN11Rows& g = nn11_rows_arg(rows_arg...);
            for (int i = tid; i < G * 2 * PIX; i += THREADS) {
                uint16_t v = 0;
                if (i < np * 2 * PIX) {
                    const int p = i / (2 * PIX), c = i - p * (2 * PIX);
                    const int64_t row = g.rows[persp0 + p];
                    if (row >= 0 && row < g.stack_rows) v = nn11_stack_bf16(in, dtype, row * (2 * PIX) + c);
                    else if (c == 0) atomicOr(g.latch, NN11_ERR_INDEX);
                }
                s[i] = v;
            }
        } else {
            for (int i = tid; i < G * 2 * PIX; i += THREADS)
                s[i] = i < np * 2 * PIX ? nn11_stack_bf16(in, dtype, persp0 * 2 * PIX + i) : (uint16_t)0;
        }
    } else {
        const uint4* src = reinterpret_cast<const uint4*>(static_cast<const uint16_t*>(in) + persp0 * NPIX_IN * CINP);
        constexpr int CH16 = CINP / 8;                                      // 16-byte chunks per row
        for (int c = tid; c < Ge::LROWS * CH16; c += THREADS) {
            const int row = c / CH16, cc = c % CH16;
            const uint4 v = row < np * NPIX_IN ? src[c] : make_uint4(0, 0, 0, 0);
            *reinterpret_cast<uint4*>(lds + row * PITCH + cc * 16) = v;
        }
    }
    __syncthreads();

    // this lane's output pixel in each of the wave's tiles (tile i of wave w is tile NW i + w)
    const int r = lane & 31, h = lane >> 5;
    int py[MW], px[MW], pbase[MW];                                          // pbase < 0: no such row
#pragma unroll
    for (int i = 0; i < MW; ++i) {
        const int row = (NW * i + wave) * 32 + r;
        const int p = row / NPIX_OUT, q = row % NPIX_OUT;
        py[i] = q / OD; px[i] = q % OD;
        pbase[i] = row < ROWS_OUT ? p * NPIX_IN : -1;
    }

    nn11_f32x16 acc[MW][NT];
#pragma unroll
    for (int i = 0; i < MW; ++i)
#pragma unroll
        for (int n = 0; n < NT; ++n)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[i][n][e] = 0.f;

    const uint4* wfrag = reinterpret_cast<const uint4*>(wimg) + lane;       // fragment f: wfrag[f * 64]

    if constexpr (MODE == NN11_CIRCULAR) {
        const uint16_t* s = reinterpret_cast<const uint16_t*>(lds);
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
            uint4 w[NT];
#pragma unroll
            for (int n = 0; n < NT; ++n) w[n] = wfrag[(ks * NT + n) * 64];
#pragma unroll
            for (int i = 0; i < MW; ++i) {
                if ((NW * i + wave) * 32 >= ROWS_OUT) continue;              // wave-uniform
                union { uint16_t e[8]; uint4 v; } a;
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const int k = 16 * ks + 8 * h + j;
                    uint16_t v = 0;
                    if (k < 18 && pbase[i] >= 0)
                        v = s[2 * pbase[i] + (k / 9) * PIX + nn11_src_pixel(NN11_CIRCULAR, D, py[i], px[i], k % 9)];
                    a.e[j] = v;
                }
#pragma unroll
                for (int n = 0; n < NT; ++n)
                    acc[i][n] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(nn11_bf16x8, w[n]),
                                                                        __builtin_bit_cast(nn11_bf16x8, a.v), acc[i][n], 0, 0, 0);
            }
        }
    } else {
        for (int tap = 0; tap < 9; ++tap) {
            int arow[MW];                                                   // LDS byte address of the lane's source row
#pragma unroll
            for (int i = 0; i < MW; ++i) {
                const int sp = pbase[i] >= 0 ? nn11_src_pixel(MODE, D, py[i], px[i], tap) : -1;
                arow[i] = (sp >= 0 ? pbase[i] + sp : Ge::ZROW) * PITCH + h * 16;
            }
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) {
                uint4 w[NT];
#pragma unroll
                for (int n = 0; n < NT; ++n) w[n] = wfrag[((tap * KS + ks) * NT + n) * 64];
#pragma unroll
                for (int i = 0; i < MW; ++i) {
                    if ((NW * i + wave) * 32 >= ROWS_OUT) continue;          // wave-uniform
                    const uint4 a = *reinterpret_cast<const uint4*>(lds + arow[i] + ks * 32);
#pragma unroll
                    for (int n = 0; n < NT; ++n)
                        acc[i][n] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(nn11_bf16x8, w[n]),
                                                                            __builtin_bit_cast(nn11_bf16x8, a), acc[i][n], 0, 0, 0);
                }
            }
        }
    }

    // epilogue: accumulator register 4 g + q of lane (r, h) = output channel 32 n + 8 g + 4 h + q of pixel r
#pragma unroll
    for (int i = 0; i < MW; ++i) {
        const int row = (NW * i + wave) * 32 + r;
        if (row >= np * NPIX_OUT || pbase[i] < 0) continue;
        uint16_t* o = out + (persp0 * NPIX_OUT + row) * COUTP;
#pragma unroll
        for (int n = 0; n < NT; ++n)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int c0 = 32 * n + 8 * g + 4 * h;
                float v0, v1, v2, v3;
                if constexpr (EPI == NN11_EPI_BIAS_RELU) {
                    const float4 b = *reinterpret_cast<const float4*>(static_cast<const float*>(aux) + c0);
                    v0 = fmaxf(acc[i][n][4 * g + 0] + b.x, 0.f); v1 = fmaxf(acc[i][n][4 * g + 1] + b.y, 0.f);
                    v2 = fmaxf(acc[i][n][4 * g + 2] + b.z, 0.f); v3 = fmaxf(acc[i][n][4 * g + 3] + b.w, 0.f);
                } else {                                                    // bf16 > 0: sign clear and not a zero
                    const uint2 m = *reinterpret_cast<const uint2*>(static_cast<const uint16_t*>(aux) + (persp0 * NPIX_OUT + row) * COUTP + c0);
                    v0 = nn11_mask((uint16_t)m.x) ? acc[i][n][4 * g + 0] : 0.f; v1 = nn11_mask((uint16_t)(m.x >> 16)) ? acc[i][n][4 * g + 1] : 0.f;
                    v2 = nn11_mask((uint16_t)m.y) ? acc[i][n][4 * g + 2] : 0.f; v3 = nn11_mask((uint16_t)(m.y >> 16)) ? acc[i][n][4 * g + 3] : 0.f;
                }
                uint2 pk;
                pk.x = (uint32_t)nn11_bf16(v0) | ((uint32_t)nn11_bf16(v1) << 16);
                pk.y = (uint32_t)nn11_bf16(v2) | ((uint32_t)nn11_bf16(v3) << 16);
                *reinterpret_cast<uint2*>(o + c0) = pk;
            }
    }
}

// The linear layer: one wavefront per perspective over conv11's image [P][npix][64]; f32 sums in a fixed order (lane-
// strided partial sums, then a butterfly over the 64 lanes), + bias, f32 out.
__global__ __launch_bounds__(256) void k_nn11_linear(const uint16_t* __restrict__ act, const float* __restrict__ limg,
                                                     const float* __restrict__ lbias, float* __restrict__ q, int64_t P, int npix) {
    const int lane = threadIdx.x & 63;
    const int64_t p = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (p >= P) return;
    const int chunks = npix * 8;                                            // 16-byte chunks of 8 features
    const uint4* a = reinterpret_cast<const uint4*>(act + p * npix * 64);
    float s[NN11_OUT] = {0.f, 0.f, 0.f};
    for (int c = lane; c < chunks; c += 64) {
        const uint4 v = a[c];
        const uint32_t wd[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const float x = nn11_f32((uint16_t)(wd[j >> 1] >> (16 * (j & 1))));
#pragma unroll
            for (int o = 0; o < NN11_OUT; ++o) s[o] += x * limg[((int64_t)o * npix * 64) + c * 8 + j];
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
