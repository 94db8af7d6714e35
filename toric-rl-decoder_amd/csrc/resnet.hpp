// Forward pass of the reference's default Q-network, ResNet18 (src/nn/torch/ResNet.py, BasicBlock nets), and of
// ResNet34, which has the same layer shapes and other block counts: eval-mode BatchNorm only.  Implicit-GEMM
// convolutions on v_mfma_f32_32x32x16_bf16 with NN_11's images, fragment order and tile geometry (nn11.hpp), cut like the
// wide nets' (nnw.hpp): at most RESNET_NTB = 4 n-tiles per workgroup across blockIdx.y, the input channels staged in equal
// chunks of at most 8 k-steps.  What is new against k_nnw_conv:
//   - BatchNorm folded at load into two f32 vectors per convolution, scale s = gamma / sqrt(var + eps) and shift
//     t = beta - mean s; the epilogue is z = acc s + t, [z = z + r,] [ReLU,] one rounding to bf16;
//   - 1x1 convolutions (the shortcuts), which read the centre pixel, and stride 2 onto the half grid of side
//     s = (d + 1) / 2: the 3x3 reads (2y + ky - 1, 2x + kx - 1), zero outside, the 1x1 reads (2y, 2x);
//   - the side of the input grid is the template parameter, even sides included (the half grid of d = 3, 7, 11, ...);
//   - the stack-reading first layer is zero padded;
//   - 512-channel layers: four block rows, four chunks;
//   - an average-pool head: Q[a] = (sum_c S[c] bf16(W[a][c])) / s^2 + b[a] with S[c] the f32 sum of channel c over the
//     pixels in pixel order, so the weights do not depend on d.
// Numerics contract: include/toricenv.h, DESIGN.md 3.11.  The order of a sum is (chunk, tap, k-step) and depends on
// (net, convolution, d) alone; no atomics.
//
// The table and the index functions are host+device: the pack kernel, the conv kernel and a g++ build of this header
// (tests/host_resnet_shim.cpp) share them.  Convolutions are numbered in the order of the module's state_dict: the stem,
// then per block conv1, conv2 and, where there is one, the shortcut's 1x1.
#pragma once
#include <math.h>

#include "nn11.hpp"

namespace tq {

constexpr int RESNET_NETS = 2;                        // slot 0: ResNet18 (TQ_NET_RESNET18), slot 1: ResNet34
constexpr int RESNET_STAGES = 4;                      // layer1 .. layer4
constexpr int RESNET_BLOCKS[RESNET_NETS][RESNET_STAGES] = {{2, 2, 2, 2}, {3, 4, 6, 3}};
constexpr int RESNET_PLANES[RESNET_STAGES] = {64, 128, 256, 512};
constexpr int RESNET_STRIDE[RESNET_STAGES] = {1, 1, 1, 2};           // of a stage's first block
constexpr int RESNET_STEM = 64;                       // channels of conv1
constexpr int RESNET_MAX_CONVS = 36;                  // ResNet34: 1 + 2 x 16 + 3
constexpr int RESNET_FEAT = 512;                      // channels of the last image: the head's features
constexpr int RESNET_MAX_CP = 256;                    // an activation image holds max_rows * d^2 * 256 bf16: 512 s^2 <= 256 d^2
constexpr int RESNET_NTB = 4;                         // n-tiles of one workgroup
constexpr int RESNET_CHUNK_KS = 8;                    // k-steps of one staged chunk, at most

enum { RESNET_STEM_CONV = 0, RESNET_CONV1 = 1, RESNET_CONV2 = 2, RESNET_SHORTCUT = 3 };       // a convolution's role
enum { RESNET_EPI_NONE = 0, RESNET_EPI_RELU = 1, RESNET_EPI_ADD_RELU = 2 };                   // what follows z = acc s + t

inline int resnet_slot(int net) { return net == 18 ? 0 : (net == 34 ? 1 : -1); }    // TQ_NET_RESNET18 / 34 -> slot
TQ_HD int resnet_half(int d) { return (d + 1) / 2; }                                // side of the grid behind the stride 2

// stage st = 0..3, block b: has the block a 1x1 convolution on its shortcut?
TQ_HD bool resnet_has_shortcut(int st, int b) {
    const int in = st == 0 ? RESNET_STEM : RESNET_PLANES[st - 1];
    return b == 0 && (RESNET_STRIDE[st] != 1 || in != RESNET_PLANES[st]);
}
TQ_HD int resnet_convs(int s) {
    int n = 1;
    for (int st = 0; st < RESNET_STAGES; ++st)
        for (int b = 0; b < RESNET_BLOCKS[s][st]; ++b) n += 2 + (resnet_has_shortcut(st, b) ? 1 : 0);
    return n;
}
// stage: 0 the stem, 1..4 layer1..layer4; half_in / half_out: the input / output grid is the half grid
struct ResConv { int cin, cout, taps, stride, role, stage, block, half_in, half_out; };
// convolution i = 0..resnet_convs(s) - 1 of slot s
TQ_HD ResConv resnet_conv(int s, int i) {
    int n = 1, in = RESNET_STEM, half = 0;
    if (i > 0)
        for (int st = 0; st < RESNET_STAGES; ++st)
            for (int b = 0; b < RESNET_BLOCKS[s][st]; ++b) {
                const int planes = RESNET_PLANES[st], stride = b == 0 ? RESNET_STRIDE[st] : 1;
                const int sc = resnet_has_shortcut(st, b) ? 1 : 0, hout = (half || stride == 2) ? 1 : 0;
                if (i == n) return ResConv{in, planes, 9, stride, RESNET_CONV1, st + 1, b, half, hout};
                if (i == n + 1) return ResConv{planes, planes, 9, 1, RESNET_CONV2, st + 1, b, hout, hout};
                if (sc && i == n + 2) return ResConv{in, planes, 1, stride, RESNET_SHORTCUT, st + 1, b, half, hout};
                n += 2 + sc; in = planes; half = hout;
            }
    return ResConv{2, RESNET_STEM, 9, 1, RESNET_STEM_CONV, 0, 0, 0, 0};
}

// ---- one convolution by its channel counts and taps.  The one whose input has 2 channels reads the stack: its weight
// image has one "tap" whose k runs over (input channel, 3x3 tap), as NN_11's conv1.
TQ_HD bool resnet_reads_stack(int cin) { return cin == 2; }
TQ_HD int resnet_img_taps(int cin, int taps) { return resnet_reads_stack(cin) ? 1 : taps; }
TQ_HD int resnet_kdim(int cin) { return resnet_reads_stack(cin) ? 18 : cin; }
TQ_HD int resnet_ksteps(int cin) { return resnet_reads_stack(cin) ? 2 : nn11_cpad(cin) / 16; }
TQ_HD int resnet_ntiles(int cout) { return nn11_cpad(cout) / 32; }
TQ_HD int resnet_chunks(int ksteps) { return (ksteps + RESNET_CHUNK_KS - 1) / RESNET_CHUNK_KS; }
TQ_HD int64_t resnet_wimg_elems(int cin, int cout, int taps) {
    return (int64_t)resnet_img_taps(cin, taps) * resnet_ksteps(cin) * resnet_ntiles(cout) * 512;
}
// the value (before rounding) of image element idx from the torch weight [cout][cin][3][3] or [cout][cin][1][1]
TQ_HD float resnet_wimg_value(int cin, int cout, int taps, int64_t idx, const float* w) {
    const NN11WCoord c = nn11_wimg_coord(idx, resnet_ksteps(cin), resnet_ntiles(cout));
    if (c.cout >= cout || c.k >= resnet_kdim(cin)) return 0.f;
    if (resnet_reads_stack(cin)) return w[(int64_t)c.cout * 18 + c.k];          // k = nn11_k1(cin, tap)
    if (taps == 1) return w[(int64_t)c.cout * cin + c.k];
    return w[((int64_t)c.cout * cin + c.k) * 9 + c.tap];
}
// where convolution i lies in the handle's one weight image and in its scale and shift arrays (i = convs: their sizes)
TQ_HD int64_t resnet_wimg_offset(int s, int i) {
    int64_t o = 0;
    for (int j = 0; j < i; ++j) { const ResConv c = resnet_conv(s, j); o += resnet_wimg_elems(c.cin, c.cout, c.taps); }
    return o;
}
TQ_HD int resnet_st_offset(int s, int i) {
    int o = 0;
    for (int j = 0; j < i; ++j) o += nn11_cpad(resnet_conv(s, j).cout);
    return o;
}

// ---- tap -> source pixel.  (y, x): the OUTPUT pixel in its own grid (side x side, or the half grid for stride 2); -> pixel
// index in the side x side input grid, or -1 for the zero padding.  A 1x1 convolution reads the centre tap.
TQ_HD int resnet_src_pixel(int side, int stride, int taps, int y, int x, int tap) {
    if (taps == 1) tap = 4;
    if (stride == 1) return nn11_src_pixel(NN11_ZERO, side, y, x, tap);
    const int sy = 2 * y + tap / 3 - 1, sx = 2 * x + tap % 3 - 1;
    return (sy < 0 || sy >= side || sx < 0 || sx >= side) ? -1 : sy * side + sx;
}

// ---- eval-mode BatchNorm folded: s = gamma / sqrt(var + eps), t = beta - mean s; every operation rounded once in f32
struct ResFold { float s, t; };
TQ_HD ResFold resnet_fold(float gamma, float beta, float mean, float var, float eps) {
    const float s = gamma / sqrtf(var + eps);
    const float ms = mean * s;
    return ResFold{s, beta - ms};
}

// ---- linear image f32 [a][512] holding bf16-rounded values
TQ_HD int64_t resnet_lin_elems() { return (int64_t)NN11_OUT * RESNET_FEAT; }
TQ_HD float resnet_lin_value(int64_t idx, const float* w) { return nn11_f32(nn11_bf16(w[idx])); }

// ---- host-side pack (what k_resnet_pack does on the device), for the header's unit test
inline void resnet_pack_conv_host(int cin, int cout, int taps, const float* w, const float* gamma, const float* beta, const float* mean,
                                  const float* var, float eps, uint16_t* wimg, float* scale, float* shift) {
    const int64_t n = resnet_wimg_elems(cin, cout, taps);
    for (int64_t i = 0; i < n; ++i) wimg[i] = nn11_bf16(resnet_wimg_value(cin, cout, taps, i, w));
    const int cp = nn11_cpad(cout);
    for (int c = 0; c < cp; ++c) {
        const ResFold f = c < cout ? resnet_fold(gamma[c], beta[c], mean[c], var[c], eps) : ResFold{0.f, 0.f};
        scale[c] = f.s; shift[c] = f.t;
    }
}
inline void resnet_pack_linear_host(const float* w, float* limg) {
    for (int64_t i = 0; i < resnet_lin_elems(); ++i) limg[i] = resnet_lin_value(i, w);
}

#if defined(__HIPCC__)
// ======================================================================================================= device side
// torch tensors of one net: per convolution the weight and gamma, beta, running mean, running var; then the linear layer
struct ResNetPack { const float* w[RESNET_MAX_CONVS]; const float* bn[RESNET_MAX_CONVS][4]; const float* lw; const float* lb; };

// one block row (blockIdx.y) per convolution of slot s (image, then its scale and shift); y = convs: the linear layer
__global__ __launch_bounds__(256) void k_resnet_pack(ResNetPack p, int s, float eps, uint16_t* wimg, float* scale, float* shift,
                                                     float* limg, float* lbias) {
    const int i = (int)blockIdx.y, n = resnet_convs(s);
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) {
        const ResConv c = resnet_conv(s, i);
        const int64_t elems = resnet_wimg_elems(c.cin, c.cout, c.taps);
        uint16_t* img = wimg + resnet_wimg_offset(s, i);
        for (int64_t e = t; e < elems; e += stride) img[e] = nn11_bf16(resnet_wimg_value(c.cin, c.cout, c.taps, e, p.w[i]));
        if (t < nn11_cpad(c.cout)) {
            const ResFold f = t < c.cout ? resnet_fold(p.bn[i][0][t], p.bn[i][1][t], p.bn[i][2][t], p.bn[i][3][t], eps) : ResFold{0.f, 0.f};
            const int o = resnet_st_offset(s, i) + (int)t;
            scale[o] = f.s; shift[o] = f.t;
        }
    } else {
        for (int64_t e = t; e < resnet_lin_elems(); e += stride) limg[e] = resnet_lin_value(e, p.lw);
        if (t < NN11_OUT) lbias[t] = p.lb[t];
    }
}

// The n-tiles n0 .. n0 + NTB - 1 of one convolution for the workgroup's G perspectives; `lds`: the kernel's tile.  See
// k_resnet_conv.
template <int S, int KS, int NT, int TAPS, int STRIDE, bool STACK, int NTB>
__device__ __forceinline__ void resnet_conv_tiles(unsigned char* lds, int n0, const void* __restrict__ in, int dtype,
                                                  const uint16_t* __restrict__ wimg, const float* __restrict__ scale,
                                                  const float* __restrict__ shift, int epi, const uint16_t* __restrict__ res,
                                                  uint16_t* __restrict__ out, int64_t P) {
    using Ge = NN11Geom<S>;
    constexpr int PIX = Ge::PIX, G = Ge::G, MW = Ge::MW, NW = Ge::NW, THREADS = Ge::THREADS;
    constexpr int OS = STRIDE == 2 ? (S + 1) / 2 : S;                       // side of the output grid
    constexpr int NPIX_OUT = OS * OS;
    constexpr int ROWS_OUT = G * NPIX_OUT;                                  // <= Ge::ROWS: tiles beyond are skipped
    constexpr int CINP = KS * 16, COUTP = NT * 32;
    constexpr int NCHUNK = (KS + RESNET_CHUNK_KS - 1) / RESNET_CHUNK_KS, CK = KS / NCHUNK;    // k-steps of one chunk
    static_assert(CK * NCHUNK == KS && CK <= RESNET_CHUNK_KS, "the k-steps of a layer are cut into equal chunks");
    static_assert(!STACK || (TAPS == 9 && STRIDE == 1 && KS == 2), "the stack layer is a 3x3 of stride 1 over 18 k values");
    constexpr int PITCH = CK * 32 + 16;                                     // as NN_11's: rows start in different banks

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t persp0 = (int64_t)blockIdx.x * G;
    const int np = (int)(P - persp0 < G ? P - persp0 : G);                  // perspectives of this workgroup

    // this lane's output pixel in each of the wave's tiles (tile i of wave w is tile NW i + w)
    const int r = lane & 31, h = lane >> 5;
    int py[MW], px[MW], pbase[MW];                                          // pbase < 0: no such row
#pragma unroll
    for (int i = 0; i < MW; ++i) {
        const int row = (NW * i + wave) * 32 + r;
        const int p = row / NPIX_OUT, q = row % NPIX_OUT;
        py[i] = q / OS; px[i] = q % OS;
        pbase[i] = row < ROWS_OUT ? p * PIX : -1;
    }

    nn11_f32x16 acc[MW][NTB];
#pragma unroll
    for (int i = 0; i < MW; ++i)
#pragma unroll
        for (int n = 0; n < NTB; ++n)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[i][n][e] = 0.f;

    const uint4* wfrag = reinterpret_cast<const uint4*>(wimg) + (int64_t)n0 * 64 + lane;    // fragment f, tile n0: wfrag[f * 64]

    if constexpr (STACK) {
        // the stack as bf16, exactly as k_nn11_conv stages it; a tap in the zero padding contributes 0
        uint16_t* s = reinterpret_cast<uint16_t*>(lds);
        for (int i = tid; i < G * 2 * PIX; i += THREADS)
            s[i] = i < np * 2 * PIX ? nn11_stack_bf16(in, dtype, persp0 * 2 * PIX + i) : (uint16_t)0;
        __syncthreads();
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
            uint4 w[NTB];
#pragma unroll
            for (int n = 0; n < NTB; ++n) w[n] = wfrag[(ks * NT + n) * 64];
#pragma unroll
            for (int i = 0; i < MW; ++i) {
                if ((NW * i + wave) * 32 >= ROWS_OUT) continue;              // wave-uniform
                union { uint16_t e[8]; uint4 v; } a;
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const int k = 16 * ks + 8 * h + j;
                    uint16_t v = 0;
                    if (k < 18 && pbase[i] >= 0) {
                        const int sp = resnet_src_pixel(S, 1, 9, py[i], px[i], k % 9);
                        if (sp >= 0) v = s[2 * pbase[i] + (k / 9) * PIX + sp];
                    }
                    a.e[j] = v;
                }
#pragma unroll
                for (int n = 0; n < NTB; ++n)
                    acc[i][n] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(nn11_bf16x8, w[n]),
                                                                        __builtin_bit_cast(nn11_bf16x8, a.v), acc[i][n], 0, 0, 0);
            }
        }
    } else {
        const uint4* src = reinterpret_cast<const uint4*>(static_cast<const uint16_t*>(in) + persp0 * PIX * CINP);
        constexpr int ROW16 = CINP / 8, CH16 = CK * 2;                      // 16-byte pieces of an image row / of its chunk
        for (int c = 0; c < NCHUNK; ++c) {
            __syncthreads();                                                // the previous chunk has been read
            for (int i = tid; i < Ge::LROWS * CH16; i += THREADS) {
                const int row = i / CH16, cc = i % CH16;
                const uint4 v = row < np * PIX ? src[row * ROW16 + c * CH16 + cc] : make_uint4(0, 0, 0, 0);
                *reinterpret_cast<uint4*>(lds + row * PITCH + cc * 16) = v;
            }
            __syncthreads();
            for (int tap = 0; tap < TAPS; ++tap) {
                int arow[MW];                                               // LDS byte address of the lane's source row
#pragma unroll
                for (int i = 0; i < MW; ++i) {
                    const int sp = pbase[i] >= 0 ? resnet_src_pixel(S, STRIDE, TAPS, py[i], px[i], tap) : -1;
                    arow[i] = (sp >= 0 ? pbase[i] + sp : Ge::ZROW) * PITCH + h * 16;
                }
#pragma unroll
                for (int ks = 0; ks < CK; ++ks) {
                    uint4 w[NTB];
#pragma unroll
                    for (int n = 0; n < NTB; ++n) w[n] = wfrag[((tap * KS + c * CK + ks) * NT + n) * 64];
#pragma unroll
                    for (int i = 0; i < MW; ++i) {
                        if ((NW * i + wave) * 32 >= ROWS_OUT) continue;      // wave-uniform
                        const uint4 a = *reinterpret_cast<const uint4*>(lds + arow[i] + ks * 32);
#pragma unroll
                        for (int n = 0; n < NTB; ++n)
                            acc[i][n] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(nn11_bf16x8, w[n]),
                                                                                __builtin_bit_cast(nn11_bf16x8, a), acc[i][n], 0, 0, 0);
                    }
                }
            }
        }
    }

    // epilogue: accumulator register 4 g + q of lane (r, h) = output channel 32 (n0 + n) + 8 g + 4 h + q of pixel r
#pragma unroll
    for (int i = 0; i < MW; ++i) {
        const int row = (NW * i + wave) * 32 + r;
        if (row >= np * NPIX_OUT || pbase[i] < 0) continue;
        const int64_t o = (persp0 * NPIX_OUT + row) * COUTP;
#pragma unroll
        for (int n = 0; n < NTB; ++n)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int c0 = 32 * (n0 + n) + 8 * g + 4 * h;
                const float4 sc = *reinterpret_cast<const float4*>(scale + c0);
                const float4 sh = *reinterpret_cast<const float4*>(shift + c0);
                float v0 = acc[i][n][4 * g + 0] * sc.x + sh.x, v1 = acc[i][n][4 * g + 1] * sc.y + sh.y;
                float v2 = acc[i][n][4 * g + 2] * sc.z + sh.z, v3 = acc[i][n][4 * g + 3] * sc.w + sh.w;
                if (epi == RESNET_EPI_ADD_RELU) {                           // uniform over the workgroup
                    const uint2 rr = *reinterpret_cast<const uint2*>(res + o + c0);
                    v0 += nn11_f32((uint16_t)rr.x); v1 += nn11_f32((uint16_t)(rr.x >> 16));
                    v2 += nn11_f32((uint16_t)rr.y); v3 += nn11_f32((uint16_t)(rr.y >> 16));
                }
                if (epi != RESNET_EPI_NONE) { v0 = fmaxf(v0, 0.f); v1 = fmaxf(v1, 0.f); v2 = fmaxf(v2, 0.f); v3 = fmaxf(v3, 0.f); }
                uint2 pk;
                pk.x = (uint32_t)nn11_bf16(v0) | ((uint32_t)nn11_bf16(v1) << 16);
                pk.y = (uint32_t)nn11_bf16(v2) | ((uint32_t)nn11_bf16(v3) << 16);
                *reinterpret_cast<uint2*>(out + o + c0) = pk;
            }
    }
}

// One convolution with its folded BatchNorm.  S: side of the INPUT grid (odd 3..21, or a half side 2..11); KS: k-steps of
// 16 input channels per tap (the stack layer: 2 steps over its 18 k values); NT: tiles of 32 output channels; TAPS: 9, or
// 1 for a 1x1, which reads the centre pixel; STRIDE 2 writes the half grid of side (S + 1) / 2: the workgroup stages the G
// input perspectives of NN11Geom<S> and computes their G ((S + 1) / 2)^2 output rows; STACK: `in` is the perspective
// stack [P][2][S][S] of element type `dtype`, zero padded, else the activation image [P][S^2][16 KS].
// `scale` / `shift`: the convolution's padded f32 vectors.  `epi` (the same for every workgroup of a launch):
// RESNET_EPI_NONE out = bf16(acc s + t); RESNET_EPI_RELU out = bf16(relu(acc s + t)); RESNET_EPI_ADD_RELU
// out = bf16(relu((acc s + t) + res)) with `res` a bf16 image of out's shape.  `out`: [P][output pixels][32 NT].
// Grid: (ceil(P / G), ceil(NT / RESNET_NTB)) workgroups of NN11Geom<S>::THREADS threads.
template <int S, int KS, int NT, int TAPS, int STRIDE, bool STACK>
__global__ __launch_bounds__(NN11Geom<S>::THREADS) void k_resnet_conv(const void* __restrict__ in, int dtype, const uint16_t* __restrict__ wimg,
                                                     const float* __restrict__ scale, const float* __restrict__ shift, int epi,
                                                     const uint16_t* __restrict__ res, uint16_t* __restrict__ out, int64_t P) {
    using Ge = NN11Geom<S>;
    constexpr int NCHUNK = (KS + RESNET_CHUNK_KS - 1) / RESNET_CHUNK_KS, CK = KS / NCHUNK;
    constexpr int LDS_BYTES = STACK ? ((Ge::G * 2 * Ge::PIX * 2 + 15) & ~15) : Ge::LROWS * (CK * 32 + 16);
    static_assert(LDS_BYTES <= 122128, "never above k_nnw_conv's tile");
    __shared__ __attribute__((aligned(16))) unsigned char lds[LDS_BYTES];
    constexpr int REM = NT % RESNET_NTB;                                    // n-tiles of the last block row, if fewer
    const int n0 = (int)blockIdx.y * RESNET_NTB;
    if constexpr (NT < RESNET_NTB) {                                        // 64 output channels: one block row of two
        resnet_conv_tiles<S, KS, NT, TAPS, STRIDE, STACK, NT>(lds, n0, in, dtype, wimg, scale, shift, epi, res, out, P);
    } else {
        if constexpr (REM != 0) {
            if (n0 + RESNET_NTB > NT) {                                     // uniform over the workgroup
                resnet_conv_tiles<S, KS, NT, TAPS, STRIDE, STACK, REM>(lds, n0, in, dtype, wimg, scale, shift, epi, res, out, P);
                return;
            }
        }
        resnet_conv_tiles<S, KS, NT, TAPS, STRIDE, STACK, RESNET_NTB>(lds, n0, in, dtype, wimg, scale, shift, epi, res, out, P);
    }
}

// The head: average pool and linear layer, one wavefront per perspective over the last image [P][npix][512].  Lane l
// holds channels 8 l .. 8 l + 7: S[c] summed over the pixels in pixel order, then the lane's partial sum over its eight
// channels in channel order, then a butterfly over the 64 lanes; Q = sum / npix + bias.
__global__ __launch_bounds__(256) void k_resnet_head(const uint16_t* __restrict__ act, const float* __restrict__ limg,
                                                     const float* __restrict__ lbias, float* __restrict__ q, int64_t P, int npix) {
    const int lane = threadIdx.x & 63;
    const int64_t p = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (p >= P) return;
    const uint4* a = reinterpret_cast<const uint4*>(act + p * npix * RESNET_FEAT) + lane;
    float S[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    for (int x = 0; x < npix; ++x) {
        const uint4 v = a[x * (RESNET_FEAT / 8)];
        const uint32_t wd[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int j = 0; j < 8; ++j) S[j] += nn11_f32((uint16_t)(wd[j >> 1] >> (16 * (j & 1))));
    }
    float s[NN11_OUT] = {0.f, 0.f, 0.f};
#pragma unroll
    for (int j = 0; j < 8; ++j)
#pragma unroll
        for (int o = 0; o < NN11_OUT; ++o) s[o] += S[j] * limg[o * RESNET_FEAT + lane * 8 + j];
#pragma unroll
    for (int o = 0; o < NN11_OUT; ++o) {
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) s[o] += __shfl_xor(s[o], m);
        if (lane == 0) q[p * NN11_OUT + o] = s[o] / (float)npix + lbias[o];
    }
}
#endif  // __HIPCC__

}  // namespace tq
