// Forward pass of the reference's two wide Q-networks (src/nn/torch/NN.py:47-133): NN_8, eight conv3x3 + ReLU, and
// NN_17, twenty of them despite its name, both with up to 256 channels, the paddings of NN_11 (circular pad before the
// unpadded first conv, zero padding 1 in the middle, the last conv unpadded) and Linear(200 (d-2)^2, 3).  Implicit-GEMM
// convolutions on v_mfma_f32_32x32x16_bf16 under NN_11's numerics contract (include/toricenv.h), with
// NN_11's images, fragment order and tile geometry (nn11.hpp): what differs is how a layer is cut.
//   - Output channels are cut across blockIdx.y: a workgroup computes at most NNW_NTB = 4 n-tiles (128 channels), so a
//     wavefront's accumulators stay at the MW x 4 x 16 = 128 registers of NN_11's 128 -> 128 layer.
//   - Input channels are staged in equal chunks of at most 8 k-steps (128 channels): 16 k-steps as 8 + 8, 14 as 7 + 7.
//     Per chunk: barrier, stage, barrier, 9 taps x k-steps.  The LDS tile is never larger than NN_11's own.
// The order of a sum is (chunk, tap, k-step) and depends on (net, layer, d) alone; no atomics.
//
// The index functions take channel counts, not layer numbers, and are host+device: the pack kernel, the conv kernel and
// a g++ build of this header (tests/host_nnw_shim.cpp) share them.  The layer whose input has 2 channels is the one
// that reads the stack: its weight image has one "tap" whose k runs over (input channel, 3x3 tap), as NN_11's conv1.
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
constexpr int NNW_NTB = 4;                    // n-tiles of one workgroup
constexpr int NNW_CHUNK_KS = 8;               // k-steps of one staged chunk, at most

inline int nnw_slot(int net) { return net == 8 ? 0 : (net == 17 ? 1 : -1); }        // TQ_NET_NN8 / TQ_NET_NN17 -> slot
// slot s, layer l = 1..nnw_layers(s)
TQ_HD int nnw_layers(int s) { return NNW_LAYERS[s]; }
TQ_HD int nnw_cin(int s, int l) { return NNW_CH[s][l - 1]; }
TQ_HD int nnw_cout(int s, int l) { return NNW_CH[s][l]; }
TQ_HD int nnw_mode(int s, int l) { return l == 1 ? NN11_CIRCULAR : (l == NNW_LAYERS[s] ? NN11_VALID : NN11_ZERO); }

// ---- one layer by its channel counts
TQ_HD bool nnw_reads_stack(int cin) { return cin == 2; }
TQ_HD int nnw_taps(int cin) { return nnw_reads_stack(cin) ? 1 : 9; }                   // taps of the weight image
TQ_HD int nnw_kdim(int cin) { return nnw_reads_stack(cin) ? 18 : cin; }                // k values per image tap
TQ_HD int nnw_ksteps(int cin) { return nnw_reads_stack(cin) ? 2 : nn11_cpad(cin) / 16; }
TQ_HD int nnw_ntiles(int cout) { return nn11_cpad(cout) / 32; }
TQ_HD int64_t nnw_wimg_elems(int cin, int cout) { return (int64_t)nnw_taps(cin) * nnw_ksteps(cin) * nnw_ntiles(cout) * 512; }
// the value (before rounding) of image element idx from the torch weight [cout][cin][3][3]; 0 in the padding
TQ_HD float nnw_wimg_value(int cin, int cout, int64_t idx, const float* w) {
    const NN11WCoord c = nn11_wimg_coord(idx, nnw_ksteps(cin), nnw_ntiles(cout));
    if (c.cout >= cout || c.k >= nnw_kdim(cin)) return 0.f;
    if (nnw_reads_stack(cin)) return w[(int64_t)c.cout * 18 + c.k];     // [cout][cin][ky][kx] with k = nn11_k1(cin, tap)
    return w[((int64_t)c.cout * cin + c.k) * 9 + c.tap];
}
// equal chunks of at most NNW_CHUNK_KS k-steps
TQ_HD int nnw_chunks(int ksteps) { return (ksteps + NNW_CHUNK_KS - 1) / NNW_CHUNK_KS; }

// ---- where a layer lies in the handle's one weight image and one padded bias array (l = layers + 1: their sizes)
TQ_HD int64_t nnw_wimg_offset(int s, int l) {
    int64_t o = 0;
    for (int i = 1; i < l; ++i) o += nnw_wimg_elems(nnw_cin(s, i), nnw_cout(s, i));
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
    const int64_t n = nnw_wimg_elems(cin, cout);
    for (int64_t i = 0; i < n; ++i) wimg[i] = nn11_bf16(nnw_wimg_value(cin, cout, i, w));
    const int cp = nn11_cpad(cout);
    for (int c = 0; c < cp; ++c) bias[c] = c < cout ? b[c] : 0.f;
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
        const int64_t n = nnw_wimg_elems(cin, cout);
        uint16_t* img = wimg + nnw_wimg_offset(s, l);
        for (int64_t e = i; e < n; e += stride) img[e] = nn11_bf16(nnw_wimg_value(cin, cout, e, p.w[l - 1]));
        if (i < nn11_cpad(cout)) bias[nnw_bias_offset(s, l) + i] = i < cout ? p.b[l - 1][i] : 0.f;
    } else {
        const int64_t n = nnw_lin_elems(d);
        for (int64_t e = i; e < n; e += stride) limg[e] = nnw_lin_value(e, nn11_out_pixels(d), p.w[L]);
        if (i < NN11_OUT) lbias[i] = p.b[L][i];
    }
}

// The n-tiles n0 .. n0 + NTB - 1 of one conv3x3 + bias + ReLU layer for the workgroup's G perspectives; `lds`: the
// kernel's tile.  See k_nnw_conv.
template <int D, int KS, int NT, int MODE, int NTB>
__device__ __forceinline__ void nnw_conv_tiles(unsigned char* lds, int n0, const void* __restrict__ in, int dtype,
                                               const uint16_t* __restrict__ wimg, const float* __restrict__ bias,
                                               uint16_t* __restrict__ out, int64_t P) {
    using Ge = NN11Geom<D>;
    constexpr int PIX = Ge::PIX, G = Ge::G, MW = Ge::MW, NW = Ge::NW, THREADS = Ge::THREADS;
    constexpr int NPIX_OUT = MODE == NN11_VALID ? Ge::OPIX : PIX;
    constexpr int OD = MODE == NN11_VALID ? D - 2 : D;                      // side of the output grid
    constexpr int ROWS_OUT = G * NPIX_OUT;
    constexpr int CINP = KS * 16, COUTP = NT * 32;
    constexpr int NCHUNK = (KS + NNW_CHUNK_KS - 1) / NNW_CHUNK_KS, CK = KS / NCHUNK;     // k-steps of one chunk
    static_assert(CK * NCHUNK == KS && CK <= NNW_CHUNK_KS, "the k-steps of a layer are cut into equal chunks");
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
        py[i] = q / OD; px[i] = q % OD;
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

    if constexpr (MODE == NN11_CIRCULAR) {
        // the stack as bf16, exactly as k_nn11_conv stages it
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
                    if (k < 18 && pbase[i] >= 0)
                        v = s[2 * pbase[i] + (k / 9) * PIX + nn11_src_pixel(NN11_CIRCULAR, D, py[i], px[i], k % 9)];
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
            for (int tap = 0; tap < 9; ++tap) {
                int arow[MW];                                               // LDS byte address of the lane's source row
#pragma unroll
                for (int i = 0; i < MW; ++i) {
                    const int sp = pbase[i] >= 0 ? nn11_src_pixel(MODE, D, py[i], px[i], tap) : -1;
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
        uint16_t* o = out + (persp0 * NPIX_OUT + row) * COUTP;
#pragma unroll
        for (int n = 0; n < NTB; ++n)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int c0 = 32 * (n0 + n) + 8 * g + 4 * h;
                const float4 b = *reinterpret_cast<const float4*>(bias + c0);
                const float v0 = fmaxf(acc[i][n][4 * g + 0] + b.x, 0.f), v1 = fmaxf(acc[i][n][4 * g + 1] + b.y, 0.f);
                const float v2 = fmaxf(acc[i][n][4 * g + 2] + b.z, 0.f), v3 = fmaxf(acc[i][n][4 * g + 3] + b.w, 0.f);
                uint2 pk;
                pk.x = (uint32_t)nn11_bf16(v0) | ((uint32_t)nn11_bf16(v1) << 16);
                pk.y = (uint32_t)nn11_bf16(v2) | ((uint32_t)nn11_bf16(v3) << 16);
                *reinterpret_cast<uint2*>(o + c0) = pk;
            }
    }
}

// One conv3x3 + bias + ReLU layer of a wide net.  KS: k-steps of 16 input channels per tap (the stack layer: 2 steps over
// its 18 k values), NT: tiles of 32 output channels, MODE: where a tap's source pixel lies.  `in`: the previous layer's
// activation image [P][d^2][16 KS] (MODE != CIRCULAR) or the perspective stack [P][2][d][d] of element type `dtype`;
// `out`: this layer's image [P][pixels][32 NT] ((d-2)^2 pixels for NN11_VALID); `bias`: its padded f32 bias.
// Grid: (ceil(P / G), ceil(NT / NNW_NTB)) workgroups of NN11Geom<D>::THREADS threads: workgroup (x, y) computes the
// n-tiles 4 y .. of the perspectives G x ..
template <int D, int KS, int NT, int MODE>
__global__ __launch_bounds__(NN11Geom<D>::THREADS) void k_nnw_conv(const void* __restrict__ in, int dtype, const uint16_t* __restrict__ wimg,
                                                  const float* __restrict__ bias, uint16_t* __restrict__ out, int64_t P) {
    using Ge = NN11Geom<D>;
    constexpr int NCHUNK = (KS + NNW_CHUNK_KS - 1) / NNW_CHUNK_KS, CK = KS / NCHUNK;
    constexpr int LDS_BYTES = MODE == NN11_CIRCULAR ? ((Ge::G * 2 * Ge::PIX * 2 + 15) & ~15) : Ge::LROWS * (CK * 32 + 16);
    __shared__ __attribute__((aligned(16))) unsigned char lds[LDS_BYTES];
    constexpr int REM = NT % NNW_NTB;                                       // n-tiles of the last block row, if fewer
    const int n0 = (int)blockIdx.y * NNW_NTB;
    if constexpr (REM != 0) {
        if (n0 + NNW_NTB > NT) {                                            // uniform over the workgroup
            nnw_conv_tiles<D, KS, NT, MODE, REM>(lds, n0, in, dtype, wimg, bias, out, P);
            return;
        }
    }
    nnw_conv_tiles<D, KS, NT, MODE, NNW_NTB>(lds, n0, in, dtype, wimg, bias, out, P);
}

// The linear layer, the 224-channel counterpart of k_nn11_linear: one wavefront per perspective over the last conv's
// image [P][npix][224]; f32 sums in a fixed order (lane-strided partial sums, then a butterfly over the 64 lanes),
// + bias, f32 out.
__global__ __launch_bounds__(256) void k_nnw_linear(const uint16_t* __restrict__ act, const float* __restrict__ limg,
                                                    const float* __restrict__ lbias, float* __restrict__ q, int64_t P, int npix) {
    const int lane = threadIdx.x & 63;
    const int64_t p = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (p >= P) return;
    const int chunks = npix * (NNW_FEAT_CP / 8);                            // 16-byte chunks of 8 features
    const uint4* a = reinterpret_cast<const uint4*>(act + p * npix * NNW_FEAT_CP);
    float s[NN11_OUT] = {0.f, 0.f, 0.f};
    for (int c = lane; c < chunks; c += 64) {
        const uint4 v = a[c];
        const uint32_t wd[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const float x = nn11_f32((uint16_t)(wd[j >> 1] >> (16 * (j & 1))));
#pragma unroll
            for (int o = 0; o < NN11_OUT; ++o) s[o] += x * limg[((int64_t)o * npix * NNW_FEAT_CP) + c * 8 + j];
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
