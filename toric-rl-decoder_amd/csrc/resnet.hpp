// Forward pass of the reference's default Q-network, ResNet18 (src/nn/torch/ResNet.py, BasicBlock nets), and of
// ResNet34, which has the same layer shapes and other block counts: eval-mode BatchNorm only.  Implicit-GEMM
// convolutions on v_mfma_f32_32x32x16_bf16 with NN_11's images, fragment order and tile geometry (nn11.hpp) over the
// shared tile body (conv_tile.hpp), cut like the wide nets' (nnw.hpp): at most CONV_NTB = 4 n-tiles per workgroup across
// blockIdx.y.  This family's own:
//   - the epilogue (ResNetScaleShift): BatchNorm folded at load into two f32 vectors per convolution, scale
//     s = gamma / sqrt(var + eps) and shift t = beta - mean s; z = acc s + t, [z = z + r,] [ReLU,] one rounding to bf16;
//   - the shape policy (ResNetShape): 1x1 convolutions (the shortcuts), which read the centre pixel, and stride 2 onto
//     the half grid of side s = (d + 1) / 2: the 3x3 reads (2y + ky - 1, 2x + kx - 1), zero outside, the 1x1 reads
//     (2y, 2x); the side of the input grid is the template parameter, even sides included (the half grid of d = 3, 7,
//     11, ...); the stack-reading first layer is zero padded;
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

// ---- one convolution by its channel counts and taps: one-line calls into nn11.hpp's conv_* functions, as NN_11's
// by-layer functions are.  The names stay because the host shim (tests/host_resnet_shim.cpp) uses them.
TQ_HD bool resnet_reads_stack(int cin) { return conv_reads_stack(cin); }
TQ_HD int resnet_img_taps(int cin, int taps) { return conv_img_taps(cin, taps); }
TQ_HD int resnet_ksteps(int cin) { return conv_ksteps(cin); }
TQ_HD int resnet_ntiles(int cout) { return conv_ntiles(cout); }
TQ_HD int resnet_chunks(int ksteps) { return conv_chunks(ksteps); }
TQ_HD int64_t resnet_wimg_elems(int cin, int cout, int taps) { return conv_wimg_elems(cin, cout, taps); }

// ---- where convolution i lies in the handle's one weight image and in its scale and shift arrays (i = convs: their sizes)
TQ_HD int64_t resnet_wimg_offset(int s, int i) {
    int64_t o = 0;
    for (int j = 0; j < i; ++j) { const ResConv c = resnet_conv(s, j); o += conv_wimg_elems(c.cin, c.cout, c.taps); }
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
    conv_pack_image_host(cin, cout, taps, w, wimg);
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
        const int64_t elems = conv_wimg_elems(c.cin, c.cout, c.taps);
        uint16_t* img = wimg + resnet_wimg_offset(s, i);
        for (int64_t e = t; e < elems; e += stride) img[e] = nn11_bf16(conv_wimg_value(c.cin, c.cout, c.taps, e, p.w[i]));
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

// The ResNets' shape policy (conv_tile.hpp): TAPS_ taps (9, or 1 for a 1x1) at stride STRIDE on the S x S grid; the
// stack layer is zero padded.
template <int S, int TAPS_, int STRIDE, bool STACK_>
struct ResNetShape {
    static_assert(!STACK_ || STRIDE == 1, "the stack layer has stride 1");
    static constexpr int SIDE = S, OSIDE = STRIDE == 2 ? (S + 1) / 2 : S;
    static constexpr int NPIX_IN = S * S, NPIX_OUT = OSIDE * OSIDE;
    static constexpr int TAPS = TAPS_, STACK = STACK_ ? CONV_STACK_ZERO : CONV_NO_STACK;
    TQ_HD static int src(int y, int x, int tap) { return resnet_src_pixel(S, STRIDE, TAPS_, y, x, tap); }
};

// The ResNets' epilogue: z = acc s + t, [z = z + r,] [ReLU]; `epi` is the same for every workgroup of a launch.
struct ResNetScaleShift {
    const float* scale; const float* shift; int epi; const uint16_t* res;
    __device__ __forceinline__ float4 operator()(const float4& a, int c0, int64_t at) const {
        const float4 sc = *reinterpret_cast<const float4*>(scale + c0);
        const float4 sh = *reinterpret_cast<const float4*>(shift + c0);
        float4 v = make_float4(a.x * sc.x + sh.x, a.y * sc.y + sh.y, a.z * sc.z + sh.z, a.w * sc.w + sh.w);
        if (epi == RESNET_EPI_ADD_RELU) {                                   // uniform over the workgroup
            const uint2 rr = *reinterpret_cast<const uint2*>(res + at);
            v.x += nn11_f32((uint16_t)rr.x); v.y += nn11_f32((uint16_t)(rr.x >> 16));
            v.z += nn11_f32((uint16_t)rr.y); v.w += nn11_f32((uint16_t)(rr.y >> 16));
        }
        if (epi != RESNET_EPI_NONE) { v.x = nn11_relu(v.x); v.y = nn11_relu(v.y); v.z = nn11_relu(v.z); v.w = nn11_relu(v.w); }
        return v;
    }
};

// One convolution with its folded BatchNorm.  S: side of the INPUT grid (odd 3..21, or a half side 2..11); KS: k-steps of
// 16 input channels per tap (the stack layer: 2 steps over its 18 k values); NT: tiles of 32 output channels; TAPS: 9, or
// 1 for a 1x1, which reads the centre pixel; STRIDE 2 writes the half grid of side (S + 1) / 2: the workgroup stages the G
// input perspectives of NN11Geom<S> and computes their G ((S + 1) / 2)^2 output rows; STACK: `in` is the perspective
// stack [P][2][S][S] of element type `dtype`, zero padded, else the activation image [P][S^2][16 KS].
// `scale` / `shift`: the convolution's padded f32 vectors.  `epi` (the same for every workgroup of a launch):
// RESNET_EPI_NONE out = bf16(acc s + t); RESNET_EPI_RELU out = bf16(relu(acc s + t)); RESNET_EPI_ADD_RELU
// out = bf16(relu((acc s + t) + res)) with `res` a bf16 image of out's shape.  `out`: [P][output pixels][32 NT].
// Grid: (ceil(P / G), ceil(NT / CONV_NTB)) workgroups of NN11Geom<S>::THREADS threads.
template <int S, int KS, int NT, int TAPS, int STRIDE, bool STACK>
__global__ __launch_bounds__(NN11Geom<S>::THREADS) void k_resnet_conv(const void* __restrict__ in, int dtype, const uint16_t* __restrict__ wimg,
                                                     const float* __restrict__ scale, const float* __restrict__ shift, int epi,
                                                     const uint16_t* __restrict__ res, uint16_t* __restrict__ out, int64_t P) {
    using Shape = ResNetShape<S, TAPS, STRIDE, STACK>;
    __shared__ __attribute__((aligned(16))) unsigned char lds[conv_lds_bytes<Shape, KS>()];
    const ResNetScaleShift e = {scale, shift, epi, res};
    constexpr int REM = NT % CONV_NTB;                                      // n-tiles of the last block row, if fewer
    const int n0 = (int)blockIdx.y * CONV_NTB;
    if constexpr (NT < CONV_NTB) {                                          // 64 output channels: one block row of two
        conv_tiles<Shape, KS, NT, NT>(lds, n0, in, dtype, wimg, out, P, e);
    } else {
        if constexpr (REM != 0) {
            if (n0 + CONV_NTB > NT) {                                       // uniform over the workgroup
                conv_tiles<Shape, KS, NT, REM>(lds, n0, in, dtype, wimg, out, P, e);
                return;
            }
        }
        conv_tiles<Shape, KS, NT, CONV_NTB>(lds, n0, in, dtype, wimg, out, P, e);
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
