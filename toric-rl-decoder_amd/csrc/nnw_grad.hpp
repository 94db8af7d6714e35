// The learner's step through the wide nets NN_8 and NN_17 (src/Learner_mp.py:140-169): NN_11's (nn11_grad.hpp; numerics
// contract in include/toricenv.h) restated for a plain conv net given by slot s.  What is shared
// as it is: the head (nn11_head, k_nn11_head, k_nn11_dblin), the last layer's gradient and the linear layer's three
// kernels over the feature pitch 224, the sum over partial images (k_nn11_wreduce over a bias pitch of 256).  What is here:
//   - the dgrad image of one layer by its channel counts, one index function under the host pack and the pack kernel; the
//     dgrad itself is k_nnw_conv<..., NN11DgradMask> (nnw.hpp) over that image;
//   - k_nnw_wgrad<NT, WAVES>: k_nn11_wgrad's scheme -- one GEMM per tap, both operands staged 64 rows at a time through LDS
//     transposed -- widened to 224 / 256 output channels;
//   - k_nnw_wgrad1: conv1's wgrad (18 k values) for 256 output channels.
// How a sum is cut depends on (net, layer, d, n) alone; no atomics.
#pragma once
#include "nn11_grad.hpp"
#include "nnw.hpp"

namespace tq {

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
// first element of layer l = 2..layers of slot s in the handle's one dgrad image (l = layers + 1: its size)
TQ_HD int64_t nnw_dimg_offset(int s, int l) {
    int64_t o = 0;
    for (int i = 2; i < l; ++i) o += conv_dimg_elems(nnw_cin(s, i), nnw_cout(s, i));
    return o;
}

// ---- how the wgrad's sum over records is cut: a function of d alone.  About 2048 rows to a workgroup, twice NN_11's:
// a partial image is up to 9 x 256 x 256 f32 = 2.25 MiB, four times NN_11's, and one is kept per chunk.
// At max_batch = 4096 and d = 21 that is 4 records to a chunk, 1024 chunks, 2.25 GiB of partial images.
TQ_HD int nnw_wgrad_persp(int d) { const int p = 2048 / (d * d); return p < 2 ? 2 : p; }
TQ_HD int64_t nnw_wgrad_chunks(int d, int64_t n) { const int p = nnw_wgrad_persp(d); return (n + p - 1) / p; }
constexpr int64_t NNW_WPART_ELEMS = (int64_t)9 * NNW_MAX_CP * NNW_MAX_CP;          // f32 per partial image, at most
constexpr int NNW_WG_WAVES = 8;                 // wavefronts of a wgrad workgroup: one per tile of 32 output channels
// layer l's output grid: (d-2)^2 pixels for the last conv, d^2 otherwise
TQ_HD int nnw_layer_pixels(int s, int l, int d) { return l == nnw_layers(s) ? nn11_out_pixels(d) : d * d; }

#if defined(__HIPCC__)
// one block row (blockIdx.y) per layer l = y + 2 of slot s
__global__ __launch_bounds__(256) void k_nnw_pack_dgrad(NNWPack p, int s, uint16_t* dimg) {
    const int l = (int)blockIdx.y + 2, cin = nnw_cin(s, l), cout = nnw_cout(s, l);
    const int64_t stride = (int64_t)gridDim.x * blockDim.x, n = conv_dimg_elems(cin, cout);
    uint16_t* img = dimg + nnw_dimg_offset(s, l);
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += stride)
        img[e] = nn11_bf16(conv_dimg_value(cin, cout, e, p.w[l - 1]));
}

// conv1's wgrad (K operand 18 wide): plain f32 FMAs, as k_nn11_wgrad1 for 256 output channels.  Workgroup = one chunk of
// records, 512 threads; thread = (output channel, input channel) with its nine taps; the stack is read with the circular
// wrap.  g: G_1 [P][d^2][256].  Partial image [chunk][256][18], and the chunk's bias partial [chunk][256].
__global__ __launch_bounds__(512) void k_nnw_wgrad1(const uint16_t* __restrict__ g, const void* __restrict__ stack, int dtype,
                                                    float* __restrict__ wpart, float* __restrict__ bpart, int64_t P, int d) {
    const int pix = d * d, pw = nnw_wgrad_persp(d);
    const int co = threadIdx.x & (NNW_MAX_CP - 1), ci = threadIdx.x >> 8;
    const int64_t persp0 = (int64_t)blockIdx.x * pw;
    const int np = (int)(P - persp0 < pw ? P - persp0 : pw);
    float acc[9], bs = 0.f;
#pragma unroll
    for (int t = 0; t < 9; ++t) acc[t] = 0.f;
    for (int p = 0; p < np; ++p)
        for (int o = 0; o < pix; ++o) {
            const float gv = nn11_f32(g[((persp0 + p) * pix + o) * NNW_MAX_CP + co]);
            bs += gv;
#pragma unroll
            for (int t = 0; t < 9; ++t) {
                const int sp = nn11_src_pixel(NN11_CIRCULAR, d, o / d, o % d, t);
                acc[t] += gv * nn11_f32(nn11_stack_bf16(stack, dtype, ((persp0 + p) * 2 + ci) * pix + sp));
            }
        }
#pragma unroll
    for (int t = 0; t < 9; ++t) wpart[((int64_t)blockIdx.x * NNW_MAX_CP + co) * 18 + nn11_k1(ci, t)] = acc[t];
    if (ci == 0) bpart[(int64_t)blockIdx.x * NNW_MAX_CP + co] = bs;
}

// wgrad of layer l >= 2.  g: G_l [P][npo][32 mt]; a: A_{l-1} [P][d^2][32 NT]; mode: the layer's forward mode (where a
// tap's source pixel lies); mt = 7 or 8 tiles of output channels.  Grid (chunks, 9 taps, ceil(mt / WAVES)), 64 WAVES
// threads: workgroup z takes the output tiles WAVES z .., wavefront w of it owns output channels 32 (WAVES z + w) .. and
// all NT tiles of input channels (NT x 16 accumulator registers).  wpart [chunk][tap][32 mt][32 NT], bpart [chunk][256]
// (written by tap 0's workgroups; 0 beyond 32 mt).
// The library holds WAVES = NNW_WG_WAVES = 8, one workgroup over all output channels: 196 / 168 VGPRs (NT = 8 / 7), 72 /
// 67.5 KiB of LDS, no scratch, and A_{l-1} staged once.  WAVES = 4, two block rows over halves of the output channels,
// compiles to 185 / 168 VGPRs and 54 / 49.5 KiB and stages A_{l-1} twice (profiles/nnw_grad_resource_usage.txt).
template <int NT, int WAVES>
__global__ __launch_bounds__(WAVES * 64) void k_nnw_wgrad(const uint16_t* __restrict__ g, const uint16_t* __restrict__ a, float* __restrict__ wpart,
                                                          float* __restrict__ bpart, int64_t P, int d, int mode, int mt) {
    constexpr int PT = NN11_WG_PITCH, KR = NN11_WG_ROWS, THREADS = WAVES * 64;
    static_assert(WAVES * 32 <= NNW_MAX_CP && NT * 32 <= NNW_MAX_CP, "a workgroup's tiles lie inside the widest image");
    __shared__ __attribute__((aligned(16))) unsigned char gt[WAVES * 32 * PT];
    __shared__ __attribute__((aligned(16))) unsigned char at[NT * 32 * PT];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 31, h = lane >> 5;
    const int tap = (int)blockIdx.y, pix = d * d, od = mode == NN11_VALID ? d - 2 : d, npo = od * od;
    const int tile0 = (int)blockIdx.z * WAVES, mtb = mt - tile0 < WAVES ? mt - tile0 : WAVES;      // this workgroup's output tiles
    const int cpo = 32 * mt, cob = 32 * mtb, cpi = 32 * NT, pw = nnw_wgrad_persp(d);
    const int64_t persp0 = (int64_t)blockIdx.x * pw;
    const int np = (int)(P - persp0 < pw ? P - persp0 : pw);
    const int rows = np * npo;
    const uint16_t* g0 = g + persp0 * npo * cpo + 32 * tile0;
    const uint16_t* a0 = a + persp0 * pix * cpi;

    nn11_f32x16 acc[NT];
#pragma unroll
    for (int n = 0; n < NT; ++n)
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[n][e] = 0.f;
    float bs = 0.f;

    for (int r0 = 0; r0 < rows; r0 += KR) {
        __syncthreads();                                                    // the previous stage has been read
        // stage, transposed: an item is two neighbouring rows x 8 channels, stored as 8 words (row pair of one channel)
        for (int it = tid; it < 32 * (cob / 8); it += THREADS) {
            const int rp = it & 31, ch = it >> 5, row = r0 + 2 * rp;
            uint4 v0 = make_uint4(0, 0, 0, 0), v1 = v0;
            if (row < rows) v0 = *reinterpret_cast<const uint4*>(g0 + (int64_t)row * cpo + ch * 8);
            if (row + 1 < rows) v1 = *reinterpret_cast<const uint4*>(g0 + (int64_t)(row + 1) * cpo + ch * 8);
            const uint32_t x0[4] = {v0.x, v0.y, v0.z, v0.w}, x1[4] = {v1.x, v1.y, v1.z, v1.w};
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const uint32_t lo = (x0[j >> 1] >> (16 * (j & 1))) & 0xffffu, hi = (x1[j >> 1] >> (16 * (j & 1))) & 0xffffu;
                *reinterpret_cast<uint32_t*>(gt + (ch * 8 + j) * PT + rp * 4) = lo | (hi << 16);
            }
        }
        for (int it = tid; it < 32 * (cpi / 8); it += THREADS) {
            const int rp = it & 31, ch = it >> 5;
            uint4 v[2];
#pragma unroll
            for (int e = 0; e < 2; ++e) {
                const int row = r0 + 2 * rp + e;
                v[e] = make_uint4(0, 0, 0, 0);
                if (row < rows) {
                    const int p = row / npo, o = row % npo;
                    const int sp = nn11_src_pixel(mode, d, o / od, o % od, tap);
                    if (sp >= 0) v[e] = *reinterpret_cast<const uint4*>(a0 + ((int64_t)p * pix + sp) * cpi + ch * 8);
                }
            }
            const uint32_t x0[4] = {v[0].x, v[0].y, v[0].z, v[0].w}, x1[4] = {v[1].x, v[1].y, v[1].z, v[1].w};
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const uint32_t lo = (x0[j >> 1] >> (16 * (j & 1))) & 0xffffu, hi = (x1[j >> 1] >> (16 * (j & 1))) & 0xffffu;
                *reinterpret_cast<uint32_t*>(at + (ch * 8 + j) * PT + rp * 4) = lo | (hi << 16);
            }
        }
        __syncthreads();
        if (wave < mtb) {                                                   // wave-uniform
#pragma unroll
            for (int ks = 0; ks < KR / 16; ++ks) {
                const uint4 fa = *reinterpret_cast<const uint4*>(gt + (32 * wave + r) * PT + ks * 32 + h * 16);
#pragma unroll
                for (int n = 0; n < NT; ++n) {
                    const uint4 fb = *reinterpret_cast<const uint4*>(at + (32 * n + r) * PT + ks * 32 + h * 16);
                    acc[n] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(nn11_bf16x8, fa),
                                                                     __builtin_bit_cast(nn11_bf16x8, fb), acc[n], 0, 0, 0);
                }
            }
        }
        if (tap == 0 && tid < cob) {                                        // the bias gradient: the channel's rows in order
            const uint16_t* line = reinterpret_cast<const uint16_t*>(gt + tid * PT);
            for (int k = 0; k < KR; ++k) bs += nn11_f32(line[k]);
        }
    }

    // accumulator register 4 q + e of lane (r, h) = (co = 32 (tile0 + wave) + 8 q + 4 h + e, ci = 32 n + r)
    if (wave < mtb) {
        float* o = wpart + (((int64_t)blockIdx.x * 9 + tap) * cpo + 32 * (tile0 + wave)) * cpi;
#pragma unroll
        for (int n = 0; n < NT; ++n)
#pragma unroll
            for (int q = 0; q < 4; ++q)
#pragma unroll
                for (int e = 0; e < 4; ++e) o[(int64_t)(8 * q + 4 * h + e) * cpi + 32 * n + r] = acc[n][4 * q + e];
    }
    if (tap == 0 && tid < 32 * WAVES && 32 * tile0 + tid < NNW_MAX_CP)
        bpart[(int64_t)blockIdx.x * NNW_MAX_CP + 32 * tile0 + tid] = tid < cob ? bs : 0.f;
}
#endif  // __HIPCC__

}  // namespace tq
