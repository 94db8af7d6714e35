// The learner's step through NN_11 (src/Learner_mp.py:140-169): the loss head, the gradient of conv11's output, the
// weight-gradient kernels and the sums over their partial images.  The forward and the dgrad convolutions are
// k_nn11_conv (nn11.hpp); the numerics contract is in include/toricenv.h and DESIGN.md 3.7.
//
// wgrad of layer l = 2..11 is one GEMM per tap: dW[co][ci] = sum over rows (record, output pixel) of G_l[row][co] *
// A_{l-1}[source pixel of the row under the tap][ci], M = co, N = ci, K = rows, on v_mfma_f32_32x32x16_bf16.  Both
// operands lie channels-last in memory and the MFMA wants 8 consecutive k per lane, so a workgroup stages 64 rows at
// a time through LDS TRANSPOSED ([channel][row], the A operand already shifted by the tap) and reads 16-byte fragments
// from there.  A workgroup takes nn11_wgrad_persp(d) records and one tap and writes an f32 partial image; k_nn11_wreduce
// sums the partial images in index order and writes torch's layout.  How a sum is cut depends on (d, n) alone.
//
// The wgrad kernels (k_conv_wgrad, k_conv_wgrad1) and the dgrad pack's body (conv_pack_dgrad) are written by channel
// counts, wave count and rows per chunk: the wide nets' learner step (nnw_grad.hpp) runs the same ones.
#pragma once
#include "nn11.hpp"

namespace tq {

constexpr int NN11_WG_ROWS = 64;                          // rows (the GEMM's K) per LDS stage
constexpr int NN11_WG_PITCH = NN11_WG_ROWS * 2 + 16;      // bytes of one channel's line: 16-byte reads stay aligned
constexpr int NN11_LIN_SLICE = 64;                        // records per partial sum of the linear layer's weight gradient
constexpr int NN11_ERR_ACTION = 1;                        // the latch: an actions_idx outside 0..2 was seen

// records per wgrad workgroup (a chunk): about chunk_rows rows of the GEMM, 1024 for NN_11
TQ_HD int conv_wgrad_persp(int chunk_rows, int d) { const int p = chunk_rows / (d * d); return p < 2 ? 2 : p; }
constexpr int NN11_WG_WAVES = 4;                          // wavefronts of a wgrad workgroup: one per tile of 32 output channels
constexpr int NN11_WG_CHUNK_ROWS = 1024;
TQ_HD int nn11_wgrad_persp(int d) { return conv_wgrad_persp(NN11_WG_CHUNK_ROWS, d); }
TQ_HD int64_t nn11_wgrad_chunks(int d, int64_t n) { const int p = nn11_wgrad_persp(d); return (n + p - 1) / p; }
constexpr int64_t NN11_WPART_ELEMS = (int64_t)9 * NN11_MAX_CP * NN11_MAX_CP;      // f32 per partial image, at most
// layer l's output grid: (d-2)^2 pixels for conv11, d^2 otherwise
TQ_HD int nn11_layer_pixels(int l, int d) { return l == NN11_LAYERS ? nn11_out_pixels(d) : d * d; }

// ---- the head, as the contract writes it: every operation rounded once, left to right (the build does not contract)
struct NN11Head { float loss, dq; };
TQ_HD NN11Head nn11_head(float q, float y, float w, int n) {
    const float e = y - q;
    NN11Head r;
    r.loss = w * (e * e);
    r.dq = (((q - y) * w) * 2.f) / (float)n;
    return r;
}

#if defined(__HIPCC__)
// the dgrad image `img` of one layer from its torch weight `w`: what one block row of a pack kernel does
__device__ __forceinline__ void conv_pack_dgrad(int cin, int cout, const float* w, uint16_t* img) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x, n = conv_dimg_elems(cin, cout);
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += stride) img[e] = nn11_bf16(conv_dimg_value(cin, cout, e, w));
}
// one block row (blockIdx.y) per layer l = y + 2
__global__ __launch_bounds__(256) void k_nn11_pack_dgrad(NN11Pack p, uint16_t* dimg) {
    const int l = (int)blockIdx.y + 2;
    conv_pack_dgrad(nn11_cin(l), nn11_cout(l), p.w[l - 1], dimg + nn11_dimg_offset(l));
}

// one thread per record
__global__ __launch_bounds__(256) void k_nn11_head(const float* __restrict__ q, const int64_t* __restrict__ actions,
                                                   const float* __restrict__ y, const float* __restrict__ w, int n,
                                                   float* __restrict__ loss, float* __restrict__ dq, int* __restrict__ latch) {
    const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (i >= n) return;
    const int64_t a = actions[i];
    float l = 0.f, g[NN11_OUT] = {0.f, 0.f, 0.f};
    if (a < 0 || a >= NN11_OUT) atomicOr(latch, NN11_ERR_ACTION);         // a flag, not a sum: no value depends on it
    else {
        const NN11Head h = nn11_head(q[i * NN11_OUT + a], y[i], w ? w[i] : 1.f, n);
        l = h.loss;
        g[a] = h.dq;
    }
    loss[i] = l;
    for (int o = 0; o < NN11_OUT; ++o) dq[i * NN11_OUT + o] = g[o];
}

// dblin[a] = sum_i dq[i][a]: thread t sums records t, t + 256, ...; the 256 sums are added in thread order
__global__ __launch_bounds__(256) void k_nn11_dblin(const float* __restrict__ dq, int n, float* __restrict__ dblin) {
    __shared__ float s[NN11_OUT][256];
    float v[NN11_OUT] = {0.f, 0.f, 0.f};
    for (int i = threadIdx.x; i < n; i += 256)
        for (int o = 0; o < NN11_OUT; ++o) v[o] += dq[i * NN11_OUT + o];
    for (int o = 0; o < NN11_OUT; ++o) s[o][threadIdx.x] = v[o];
    __syncthreads();
    if (threadIdx.x < NN11_OUT) {
        float t = 0.f;
        for (int i = 0; i < 256; ++i) t += s[threadIdx.x][i];
        dblin[threadIdx.x] = t;
    }
}

// The last conv layer's gradient and the linear layer's, over the feature pitch FEAT_CP of that layer's image: 64 for
// NN_11 (l = 11), 224 with FEAT = 200 real channels for the wide nets (nnw_grad.hpp).
// G_11 = bf16(mask_11 * sum_a dq[.][a] Wlin_bf16[a][.]), one thread per element of conv11's image [n][npix][FEAT_CP]
template <int FEAT_CP>
__global__ __launch_bounds__(256) void k_nn11_g11(const float* __restrict__ dq, const float* __restrict__ limg,
                                                  const uint16_t* __restrict__ a11, uint16_t* __restrict__ g11, int64_t n, int npix) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, F = (int64_t)npix * FEAT_CP;
    if (e >= n * F) return;
    const int64_t i = e / F, f = e % F;
    float s = 0.f;
    for (int o = 0; o < NN11_OUT; ++o) s += dq[i * NN11_OUT + o] * limg[o * F + f];
    g11[e] = nn11_mask(a11[e]) ? nn11_bf16(s) : (uint16_t)0;
}

// dWlin partial sums: blockIdx.y = slice of NN11_LIN_SLICE records, one thread per feature f = pixel * FEAT_CP + channel
template <int FEAT_CP>
__global__ __launch_bounds__(256) void k_nn11_lin_part(const float* __restrict__ dq, const uint16_t* __restrict__ a11,
                                                       float* __restrict__ lpart, int n, int npix) {
    const int F = npix * FEAT_CP, f = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (f >= F) return;
    const int i0 = (int)blockIdx.y * NN11_LIN_SLICE, i1 = i0 + NN11_LIN_SLICE < n ? i0 + NN11_LIN_SLICE : n;
    float s[NN11_OUT] = {0.f, 0.f, 0.f};
    for (int i = i0; i < i1; ++i) {
        const float x = nn11_f32(a11[(int64_t)i * F + f]);
        for (int o = 0; o < NN11_OUT; ++o) s[o] += dq[i * NN11_OUT + o] * x;
    }
    for (int o = 0; o < NN11_OUT; ++o) lpart[((int64_t)blockIdx.y * NN11_OUT + o) * F + f] = s[o];
}
// ... summed over the slices in index order, written in torch's (channel, y, x) feature order over the FEAT real channels
template <int FEAT_CP, int FEAT>
__global__ __launch_bounds__(256) void k_nn11_lin_reduce(const float* __restrict__ lpart, int slices, int npix, float* __restrict__ dwlin) {
    const int F = npix * FEAT_CP, e = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (e >= NN11_OUT * F) return;
    const int o = e / F, f = e % F;
    constexpr bool POW2 = (FEAT_CP & (FEAT_CP - 1)) == 0;                   // NN_11's 64: a mask and a shift, as before
    const int c = POW2 ? (f & (FEAT_CP - 1)) : f % FEAT_CP, pixel = POW2 ? (f >> __builtin_ctz(FEAT_CP)) : f / FEAT_CP;
    if (FEAT < FEAT_CP && c >= FEAT) return;
    float s = 0.f;
    for (int k = 0; k < slices; ++k) s += lpart[((int64_t)k * NN11_OUT + o) * F + f];
    dwlin[(int64_t)o * (npix * FEAT) + (int64_t)c * npix + pixel] = s;
}

// conv1's wgrad (K operand 18 wide): plain f32 FMAs.  CP: the padded output channels, 128 for NN_11 and 256 for the wide
// nets.  Workgroup = one chunk of records, 2 CP threads; thread = (output channel, input channel) with its nine taps; the
// stack is read with the circular wrap.  g: G_1 [P][d^2][CP].  Partial image [chunk][CP][18], and the chunk's bias partial
// [chunk][CP].
template <int CP, int CHUNK_ROWS>
__global__ __launch_bounds__(2 * CP) void k_conv_wgrad1(const uint16_t* __restrict__ g, const void* __restrict__ stack, int dtype,
                                                        float* __restrict__ wpart, float* __restrict__ bpart, int64_t P, int d) {
    static_assert((CP & (CP - 1)) == 0, "a thread's channels are a mask and a shift of its index");
    const int pix = d * d, pw = conv_wgrad_persp(CHUNK_ROWS, d);
    const int co = threadIdx.x & (CP - 1), ci = threadIdx.x >> __builtin_ctz(CP);
    const int64_t persp0 = (int64_t)blockIdx.x * pw;
    const int np = (int)(P - persp0 < pw ? P - persp0 : pw);
    float acc[9], bs = 0.f;
#pragma unroll
    for (int t = 0; t < 9; ++t) acc[t] = 0.f;
    for (int p = 0; p < np; ++p)
        for (int o = 0; o < pix; ++o) {
            const float gv = nn11_f32(g[((persp0 + p) * pix + o) * CP + co]);
            bs += gv;
#pragma unroll
            for (int t = 0; t < 9; ++t) {
                const int sp = nn11_src_pixel(NN11_CIRCULAR, d, o / d, o % d, t);
                acc[t] += gv * nn11_f32(nn11_stack_bf16(stack, dtype, ((persp0 + p) * 2 + ci) * pix + sp));
            }
        }
#pragma unroll
    for (int t = 0; t < 9; ++t) wpart[((int64_t)blockIdx.x * CP + co) * 18 + nn11_k1(ci, t)] = acc[t];
    if (ci == 0) bpart[(int64_t)blockIdx.x * CP + co] = bs;
}

// wgrad of a layer l >= 2.  g: G_l [P][npo][32 mt]; a: A_{l-1} [P][d^2][32 NT]; mode: the layer's forward mode (where a
// tap's source pixel lies); mt <= WAVES tiles of output channels.  Grid (chunks, 9 taps), 64 WAVES threads: wavefront
// w < mt owns output channels 32 w .. 32 w + 31 and all NT tiles of input channels (NT x 16 accumulator registers).  A chunk
// is conv_wgrad_persp(CHUNK_ROWS, d) records.  wpart [chunk][tap][32 mt][32 NT], bpart [chunk][32 WAVES] (written by tap 0's
// workgroup; 0 beyond 32 mt).
// The library holds NN_11's <3 | 4, 4, 1024> and the wide nets' <7 | 8, 8, 2048>: one workgroup over all output channels
// of the widest layer, so that A_{l-1} is staged once.  Four waves over halves of the wide nets' output channels compile
// to fewer registers and less LDS and stage A_{l-1} twice (profiles/nnw_grad_resource_usage.txt).
template <int NT, int WAVES, int CHUNK_ROWS>
__global__ __launch_bounds__(WAVES * 64) void k_conv_wgrad(const uint16_t* __restrict__ g, const uint16_t* __restrict__ a, float* __restrict__ wpart,
                                                           float* __restrict__ bpart, int64_t P, int d, int mode, int mt) {
    constexpr int PT = NN11_WG_PITCH, KR = NN11_WG_ROWS, THREADS = WAVES * 64, MAX_CP = WAVES * 32;
    static_assert(NT <= WAVES, "the input channels lie inside the widest image");
    __shared__ __attribute__((aligned(16))) unsigned char gt[MAX_CP * PT];
    __shared__ __attribute__((aligned(16))) unsigned char at[NT * 32 * PT];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 31, h = lane >> 5;
    const int tap = (int)blockIdx.y, pix = d * d, od = mode == NN11_VALID ? d - 2 : d, npo = od * od;
    const int cpo = 32 * mt, cpi = 32 * NT, pw = conv_wgrad_persp(CHUNK_ROWS, d);
    const int64_t persp0 = (int64_t)blockIdx.x * pw;
    const int np = (int)(P - persp0 < pw ? P - persp0 : pw);
    const int rows = np * npo;
    const uint16_t* g0 = g + persp0 * npo * cpo;
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
        for (int it = tid; it < 32 * (cpo / 8); it += THREADS) {
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
        if (wave < mt) {                                                    // wave-uniform
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
        if (tap == 0 && tid < cpo) {                                        // the bias gradient: the channel's rows in order
            const uint16_t* line = reinterpret_cast<const uint16_t*>(gt + tid * PT);
            for (int k = 0; k < KR; ++k) bs += nn11_f32(line[k]);
        }
    }

    // accumulator register 4 q + e of lane (r, h) = (co = 32 wave + 8 q + 4 h + e, ci = 32 n + r)
    if (wave < mt) {
        float* o = wpart + (((int64_t)blockIdx.x * 9 + tap) * cpo + 32 * wave) * cpi;
#pragma unroll
        for (int n = 0; n < NT; ++n)
#pragma unroll
            for (int q = 0; q < 4; ++q)
#pragma unroll
                for (int e = 0; e < 4; ++e) o[(int64_t)(8 * q + 4 * h + e) * cpi + 32 * n + r] = acc[n][4 * q + e];
    }
    if (tap == 0 && tid < MAX_CP) bpart[(int64_t)blockIdx.x * MAX_CP + tid] = tid < cpo ? bs : 0.f;
}

// dW (torch layout [cout][cin][taps], written) = the partial images summed in chunk order; db likewise.  wpart is
// [chunk][taps][cpo][cpi] (conv1: taps = 1, its 18 k values as cin = cpi = 18); one thread per element, tap-major so
// that neighbouring threads read neighbouring words.  BPITCH: f32 per chunk in bpart (128; the wide nets: 256).
template <int BPITCH>
__global__ __launch_bounds__(256) void k_nn11_wreduce(const float* __restrict__ wpart, const float* __restrict__ bpart, int chunks, int taps,
                                                      int cout, int cin, int cpo, int cpi, float* __restrict__ dw, float* __restrict__ db) {
    const int e = (int)(blockIdx.x * blockDim.x + threadIdx.x), nw = taps * cout * cin;
    if (e < nw) {
        const int tap = e / (cout * cin), co = e % (cout * cin) / cin, ci = e % cin;
        const int64_t img = (int64_t)taps * cpo * cpi;
        const float* p = wpart + ((int64_t)tap * cpo + co) * cpi + ci;
        float s = 0.f;
        for (int c = 0; c < chunks; ++c) s += p[c * img];
        dw[((int64_t)co * cin + ci) * taps + tap] = s;
    } else if (e < nw + cout) {
        const int co = e - nw;
        float s = 0.f;
        for (int c = 0; c < chunks; ++c) s += bpart[(int64_t)c * BPITCH + co];
        db[co] = s;
    }
}
#endif  // __HIPCC__

}  // namespace tq
