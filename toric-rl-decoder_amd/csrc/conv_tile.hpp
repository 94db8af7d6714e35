// The one implicit-GEMM tile body under k_nn11_conv, k_nnw_conv and k_resnet_conv: a workgroup's G perspectives, NTB of a
// layer's NT n-tiles, on v_mfma_f32_32x32x16_bf16 with NN_11's images, fragment order and tile geometry (nn11.hpp, which
// includes this header after the declarations it uses).  A kernel declares the LDS tile, picks its n-tiles and its
// epilogue and calls conv_tiles; what differs between the families is in two template arguments.
//
// Shape: a struct of static constexpr members and one function.
//   SIDE      side of the input grid: NN11Geom<SIDE> is the workgroup's geometry
//   OSIDE     side of the output grid
//   NPIX_IN   pixels of one perspective in `in` (SIDE^2, or (SIDE - 2)^2 for the transpose of an unpadded conv)
//   NPIX_OUT  pixels of one perspective in `out`, OSIDE^2
//   TAPS      taps of the weight image that the staged loop walks: 9, or 1 for a 1x1
//   STACK     CONV_NO_STACK: `in` is an activation image [P][NPIX_IN][16 KS]; CONV_STACK_CIRCULAR / CONV_STACK_ZERO: `in`
//             is the perspective stack [P][2][SIDE][SIDE] of element type `dtype`, read with that padding; the weight
//             image then has one "tap" whose k runs over (input channel, 3x3 tap) = 18 values in KS = 2 k-steps
//   src(y, x, tap)  the source pixel in the input grid of tap `tap` of output pixel (y, x), or -1 for the zero padding
// Epi: a functor float4 (float4 sums, int c0, int64_t at): the four values to round for output channels c0 .. c0 + 3,
// which are elements at .. at + 3 of `out`.
//
// Input channels are staged in equal chunks of at most CONV_CHUNK_KS k-steps (conv_chunks): per chunk stage, barrier,
// TAPS x k-steps, and before every chunk but the first one more barrier, because the tile is still being read.  The LDS
// tile holds the workgroup's input rows, channels last, with 16 bytes of padding per row (consecutive rows start in
// different banks: the 16-byte fragment reads of 8 neighbouring pixels are conflict-free) and one zero row; a stack
// layer stages its G x 2 x SIDE^2 stack elements as bf16 instead.  The order of a sum is (chunk, tap, k-step).
#pragma once
#if !defined(TQ_NN11_DEVICE_DECLARATIONS)
#error "conv_tile.hpp is not included on its own: include nn11.hpp, which includes it after the declarations it uses"
#endif

namespace tq {

enum { CONV_NO_STACK = 0, CONV_STACK_CIRCULAR = 1, CONV_STACK_ZERO = 2 };

template <class Shape, int KS>
constexpr int conv_lds_bytes() {
    using Ge = NN11Geom<Shape::SIDE>;
    constexpr int CK = KS / conv_chunks(KS);
    constexpr int BYTES = Shape::STACK != CONV_NO_STACK ? ((Ge::G * 2 * Ge::PIX * 2 + 15) & ~15) : Ge::LROWS * (CK * 32 + 16);
    static_assert(BYTES <= 122128, "never above the tile of NN_11's 128-channel layers at d = 21");
    return BYTES;
}

// The n-tiles n0 .. n0 + NTB - 1 of one layer for the workgroup's G perspectives; `lds`: conv_lds_bytes<Shape, KS>()
// bytes, 16-byte aligned.  `rows`: nothing, or (stack layers only) one NN11Rows: perspective i of the call is then row
// rows[i] of the stack -- any list, unsorted, with repeats; an index outside [0, stack_rows) stages zeros, reads
// nothing and sets NN11_ERR_INDEX in the latch.
template <class Shape, int KS, int NT, int NTB, class Epi, class... Rows>
__device__ __forceinline__ void conv_tiles(unsigned char* lds, int n0, const void* __restrict__ in, int dtype,
                                           const uint16_t* __restrict__ wimg, uint16_t* __restrict__ out, int64_t P,
                                           const Epi& epi, Rows... rows) {
    using Ge = NN11Geom<Shape::SIDE>;
    constexpr int PIX = Ge::PIX, G = Ge::G, MW = Ge::MW, NW = Ge::NW, THREADS = Ge::THREADS;
    constexpr int NPIX_IN = Shape::NPIX_IN, NPIX_OUT = Shape::NPIX_OUT, OS = Shape::OSIDE;
    constexpr int ROWS_OUT = G * NPIX_OUT;                                  // <= Ge::ROWS: tiles beyond are skipped
    constexpr int CINP = KS * 16, COUTP = NT * 32;
    constexpr int NCHUNK = conv_chunks(KS), CK = KS / NCHUNK;               // k-steps of one chunk
    constexpr bool STACK = Shape::STACK != CONV_NO_STACK, GATHER = sizeof...(Rows) == 1;
    static_assert(CK * NCHUNK == KS && CK <= CONV_CHUNK_KS, "the k-steps of a layer are cut into equal chunks");
    static_assert(!STACK || (Shape::TAPS == 9 && KS == 2 && NPIX_IN == PIX && NPIX_OUT == PIX),
                  "a stack layer is a 3x3 of stride 1 over 18 k values");
    static_assert(sizeof...(Rows) == 0 || (GATHER && STACK), "only a stack layer gathers, by one NN11Rows");
    constexpr int PITCH = CK * 32 + 16;

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
        pbase[i] = row < ROWS_OUT ? p * NPIX_IN : -1;
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
        uint16_t* s = reinterpret_cast<uint16_t*>(lds);
        if constexpr (GATHER) {
            const NN11Rows& g = nn11_rows_arg(rows...);
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
                        const int sp = Shape::src(py[i], px[i], k % 9);
                        if (Shape::STACK == CONV_STACK_CIRCULAR || sp >= 0) v = s[2 * pbase[i] + (k / 9) * PIX + sp];
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
        const uint4* src = reinterpret_cast<const uint4*>(static_cast<const uint16_t*>(in) + persp0 * NPIX_IN * CINP);
        constexpr int ROW16 = CINP / 8, CH16 = CK * 2;                      // 16-byte pieces of an image row / of its chunk
        for (int c = 0; c < NCHUNK; ++c) {
            if (c > 0) __syncthreads();                                     // the previous chunk has been read
            for (int i = tid; i < Ge::LROWS * CH16; i += THREADS) {
                const int row = i / CH16, cc = i % CH16;
                const uint4 v = row < np * NPIX_IN ? src[row * ROW16 + c * CH16 + cc] : make_uint4(0, 0, 0, 0);
                *reinterpret_cast<uint4*>(lds + row * PITCH + cc * 16) = v;
            }
            __syncthreads();
            for (int tap = 0; tap < Shape::TAPS; ++tap) {
                int arow[MW];                                               // LDS byte address of the lane's source row
#pragma unroll
                for (int i = 0; i < MW; ++i) {
                    const int sp = pbase[i] >= 0 ? Shape::src(py[i], px[i], tap) : -1;
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
                const float4 v = epi(make_float4(acc[i][n][4 * g + 0], acc[i][n][4 * g + 1], acc[i][n][4 * g + 2], acc[i][n][4 * g + 3]),
                                     c0, o + c0);
                uint2 pk;
                pk.x = (uint32_t)nn11_bf16(v.x) | ((uint32_t)nn11_bf16(v.y) << 16);
                pk.y = (uint32_t)nn11_bf16(v.z) | ((uint32_t)nn11_bf16(v.w) << 16);
                *reinterpret_cast<uint2*>(out + o + c0) = pk;
            }
    }
}

}  // namespace tq
