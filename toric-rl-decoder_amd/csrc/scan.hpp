// Exclusive scan of the per-lattice perspective counts (gfx950 / CDNA4), and -- a by-product -- the table of cut points
// for the stack write (cut_points.hpp).
//
// Two-level scan.  Level 1: one sum per 256 counts (part256), left behind by the kernel that produced
// the counts (block_count_partial) or, when lattices were reset by index, recomputed by
// k_scan_partials.  Level 2 (k_scan_final): a 256-thread workgroup owns SCAN_CHUNK = 2048 counts
// (8 per thread, two int4 loads), adds the partials before its chunk (<= N/256 values, one strided
// wave reduction) and writes the offsets.
#pragma once
#include "cut_points.hpp"

namespace tq {

// First pass of the exclusive scan, folded into the kernels that produce the hit counts: every
// 256-thread block of an all-lattice kernel leaves the sum of its 256 counts in part256[blockIdx.x].
// All 256 threads must call it (threads past N pass 0).
constexpr int PART_BLOCK = 256;
__device__ __forceinline__ void block_count_partial(int my_count, int64_t* __restrict__ part256) {
    __shared__ int ws_[4];
    int s = my_count;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    if ((threadIdx.x & 63) == 0) ws_[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) part256[blockIdx.x] = (int64_t)ws_[0] + ws_[1] + ws_[2] + ws_[3];
}

constexpr int SCAN_CHUNK = 256 * CUT_NL;                      // 2048

__device__ __forceinline__ int64_t wave_sum64(int64_t x) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o, 64);
    return x;
}

__device__ __forceinline__ void scan_load8(const int32_t* __restrict__ counts, int64_t N, int64_t i0, int (&c)[8]) {
    if (i0 + 8 <= N) {
        const int4 a = *reinterpret_cast<const int4*>(counts + i0);
        const int4 b = *reinterpret_cast<const int4*>(counts + i0 + 4);
        c[0] = a.x; c[1] = a.y; c[2] = a.z; c[3] = a.w; c[4] = b.x; c[5] = b.y; c[6] = b.z; c[7] = b.w;
    } else {
#pragma unroll
        for (int k = 0; k < 8; ++k) c[k] = i0 + k < N ? counts[i0 + k] : 0;
    }
}

__global__ __launch_bounds__(256) void k_scan_partials(const int32_t* __restrict__ counts, int64_t* __restrict__ part256,
                                                       int64_t N) {
    const int64_t e = (int64_t)blockIdx.x * PART_BLOCK + threadIdx.x;
    block_count_partial(e < N ? counts[e] : 0, part256);
}

// `split` (may be NULL): the table of the batch's cut points into 1 << LG parts, cut_table_words(LG) words
// (cut_points.hpp).  A by-product of the scan: every thread knows the offsets around its eight lattices, the workgroup
// sums all level-1 partials for P, and the thread whose interval holds a cut point writes it; workgroup 0 writes the
// entries no interval holds, and the header.
__global__ __launch_bounds__(256) void k_scan_final(const int32_t* __restrict__ counts, const int64_t* __restrict__ partial,
                                                    int64_t* __restrict__ offsets, int32_t* __restrict__ counts_out,
                                                    int64_t N, int32_t* __restrict__ split, int LG) {
    __shared__ int64_t ws[4];
    __shared__ int64_t base_s, total_s;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t i0 = (int64_t)blockIdx.x * SCAN_CHUNK + tid * 8;
    int c[8];
    scan_load8(counts, N, i0, c);
    int64_t mine = 0;
#pragma unroll
    for (int k = 0; k < 8; ++k) mine += c[k];
    int64_t inc = mine;                                       // inclusive scan of thread sums in the wave
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int64_t t = __shfl_up(inc, o, 64);
        if (lane >= o) inc += t;
    }
    if (lane == 63) ws[wave] = inc;
    if (wave == 0) {                                          // sum of the 256-count partials before this chunk
        int64_t b = 0;
        for (int j = lane; j < (int)blockIdx.x * (SCAN_CHUNK / PART_BLOCK); j += 64) b += partial[j];
        b = wave_sum64(b);
        if (lane == 0) base_s = b;
    }
    if (wave == 1 && split) {                                 // P = sum of all partials
        int64_t b = 0;
        const int nparts = (int)((N + PART_BLOCK - 1) / PART_BLOCK);
        for (int j = lane; j < nparts; j += 64) b += partial[j];
        b = wave_sum64(b);
        if (lane == 0) total_s = b;
    }
    __syncthreads();
    int64_t run = base_s + inc - mine;
    for (int w = 0; w < wave; ++w) run += ws[w];
    int64_t o[9];
    o[0] = run;
#pragma unroll
    for (int k = 0; k < 8; ++k) o[k + 1] = o[k] + c[k];       // counts past N were loaded as 0
    if (i0 + 8 <= N) {
        longlong2* dst = reinterpret_cast<longlong2*>(offsets + i0);
#pragma unroll
        for (int k = 0; k < 4; ++k) dst[k] = make_longlong2(o[2 * k], o[2 * k + 1]);
        if (counts_out) {
            *reinterpret_cast<int4*>(counts_out + i0) = make_int4(c[0], c[1], c[2], c[3]);
            *reinterpret_cast<int4*>(counts_out + i0 + 4) = make_int4(c[4], c[5], c[6], c[7]);
        }
        if (i0 + 8 == N) offsets[N] = o[8];
    } else {
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            if (i0 + k < N) {
                offsets[i0 + k] = o[k];
                if (counts_out) counts_out[i0 + k] = c[k];
                if (i0 + k + 1 == N) offsets[N] = o[k + 1];
            }
        }
    }
    if (split) {
        const int64_t total = total_s;
        auto put = [&](int64_t k, int32_t e) { split[k] = e; };
        if (blockIdx.x == 0) {
            if (tid == 0) cut_header_store(split, LG, total, N);
            cut_block0_entries(total, LG, tid, 256, put);
        }
        cut_thread_entries(o, i0, total, LG, put);
    }
}

}  // namespace tq
