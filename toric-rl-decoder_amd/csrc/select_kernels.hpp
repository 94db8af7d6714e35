// Kernels of the planned selection (gfx950 / CDNA4): which rows of the Q-table the epsilon-greedy selection reads, and
// the selection over the compact table of those rows.  select_plan.hpp has the arithmetic; DESIGN.md 3.9 the design.
#pragma once
#include "stream_write.hpp"

namespace tq {

// ------------------------------------------------------------------ planned selection (select_plan.hpp)
// The rows of the Q-table tq_select_action would read, so that the forward pass runs on those perspectives only.
// k_select_need: thread per lattice, need[e] and -- like every all-lattice kernel -- the level-1 sums of the scan that
// turns need into plan_offsets.  A count outside [0, 2 d^2] (offsets that are no scan of perspective counts) needs
// nothing and latches ERR_INTERNAL.
template <int D>
__global__ __launch_bounds__(256) void k_select_need(const int64_t* __restrict__ offsets, const double* __restrict__ eps,
                                                     const uint32_t* __restrict__ episodes, const uint32_t* __restrict__ steps,
                                                     int32_t* __restrict__ need, uint64_t seed, int64_t first_env, int64_t N,
                                                     int64_t* __restrict__ part256, int* __restrict__ err) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    int k = 0;
    if (e < N) {
        const int64_t n = offsets[e + 1] - offsets[e];
        if (n < 0 || n > Lat<D>::NQ) atomicOr(err, ERR_INTERNAL);
        else {
            const U4 w = sel_draw(seed, (uint32_t)(first_env + e), episodes[e], steps[e], DOMAIN_SEL);
            k = sel_need((int)n, sel_greedy(w, eps[e]));
        }
        need[e] = k;
    }
    block_count_partial(k, part256);
}

// One wavefront per lattice writes its slice of the row list: lo .. lo + n - 1 of a greedy lattice, the one row of
// another (the same draw again).  Nothing is written at or past rows_cap; a lattice whose slice does not fit latches
// ERR_CAPACITY, a row number that int32 does not hold ERR_INTERNAL.
template <int D>
__global__ __launch_bounds__(256) void k_select_rows(const int64_t* __restrict__ offsets, const int64_t* __restrict__ plan_offsets,
                                                     const double* __restrict__ eps, const uint32_t* __restrict__ episodes,
                                                     const uint32_t* __restrict__ steps, int32_t* __restrict__ rows,
                                                     int64_t rows_cap, uint64_t seed, int64_t first_env, int64_t N,
                                                     int* __restrict__ err) {
    const int lane = threadIdx.x & 63;
    const int64_t e = (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (e >= N) return;
    const int64_t plo = plan_offsets[e];
    const int k = (int)(plan_offsets[e + 1] - plo);
    if (k <= 0 || plo < 0) return;
    const int64_t lo = offsets[e];
    const int n = (int)(offsets[e + 1] - lo);
    if (lo < 0 || lo + n > 0x7fffffffll) { if (lane == 0) atomicOr(err, ERR_INTERNAL); return; }
    if (lane == 0 && plo + k > rows_cap) atomicOr(err, ERR_CAPACITY);
    const U4 w = sel_draw(seed, (uint32_t)(first_env + e), episodes[e], steps[e], DOMAIN_SEL);
    const bool greedy = sel_greedy(w, eps[e]);
    for (int i = lane; i < k; i += 64)
        if (plo + i < rows_cap) rows[plo + i] = (int32_t)(greedy ? lo + i : sel_random_row(w, lo, n));
}

// k_select over the compact table q_rows f32[R][3] of the planned rows: the same draw, the greedy search over the
// lattice's slice plan_offsets[e].. of it, positions from the full table.  The slice must be as long as this eps and
// these counters need (another eps, or a step between plan and selection, make it differ): otherwise action 0, zero
// q_values and ERR_INTERNAL.
template <int D>
__global__ __launch_bounds__(256) void k_select_planned(const float* __restrict__ q_rows, const int64_t* __restrict__ offsets,
                                                        const int64_t* __restrict__ plan_offsets, const int32_t* __restrict__ pos,
                                                        const double* __restrict__ eps, const uint32_t* __restrict__ episodes,
                                                        const uint32_t* __restrict__ steps, int32_t* __restrict__ actions,
                                                        float* __restrict__ qv, uint64_t seed, int64_t first_env, int64_t N,
                                                        int* __restrict__ err) {
    const int lane = threadIdx.x & 63;
    const int64_t e = (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (e >= N) return;
    const int64_t lo = offsets[e], plo = plan_offsets[e];
    const int64_t cnt = offsets[e + 1] - lo;
    const U4 w = sel_draw(seed, (uint32_t)(first_env + e), episodes[e], steps[e], DOMAIN_SEL);
    const bool greedy = sel_greedy(w, eps[e]);
    const bool ok = cnt >= 0 && cnt <= Lat<D>::NQ && plo >= 0 && plan_offsets[e + 1] - plo == (int64_t)sel_need((int)cnt, greedy);
    if (!ok || cnt == 0) {
        if (lane < 4) actions[4 * e + lane] = 0;
        if (qv && lane < 3) qv[3 * e + lane] = 0.f;
        if (!ok && lane == 0) atomicOr(err, ERR_INTERNAL);
        return;
    }
    const int n = (int)cnt;
    int pidx, a, qrow;
    if (greedy) {
        float best = -__builtin_inff();
        int bk = 0x7fffffff;
        for (int k = lane; k < 3 * n; k += 64) {
            const float x = q_rows[3 * plo + k];
            if (sel_beats(x, k, best, bk)) { best = x; bk = k; }   // first NaN, else first maximum within the lane
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const float ob = __shfl_xor(best, o, 64);
            const int ok2 = __shfl_xor(bk, o, 64);
            if (sel_beats(ob, ok2, best, bk)) { best = ob; bk = ok2; }
        }
        bk = bk == 0x7fffffff ? 0 : bk;
        pidx = bk / 3; a = bk - 3 * pidx; qrow = pidx;
    } else {
        pidx = sel_random_persp(w, n);
        a = sel_random_op(w);
        qrow = 0;
    }
    if (lane < 3) {
        actions[4 * e + lane] = pos[3 * (lo + pidx) + lane];
        if (qv) qv[3 * e + lane] = q_rows[3 * (plo + qrow) + lane];
    }
    if (lane == 3) actions[4 * e + 3] = a + 1;
}

}  // namespace tq
