// What the epsilon-greedy selection reads, decided before it looks at a Q-value (host + device, like cut_points.hpp and
// sum_tree.hpp; a g++ build of this header is tests/host_select_plan_shim.cpp).
//
// _selectActionBatch_prime (numba/util_actor.py:69-107) takes one Philox draw per lattice, keyed by the lattice's
// (episode, step): word x decides greedy or not, and a lattice that is not greedy takes perspective mulhi32(y, n) and
// op mulhi32(z, 3) -- it reads ONE row of the (P,3) Q-table (for the q_values it returns), a greedy lattice all n of its
// rows, a lattice without perspectives none.  The plan is that list of rows, lattice by lattice, so that the forward pass
// runs on those perspectives only; the selection over the compact table redraws with the same counters.
//
//   need[e]          sel_need(n_e, greedy_e)
//   plan_offsets     the exclusive scan of need, i64[N+1]; R = plan_offsets[N]
//   rows             i32[R], strictly increasing: lo_e .. lo_e + n_e - 1 of a greedy lattice, sel_random_row of another
//   compact table    q_rows f32[R][3], q_rows[i] = Q(perspective rows[i])
#pragma once
#include "lattice.hpp"

namespace tq {

// the lattice's draw: counters = its (episode, step) for a handle, the caller's call counter for the stateless form
TQ_HD U4 sel_draw(uint64_t seed, uint32_t env, uint32_t c1, uint32_t c2, uint32_t domain) {
    return draw(seed, env, c1, c2, domain, 0);
}
TQ_HD bool sel_greedy(const U4& w, double eps) { return (1.0 - eps) > u01(w.x); }
// rows of the Q-table the selection of a lattice with n perspectives reads
TQ_HD int sel_need(int n, bool greedy) { return n == 0 ? 0 : (greedy ? n : 1); }
// what a lattice that is not greedy takes
TQ_HD int sel_random_persp(const U4& w, int n) { return (int)mulhi32(w.y, (uint32_t)n); }
TQ_HD int sel_random_op(const U4& w) { return (int)mulhi32(w.z, 3); }
// ... and the one row it reads: lo = offsets[e]
TQ_HD int64_t sel_random_row(const U4& w, int64_t lo, int n) { return lo + sel_random_persp(w, n); }

// np.argmax's order on (value, flat index) pairs: does (x, k) come before (best, bk)?  A NaN comes before every number,
// the larger of two numbers before the smaller, and the lower index first among NaNs or equal numbers.
TQ_HD bool sel_beats(float x, int k, float best, int bk) {
    const bool xn = x != x, bn = best != best;
    if (xn || bn) return xn && (!bn || k < bk);
    return x > best || (x == best && k < bk);
}

// np.argmax of a lattice's slice in row-major order (:93-95) as the flat index 3 * perspective + op: the first NaN if
// there is one, else the first maximum (0 for a slice of -inf).  What the wave-wide search of k_select /
// k_select_planned computes; here for the host.
inline int sel_first_max(const float* q, int n) {
    float best = -__builtin_inff();
    int bk = 0;
    for (int k = 0; k < 3 * n; ++k)
        if (sel_beats(q[k], k, best, bk)) { best = q[k]; bk = k; }
    return bk;
}

// ---- the whole plan and the planned selection on host memory: what k_select_need / the scan / k_select_rows and
// k_select_planned do on the device, lattice by lattice.
// -> R = the sum of need; rows past rows_cap are not written (the device latches ERR_CAPACITY then).
inline int64_t sel_plan_host(int64_t N, const int64_t* offsets, const double* eps, const uint32_t* episodes, const uint32_t* steps,
                             uint64_t seed, int64_t first_env, uint32_t domain, int32_t* need, int64_t* plan_offsets,
                             int32_t* rows, int64_t rows_cap) {
    int64_t r = 0;
    for (int64_t e = 0; e < N; ++e) {
        const int64_t lo = offsets[e];
        const int n = (int)(offsets[e + 1] - lo);
        const U4 w = sel_draw(seed, (uint32_t)(first_env + e), episodes[e], steps[e], domain);
        const bool greedy = sel_greedy(w, eps[e]);
        const int k = sel_need(n, greedy);
        need[e] = k;
        plan_offsets[e] = r;
        for (int i = 0; i < k; ++i)
            if (r + i < rows_cap) rows[r + i] = (int32_t)(greedy ? lo + i : sel_random_row(w, lo, n));
        r += k;
    }
    plan_offsets[N] = r;
    return r;
}

// -> the number of lattices whose slice of the plan is not what this eps and these counters need (they get action 0 and
// zero q_values; the device latches ERR_INTERNAL).
inline int64_t sel_planned_host(int64_t N, const float* q_rows, const int64_t* offsets, const int64_t* plan_offsets,
                                const int32_t* pos, const double* eps, const uint32_t* episodes, const uint32_t* steps,
                                uint64_t seed, int64_t first_env, uint32_t domain, int32_t* actions, float* qv) {
    int64_t bad = 0;
    for (int64_t e = 0; e < N; ++e) {
        const int64_t lo = offsets[e], plo = plan_offsets[e];
        const int n = (int)(offsets[e + 1] - lo);
        for (int j = 0; j < 4; ++j) actions[4 * e + j] = 0;
        for (int j = 0; j < 3; ++j) qv[3 * e + j] = 0.f;
        const U4 w = sel_draw(seed, (uint32_t)(first_env + e), episodes[e], steps[e], domain);
        const bool greedy = sel_greedy(w, eps[e]);
        if ((int64_t)sel_need(n, greedy) != plan_offsets[e + 1] - plo) { ++bad; continue; }
        if (n == 0) continue;
        int pidx, a, qrow;
        if (greedy) {
            const int bk = sel_first_max(q_rows + 3 * plo, n);
            pidx = bk / 3; a = bk - 3 * pidx; qrow = pidx;
        } else {
            pidx = sel_random_persp(w, n); a = sel_random_op(w); qrow = 0;
        }
        for (int j = 0; j < 3; ++j) {
            actions[4 * e + j] = pos[3 * (lo + pidx) + j];
            qv[3 * e + j] = q_rows[3 * (plo + qrow) + j];
        }
        actions[4 * e + 3] = a + 1;
    }
    return bad;
}

}  // namespace tq
