// Host-side instantiation of the planned selection's arithmetic (csrc/select_plan.hpp), beside host_cut_points_shim.cpp
// and host_sum_tree_shim.cpp: the plan (need -> scan -> rows) and the selection over the compact table, lattice by
// lattice, over the functions k_select, k_select_need, k_select_rows and k_select_planned call.
// TEST ONLY: built by tests/test_select_plan_host.py into a temp dir with g++; it is not a backend of the product.
#include <stddef.h>
#include <stdint.h>

#include "select_plan.hpp"

extern "C" int shim_need(int n, int greedy) { return tq::sel_need(n, greedy != 0); }

extern "C" int shim_greedy(uint64_t seed, uint32_t env, uint32_t episode, uint32_t step, double eps) {
    return tq::sel_greedy(tq::sel_draw(seed, env, episode, step, tq::DOMAIN_SEL), eps) ? 1 : 0;
}

extern "C" int64_t shim_plan(int64_t N, const int64_t* offsets, const double* eps, const uint32_t* episodes, const uint32_t* steps,
                             uint64_t seed, int64_t first_env, int32_t* need, int64_t* plan_offsets, int32_t* rows,
                             int64_t rows_cap) {
    return tq::sel_plan_host(N, offsets, eps, episodes, steps, seed, first_env, tq::DOMAIN_SEL, need, plan_offsets, rows, rows_cap);
}

extern "C" int64_t shim_select_planned(int64_t N, const float* q_rows, const int64_t* offsets, const int64_t* plan_offsets,
                                       const int32_t* pos, const double* eps, const uint32_t* episodes, const uint32_t* steps,
                                       uint64_t seed, int64_t first_env, int32_t* actions, float* qv) {
    return tq::sel_planned_host(N, q_rows, offsets, plan_offsets, pos, eps, episodes, steps, seed, first_env, tq::DOMAIN_SEL,
                                actions, qv);
}
