// Host-side instantiation of the product's TD-target header (csrc/td_target.hpp), beside host_lattice_shim.cpp: the
// per-state functions the HIP kernel k_td_target calls, driven by a serial restatement of the kernel's own loop
// (longest slice of the batch, f32 maximum of each slice).
// TEST ONLY: built by tests/test_replay_targets_host.py into a temp dir with g++; it is not a backend of the product.
#include <math.h>
#include <stdint.h>

#include "td_target.hpp"

extern "C" void shim_td_target(const float* q, const int64_t* offsets, int n, const float* rewards, const uint8_t* terminals,
                               float discount, float lo, float hi, float* y) {
    int64_t longest = 0;
    for (int i = 0; i < n; ++i) {
        const int64_t c = offsets[i + 1] - offsets[i];
        longest = c > longest ? c : longest;
    }
    for (int e = 0; e < n; ++e) {
        const int64_t first = offsets[e], cnt = offsets[e + 1] - first;
        float best = -INFINITY;
        for (int64_t k = 0; k < 3 * cnt; ++k) best = tq::td_max(best, q[3 * first + k]);
        y[e] = tq::td_target_value(rewards[e], terminals[e], discount, tq::td_next_max(best, cnt, longest), lo, hi);
    }
}
