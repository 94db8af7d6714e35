// Host-side instantiation of the stack write's range arithmetic (csrc/stream_range.hpp), beside host_td_target_shim.cpp:
// the functions k_persp_stream calls to decide which bytes a workgroup owns.
// TEST ONLY: built by tests/test_stream_range_host.py into a temp dir with g++; it is not a backend of the product.
#include <stddef.h>
#include <stdint.h>

#include "stream_range.hpp"

// out[i] = {org, head, a0, a1, porg, phead, pa0, pa1, need_extra, last, has_stack, has_pos} of the range [q0[i], q1[i])
extern "C" void shim_stream_range(int n, const int64_t* q0, const int64_t* q1, int64_t p_all, int nq, int esize, int want_pos,
                                  int64_t* out) {
    for (int i = 0; i < n; ++i) {
        const tq::StreamRange r = tq::stream_range(q0[i], q1[i], p_all, nq, esize, want_pos != 0);
        const int64_t row[12] = {r.org, r.head, r.a0, r.a1, r.porg, r.phead, r.pa0, r.pa1, r.need_extra, r.last, r.has_stack, r.has_pos};
        for (int j = 0; j < 12; ++j) out[12 * i + j] = row[j];
    }
}

extern "C" void shim_slot_fine_parts(int large, int idx, int rr, int bias, int32_t* lo_hi) {
    int lo, hi;
    tq::slot_fine_parts(large, idx, rr, bias, lo, hi);
    lo_hi[0] = lo; lo_hi[1] = hi;
}
