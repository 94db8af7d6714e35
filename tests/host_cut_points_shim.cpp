// Host-side instantiation of the stack write's cut points (csrc/cut_points.hpp), beside host_stream_range_shim.cpp: the
// functions k_scan_final calls to write its table and stream_setup to decide whether a table is followed.  What is about
// threads is walked here in a loop: the scan's grid.
// TEST ONLY: built by tests/test_cut_points_host.py into a temp dir with g++; it is not a backend of the product.
#include <stddef.h>
#include <stdint.h>

#include "cut_points.hpp"

extern "C" int64_t shim_cut_target(int64_t total, int64_t k, int lg) { return tq::cut_target(total, k, lg); }
extern "C" int64_t shim_cut_floor(int64_t total, int64_t x, int lg) { return tq::cut_floor(total, x, lg); }
extern "C" int64_t shim_cut_table_words(int lg) { return (int64_t)tq::cut_table_words(lg); }
extern "C" int shim_cut_header_words() { return tq::CUT_HEADER_WORDS; }

// The table as the grid of k_scan_final writes it for the scan offsets[0..N] of N lattices: workgroups of 256 threads,
// CUT_NL lattices per thread, lattices past N counted as 0; workgroup 0 adds its entries and the header.
// table: cut_table_words(lg) words, filled by the caller; writes[k] += 1 for every store to entry k = 0..G.
extern "C" void shim_scan_table(const int64_t* offsets, int64_t N, int lg, int32_t* table, int32_t* writes) {
    constexpr int NL = tq::CUT_NL, THREADS = 256;
    const int64_t total = offsets[N];
    auto put = [&](int64_t k, int32_t e) { table[k] = e; ++writes[k]; };
    const int64_t blocks = (N + THREADS * NL - 1) / (THREADS * NL);
    for (int64_t b = 0; b < blocks; ++b) {
        for (int tid = 0; tid < THREADS; ++tid) {
            const int64_t i0 = (b * THREADS + tid) * NL;
            int64_t o[NL + 1];
            for (int j = 0; j <= NL; ++j) o[j] = offsets[i0 + j < N ? i0 + j : N];
            if (b == 0) {
                if (tid == 0) tq::cut_header_store(table, lg, total, N);
                tq::cut_block0_entries(total, lg, tid, THREADS, put);
            }
            tq::cut_thread_entries(o, i0, total, lg, put);
        }
    }
}

extern "C" int shim_cut_header_matches(const int32_t* table, int lg, int64_t p_tab, int64_t e_begin, int64_t e_end) {
    return tq::cut_header_matches(table, lg, p_tab, e_begin, e_end);
}
