// The cut points of the stack write (stream_write.hpp): plain integer arithmetic for host and device, like the lattice
// algebra -- the scan (scan.hpp) that writes them all as a table, the stack write's set-up that decides whether a table
// is followed, the handle that allocates it, and tests/test_cut_points_host.py (g++) call the same functions.  (The
// search that finds two cut points where there is no table, find_cut in stream_write.hpp, uses cut_target only.)
//
// The stack of P perspectives is cut into G = 1 << LG fine parts of equal perspective count.  Cut point k = 0..G is the
// first lattice e with offsets[e] >= cut_target(P, k, LG).  Two workgroups that disagree on one overlap or leave a gap.
#pragma once
#include "lattice.hpp"

namespace tq {

// Part k begins at the first lattice whose offset reaches this many perspectives.
TQ_HD int64_t cut_target(int64_t total, int64_t k, int LG) { return (int64_t)(((uint64_t)total * (uint64_t)k) >> LG); }

// The largest k in [0, G] with cut_target(total, k, LG) <= x, for x >= 0: float estimate, exact fix-up.  An empty stack
// has every target at 0.
TQ_HD int64_t cut_floor(int64_t total, int64_t x, int LG) {
    const int64_t G = (int64_t)1 << LG;
    if (total == 0) return G;
    int64_t k = (int64_t)((double)(x + 1) * (double)G / (double)total);
    k = k < 0 ? 0 : (k > G ? G : k);
    while (k < G && cut_target(total, k + 1, LG) <= x) ++k;
    while (k > 0 && cut_target(total, k, LG) > x) --k;
    return k;
}

// ---- the scan's table: put(k, e) is called exactly once for every k = 0..G over the two functions below, whatever
// the counts -- nothing of an earlier, larger stack survives in a table that a scan has written.
// One scan thread knows the offsets o[0..NL] around its NL lattices i0 .. i0 + NL - 1 (lattices past the batch count 0)
// and puts the cut points whose target lies in (o[0], o[NL]]: usually none, rarely one.
constexpr int CUT_NL = 8;
template <class Put>
TQ_HD void cut_thread_entries(const int64_t (&o)[CUT_NL + 1], int64_t i0, int64_t total, int LG, Put&& put) {
    if (o[CUT_NL] <= o[0]) return;
    const int64_t kA = cut_floor(total, o[0], LG) + 1, kB = cut_floor(total, o[CUT_NL], LG);
    for (int64_t k = kA; k <= kB; ++k) {
        const int64_t t = cut_target(total, k, LG);
        int j = 0;
#pragma unroll
        for (int q = 1; q < CUT_NL; ++q) j += o[q] < t;       // smallest j with o[j + 1] >= t
        put(k, (int32_t)(i0 + j + 1));
    }
}
// The cut points with target 0 (k = 0, every k < G / total when the stack has fewer perspectives than parts, the whole
// table when it is empty) lie in no thread's interval: lattice 0 is their answer, and thread `tid` of the `nthreads` of
// the scan's workgroup 0 puts its share of them.
template <class Put>
TQ_HD void cut_block0_entries(int64_t total, int LG, int tid, int nthreads, Put&& put) {
    const int64_t kz = cut_floor(total, 0, LG);
    for (int64_t k = tid; k <= kz; k += nthreads) put(k, 0);
}

// ---- the table's layout: G + 1 cut points, then a header -- P (low word, high word) and N, the last lattice of the
// scan -- by which the stack write tells that a table belongs to the offsets it was handed (a table is matched to an
// offsets POINTER, whose contents the caller owns).  A scan covers the lattices [0, N].
constexpr int CUT_HEADER_WORDS = 3;
TQ_HD constexpr int cut_table_words(int LG) { return (1 << LG) + 1 + CUT_HEADER_WORDS; }
TQ_HD void cut_header_store(int32_t* split, int LG, int64_t total, int64_t N) {
    int32_t* h = split + (1 << LG) + 1;
    h[0] = (int32_t)(uint32_t)total; h[1] = (int32_t)(uint32_t)((uint64_t)total >> 32); h[2] = (int32_t)N;
}
TQ_HD constexpr int cut_header_at(int LG) { return (1 << LG) + 1; }                          // index of the header's first word
TQ_HD bool cut_header_words_match(int32_t h0, int32_t h1, int32_t h2, int64_t p_tab, int64_t e_begin, int64_t e_end) {
    const int64_t t_all = (int64_t)(((uint64_t)(uint32_t)h1 << 32) | (uint32_t)h0);
    return t_all == p_tab && e_begin == 0 && (int64_t)h2 == e_end;
}
TQ_HD bool cut_header_matches(const int32_t* split, int LG, int64_t p_tab, int64_t e_begin, int64_t e_end) {
    const int32_t* h = split + cut_header_at(LG);
    return cut_header_words_match(h[0], h[1], h[2], p_tab, e_begin, e_end);
}

}  // namespace tq
