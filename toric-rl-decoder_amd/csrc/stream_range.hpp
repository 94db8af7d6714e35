// Which bytes a workgroup of the stack write (stream_write.hpp) owns: plain integer arithmetic for host and device, like
// the lattice algebra and the TD target -- the kernel and tests/test_stream_range_host.py (g++) call the same functions.
#pragma once
#include "cut_points.hpp"

namespace tq {

// Fine parts [f_lo, f_hi) of a slot (the stack is cut into 1 << LG fine parts of equal perspective count at the cut points
// of cut_points.hpp).  Every pair of shares (2 RR fine parts) is cut into a LARGE slot of RR + bias parts
// and a SMALL one of RR - bias behind it; `idx` counts the pairs.
TQ_HD void slot_fine_parts(int large, int idx, int RR, int bias, int& f_lo, int& f_hi) {
    f_lo = idx * 2 * RR + (large ? 0 : RR + bias);
    f_hi = f_lo + (large ? RR + bias : RR - bias);
}

// Which of its pair's two slots a workgroup takes.  Workgroups b and b ^ 1 share pair b >> 1 and one word, zero between
// launches; each adds pair_claim(0, prefers_large).add to it once (a returning atomic) and reads its kind from what the
// word held before: 0 = it is the first of the pair and takes the kind it prefers; 1 / 3 = the other one came first and
// took the small / large slot, this one takes what is left (its own preference if the two differ) and stores 0 to the
// word again.  Anything else (kind = -1) is a word that no launch leaves behind: refused.
constexpr int PAIR_WORD_STRIDE = 32;                          // dwords: every pair's word on a 128-byte line of its own
TQ_HD constexpr int pair_set_words(int workgroups) { return workgroups / 2 * PAIR_WORD_STRIDE; }    // words of one launch
struct PairClaim {
    unsigned add;                     // what this workgroup adds to the pair's word
    int kind;                         // 1 = the large slot, 0 = the small one, -1 = refused
    bool second;                      // the second of the pair: it leaves the word zero
};
TQ_HD PairClaim pair_claim(unsigned old, int prefers_large) {
    PairClaim c;
    c.add = 1u + 2u * (unsigned)(prefers_large != 0);
    c.second = old != 0u;
    c.kind = old == 0u ? (prefers_large != 0) : (old == 1u ? 1 : (old == 3u ? 0 : -1));
    return c;
}

// One workgroup's part of the output.  It produces the perspectives [Q0, Q1) of a stack of p_all (NQ elements of `esize`
// bytes and 3 position dwords each) and stores the 128-byte lines whose FIRST element lies in that range, whole: the
// leading elements of the line that holds its first element are left to the range before, and for the trailing elements
// of its last line its producers go on for `need_extra` perspectives behind Q1.
struct StreamRange {
    int64_t org, porg;                // start of the line that holds element Q0 * NQ / dword Q0 * 3: ring bit x <-> element org + x
    uint32_t head, a0, a1;            // Q0 * NQ - org; this workgroup stores the elements [a0, a1) from org
    uint32_t phead, pa0, pa1;         // the same for the positions: dwords, 3 per perspective, lines of 32
    int64_t need_extra;               // perspectives behind Q1 that the last stack line / positions line needs
    bool last, has_stack, has_pos;    // last: no perspective behind this range
};
TQ_HD StreamRange stream_range(int64_t Q0, int64_t Q1, int64_t p_all, int NQ, int esize, bool want_pos) {
    StreamRange r;
    const int LE = 128 / esize;                               // elements per 128-byte line
    r.last = Q1 >= p_all;
    const int64_t S0 = Q0 * NQ, S1 = Q1 * NQ;                 // element range
    r.org = S0 / LE * LE;
    r.head = (uint32_t)(S0 - r.org);  r.a0 = r.head ? (uint32_t)LE : 0u;
    int64_t A1 = (S1 + LE - 1) / LE * LE;                     // the line that holds the end of the range is stored whole ...
    if (r.last || A1 > p_all * NQ) A1 = p_all * NQ;           // ... unless the stack ends inside it
    r.a1 = A1 > r.org ? (uint32_t)(A1 - r.org) : 0u;
    r.porg = Q0 * 3 / 32 * 32;
    r.phead = (uint32_t)(Q0 * 3 - r.porg);  r.pa0 = r.phead ? 32u : 0u;
    int64_t PA1 = (Q1 * 3 + 31) / 32 * 32;
    if (r.last || PA1 > p_all * 3) PA1 = p_all * 3;
    r.pa1 = PA1 > r.porg ? (uint32_t)(PA1 - r.porg) : 0u;
    const int64_t ne_s = (A1 - S1 + NQ - 1) / NQ, ne_p = (PA1 - Q1 * 3 + 2) / 3;
    r.need_extra = r.last ? 0 : ((want_pos && ne_p > ne_s) ? ne_p : ne_s);
    r.has_stack = r.a1 > r.a0;  r.has_pos = want_pos && r.pa1 > r.pa0;
    return r;
}

}  // namespace tq
