// Host-side instantiation of the stack write's slot decision (csrc/stream_range.hpp: pair_claim, slot_fine_parts), beside
// host_stream_range_shim.cpp: what a workgroup of k_persp_stream adds to its pair's word, which slot it takes given what
// the word held, and who stores 0 to it.
// TEST ONLY: built by tests/test_stream_slots_host.py into a temp dir with g++; it is not a backend of the product.
#include <stddef.h>
#include <stdint.h>

#include "stream_range.hpp"

extern "C" int shim_pair_word_stride(void) { return tq::PAIR_WORD_STRIDE; }
extern "C" int shim_pair_set_words(int workgroups) { return tq::pair_set_words(workgroups); }

// out = {add, kind, second} of pair_claim(old, prefers_large)
extern "C" void shim_pair_claim(uint32_t old, int prefers_large, int32_t* out) {
    const tq::PairClaim c = tq::pair_claim(old, prefers_large);
    out[0] = (int32_t)c.add; out[1] = c.kind; out[2] = c.second;
}

// The workgroups of one launch arrive at their pairs' words in the order `order[0 .. n)` (workgroup numbers), workgroup b
// preferring the large slot iff prefers_large[b]: the kernel's steps in that order -- a returning add on words[b >> 1],
// pair_claim on the answer, the second arriver's store of 0.  kind[b] = -1 where the workgroup refuses; otherwise
// lo_hi[2 b ..] = its fine parts (slot_fine_parts).  Returns the number of workgroups that refused.
extern "C" int shim_launch(int n, const int32_t* order, const int32_t* prefers_large, uint32_t* words, int rr, int bias, int32_t* kind,
                           int32_t* lo_hi) {
    int refused = 0;
    for (int i = 0; i < n; ++i) {
        const int b = order[i];
        uint32_t& w = words[b >> 1];
        const uint32_t old = w;
        w += tq::pair_claim(0u, prefers_large[b]).add;
        const tq::PairClaim c = tq::pair_claim(old, prefers_large[b]);
        if (c.second) w = 0u;
        kind[b] = c.kind;
        refused += c.kind < 0;
        if (c.kind >= 0) {
            int lo, hi;
            tq::slot_fine_parts(c.kind, b >> 1, rr, bias, lo, hi);
            lo_hi[2 * b] = lo; lo_hi[2 * b + 1] = hi;
        }
    }
    return refused;
}
