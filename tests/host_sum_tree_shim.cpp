// Host-side instantiation of the sum tree's arithmetic (csrc/sum_tree.hpp), beside host_cut_points_shim.cpp: the
// functions the replay kernels (replay.hpp) and the tq_replay_* entry points call.  What is about lanes is walked here in
// a loop, lanes 0..63, the earlier picks in pick order: k_replay_sample's wave 0.
// TEST ONLY: built by tests/test_sum_tree_host.py into a temp dir with g++; it is not a backend of the product.
#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "sum_tree.hpp"

extern "C" int shim_tree_levels(int64_t cap) { return tq::tree_levels(cap); }
extern "C" int64_t shim_tree_nodes(int L) { return tq::tree_nodes(L); }
extern "C" int64_t shim_level_first(int lvl) { return tq::level_first(lvl); }
extern "C" int64_t shim_left_child(int64_t node) { return tq::left_child(node); }
extern "C" int64_t shim_leaf_node(int L, int64_t i) { return tq::leaf_node(L, i); }
extern "C" int64_t shim_leaf_of_node(int L, int64_t node) { return tq::leaf_of_node(L, node); }
extern "C" int64_t shim_ancestor_at(int L, int64_t leaf, int lvl) { return tq::ancestor_at(L, leaf, lvl); }
extern "C" int64_t shim_first_leaf_under(int L, int64_t node, int lvl) { return tq::first_leaf_under(L, node, lvl); }

extern "C" int shim_chunk_lg(int L) { return tq::chunk_lg(L); }
extern "C" int shim_chunk_root_level(int L, int clg) { return tq::chunk_root_level(L, clg); }
extern "C" int64_t shim_chunk_count(int64_t cap, int clg) { return tq::chunk_count(cap, clg); }

// What an ingest of `span` slots rebuilds when it starts at `cursor`, as tq_replay_save_block sizes the grid of
// k_replay_chunks and the kernel names its chunk: marks[c] = 1 for every chunk c rebuilt.  Returns the grid size.
extern "C" int64_t shim_rebuilt_chunks(int64_t cap, int clg, int64_t cursor, int64_t span, uint8_t* marks) {
    const int64_t nchunks = tq::chunk_count(cap, clg);
    const int64_t grid = tq::chunks_to_rebuild(span, cap, clg, nchunks);
    for (int64_t j = 0; j < grid; ++j) marks[tq::chunk_of(cursor >> clg, j, nchunks)] = 1;
    return grid;
}
// The same for every cursor 0 .. cap-1 and every span 1 .. max_span: marks is u8[cap][max_span][nchunks], zeroed by the
// caller; grids is i64[max_span] (the grid size does not depend on the cursor).
extern "C" void shim_rebuilt_chunks_all(int64_t cap, int clg, int64_t max_span, uint8_t* marks, int64_t* grids) {
    const int64_t nchunks = tq::chunk_count(cap, clg);
    for (int64_t cursor = 0; cursor < cap; ++cursor)
        for (int64_t span = 1; span <= max_span; ++span)
            grids[span - 1] = shim_rebuilt_chunks(cap, clg, cursor, span, marks + (cursor * max_span + span - 1) * nchunks);
}

extern "C" int shim_staged_levels(int L) { return tq::staged_levels(L); }
extern "C" int shim_seg_depth(int L, int lvl) { return tq::seg_depth(L, lvl); }
extern "C" int shim_seg_words(int depth) { return tq::seg_words(depth); }
extern "C" int shim_seg_slot(int r, int q) { return tq::seg_slot(r, q); }
extern "C" int shim_seg_child_index(int q, int right) { return tq::seg_child_index(q, right != 0); }
extern "C" int shim_levels_below(int L, int lvl) { return tq::levels_below(L, lvl); }
extern "C" int64_t shim_seg_child_node(int64_t node, int depth, int64_t q) { return tq::seg_child_node(node, depth, q); }
extern "C" int64_t shim_seg_source(int64_t node, int t) { return tq::seg_source(node, t); }
extern "C" int shim_seg_ancestor_slot(int64_t rel, int below, int r) { return tq::seg_ancestor_slot(rel, below, r); }

// B draws with the uniforms u on `tree` (L levels), the top T levels staged (the device passes staged_levels(L)): the
// header's steps in the order k_replay_sample's wave 0 takes them, a lane's share for each lane in turn, the earlier picks
// in pick order where the kernel takes them off a ballot.  idx / prio: the picks.  after: the tree with the effective
// values the draws leave -- the staged levels as corrected in place, below them every node less the picks under it, in
// pick order, which is what a segment fetched for a further draw would hold.
extern "C" void shim_sample(const double* tree, int L, int T, int B, const double* u, int64_t* idx, double* prio, double* after) {
    std::vector<double> stg(tree, tree + tq::tree_nodes(T)), pv(B), seg(tq::seg_words(tq::RP_SEG));
    std::vector<int32_t> pleaf(B);
    for (int k = 0; k < B; ++k) {
        double value = u[k] * stg[0], cur = stg[0];
        int64_t node = tq::descend_staged(stg.data(), T, value, cur);
        for (int lvl = T - 1; lvl < L - 1;) {
            const int depth = tq::seg_depth(L, lvl);
            for (int lane = 0; lane < tq::SEG_LANES; ++lane) tq::seg_fetch(seg.data(), tree, node, depth, lane);
            for (int j = 0; j < k; ++j) {
                if (!tq::leaf_under(L, pleaf[j], node, lvl)) continue;
                for (int lane = 0; lane < tq::SEG_LANES; ++lane) tq::seg_apply_pick(seg.data(), L, node, lvl, depth, pleaf[j], pv[j], lane);
            }
            node = tq::seg_child_node(node, depth, tq::seg_walk(seg.data(), depth, value, cur));
            lvl += depth;
        }
        const int64_t leaf = tq::leaf_of_node(L, node);
        pleaf[k] = (int32_t)leaf;
        pv[k] = cur;
        idx[k] = leaf;
        prio[k] = cur;
        for (int lane = 0; lane < tq::SEG_LANES; ++lane) tq::stage_correct(stg.data(), L, T, leaf, cur, lane);
    }
    for (int64_t n = 0; n < tq::tree_nodes(L); ++n) after[n] = n < tq::tree_nodes(T) ? stg[n] : tree[n];
    for (int k = 0; k < B; ++k)
        for (int lvl = T; lvl < L; ++lvl) {
            const int64_t a = tq::ancestor_at(L, pleaf[k], lvl);
            after[a] = after[a] - pv[k];
        }
}
