// The arithmetic of the replay memory's sum tree (replay.hpp): plain index arithmetic and the descent, for host
// and device like the lattice algebra -- the kernels, the entry points of abi_replay.hpp and
// tests/test_sum_tree_host.py (g++) call the same functions.  The sampler's steps that are plain loads, stores and
// arithmetic are here whole, one lane's share each; what needs the wavefront (the ballot over the pick list, the
// barriers, the Philox stream, the weights) stays in replay.hpp.
//
// Tree: L levels (root = level 0), heap order, node n has children 2n+1 and 2n+2, level lvl holds the nodes
// 2^lvl - 1 .. 2^(lvl+1) - 2, leaf i is node 2^(L-1) - 1 + i and holds record i.
#pragma once
#include "lattice.hpp"

namespace tq {

constexpr int RP_CHUNK_LG = 11;          // leaves per range-rebuild workgroup: 2048 (16 KiB of f64, two LDS buffers)
constexpr int RP_STAGE_LEVELS = 13;      // top levels of the tree staged in LDS by the sample kernel: 8191 nodes, 64 KiB
constexpr int RP_SEG = 6;                // levels below the staged ones are fetched in subtrees of this depth (126 nodes)

// ---- shape
// SumTree.tree_level: math.ceil(math.log(max_size+1, 2))+1, in floating point as the reference has it (host only: the
// handle is shaped once, when it is made).
inline int tree_levels(int64_t cap) { return (int)__builtin_ceil(__builtin_log((double)cap + 1.0) / __builtin_log(2.0)) + 1; }
TQ_HD constexpr int64_t tree_nodes(int L) { return ((int64_t)1 << L) - 1; }
TQ_HD int64_t level_first(int lvl) { return ((int64_t)1 << lvl) - 1; }
TQ_HD int64_t left_child(int64_t node) { return 2 * node + 1; }              // the right one is the next node
TQ_HD int levels_below(int L, int lvl) { return L - 1 - lvl; }                // leaf levels under a node of level lvl
TQ_HD int64_t leaf_node(int L, int64_t i) { return level_first(L - 1) + i; }
TQ_HD int64_t leaf_of_node(int L, int64_t node) { return node - level_first(L - 1); }
// the node of level lvl above leaf `leaf` (the leaf's own node at lvl = L - 1)
TQ_HD int64_t ancestor_at(int L, int64_t leaf, int lvl) { return ((leaf_node(L, leaf) + 1) >> levels_below(L, lvl)) - 1; }
// the first of the 2^levels_below leaves under `node` of level lvl
TQ_HD int64_t first_leaf_under(int L, int64_t node, int lvl) { return ((node + 1) << levels_below(L, lvl)) - ((int64_t)1 << (L - 1)); }

// ---- rebuild chunks: the leaves in runs of 2^clg, each the leaves of one subtree whose root is at level L-1-clg; the
// first `nchunks` of them hold ring positions.
TQ_HD int chunk_lg(int L) { return L - 1 < RP_CHUNK_LG ? L - 1 : RP_CHUNK_LG; }
TQ_HD int chunk_root_level(int L, int clg) { return L - 1 - clg; }            // clg leaf levels lie under it
TQ_HD int64_t chunk_count(int64_t cap, int clg) { return (cap + ((int64_t)1 << clg) - 1) >> clg; }
// the j-th chunk to rebuild after an ingest that began in chunk `cursor_chunk` = cursor >> clg
TQ_HD int64_t chunk_of(int64_t cursor_chunk, int64_t j, int64_t nchunks) { return (cursor_chunk + j) % nchunks; }
// An ingest of a block of `span` slots touches positions that start at the cursor and span at most min(span, cap),
// modulo the capacity.  Counted in chunk slots, a range that wraps also crosses the unused tail of the last chunk
// (nchunks * 2^clg - cap leaves): so the chunks to rebuild are those of span + tail consecutive slots -- that many
// chunks and one more (the cursor lies anywhere in its chunk), and never more than there are.
TQ_HD int64_t chunks_to_rebuild(int64_t span, int64_t cap, int clg, int64_t nchunks) {
    if (span > cap) span = cap;
    const int64_t tail = (nchunks << clg) - cap;
    const int64_t n = chunk_count(span + tail, clg) + 1;
    return n < nchunks ? n : nchunks;
}

// ---- the sampler (k_replay_sample): the top staged_levels(L) levels live in LDS; below them the descent goes through
// segments -- the subtree of depth seg_depth under the current node without that node, level by level: the 2^r nodes
// r levels down are slots seg_slot(r, 0) .. seg_slot(r, 2^r - 1), r = 1 .. depth.
TQ_HD int staged_levels(int L) { return L < RP_STAGE_LEVELS ? L : RP_STAGE_LEVELS; }
TQ_HD int seg_depth(int L, int lvl) { return levels_below(L, lvl) < RP_SEG ? levels_below(L, lvl) : RP_SEG; }
TQ_HD constexpr int seg_words(int depth) { return (2 << depth) - 2; }
TQ_HD int seg_slot(int r, int q) { return (1 << r) - 2 + q; }
// of the two nodes under the q-th node of a segment's level, the number of the left or the right one in the next level
TQ_HD int seg_child_index(int q, bool right) { return right ? 2 * q + 1 : 2 * q; }
// the q-th node `depth` levels under `node`
TQ_HD int64_t seg_child_node(int64_t node, int depth, int64_t q) { return ((node + 1) << depth) - 1 + q; }
// the tree node that slot t of the segment under `node` is loaded from
TQ_HD int64_t seg_source(int64_t node, int t) {
    const int r = 31 - __builtin_clz((unsigned)(t + 2));
    return seg_child_node(node, r, t + 2 - (1 << r));
}
// the slot r levels down that a pick corrects which lies `below` levels down at relative leaf `rel`
TQ_HD int seg_ancestor_slot(int64_t rel, int below, int r) { return seg_slot(r, (int)(rel >> (below - r))); }

// The descent step is SumTree._find's, value <= left ? left : (value -= left, right), spelled as the branch it is in
// the two loops below and nowhere else: the right child is loaded only when it is taken.  (One helper for the step,
// taking both children by value, made k_replay_sample 3 per cent slower: profiles/sum_tree_ab.txt.)
// The descent through the T staged levels `stg`: the node of level T - 1 it ends on, that node's value in `cur`.
TQ_HD int64_t descend_staged(const double* stg, int T, double& value, double& cur) {
    int64_t node = 0;
    for (int lvl = 0; lvl < T - 1; ++lvl) {
        const int64_t lc = left_child(node);
        const double left = stg[lc];
        if (value <= left) { node = lc; cur = left; }
        else { value = value - left; node = lc + 1; cur = stg[lc + 1]; }
    }
    return node;
}
// A segment, in three steps, each one lane's share of the 64.  Fetch: the subtree of `depth` levels under `node`, as
// the tree in memory has it.
constexpr int SEG_LANES = 64;
TQ_HD void seg_fetch(double* seg, const double* __restrict__ tree, int64_t node, int depth, int lane) {
    for (int t = lane; t < seg_words(depth); t += SEG_LANES) seg[t] = tree[seg_source(node, t)];
}
// Apply: whether an earlier pick lies under `node` of level lvl, and if so its value off the segment: lane r - 1 corrects
// the pick's ancestor r levels down.  The picks are applied in pick order.
TQ_HD bool leaf_under(int L, int64_t leaf, int64_t node, int lvl) { return ancestor_at(L, leaf, lvl) == node; }
TQ_HD void seg_apply_pick(double* seg, int L, int64_t node, int lvl, int depth, int64_t leaf, double v, int lane) {
    if (lane >= depth) return;
    const int slot = seg_ancestor_slot(leaf - first_leaf_under(L, node, lvl), levels_below(L, lvl), lane + 1);
    seg[slot] = seg[slot] - v;
}
// Walk: down the segment's levels; which of the 2^depth nodes at its bottom the descent ends on.
TQ_HD int seg_walk(const double* seg, int depth, double& value, double& cur) {
    int q = 0;
    for (int r = 1; r <= depth; ++r) {
        const int lc = seg_slot(r, seg_child_index(q, false));
        const double left = seg[lc];
        if (value <= left) { q = seg_child_index(q, false); cur = left; }
        else { value = value - left; q = seg_child_index(q, true); cur = seg[lc + 1]; }
    }
    return q;
}
// The pick's value off its staged ancestors (distinct nodes): lane `lane` corrects the one of level `lane`.
TQ_HD void stage_correct(double* stg, int L, int T, int64_t leaf, double cur, int lane) {
    if (lane >= T) return;
    const int64_t a = ancestor_at(L, leaf, lane);
    stg[a] = stg[a] - cur;
}

}  // namespace tq
