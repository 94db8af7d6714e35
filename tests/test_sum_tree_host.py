"""The sum tree's arithmetic without a GPU (toric-rl-decoder_amd/csrc/sum_tree.hpp), built with g++ through
tests/host_sum_tree_shim.cpp, against the test-local oracle (tests/replay_oracle.py): the tree's shape and heap functions,
the chunks an ingest rebuilds, and the sampler -- the draws of k_replay_sample walked over the header's functions, equal to
the reference's sample loop pick for pick.  Exact; test-only build: the product itself has no CPU path."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import replay_oracle as RO  # noqa: E402
from host_build import build_shim  # noqa: E402

I64 = C.c_int64
P64 = C.POINTER(C.c_int64)
PF64 = C.POINTER(C.c_double)
PU8 = C.POINTER(C.c_uint8)
STAGE_LEVELS, SEG, CHUNK_LG = 13, 6, 11          # RP_STAGE_LEVELS, RP_SEG, RP_CHUNK_LG


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    lib = build_shim(tmp_path_factory, "host_sum_tree_shim.cpp")
    for name, res, args in (
            ("tree_levels", C.c_int, [I64]), ("tree_nodes", I64, [C.c_int]), ("level_first", I64, [C.c_int]),
            ("left_child", I64, [I64]), ("leaf_node", I64, [C.c_int, I64]), ("leaf_of_node", I64, [C.c_int, I64]),
            ("ancestor_at", I64, [C.c_int, I64, C.c_int]), ("first_leaf_under", I64, [C.c_int, I64, C.c_int]),
            ("chunk_lg", C.c_int, [C.c_int]), ("chunk_root_level", C.c_int, [C.c_int, C.c_int]),
            ("chunk_count", I64, [I64, C.c_int]), ("rebuilt_chunks", I64, [I64, C.c_int, I64, I64, PU8]),
            ("rebuilt_chunks_all", None, [I64, C.c_int, I64, PU8, P64]),
            ("staged_levels", C.c_int, [C.c_int]), ("seg_depth", C.c_int, [C.c_int, C.c_int]),
            ("seg_words", C.c_int, [C.c_int]), ("seg_slot", C.c_int, [C.c_int, C.c_int]),
            ("seg_child_index", C.c_int, [C.c_int, C.c_int]), ("levels_below", C.c_int, [C.c_int, C.c_int]),
            ("seg_child_node", I64, [I64, C.c_int, I64]), ("seg_source", I64, [I64, C.c_int]),
            ("seg_ancestor_slot", C.c_int, [I64, C.c_int, C.c_int]),
            ("sample", None, [PF64, C.c_int, C.c_int, C.c_int, PF64, P64, PF64, PF64])):
        fn = getattr(lib, "shim_" + name)
        fn.restype, fn.argtypes = res, args
        setattr(lib, name, fn)
    return lib


# ---------------------------------------------------------------- shape and heap functions
def test_tree_levels_is_the_references_count(shim):
    caps = {1, 2, 3, 37, 1000, 10 ** 6}
    for k in range(1, 27):
        caps |= {c for c in (2 ** k - 2, 2 ** k - 1, 2 ** k, 2 ** k + 1) if 1 <= c <= 2 ** 26}
    assert len(caps) > 100 and max(caps) == 2 ** 26
    for cap in sorted(caps):
        L = shim.tree_levels(cap)
        assert L == RO.levels(cap) == cap.bit_length() + 1, cap
        assert shim.tree_nodes(L) == 2 ** L - 1


def test_heap_functions_on_the_oracles_array(shim):
    """On the array RO.canonical builds: where a level starts, where the leaves lie, and that every internal node is the
    sum of the two nodes left_child names."""
    for cap in (1, 2, 3, 37, 1000, 5000):
        L = shim.tree_levels(cap)
        leaves = np.random.default_rng(cap).uniform(0.5, 2, cap)
        t = RO.canonical(leaves, cap)
        assert shim.tree_nodes(L) == t.size
        assert [shim.level_first(lvl) for lvl in range(L)] == [2 ** lvl - 1 for lvl in range(L)]
        assert shim.level_first(L) == t.size
        assert np.array_equal(t[shim.leaf_node(L, 0):shim.leaf_node(L, cap)], leaves) and not t[shim.leaf_node(L, cap):].any()
        assert shim.leaf_node(L, 0) == shim.level_first(L - 1)
        for n in range(shim.level_first(L - 1)):
            lc = shim.left_child(n)
            assert t[n] == t[lc] + t[lc + 1]
        for i in (0, cap - 1, cap // 2):
            assert shim.leaf_of_node(L, shim.leaf_node(L, i)) == i


def check_leaf(shim, L, i):
    """leaf_node, ancestor_at and first_leaf_under agree: the ancestors of leaf i are a chain of parents from its node to
    the root, each on its level, and leaf i lies among the 2^(L-1-lvl) leaves that start at first_leaf_under of each."""
    node = shim.leaf_node(L, i)
    assert shim.ancestor_at(L, i, L - 1) == node and shim.ancestor_at(L, i, 0) == 0
    for lvl in range(L - 1, -1, -1):
        a = shim.ancestor_at(L, i, lvl)
        assert a == node and shim.level_first(lvl) <= a < shim.level_first(lvl + 1), (L, i, lvl)
        first = shim.first_leaf_under(L, a, lvl)
        assert shim.levels_below(L, lvl) == L - 1 - lvl
        assert first <= i < first + (1 << (L - 1 - lvl)) and first % (1 << (L - 1 - lvl)) == 0, (L, i, lvl)
        assert shim.ancestor_at(L, first, lvl) == a
        node = (node - 1) // 2


def test_leaf_ancestor_and_first_leaf_are_mutually_consistent(shim):
    n = 0
    for L in range(2, 13):
        for i in range(1 << (L - 1)):
            check_leaf(shim, L, i)
            n += 1
    rng = np.random.default_rng(3)
    for L in (21, 28):
        for i in [0, (1 << (L - 1)) - 1] + [int(x) for x in rng.integers(0, 1 << (L - 1), 200)]:
            check_leaf(shim, L, i)
            n += 1
    assert n == 2 ** 12 - 2 + 404


# ---------------------------------------------------------------- rebuild chunks
def test_chunk_geometry_of_a_handle(shim):
    for cap, L, clg, nchunks in ((1, 2, 1, 1), (37, 7, 6, 1), (1000, 11, 10, 1), (2048, 13, 11, 1), (6148, 14, 11, 4),
                                 (10 ** 6, 21, 11, 489), (2 ** 26, 28, 11, 2 ** 15)):
        assert (shim.tree_levels(cap), shim.chunk_lg(L), shim.chunk_count(cap, clg)) == (L, clg, nchunks)
        assert shim.chunk_lg(L) == min(L - 1, CHUNK_LG) and shim.chunk_root_level(L, clg) == L - 1 - clg


def chunks_needed(cap, clg, cursor, span):
    """The chunks that hold a ring position of [cursor, cursor + min(span, cap)) modulo cap: those of the run up to the
    ring's end and of the run that wrapped."""
    end = cursor + min(span, cap)
    runs = [(cursor, min(end, cap))] + ([(0, end - cap)] if end > cap else [])
    return np.concatenate([np.arange(a >> clg, ((b - 1) >> clg) + 1) for a, b in runs])


@pytest.mark.parametrize("clg", (1, 2, 3, 4))
def test_rebuilt_chunks_contain_every_touched_chunk_exhaustively(shim, clg):
    cases = 0
    for cap in range(1, 201):
        nchunks, max_span = shim.chunk_count(cap, clg), cap + 3
        assert nchunks == -(-cap // (1 << clg))
        marks = np.zeros((cap, max_span, nchunks), np.uint8)
        grids = np.zeros(max_span, np.int64)
        shim.rebuilt_chunks_all(cap, clg, max_span, marks.ctypes.data_as(PU8), grids.ctypes.data_as(P64))
        assert (grids >= 1).all() and (grids <= nchunks).all(), (cap, clg)
        assert (marks.sum(axis=2) == grids[None, :]).all(), (cap, clg)     # `grid` distinct chunks
        # needed[cursor, k, c]: chunk c holds one of the first k + 1 positions from the cursor on
        chunk = ((np.arange(cap)[:, None] + np.arange(cap)[None, :]) % cap) >> clg
        needed = np.maximum.accumulate(chunk[:, :, None] == np.arange(nchunks)[None, None, :], axis=1)
        needed = needed[:, np.minimum(np.arange(1, max_span + 1), cap) - 1, :]
        assert not (needed & (marks == 0)).any(), (cap, clg)
        cases += cap * max_span
    assert cases == sum(c * (c + 3) for c in range(1, 201))


@pytest.mark.parametrize("cap", (6148, 10_000, 10 ** 6))
def test_rebuilt_chunks_contain_every_touched_chunk_at_the_products_chunk_size(shim, cap):
    clg = CHUNK_LG
    assert shim.chunk_lg(shim.tree_levels(cap)) == clg
    nchunks = shim.chunk_count(cap, clg)
    rng = np.random.default_rng(cap)
    for cursor in [0, cap - 1] + [int(x) for x in rng.integers(0, cap, 100)]:
        for span in (1, 1000, 3000, 524_288, cap):
            marks = np.zeros(nchunks, np.uint8)
            grid = shim.rebuilt_chunks(cap, clg, cursor, span, marks.ctypes.data_as(PU8))
            assert 1 <= grid <= nchunks and marks.sum() == grid
            assert marks[chunks_needed(cap, clg, cursor, span)].all(), (cap, cursor, span)


# ---------------------------------------------------------------- the sampler
def test_segment_layout(shim):
    """A segment holds the subtree under a node without the node, level by level; seg_source names where each slot is
    loaded from, seg_ancestor_slot the slot above a relative leaf."""
    assert [shim.staged_levels(L) for L in (2, 12, 13, 14, 28)] == [2, 12, 13, 13, 13]
    for L in (14, 15, 19, 20, 21, 28):
        depths, lvl = [], STAGE_LEVELS - 1
        while lvl < L - 1:
            depths.append(shim.seg_depth(L, lvl))
            lvl += depths[-1]
        assert lvl == L - 1 and all(d == SEG for d in depths[:-1]) and 1 <= depths[-1] <= SEG
    for depth in range(1, SEG + 1):
        assert shim.seg_words(depth) == 2 ** (depth + 1) - 2
        for node in (0, 1, 4095, 8190, 2 ** 21 + 12345):
            want, level = [], [node]
            for r in range(1, depth + 1):
                level = [c for n in level for c in (2 * n + 1, 2 * n + 2)]
                assert [shim.seg_slot(r, q) for q in range(2 ** r)] == list(range(len(want), len(want) + 2 ** r))
                assert [shim.seg_child_index(q, right) for q in range(2 ** (r - 1)) for right in (0, 1)] == list(range(2 ** r))
                assert [shim.seg_child_node(node, r, q) for q in range(2 ** r)] == level
                want += level
            assert [shim.seg_source(node, t) for t in range(shim.seg_words(depth))] == want
        for below in (depth, depth + 1, depth + SEG):
            for rel in {0, 1, 2 ** below - 1, 2 ** below // 3}:
                for r in range(1, depth + 1):
                    assert shim.seg_ancestor_slot(rel, below, r) == shim.seg_slot(r, rel >> (below - r))


def run_sampler(shim, tree, L, T, u):
    tree = np.ascontiguousarray(tree, np.float64)
    u = np.ascontiguousarray(u, np.float64)
    idx, prio, after = np.zeros(u.size, np.int64), np.zeros(u.size), np.zeros(tree.size)
    shim.sample(tree.ctypes.data_as(PF64), L, T, u.size, u.ctypes.data_as(PF64), idx.ctypes.data_as(P64),
                prio.ctypes.data_as(PF64), after.ctypes.data_as(PF64))
    return idx, prio, after


def segments_below(shim, L, T):
    out, lvl = [], T - 1
    while lvl < L - 1:
        out.append(shim.seg_depth(L, lvl))
        lvl += out[-1]
    return out


def check_sampler(shim, cap, segments, staged=None):
    """64 draws on the canonical tree of RO.segment_draws(cap): picks, priorities and the tree the draws leave are the
    oracle's, and -- where there are segments -- the oracle's picks do revisit a bottom segment."""
    leaves, u = RO.segment_draws(cap)
    assert u.size == 64 and u[0] == u[1] == 0.0 and u[62] == u[63] == 1 - 2.0 ** -53 and (u[0::2] == u[1::2]).all()
    tree = RO.canonical(leaves, cap)
    L = shim.tree_levels(cap)
    T = shim.staged_levels(L) if staged is None else staged
    assert segments_below(shim, L, T) == segments, (cap, L, T)
    oi, _, op, oafter = RO.sample_tree(tree, cap, u, 0.4)
    if segments:
        shared = RO.picks_sharing_the_bottom_segment(oi, cap, staged=T, seg=SEG)
        assert shared >= 5, f"capacity {cap}: only {shared} picks share a bottom segment with an earlier one"
    assert oi[0] == oi[1] == 0 and op[1] == 0.0
    idx, prio, after = run_sampler(shim, tree, L, T, u)
    assert np.array_equal(idx, oi), f"capacity {cap}: indices"
    assert np.array_equal(prio, op), f"capacity {cap}: priorities"
    assert np.array_equal(after, oafter), f"capacity {cap}: tree after the draws"


@pytest.mark.parametrize("cap,segments", [
    (1, []), (2, []), (3, []), (37, []), (1000, []), (4095, []), (4096, [1]), (8191, [1]), (8192, [2]), (40_000, [4]),
    (70_000, [5]), (300_000, [6, 1]), (10 ** 6, [6, 2]), (2 ** 22, [6, 5])])
def test_sampler_walk_equals_the_oracle_draw_by_draw(shim, cap, segments):
    check_sampler(shim, cap, segments)


def test_sampler_walk_through_three_segments(shim):
    """6 + 6 + 3 levels below the staged ones, as at the largest capacity (2^26: 28 levels), on a tree of 18 levels with 3
    of them staged."""
    assert segments_below(shim, shim.tree_levels(2 ** 26), STAGE_LEVELS) == [6, 6, 3]
    check_sampler(shim, 100_000, [6, 6, 3], staged=3)
