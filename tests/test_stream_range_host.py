"""The stack write's range arithmetic without a GPU: which bytes a workgroup of k_persp_stream owns
(toric-rl-decoder_amd/csrc/stream_range.hpp), built with g++ through tests/host_stream_range_shim.cpp, against the
contract stated here in numpy: the workgroups' stack and positions intervals tile the output in whole 128-byte lines,
a range's origin is the line that holds its first element, need_extra is the fewest perspectives that fill its last
lines, and the slots' fine parts tile the table.  Exact; test-only build: the product itself has no CPU path."""
import ctypes as C

import numpy as np
import pytest

from host_build import build_shim
I64 = np.int64
WGS = 8
P_ALL = (0, 1, 2, 3, 10, 11, 43, 1000, 100003)
FIELDS = ("org", "head", "a0", "a1", "porg", "phead", "pa0", "pa1", "need_extra", "last", "has_stack", "has_pos")


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    lib = build_shim(tmp_path_factory, "host_stream_range_shim.cpp")
    lib.shim_stream_range.restype = None
    lib.shim_stream_range.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_int, C.c_void_p]
    lib.shim_slot_fine_parts.restype = None
    lib.shim_slot_fine_parts.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]
    return lib


def compiled(shim, cuts, p_all, nq, size, want_pos):
    """The header's StreamRange of every workgroup [cuts[g], cuts[g + 1]) as a dict of int64 arrays."""
    q0, q1 = np.ascontiguousarray(cuts[:-1], I64), np.ascontiguousarray(cuts[1:], I64)
    out = np.full((q0.size, len(FIELDS)), -7, I64)
    shim.shim_stream_range(q0.size, q0.ctypes.data_as(C.c_void_p), q1.ctypes.data_as(C.c_void_p), p_all, nq, size,
                           int(want_pos), out.ctypes.data_as(C.c_void_p))
    return {f: out[:, j] for j, f in enumerate(FIELDS)}


def cut_sets(p_all):
    """0 = Q[0] <= ... <= Q[8] = p_all: equal parts, everything in the last range, everything in the first, and seeded
    random cuts drawn with repeats from a few places and their neighbours (empty ranges, and ranges of one or two
    perspectives that begin and end inside one 128-byte line)."""
    ends = lambda inner: np.concatenate(([0], np.sort(np.asarray(inner, I64)), [p_all])).astype(I64)
    yield ends([p_all * k // WGS for k in range(1, WGS)])
    yield ends([0] * (WGS - 1))
    yield ends([p_all] * (WGS - 1))
    for seed in range(9):
        rng = np.random.default_rng(1000 * seed + p_all % 997)
        base = rng.integers(0, p_all + 1, 3)
        pool = np.clip(np.concatenate((base, base + 1, base + 2)), 0, p_all)
        yield ends(rng.choice(pool, WGS - 1))


def assert_tiling(start, end, has, total, line, what):
    """Taken in order, the intervals [start, end) of the workgroups that have one are contiguous, disjoint and cover
    [0, total); they begin on a line and end on a line or where the output ends."""
    assert ((end > start) == has).all(), what
    s, e = start[has], end[has]
    if total == 0:
        assert s.size == 0, what
        return
    assert s.size and s[0] == 0 and e[-1] == total, what
    assert (s[1:] == e[:-1]).all(), what
    assert (s % line == 0).all() and ((e % line == 0) | (e == total)).all(), what


@pytest.mark.parametrize("size", (1, 2, 4))
@pytest.mark.parametrize("d", (3, 5, 7, 9, 21))
def test_workgroup_ranges_tile_the_stack_and_the_positions_in_whole_lines(shim, d, size):
    nq, le = 2 * d * d, 128 // size
    n_ranges = 0
    for want_pos in (False, True):
        for p_all in P_ALL:
            for cuts in cut_sets(p_all):
                what = (d, size, want_pos, p_all, cuts.tolist())
                assert cuts[0] == 0 and cuts[-1] == p_all and (np.diff(cuts) >= 0).all() and cuts.size == WGS + 1
                q0, q1 = cuts[:-1], cuts[1:]
                r = compiled(shim, cuts, p_all, nq, size, want_pos)
                n_ranges += q0.size
                assert (r["last"] == (q1 >= p_all)).all(), what
                # 1. stack tiling, in elements, lines of `le`
                assert_tiling(r["org"] + r["a0"], r["org"] + r["a1"], r["has_stack"] != 0, p_all * nq, le, what)
                # 2. positions tiling, in dwords, lines of 32
                if want_pos:
                    assert_tiling(r["porg"] + r["pa0"], r["porg"] + r["pa1"], r["has_pos"] != 0, 3 * p_all, 32, what)
                else:
                    assert not r["has_pos"].any(), what
                # 3. origin: the line that holds the range's first element / dword
                assert (r["org"] % le == 0).all() and (r["org"] + r["head"] == q0 * nq).all(), what
                assert ((0 <= r["head"]) & (r["head"] < le)).all(), what
                assert (r["porg"] % 32 == 0).all() and (r["porg"] + r["phead"] == 3 * q0).all(), what
                assert ((0 <= r["phead"]) & (r["phead"] < 32)).all(), what
                # 4. need_extra: the smallest k >= 0 with which the producers reach the end of the last lines
                want = np.full(q0.size, -1, I64)
                for k in range(40, -1, -1):
                    ok = (q1 + k) * nq >= r["org"] + r["a1"]
                    if want_pos:
                        ok &= 3 * (q1 + k) >= r["porg"] + r["pa1"]
                    want[ok] = k
                assert (want >= 0).all() and (r["need_extra"] == want).all(), what
                assert (q1 + r["need_extra"] <= p_all).all(), what
    assert n_ranges == 2 * len(P_ALL) * 12 * WGS


@pytest.mark.parametrize("rr", (2, 32))
def test_slots_fine_parts_tile_the_table(shim, rr):
    pairs = WGS // 2
    for bias in range(rr):
        got = []
        for idx in range(pairs):
            for large in (1, 0):
                lo_hi = np.full(2, -7, np.int32)
                shim.shim_slot_fine_parts(large, idx, rr, bias, lo_hi.ctypes.data_as(C.c_void_p))
                assert lo_hi[1] - lo_hi[0] == (rr + bias if large else rr - bias), (rr, bias, idx, large)
                got.append(tuple(int(x) for x in lo_hi))
        got.sort()
        assert got[0][0] == 0 and got[-1][1] == WGS * rr, (rr, bias)
        assert all(a[1] == b[0] for a, b in zip(got, got[1:])), (rr, bias, got)
