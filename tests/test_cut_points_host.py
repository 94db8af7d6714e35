"""The stack write's cut points without a GPU (toric-rl-decoder_amd/csrc/cut_points.hpp), built with g++ through
tests/host_cut_points_shim.cpp, against the contract stated here in numpy: cut point k of a stack of P perspectives is the
first lattice e with offsets[e] >= (P * k) >> LG.  The scan's table (k_scan_final) holds all of them, every entry written
exactly once, under a header that tells whose table it is.  Exact; test-only build: the product itself has no CPU path.
(find_cut, the stack write's own search for two cut points where there is no table, stays a device function: the GPU tests
of lattice ranges and of cloned offsets hold it against the same contract.)"""
import ctypes as C

import numpy as np
import pytest

from host_build import build_shim
I64 = np.int64
SENTINEL = -7
P64 = C.POINTER(C.c_int64)
P32 = C.POINTER(C.c_int32)


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    lib = build_shim(tmp_path_factory, "host_cut_points_shim.cpp")
    lib.shim_cut_target.restype = C.c_int64
    lib.shim_cut_target.argtypes = [C.c_int64, C.c_int64, C.c_int]
    lib.shim_cut_floor.restype = C.c_int64
    lib.shim_cut_floor.argtypes = [C.c_int64, C.c_int64, C.c_int]
    lib.shim_cut_table_words.restype = C.c_int64
    lib.shim_cut_table_words.argtypes = [C.c_int]
    lib.shim_cut_header_words.restype = C.c_int
    lib.shim_cut_header_words.argtypes = []
    lib.shim_scan_table.restype = None
    lib.shim_scan_table.argtypes = [P64, C.c_int64, C.c_int, P32, P32]
    lib.shim_cut_header_matches.restype = C.c_int
    lib.shim_cut_header_matches.argtypes = [P32, C.c_int, C.c_int64, C.c_int64, C.c_int64]
    return lib


TOTALS = [0, 1, 2, 255, 256, 257, 100003, 2**31 - 1, 2**31, 2**40 + 12345, 2**50 - 1]


def totals_and_rng():
    rng = np.random.default_rng(5)
    return TOTALS + [int(x) for x in rng.integers(0, 2**50, 20)], rng


def test_cut_target_is_the_floor_of_the_kth_share(shim):
    totals, rng = totals_and_rng()
    for lg in (0, 1, 8, 13):
        for total in totals:
            for k in {0, 1, 2, (1 << lg) // 2, (1 << lg) - 1, 1 << lg} | {int(x) for x in rng.integers(0, (1 << lg) + 1, 8)}:
                assert shim.shim_cut_target(total, k, lg) == (total * k) >> lg, (total, k, lg)


def test_cut_floor_is_the_last_part_whose_target_is_not_above_x(shim):
    """cut_floor(total, x, LG) = the largest k in [0, G] with (total * k) >> LG <= x.  The targets do not decrease with k,
    so that is: k's target is not above x, and k is G or the next target is above x."""
    totals, rng = totals_and_rng()
    n = 0
    for lg in (0, 1, 8, 13):
        g = 1 << lg
        target = lambda total, k: (total * k) >> lg
        for total in totals:
            ks = {0, 1, 2, g // 2, g - 1, g} | {int(x) for x in rng.integers(0, g + 1, 8)}
            xs = {0, 1, total - 1, total}
            for k in ks:
                xs |= {target(total, k) - 1, target(total, k), target(total, k) + 1}
            for x in sorted(x for x in xs if x >= 0):
                k = shim.shim_cut_floor(total, x, lg)
                assert 0 <= k <= g and target(total, k) <= x and (k == g or target(total, k + 1) > x), (total, x, lg, k)
                n += 1
    assert n > 2000


def want_cuts(offsets, lg):
    """The contract: for k = 0..G the first e with offsets[e] >= (P * k) >> LG (P * G < 2^63 in every case here)."""
    p = int(offsets[-1])
    assert p << lg < 2**63
    targets = (I64(p) * np.arange((1 << lg) + 1, dtype=I64)) >> I64(lg)
    return np.searchsorted(offsets, targets, side="left")


def check_table(shim, offsets, lg, what):
    """One scan of `offsets` into a sentinel-filled table: every entry written exactly once and right, and the header
    names this stack and no other."""
    offsets = np.ascontiguousarray(offsets, I64)
    n, g, p = offsets.size - 1, 1 << lg, int(offsets[-1])
    words = shim.shim_cut_table_words(lg)
    assert words == g + 1 + shim.shim_cut_header_words()
    table = np.full(words, SENTINEL, np.int32)
    writes = np.zeros(g + 1, np.int32)
    shim.shim_scan_table(offsets.ctypes.data_as(P64), n, lg, table.ctypes.data_as(P32), writes.ctypes.data_as(P32))
    assert (table != SENTINEL).all(), what
    assert (writes == 1).all(), (what, np.flatnonzero(writes != 1)[:8], writes[writes != 1][:8])
    assert (table[:g + 1] == want_cuts(offsets, lg)).all(), what
    matches = lambda p_tab, e_begin, e_end: bool(shim.shim_cut_header_matches(table.ctypes.data_as(P32), lg, p_tab, e_begin, e_end))
    assert matches(p, 0, n), what
    for other_p in (p + 1, p - 1, p + 2**32, p - 2**32, p ^ 1):            # (the table stores P in two words)
        assert not matches(other_p, 0, n), (what, other_p)
    assert not matches(p, 0, n + 1) and not matches(p, 0, n - 1), what
    assert not matches(p, 1, n) and not matches(p, 1, n + 1), what


def count_distributions(n, rng):
    """Eight make-ups of the counts of n lattices (a lattice of d = 21 has at most 882 perspectives)."""
    one_hot = lambda i, v: np.bincount([i], [v], n).astype(I64)
    yield "all zero", np.zeros(n, I64)
    yield "all one", np.ones(n, I64)
    yield "random in 0..98", rng.integers(0, 99, n)
    yield "random in 0..882", rng.integers(0, 883, n)
    yield "1 % non-zero", rng.integers(1, 883, n) * (rng.random(n) < 0.01)
    yield "one lattice holding 882", one_hot(int(rng.integers(0, n)), 882)
    yield "only the last lattice", one_hot(n - 1, int(rng.integers(1, 883)))
    yield "only the first lattice", one_hot(0, int(rng.integers(1, 883)))


@pytest.mark.parametrize("lg", (3, 8, 13))
@pytest.mark.parametrize("n", (1, 7, 8, 9, 2047, 2048, 2049, 5000))
def test_scan_table_has_every_cut_point_written_once_under_a_header_that_names_it(shim, n, lg):
    rng = np.random.default_rng(100 * n + lg)
    names = []
    for name, counts in count_distributions(n, rng):
        assert counts.shape == (n,) and (counts >= 0).all() and (counts <= 882).all()
        check_table(shim, np.concatenate(([0], np.cumsum(counts, dtype=I64))), lg, (n, lg, name))
        names.append(name)
    assert len(names) == 8


@pytest.mark.parametrize("lg", (3, 13))
def test_scan_table_of_a_stack_around_2_to_the_31_and_2_to_the_40(shim, lg):
    """Synthetic offsets (no batch of counts sums so high with so few lattices): the header's two words and the 64-bit
    targets."""
    rng = np.random.default_rng(77 + lg)
    n_cases = 0
    for p in (2**31 - 1, 2**31, 2**31 + 1, 2**32 - 1, 2**32, 2**32 + 5, 2**40 - 1, 2**40, 2**40 + 12345):
        for n in (1, 3, 9, 20):
            inner = np.sort(rng.integers(0, p + 1, n - 1))
            check_table(shim, np.concatenate(([0], inner, [p])), lg, (p, n, lg, "random"))
            check_table(shim, np.concatenate((np.zeros(n, I64), [p])), lg, (p, n, lg, "all in the last lattice"))
            n_cases += 2
    assert n_cases == 72
