"""The stack write's slot decision without a GPU: what a workgroup of k_persp_stream adds to its pair's word and which of
the pair's two slots it takes (toric-rl-decoder_amd/csrc/stream_range.hpp: pair_claim, slot_fine_parts), built with g++
through tests/host_stream_slots_shim.cpp.  The contract, stated here: workgroups b and b ^ 1 share one word that is zero
between launches; whatever the two prefer and whoever arrives first, they take different kinds, the first gets what it
prefers, the word is zero again afterwards, and a word that did not start at zero does not go unnoticed.  Exact;
test-only build: the product itself has no CPU path."""
import ctypes as C
import itertools

import numpy as np
import pytest
from hypothesis import given, settings, strategies as st

from host_build import build_shim

G, RR = 256, 32
_lib = None


def load(tmp_path_factory):
    global _lib
    if _lib is None:
        lib = build_shim(tmp_path_factory, "host_stream_slots_shim.cpp")
        lib.shim_pair_claim.restype = None
        lib.shim_pair_claim.argtypes = [C.c_uint32, C.c_int, C.c_void_p]
        lib.shim_launch.restype = C.c_int
        lib.shim_launch.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
        lib.shim_pair_word_stride.restype = C.c_int
        lib.shim_pair_set_words.restype = C.c_int
        lib.shim_pair_set_words.argtypes = [C.c_int]
        _lib = lib
    return _lib


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    return load(tmp_path_factory)


def claim(shim, old, prefers_large):
    out = np.full(3, -7, np.int32)
    shim.shim_pair_claim(old, prefers_large, out.ctypes.data_as(C.c_void_p))
    return int(out[0]), int(out[1]), bool(out[2])


def launch(shim, order, prefers, words, bias=5):
    """The launch of the shim: (refused, kind[G], lo_hi[G, 2]); `words` is updated in place."""
    order = np.ascontiguousarray(order, np.int32)
    prefers = np.ascontiguousarray(prefers, np.int32)
    kind = np.full(prefers.size, -7, np.int32)
    lo_hi = np.full((prefers.size, 2), -7, np.int32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    refused = shim.shim_launch(order.size, p(order), p(prefers), p(words), RR, bias, p(kind), p(lo_hi))
    return refused, kind, lo_hi


def test_what_a_workgroup_adds_and_the_layout_of_the_words(shim):
    assert claim(shim, 0, 0)[0] == 1 and claim(shim, 0, 1)[0] == 3            # 1 + 2 * prefers_large, whatever the word held
    assert all(claim(shim, old, pl)[0] == 1 + 2 * pl for old in range(9) for pl in (0, 1))
    assert shim.shim_pair_word_stride() * 4 == 128                            # one word per pair, on a 128-byte line of its own
    assert shim.shim_pair_set_words(256) * 4 == 16 << 10                      # 128 lines, 16 KB per set


@pytest.mark.parametrize("prefs", list(itertools.product((0, 1), repeat=2)))
@pytest.mark.parametrize("order", [(0, 1), (1, 0)])
def test_a_pair_takes_two_different_kinds_and_leaves_its_word_zero(shim, prefs, order):
    words = np.zeros(1, np.uint32)
    refused, kind, lo_hi = launch(shim, order, prefs, words)
    assert refused == 0 and sorted(kind.tolist()) == [0, 1], (prefs, order, kind)
    assert kind[order[0]] == prefs[order[0]]                                  # the first arriver gets what it prefers
    if prefs[0] != prefs[1]:
        assert kind.tolist() == list(prefs)                                   # and so does the second if the two differ
    assert words[0] == 0
    # the same, step by step, through pair_claim alone
    first, second = order
    add1, k1, s1 = claim(shim, 0, prefs[first])
    add2, k2, s2 = claim(shim, add1, prefs[second])
    assert (k1, s1) == (prefs[first], False) and (k2, s2) == (1 - k1, True)
    # a second launch over the same word decides again from scratch
    refused, kind2, _ = launch(shim, order[::-1], prefs, words)
    assert refused == 0 and sorted(kind2.tolist()) == [0, 1] and kind2[order[1]] == prefs[order[1]] and words[0] == 0


@pytest.mark.parametrize("start", list(range(1, 10)) + [0x7FFFFFFF, 0xFFFFFFFF])
def test_a_word_that_does_not_start_at_zero_is_reported(shim, start):
    """A launch that finds a pair's word at anything but 0 must not pass for a good one: a workgroup refuses (the kernel
    latches ERR_INTERNAL), or the word is not zero afterwards (what the GPU tests read back after every case) -- in
    either interleaving a device allows: the second arriver's store of 0 lands before the other's add, or after it."""
    for prefs in itertools.product((0, 1), repeat=2):
        for order in ((0, 1), (1, 0)):
            words = np.array([start], np.uint32)
            refused, kind, _ = launch(shim, order, prefs, words)
            assert refused > 0 or words[0] != 0, (start, prefs, order, kind)
            # both adds first, the stores afterwards
            a, b = order
            add_a, kind_a, sec_a = claim(shim, start, prefs[a])
            add_b, kind_b, sec_b = claim(shim, (start + add_a) & 0xFFFFFFFF, prefs[b])
            word = 0 if (sec_a or sec_b) else (start + add_a + add_b) & 0xFFFFFFFF
            assert kind_a < 0 or kind_b < 0 or word != 0, (start, prefs, order)


@settings(max_examples=120, deadline=None)
@given(bias=st.integers(0, 16), seed=st.integers(0, 2**31 - 1), irregular=st.integers(0, 40))
def test_pair_local_shares_partition_the_fine_parts_whatever_the_dispatch(tmp_path_factory, bias, seed, irregular):
    """256 workgroups on any XCD assignment (round-robin from any start, or up to 40 of them anywhere), their atomics in
    any arrival order, two launches over the same words: the ranges [f_lo, f_hi) are a partition of the 8192 fine parts,
    nobody refuses, the words end zero, and under pure round-robin dispatch every workgroup on an even XCD holds a large
    slot."""
    shim = load(tmp_path_factory)
    rng = np.random.default_rng(seed)
    start = int(rng.integers(0, 8))
    xcd = (start + np.arange(G)) % 8
    if irregular:
        xcd[rng.choice(G, irregular, replace=False)] = rng.integers(0, 8, irregular)
    prefers = (xcd % 2 == 0).astype(np.int32)
    words = np.zeros(G // 2, np.uint32)
    for _ in range(2):
        refused, kind, lo_hi = launch(shim, rng.permutation(G), prefers, words, bias)
        assert refused == 0 and not words.any()
        covered = np.zeros(G * RR, np.int32)
        for b in range(G):
            lo, hi = lo_hi[b]
            assert lo // (2 * RR) == b // 2 and hi - lo == (RR + bias if kind[b] else RR - bias)    # inside its own pair
            covered[lo:hi] += 1
        assert (covered == 1).all()
        assert (kind.reshape(-1, 2).sum(1) == 1).all()
        if not irregular:
            assert np.array_equal(kind, prefers)
