"""The replay memory's contract without a GPU: the test-local oracle (tests/replay_oracle.py) reproduces every op the
imported reference recorded (tests/golden/replay_*.npz, make_replay_golden.py), and the tq_replay_* entry points of
the C-ABI reject bad arguments with error codes before touching a device."""
import ctypes as C
import glob
import os
import sys

import numpy as np
import pytest

import toric_rl_decoder_amd as T
from toric_rl_decoder_amd import _lib, replay, wire

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import replay_oracle as RO  # noqa: E402

GOLDEN = sorted(glob.glob(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "replay_*.npz")))


class _OracleOps(RO.OracleReplay):
    def save_many(self, prios):
        self.save(prios)

    def sample_u(self, u, beta):
        return self.sample(u, beta)


@pytest.mark.parametrize("path", GOLDEN, ids=[os.path.basename(p) for p in GOLDEN])
def test_oracle_reproduces_the_reference_op_sequences(path):
    assert len(GOLDEN) == 2 and 4 in np.load(GOLDEN[1])["kinds"]
    g = np.load(path)
    mem = _OracleOps(int(g["capacity"]), float(g["alpha"]))
    RO.replay_golden(g, mem, lambda m: m.leaves)


def test_oracle_tree_is_the_reference_shape_and_canonical():
    for cap, L in ((1, 2), (2, 3), (3, 3), (37, 7), (1000, 11), (1 << 20, 22), (10 ** 6, 21)):
        assert RO.levels(cap) == L
    leaves = np.random.default_rng(0).uniform(0, 2, 37)
    t = RO.canonical(leaves, 37)
    assert t.size == 127 and t[0] == t[1] + t[2] and np.array_equal(t[63:100], leaves) and not t[100:].any()
    for n in range(63):
        assert t[n] == t[2 * n + 1] + t[2 * n + 2]


def test_oracle_sampling_counts_a_picked_leaf_as_zero():
    leaves = np.array([1.0, 0.0, 3.0, 4.0])
    t = RO.canonical(leaves, 4)
    idx, w, p, after = RO.sample_tree(t, 4, [0.99, 0.99, 0.99], 0.4)
    assert idx.tolist() == [3, 2, 0] and p.tolist() == [4.0, 3.0, 1.0]
    assert after[0] == 0.0 and w.max() == 1.0
    idx, w, p, _ = RO.sample_tree(RO.canonical(np.zeros(4), 4), 4, [0.5], 0.4)
    assert idx.tolist() == [0] and w.tolist() == [0.0]          # the reference raises ZeroDivisionError here


def test_block_capacity_inverts_the_block_size():
    for d in (3, 7, 9, 21):
        for cap in (1, 2, 7, 8, 1000, 65536 * 8):
            assert replay.block_capacity(d, wire.block_bytes(d, cap)) == cap
    with pytest.raises(ValueError):
        replay.block_capacity(7, 12345)


def test_replay_entry_points_reject_bad_arguments_without_a_device():
    lib = _lib.load()
    h = C.c_void_p(None)
    for d, cap, alpha, faithful, what in ((7, 0, 0.6, 1, b"capacity"), (8, 100, 0.6, 1, b"lattice size"),
                                          (7, 100, -0.1, 1, b"alpha"), (7, (1 << 26) + 1, 0.6, 1, b"capacity"),
                                          (7, 100, float("nan"), 1, b"alpha"), (7, 100, 0.6, 2, b"faithful")):
        assert lib.tq_replay_create(C.byref(h), d, cap, alpha, 0, 1, faithful) == _lib.TQ_E_INVALID
        assert what in lib.tq_last_error() and not h.value
    assert lib.tq_replay_create(None, 7, 100, 0.6, 0, 1, 1) == _lib.TQ_E_INVALID
    assert lib.tq_replay_destroy(None) == 0
    null = None
    assert lib.tq_replay_save_block(null, None, 8, None) == _lib.TQ_E_INVALID
    assert b"NULL replay handle" in lib.tq_last_error()
    assert lib.tq_replay_filled(null, None) == _lib.TQ_E_INVALID
    assert lib.tq_replay_sample(null, 4, 0.4, *([None] * 11)) == _lib.TQ_E_INVALID
    assert lib.tq_replay_get(null, None, 4, *([None] * 7)) == _lib.TQ_E_INVALID
    assert lib.tq_replay_update(null, None, None, 4, None) == _lib.TQ_E_INVALID
    assert lib.tq_replay_reset_alpha(null, 0.5, None) == _lib.TQ_E_INVALID
    assert lib.tq_replay_leaves(null, None, None) == _lib.TQ_E_INVALID
    assert lib.tq_replay_tree(null, None, None) == _lib.TQ_E_INVALID
    assert lib.tq_replay_tree_nodes(null) == _lib.TQ_E_INVALID
    assert lib.tq_replay_check(null, None) == _lib.TQ_E_INVALID
    import torch
    if not torch.cuda.is_available():
        assert lib.tq_replay_create(C.byref(h), 7, 100, 0.6, 0, 1, 1) < 0 and lib.tq_last_error()
        with pytest.raises((T.ToricEnvError, ValueError)):
            T.PrioritizedReplayMemory(100, 0.6, d=7)
