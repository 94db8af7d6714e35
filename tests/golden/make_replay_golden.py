#!/usr/bin/env python3
"""Generate tests/golden/replay_*.npz from the IMPORTED reference replay memory (src/ReplayMemory.py, src/SumTree.py).

Runs only where the reference tree is (TORIC_REFERENCE, default as in make_golden.py); the files it writes are data.
Each file is one op sequence on one PrioritizedReplayMemory(capacity, alpha):
  kinds[k]  0 save (k_prio: the priorities saved one by one, f32-representable, passed as Python floats)
            1 sample (k_B, k_beta, k_u: the uniforms random.random() gave; k_idx, k_w, k_p: indices, weights,
              priorities it returned)
            2 priority_update (k_idx, k_p; with duplicate indices)
            3 reset_alpha (k_alpha)
            4 under-filled sample (k_B, k_beta: the reference returned (None, None, None))
  k_leaves  all leaves of the reference's tree after op k (f64[capacity]).
Every recorded draw is asserted to lie at least 1e-9 * root away from every boundary it was compared with, so that the
indices are meaningful for a tree summed in another order.
"""
import os
import random
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get("TORIC_REFERENCE", "/root/reference")
sys.dont_write_bytecode = True
sys.path.insert(0, REF)

import src.ReplayMemory as RM    # noqa: E402  (reference)

MARGIN = 1e-9


class Recorder:
    """random.random as the reference calls it (ReplayMemory.py:110), from a seeded generator, recorded."""

    def __init__(self, seed):
        self.rng = random.Random(seed)
        self.drawn = []

    def __call__(self):
        u = self.rng.random()
        self.drawn.append(u)
        return u


def instrument(tree):
    """Wraps SumTree._find of this instance: asserts the draw's distance to every boundary it is compared with."""
    orig = tree._find
    base = 2 ** (tree.tree_level - 1) - 1

    def _find(value, index):
        if index < base:
            left = tree.tree[2 * index + 1]
            assert abs(value - left) >= MARGIN * tree.tree[0], ("draw too close to a boundary", value, left)
        return orig(value, index)
    tree._find = _find


def run(path, capacity, alpha, ops, seed):
    rec = Recorder(seed)
    RM.random.random = rec
    prio_rng = np.random.default_rng(seed)
    mem = RM.PrioritizedReplayMemory(capacity, alpha)
    instrument(mem.tree)
    base = 2 ** (mem.tree.tree_level - 1) - 1
    out, kinds, saved = {}, [], 0
    for k, op in enumerate(ops):
        kind = op[0]
        if kind == "save":
            pr = [float(np.float32(x)) for x in prio_rng.uniform(0.05, 5.0, op[1])]
            for p in pr:
                mem.save(saved, p)
                saved += 1
            kinds.append(0)
            out[f"{k}_prio"] = np.array(pr, np.float64)
        elif kind == "sample":
            B, beta = op[1], op[2]
            rec.drawn = []
            res = mem.sample(B, beta)
            assert len(res) == 4, "expected a full sample"
            data, w, idx, p = res
            assert list(data) == [mem.tree.data[i] for i in idx]
            kinds.append(1)
            out[f"{k}_B"], out[f"{k}_beta"] = np.int64(B), np.float64(beta)
            out[f"{k}_u"] = np.array(rec.drawn, np.float64)
            out[f"{k}_idx"] = np.array(idx, np.int64)
            out[f"{k}_w"] = np.array(w, np.float64)
            out[f"{k}_p"] = np.array(p, np.float64)
        elif kind == "update":
            n = op[1]
            filled = mem.filled_size()
            idx = [int(i) for i in prio_rng.integers(0, filled, n)]
            idx += idx[: n // 4]                           # duplicates: the last occurrence must win
            p = [float(x) for x in prio_rng.uniform(0.01, 3.0, len(idx))]
            mem.priority_update(idx, p)
            kinds.append(2)
            out[f"{k}_idx"], out[f"{k}_p"] = np.array(idx, np.int64), np.array(p, np.float64)
        elif kind == "reset_alpha":
            mem.reset_alpha(op[1])
            kinds.append(3)
            out[f"{k}_alpha"] = np.float64(op[1])
        elif kind == "underfilled":
            B, beta = op[1], op[2]
            assert mem.filled_size() < B
            assert mem.sample(B, beta) == (None, None, None)
            kinds.append(4)
            out[f"{k}_B"], out[f"{k}_beta"] = np.int64(B), np.float64(beta)
        out[f"{k}_leaves"] = np.array([float(x) for x in mem.tree.tree[base:base + capacity]], np.float64)
    out["kinds"] = np.array(kinds, np.int64)
    out["capacity"], out["alpha"] = np.int64(capacity), np.float64(alpha)
    np.savez_compressed(path, **out)
    print(path, len(kinds), "ops")


def main():
    run(os.path.join(HERE, "replay_cap37.npz"), 37, 0.6,
        [("underfilled", 4, 0.4), ("save", 3), ("underfilled", 8, 0.4), ("save", 20), ("sample", 8, 0.4),
         ("update", 12), ("save", 40), ("sample", 16, 0.4), ("sample", 37, 0.4), ("reset_alpha", 0.7),
         ("sample", 5, 0.4), ("update", 8), ("save", 90), ("sample", 12, 0.4)], seed=37)
    run(os.path.join(HERE, "replay_cap1000.npz"), 1000, 0.6,
        [("save", 600), ("sample", 64, 0.4), ("update", 100), ("save", 700), ("sample", 256, 0.4),
         ("reset_alpha", 0.5), ("sample", 32, 0.4), ("update", 40), ("sample", 1000, 0.4), ("save", 2500),
         ("sample", 128, 0.4)], seed=1000)


if __name__ == "__main__":
    main()
