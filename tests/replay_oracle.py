"""Test-local oracle of the device replay memory (toric-rl-decoder_amd/replay.py).

* the canonical sum tree: the reference's shape (src/SumTree.py: L = ceil(log2(capacity+1)) + 1 levels, heap order,
  leaf i = record i), every internal node fl(left + right), built level by level from the leaves;
* a literal restatement of PrioritizedReplayMemory.sample over SumTree (src/ReplayMemory.py:85-124, SumTree.find /
  val_update / reconstruct): the += diff updates, on a copy of a given tree;
* dataToBatch (src/util_learner.py:7-46) over decoded records.
"""
import math

import numpy as np

from oracle.toric_oracle import philox4x32


def levels(capacity):
    return math.ceil(math.log(capacity + 1, 2)) + 1


def canonical(leaves, capacity):
    """f64 tree (2^L - 1 nodes) whose leaf i is leaves[i] (i < capacity; the rest 0) and whose internal nodes are the
    pairwise sums, bottom up."""
    L = levels(capacity)
    tree = np.zeros((1 << L) - 1, np.float64)
    base = (1 << (L - 1)) - 1
    tree[base:base + capacity] = np.asarray(leaves, np.float64)[:capacity]
    for lvl in range(L - 2, -1, -1):
        lo, n = (1 << lvl) - 1, 1 << lvl
        ch = tree[2 * lo + 1:2 * lo + 1 + 2 * n]
        tree[lo:lo + n] = ch[0::2] + ch[1::2]
    return tree


def sample_tree(tree, capacity, uniforms, beta):
    """PrioritizedReplayMemory.sample on a copy of ``tree`` with the draws ``uniforms`` -> (indices, weights,
    priorities, tree after the draws, before the revert).  Weights that are all 0 come back as zeros (the reference
    raises ZeroDivisionError)."""
    t = np.asarray(tree, np.float64).tolist()
    L = levels(capacity)
    base = (1 << (L - 1)) - 1
    idx, pri, w = [], [], []
    for r in uniforms:
        value = float(r) * t[0]                       # SumTree.find, norm=True
        i = 0
        while i < base:                               # SumTree._find
            left = t[2 * i + 1]
            if value <= left:
                i = 2 * i + 1
            else:
                value -= left
                i = 2 * (i + 1)
        v = t[i]
        pri.append(v)
        w.append((1. / capacity / v) ** beta if v > 1e-16 else 0)
        idx.append(i - base)
        diff = 0.0 - t[i]                             # priority_update([index], [0]) -> val_update -> reconstruct
        while True:
            t[i] += diff
            if i == 0:
                break
            i = int((i - 1) / 2)
    m = max(w)
    w = [x / m for x in w] if m > 0 else [0.0] * len(w)
    return np.array(idx, np.int64), np.array(w, np.float64), np.array(pri, np.float64), np.array(t, np.float64)


class OracleReplay:
    """The device memory's contract on the host: leaves + canonical tree, ring cursor, the two quirks."""

    def __init__(self, capacity, alpha, faithful=True):
        self.capacity, self.alpha, self.faithful = int(capacity), float(alpha), bool(faithful)
        self.leaves = np.zeros(self.capacity, np.float64)
        self.cursor = self.filled = 0

    def tree(self):
        return canonical(self.leaves, self.capacity)

    def save(self, priorities):
        for p in priorities:
            self.leaves[self.cursor] = float(p) ** self.alpha
            self.cursor = (self.cursor + 1) % self.capacity
            self.filled = min(self.filled + 1, self.capacity)

    def set_leaves(self, leaves, filled, cursor=0):
        self.leaves = np.array(leaves, np.float64)
        self.filled, self.cursor = int(filled), int(cursor)

    def sample(self, uniforms, beta):
        if self.filled < len(uniforms):
            return None
        idx, w, pri, _ = sample_tree(self.tree(), self.capacity, uniforms, beta)
        if self.faithful:
            self.priority_update(idx, pri)            # the reference's "revert" (ReplayMemory.py:119)
        return idx, w, pri

    def priority_update(self, indices, priorities):
        for i, p in zip(indices, priorities):         # last occurrence wins
            self.leaves[int(i)] = float(p) ** self.alpha

    def reset_alpha(self, alpha):
        old, self.alpha = self.alpha, float(alpha)
        e = -old if self.faithful else 1.0 / old
        for i in range(self.filled):
            v = float(self.leaves[i])
            if v != 0.0:
                self.leaves[i] = (v ** e) ** self.alpha


def data_to_batch(records, weights, indices):
    """dataToBatch (util_learner.py:7-46) over a dict of decoded records (perspective / next_perspective u8 (n,2,d,d),
    action i32 (n,4), reward, terminal) -> numpy (state f32, actions i64 = op - 1, reward f32, next_state f32,
    terminal bool, weights f32, indices)."""
    return (np.asarray(records["perspective"]).astype(np.float32),
            np.asarray(records["action"])[:, 3].astype(np.int64) - 1,
            np.asarray(records["reward"]).astype(np.float32),
            np.asarray(records["next_perspective"]).astype(np.float32),
            np.asarray(records["terminal"]).astype(bool),
            np.asarray(weights).astype(np.float32),
            indices)


def uniforms(seed, call, n):
    """The draws of a handle's own stream (RNG domain 5): Philox4x32-10 keyed by the seed, counter
    (call lo, call hi, 0, 5<<24 | k), u = ((w0>>5) * 2^26 + (w1>>6)) * 2^-53."""
    k = np.arange(n, dtype=np.uint64)
    w0, w1, _, _ = philox4x32(call & 0xFFFFFFFF, call >> 32, 0, (5 << 24) | k, seed & 0xFFFFFFFF, seed >> 32)
    return ((w0 >> 5).astype(np.float64) * 67108864.0 + (w1 >> 6).astype(np.float64)) * (1.0 / 9007199254740992.0)


def segment_draws(capacity):
    """Inputs that send the sampler's later picks below the staged levels into subtrees that earlier picks already
    corrected -> (leaf values in [0.01, 10) with a tenth of them 0, 64 uniforms).  The uniforms come in equal pairs; the
    first pair is 0.0 (leaf 0 twice, the second time at priority 0 and weight 0), the last the largest double below 1."""
    rng = np.random.default_rng(capacity)
    leaves = rng.uniform(0.01, 10, capacity)
    leaves[rng.random(capacity) < 0.1] = 0.0
    u = np.repeat(rng.uniform(0, 1, 32), 2)
    u[0] = u[1] = 0.0
    u[62] = u[63] = 1 - 2.0 ** -53
    return leaves, u


def picks_sharing_the_bottom_segment(indices, capacity, staged=13, seg=6):
    """How many of the picks lie under the same bottom segment of the sampler as an earlier pick: the levels below the
    top ``staged`` ones are walked in subtrees of depth ``seg`` and a last one of what remains (0 without segments)."""
    below = levels(capacity) - staged
    if below <= 0:
        return 0
    roots = [int(i) >> ((below - 1) % seg + 1) for i in indices]
    return sum(r in roots[:k] for k, r in enumerate(roots))


def close(a, b, rel=1e-12):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return a.shape == b.shape and bool(np.all(np.abs(a - b) <= rel * np.maximum(np.abs(b), 1e-300)))


def replay_golden(g, mem, leaves_of):
    """Runs the op sequence of golden file ``g`` through ``mem`` (oracle or device memory); checks every result."""
    kinds = g["kinds"]
    assert len(kinds) >= 10 and {0, 1, 2, 3} <= set(kinds.tolist()) <= {0, 1, 2, 3, 4}
    for k, kind in enumerate(kinds):
        if kind == 0:
            mem.save_many(g[f"{k}_prio"])
        elif kind == 1:
            idx, w, p = mem.sample_u(g[f"{k}_u"], float(g[f"{k}_beta"]))
            assert np.array_equal(idx, g[f"{k}_idx"]), f"op {k}: indices"
            assert close(w, g[f"{k}_w"]) and close(p, g[f"{k}_p"]), f"op {k}: weights / priorities"
        elif kind == 2:
            mem.priority_update(g[f"{k}_idx"], g[f"{k}_p"])
        elif kind == 3:
            mem.reset_alpha(float(g[f"{k}_alpha"]))
        elif kind == 4:
            assert mem.sample_u(np.zeros(int(g[f"{k}_B"])), float(g[f"{k}_beta"])) is None, f"op {k}: under-filled"
        assert close(leaves_of(mem), g[f"{k}_leaves"]), f"op {k}: leaves"
