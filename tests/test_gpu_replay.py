"""The device replay memory (toric_rl_decoder_amd.PrioritizedReplayMemory, tq_replay_*) on an MI355X against the
test-local oracle (tests/replay_oracle.py) and the reference's recorded op sequences (tests/golden/replay_*.npz)."""
import glob
import os
import sys

import numpy as np
import pytest
import torch

import toric_rl_decoder_amd as T
from toric_rl_decoder_amd import wire

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import replay_oracle as RO  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GOLDEN = sorted(glob.glob(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "replay_*.npz")))


def ulps(a, b):
    """Distance in units in the last place of b."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.abs(a - b) / np.spacing(np.abs(b))


def synthetic_block(d, prios, seed=0, empty_every=0):
    """A packed block on the device with len(prios) slots: random planes / rewards / terminals, op 1..3, the given f32
    priorities; every empty_every-th slot empty (action word 0)."""
    rng = np.random.default_rng(seed)
    n = len(prios)
    per = rng.integers(0, 2, (n, 2, d, d), dtype=np.uint8)
    nxt = rng.integers(0, 2, (n, 2, d, d), dtype=np.uint8)
    act = np.stack([rng.integers(0, 2, n), rng.integers(0, d, n), rng.integers(0, d, n), rng.integers(1, 4, n)], 1)
    if empty_every:
        act[::empty_every] = 0
    buf = wire.encode(d, per, nxt, act, rng.normal(size=n).astype(np.float32), rng.integers(0, 2, n),
                      priority=np.asarray(prios, np.float32))
    return torch.from_numpy(buf).to(DEV)


def actor_blocks(d, n, steps, seed):
    """TransitionBlocks written by EnvSet.actorStep (pure exploration) with computePriorities from random Q-values."""
    env = T.make("toric-code-v0", {"size": d, "min_qubit_errors": 0, "p_error": 0.1})
    gpu = T.EnvSet(env, n, device=DEV, seed=seed, numpy_io=False)
    gpu.resetAll()
    blk = gpu.newTransitionBlock(steps=steps)
    for t in range(steps):
        gpu.actorStep(None, block=blk, slot=t)
    g = torch.Generator(device=DEV).manual_seed(seed)
    q = torch.rand((steps + 1, n, 3), generator=g, device=DEV, dtype=torch.float32) * 4 - 2
    blk.computePriorities(n, steps, q, 0.95)
    gpu.check()
    gpu.close()
    return blk


def decoded(buf, d, cap):
    return wire.decode(buf.cpu().numpy(), d, cap)


def assert_canonical(mem):
    tree = mem.tree().cpu().numpy()
    leaves = mem.leaves().cpu().numpy()
    assert np.array_equal(tree, RO.canonical(leaves, mem.memory_size)), "tree is not the canonical sum of its leaves"


def test_save_block_of_actor_blocks_matches_decode_in_ring_order():
    d, n, alpha, cap = 7, 256, 0.6, 1500
    mem = T.PrioritizedReplayMemory(cap, alpha, d=d, device=DEV, seed=3)
    ring = [None] * cap                                   # expected (row dict, priority) per ring position
    cursor, filled = 0, 0
    blocks = [actor_blocks(d, n, 4, 11), actor_blocks(d, n, 4, 12), actor_blocks(d, n, 8, 13)]
    # empty slots: clear the action words of every 7th slot of the first two blocks (consumers drop them)
    for b in blocks[:2]:
        off, _, _ = wire.sections(d, b.capacity)["action"]
        b.buf[off:off + 4 * b.capacity].view(torch.int32)[::7] = 0
    for b in blocks:                                      # 2nd: more than the free ring; 3rd: more than the capacity
        dec = decoded(b.buf, d, b.capacity)
        m = dec["action"].shape[0]
        assert m > 0
        for k in range(max(0, m - cap), m):
            ring[(cursor + k) % cap] = {key: v[k] for key, v in dec.items()}
        cursor, filled = (cursor + m) % cap, min(filled + m, cap)
        mem.save_block(b if b is not blocks[1] else b.buf)   # a TransitionBlock, or the raw bytes of a ring row
        assert mem.filled_size() == filled
    assert filled == cap and blocks[2].capacity > cap
    got = mem.get(torch.arange(cap, device=DEV))
    mem.check()
    exp = {key: np.stack([r[key] for r in ring]) for key in ring[0]}
    assert np.array_equal(got["state"].cpu().numpy(), exp["perspective"].astype(np.float32))
    assert np.array_equal(got["next_state"].cpu().numpy(), exp["next_perspective"].astype(np.float32))
    assert np.array_equal(got["action"].cpu().numpy(), exp["action"])
    assert np.array_equal(got["actions"].cpu().numpy(), exp["action"][:, 3].astype(np.int64) - 1)
    assert np.array_equal(got["reward"].cpu().numpy(), exp["reward"])
    assert np.array_equal(got["terminal"].cpu().numpy(), exp["terminal"])
    leaves = mem.leaves().cpu().numpy()
    want = np.float64(exp["priority"]) ** alpha
    assert np.all(ulps(leaves, want) <= 1.0), "leaf != float64(priority)**alpha within 1 ulp"
    assert_canonical(mem)
    mem.close()


def device_block(d, n, seed):
    """A packed block of n slots built on the device, every slot a transition: random planes, op 1..3, 0/1 terminals,
    f32 priorities uniform in [0.01, 10)."""
    g = torch.Generator(device=DEV).manual_seed(seed)
    buf = torch.randint(0, 256, (wire.block_bytes(d, n),), dtype=torch.uint8, device=DEV, generator=g)
    s = wire.sections(d, n)
    off = s["action"][0]
    buf[off:off + 4 * n].view(torch.int32).copy_(torch.randint(1, 4, (n,), dtype=torch.int32, device=DEV, generator=g) << 24)
    off = s["priority"][0]
    buf[off:off + 4 * n].view(torch.float32).uniform_(0.01, 10.0, generator=g)
    off = s["terminal"][0]
    buf[off:off + n].copy_(torch.randint(0, 2, (n,), dtype=torch.uint8, device=DEV, generator=g))
    return buf


@pytest.mark.parametrize("cap,m,saves", [(6148, 1000, 8), (10_000, 3000, 6), (10 ** 6, 65536 * 8, 6)])
def test_wrapping_ingests_over_several_chunks_keep_the_tree_canonical(cap, m, saves):
    """Capacities that are not a multiple of the 2048-leaf rebuild chunk, several chunks, blocks that wrap the ring:
    after every save the leaves are the saved priorities**alpha in ring order and the tree is canonical (the 10^6 case
    is the bench's shape)."""
    d, alpha = 3, 0.6
    mem = T.PrioritizedReplayMemory(cap, alpha, d=d, device=DEV, seed=4)
    want = np.zeros(cap)
    cursor, wrapped = 0, False
    for k in range(saves):
        b = device_block(d, m, seed=100 + k)
        mem.save_block(b)
        p = wire.view(b.cpu().numpy(), d, m)["priority"].astype(np.float64)
        want[(cursor + np.arange(m)) % cap] = p ** alpha
        wrapped |= cursor + m > cap
        cursor = (cursor + m) % cap
        assert mem.filled_size() == min((k + 1) * m, cap)
        assert np.all(ulps(mem.leaves().cpu().numpy(), want) <= 1.0), f"save {k}: leaves"
        assert_canonical(mem)
    assert wrapped
    mem.check()
    with pytest.raises(ValueError, match="memory on"):
        mem.save_block(T.TransitionBlock(d, 8, "cpu"))      # a block on another device is refused
    mem.close()


class _DeviceOps:
    def __init__(self, mem, d):
        self.mem, self.d, self.blocks = mem, d, 0

    def save_many(self, prios):
        self.blocks += 1
        self.mem.save_block(synthetic_block(self.d, prios, seed=self.blocks))

    def sample_u(self, u, beta):
        res = self.mem.sample(len(u), beta, uniforms=u)
        if res[0] is None:
            return None
        _, w, idx, p = res
        return idx, w, p

    def priority_update(self, idx, p):
        self.mem.priority_update(idx, p)

    def reset_alpha(self, a):
        self.mem.reset_alpha(a)


@pytest.mark.parametrize("path", GOLDEN, ids=[os.path.basename(p) for p in GOLDEN])
def test_golden_op_sequences_replay_on_the_device(path):
    g = np.load(path)
    mem = T.PrioritizedReplayMemory(int(g["capacity"]), float(g["alpha"]), d=5, device=DEV)
    RO.replay_golden(g, _DeviceOps(mem, 5), lambda ops: ops.mem.leaves().cpu().numpy())
    assert_canonical(mem)
    mem.check()
    mem.close()


@pytest.mark.parametrize("faithful", [True, False])
def test_philox_draws_match_the_oracle_on_the_devices_tree(faithful):
    d, cap, alpha, beta, seed = 3, 10 ** 6, 0.6, 0.4, 0x1234_5678_9ABC
    mem = T.PrioritizedReplayMemory(cap, alpha, d=d, device=DEV, seed=seed, faithful=faithful)
    rng = np.random.default_rng(5)
    mem.save_block(synthetic_block(d, rng.uniform(0.01, 10.0, 700_000), seed=1))
    assert mem.filled_size() == 700_000
    for call, B in enumerate((1, 16, 1024)):
        tree0 = mem.tree().cpu().numpy()
        leaves0 = mem.leaves().cpu().numpy()
        assert np.array_equal(tree0, RO.canonical(leaves0, cap))
        _, w, idx, p = mem.sample(B, beta)
        oi, ow, op, _ = RO.sample_tree(tree0, cap, RO.uniforms(seed, call, B), beta)
        assert np.array_equal(idx, oi), f"B={B}: indices"
        assert np.array_equal(p, op), f"B={B}: priorities"
        assert np.all(ulps(w, ow) <= 2.0), f"B={B}: weights"
        tree1, leaves1 = mem.tree().cpu().numpy(), mem.leaves().cpu().numpy()
        if not faithful:
            assert np.array_equal(tree1, tree0), "faithful=False: a sample must leave the tree untouched"
            continue
        want = leaves0.copy()
        for i, v in zip(oi, op):                          # the revert: leaf**alpha, last pick wins
            want[i] = float(v) ** alpha
        picked = np.zeros(cap, bool)
        picked[oi] = True
        assert np.array_equal(leaves1[~picked], leaves0[~picked])
        assert np.all(ulps(leaves1[picked], want[picked]) <= 1.0)
        assert np.array_equal(tree1, RO.canonical(leaves1, cap))
    mem.check()
    mem.close()


@pytest.mark.parametrize("cap,faithful", [(5000, True), (40_000, True), (40_000, False), (300_000, True)])
def test_draws_below_the_staged_levels_match_the_oracle(cap, faithful):
    """The smallest capacities whose levels below the staged ones are a lone short segment (1 level), a mid-depth one (4)
    and a full one followed by a short one (6 + 1), with draws that come back to segments earlier picks corrected."""
    d, alpha, beta = 3, 0.6, 0.4
    prios, u = RO.segment_draws(cap)
    mem = T.PrioritizedReplayMemory(cap, alpha, d=d, device=DEV, seed=7, faithful=faithful)
    mem.save_block(synthetic_block(d, prios, seed=cap))
    assert mem.filled_size() == cap
    tree0 = mem.tree().cpu().numpy()
    _, w, idx, p = mem.sample(u.size, beta, uniforms=u)
    oi, ow, op, _ = RO.sample_tree(tree0, cap, u, beta)
    shared = RO.picks_sharing_the_bottom_segment(oi, cap)
    assert shared >= 5, f"only {shared} of the oracle's picks share a bottom segment with an earlier one"
    assert np.array_equal(idx, oi), "indices"
    assert np.array_equal(p, op), "priorities"
    assert np.all(ulps(w, ow) <= 2.0), "weights"
    if not faithful:
        assert np.array_equal(mem.tree().cpu().numpy(), tree0), "faithful=False: a sample must leave the tree untouched"
    assert_canonical(mem)
    mem.check()
    mem.close()


def test_priority_update_last_occurrence_wins_and_tree_stays_canonical():
    d, cap, alpha = 5, 50_000, 0.7
    mem = T.PrioritizedReplayMemory(cap, alpha, d=d, device=DEV)
    mem.save_block(synthetic_block(d, np.random.default_rng(1).uniform(0.1, 2.0, 40_000)))
    before = mem.leaves().cpu().numpy()
    rng = np.random.default_rng(2)
    idx = rng.integers(0, 40_000, 300)
    idx = np.concatenate([idx, idx[:100], idx[:50]])      # listed two and three times
    p = rng.uniform(0.01, 3.0, idx.size)
    mem.update_priorities(torch.as_tensor(idx, device=DEV), torch.as_tensor(p, device=DEV))
    want = before.copy()
    for i, v in zip(idx, p):
        want[i] = v ** alpha
    got = mem.leaves().cpu().numpy()
    touched = np.zeros(cap, bool)
    touched[idx] = True
    assert np.array_equal(got[~touched], before[~touched])
    assert np.all(ulps(got[touched], want[touched]) <= 1.0)
    assert_canonical(mem)
    # a bulk update (every filled leaf) takes the full rebuild: canonical too
    mem.update_priorities(torch.arange(40_000, device=DEV), torch.full((40_000,), 0.5, device=DEV, dtype=torch.float64))
    assert np.all(ulps(mem.leaves().cpu().numpy()[:40_000], np.full(40_000, 0.5 ** alpha)) <= 1.0)
    assert_canonical(mem)
    mem.check()
    mem.update_priorities(torch.tensor([40_000], device=DEV), torch.tensor([1.0], device=DEV))
    with pytest.raises(ValueError, match="outside"):
        mem.check()
    mem.close()


def test_sample_batch_is_data_to_batch_and_one_learner_step_runs():
    d, cap, alpha, beta, B = 7, 4096, 0.6, 0.4, 256
    mem = T.PrioritizedReplayMemory(cap, alpha, d=d, device=DEV, seed=9)
    blk = actor_blocks(d, 512, 6, 21)
    mem.save_block(blk)
    tree0 = mem.tree().cpu().numpy()
    batch = mem.sample_batch(B, beta)
    state, actions, reward, next_state, terminal, weights, indices = batch
    assert [t.device.type for t in batch] == ["cuda"] * 7
    assert (state.dtype, actions.dtype, reward.dtype, next_state.dtype, terminal.dtype, weights.dtype, indices.dtype) == \
        (torch.float32, torch.int64, torch.float32, torch.float32, torch.bool, torch.float32, torch.int64)
    oi, ow, _, _ = RO.sample_tree(tree0, cap, RO.uniforms(9, 0, B), beta)
    assert np.array_equal(indices.cpu().numpy(), oi)
    g = mem.get(indices)
    rec = dict(perspective=g["state"].cpu().numpy().astype(np.uint8), next_perspective=g["next_state"].cpu().numpy().astype(np.uint8),
               action=g["action"].cpu().numpy(), reward=g["reward"].cpu().numpy(), terminal=g["terminal"].cpu().numpy())
    exp = RO.data_to_batch(rec, ow, oi)
    for got, want in zip(batch[:5], exp[:5]):
        assert np.array_equal(got.cpu().numpy(), want)
    assert np.all(np.abs(weights.cpu().numpy() - exp[5]) <= 2 * np.spacing(exp[5]))
    # one learner step (Learner_mp.py:134-169) on these tensors
    torch.manual_seed(0)
    net = torch.nn.Sequential(torch.nn.Flatten(), torch.nn.Linear(2 * d * d, 3)).to(DEV)
    out = net(state).gather(1, actions.view(-1, 1)).squeeze(1)
    target = T.predictMaxOptimized(net, next_state, d // 2, d, DEV)
    y = (reward + (~terminal).type(torch.float) * 0.95 * target).clamp(-100, 100)
    loss = weights * torch.nn.functional.mse_loss(y, out, reduction="none")
    pr = loss.abs().detach()
    leaves_before = mem.leaves().cpu().numpy()
    mem.update_priorities(indices, pr)
    want = leaves_before.copy()
    for i, v in zip(oi, pr.cpu().numpy()):
        want[i] = np.float64(v) ** alpha
    got = mem.leaves().cpu().numpy()
    assert np.all(ulps(got, want) <= 1.0)
    assert_canonical(mem)
    mem.check()
    mem.close()


def test_under_filled_sample():
    mem = T.PrioritizedReplayMemory(100, 0.6, d=3, device=DEV)
    mem.save_block(synthetic_block(3, np.full(10, 0.5)))
    assert mem.sample(16, 0.4) == (None, None, None)
    tree0 = mem.tree().cpu().numpy()
    idx = mem.sample_batch(16, 0.4)[6]
    with pytest.raises(T.ToricEnvError, match="fewer records"):
        mem.check()
    assert (idx.cpu().numpy() == -1).all()
    assert np.array_equal(mem.tree().cpu().numpy(), tree0)
    mem.check()                                           # the latch was cleared
    mem.close()
