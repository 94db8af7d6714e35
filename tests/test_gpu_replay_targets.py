"""The learner's target side straight from the device replay memory on an MI355X: PrioritizedReplayMemory.
next_perspectives (tq_replay_next_persp_count / _write), policy.td_target (tq_td_target) and policy.learnerTargets
against the path they replace -- mem.get's f32 next_state -> generatePerspectiveBatch -> segment_max -> the torch
target expression -- and against the oracle.  Every comparison is exact."""
import os
import sys

import numpy as np
import pytest
import torch

import toric_rl_decoder_amd as T
from oracle import toric_oracle as O
from toric_rl_decoder_amd import wire
from toric_rl_decoder_amd._lib import _ptr
from toric_rl_decoder_amd.envset import _DTYPES

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import replay_oracle as RO  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SIZES = (3, 5, 7, 9, 13, 17, 21)
LENGTHS = (1, 33, 256, 4096)
ALL_DTYPES = (torch.float32, torch.float16, torch.bfloat16, torch.uint8)


def actor_block(d, n, steps, seed, min_errors):
    """A TransitionBlock written by EnvSet.actorStep (pure exploration).  min_errors = 1: every episode starts from one
    error, so a good share of the random actions end it -- real terminal records, whose next syndrome is empty;
    min_errors = 0: depolarizing noise of about eight errors per lattice."""
    p = min(0.1, 8.0 / (2 * d * d))
    env = T.make("toric-code-v0", {"size": d, "min_qubit_errors": min_errors, "p_error": p})
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


def synthetic_block(d, n, seed):
    """A packed block of n transitions with random next planes of a few defects each; every fifth next syndrome is
    forced empty.  The terminal bytes are random: empty next syndromes with terminal 0 and non-empty ones with
    terminal 1 both occur."""
    rng = np.random.default_rng(seed)
    per = (rng.random((n, 2, d, d)) < 3.0 / (d * d)).astype(np.uint8)
    nxt = (rng.random((n, 2, d, d)) < 3.0 / (d * d)).astype(np.uint8)
    nxt[::5] = 0
    nxt[1] = 1                                            # one full syndrome: 2 d^2 perspectives
    act = np.stack([rng.integers(0, 2, n), rng.integers(0, d, n), rng.integers(0, d, n), rng.integers(1, 4, n)], 1)
    buf = wire.encode(d, per, nxt, act, rng.normal(size=n).astype(np.float32), rng.integers(0, 2, n),
                      priority=rng.uniform(0.01, 10.0, n).astype(np.float32))
    return torch.from_numpy(buf).to(DEV)


_memories = {}
FULL = 2 * 2048 + 1                                       # ring position of the synthetic block's record 1


def filled_memory(d):
    """One memory per size for the whole module: two actor-written blocks and a synthetic one, not full."""
    if d not in _memories:
        mem = T.PrioritizedReplayMemory(8192, 0.6, d=d, device=DEV, seed=d)
        mem.save_block(actor_block(d, 256, 8, 100 + d, 1))
        mem.save_block(actor_block(d, 256, 8, 200 + d, 0))
        mem.save_block(synthetic_block(d, 3000, 300 + d))
        mem.check()
        assert mem.filled_size() == 2 * 2048 + 3000       # every slot of the three blocks holds a transition
        _memories[d] = (mem, mem.filled_size())
    return _memories[d]


def index_list(rng, filled, n):
    idx = rng.integers(0, filled, n)
    if n > 1:
        idx[n // 2] = idx[0]                              # a repeat
        idx[-1] = FULL                                    # the full synthetic syndrome
    return torch.as_tensor(idx, dtype=torch.int64, device=DEV)


def old_path(mem, idx, dtype=torch.float32):
    d = mem.size
    return T.generatePerspectiveBatch(d // 2, d, mem.get(idx)["next_state"], dtype=dtype, device=DEV, return_offsets=True)


def assert_same(got, want, what):
    names = ("stack", "positions", "counts", "offsets")
    for g, w, name in zip(got, want, names):
        assert g.dtype == w.dtype and g.shape == w.shape, f"{what}: {name} {g.dtype}{tuple(g.shape)} != {w.dtype}{tuple(w.shape)}"
        raw = torch.int16 if g.dtype in (torch.float16, torch.bfloat16) else g.dtype
        assert torch.equal(g.view(raw), w.view(raw)), f"{what}: {name}"


def assert_oracle(got, next_state, what):
    """Against oracle.generate_perspective_batch, in chunks of states (the oracle gathers through an index array)."""
    stack, pos, counts, offsets = (t.cpu() for t in got)
    ns = next_state.cpu().numpy().astype(np.uint8)
    off = offsets.numpy()
    for c0 in range(0, ns.shape[0], 512):
        c1 = min(c0 + 512, ns.shape[0])
        per, opos, ocnt, ooff = O.generate_perspective_batch(ns[c0:c1])
        assert np.array_equal(counts.numpy()[c0:c1], ocnt), what
        assert np.array_equal(off[c0:c1 + 1] - off[c0], ooff), what
        assert np.array_equal(stack[off[c0]:off[c1]].float().numpy(), per.astype(np.float32)), what
        assert np.array_equal(pos.numpy()[off[c0]:off[c1]], opos), what


@pytest.mark.parametrize("d", SIZES)
def test_next_perspectives_equal_the_stack_of_the_expanded_next_states_bit_for_bit(d):
    mem, filled = filled_memory(d)
    rng = np.random.default_rng(d)
    everything = mem.get(torch.arange(filled, device=DEV))
    empty = ~everything["next_state"].flatten(1).any(1)
    actor_rows = torch.arange(filled, device=DEV) < 4096
    assert bool((empty & actor_rows & everything["terminal"]).any()), "no real terminal record among the actors'"
    assert bool((empty & ~everything["terminal"]).any()) and bool((~empty & everything["terminal"]).any())
    for n in LENGTHS:
        idx = index_list(rng, filled, n)
        if n == 1:
            idx = torch.nonzero(~empty)[:1, 0].contiguous()
        for dtype in (ALL_DTYPES if d in (7, 9) else (torch.float32,)):
            what = f"d={d} n={n} {dtype}"
            got = mem.next_perspectives(idx, dtype=dtype)
            mem.check()
            assert_same(got, old_path(mem, idx, dtype), what)
            if dtype in (torch.float32, torch.uint8):
                assert_oracle(got, mem.get(idx)["next_state"], what)
            assert bool((got[2][empty[idx]] == 0).all()) and bool((got[2][~empty[idx]] > 0).all()), what
    # a single record without a next syndrome: an empty stack, no launch of the writer
    one = torch.nonzero(empty)[:1, 0].contiguous()
    stack, pos, counts, offsets = mem.next_perspectives(one)
    assert stack.shape == (0, 2, d, d) and pos.shape == (0, 3) and counts.tolist() == [0] and offsets.tolist() == [0, 0]
    mem.check()


def test_indices_outside_the_filled_records_count_zero_and_latch():
    d = 7
    mem, filled = filled_memory(d)
    idx = torch.tensor([FULL, filled, 5, -1, 8192 + 100, FULL, -(1 << 40), 17], dtype=torch.int64, device=DEV)
    bad = torch.tensor([0, 1, 0, 1, 1, 0, 1, 0], dtype=torch.bool, device=DEV)
    got = mem.next_perspectives(idx)
    with pytest.raises(ValueError, match="outside"):
        mem.check()
    mem.check()                                           # the latch was cleared
    assert bool((got[2][bad] == 0).all())
    # the other rows are what they are without the bad ones: the stack of the good indices alone
    want = mem.next_perspectives(idx[~bad].contiguous())
    mem.check()
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]) and torch.equal(got[2][~bad], want[2])
    assert_same(want, old_path(mem, idx[~bad].contiguous()), "good rows")
    with pytest.raises(ValueError):
        mem.next_perspectives(torch.zeros(4097, dtype=torch.int64, device=DEV))
    # the -1 indices of an under-filled sample_batch
    small = T.PrioritizedReplayMemory(100, 0.6, d=3, device=DEV)
    small.save_block(synthetic_block(3, 10, 1))
    sampled = small.sample_batch(16, 0.4, next_state=False)
    assert sampled[3] is None and (sampled[6] == -1).all()
    with pytest.raises(T.ToricEnvError, match="fewer records"):
        small.check()
    stack, pos, counts, offsets = small.next_perspectives(sampled[6])
    assert stack.shape[0] == 0 and not counts.any() and not offsets.any()
    with pytest.raises(ValueError, match="outside"):
        small.check()
    small.check()
    small.close()


def _raw_write(mem, idx, offsets, out, pos, capacity):
    mem._call(mem._L.tq_replay_next_persp_write, _ptr(idx), int(idx.numel()), _ptr(offsets), _ptr(out), _ptr(pos),
              int(capacity), _DTYPES[out.dtype])


@pytest.mark.parametrize("d,dtype", [(7, torch.float32), (5, torch.uint8), (9, torch.bfloat16)])
def test_capacity_shortfall_and_foreign_offsets(d, dtype):
    mem, filled = filled_memory(d)
    rng = np.random.default_rng(50 + d)
    idx = index_list(rng, filled, 256)                    # ends on the full syndrome: the last lattice has 2 d^2 perspectives
    stack, pos, counts, offsets = mem.next_perspectives(idx, dtype=dtype)
    mem.check()
    P, tail = int(offsets[-1]), 64
    last = int(offsets[-2])
    assert P - last == 2 * d * d
    other = index_list(np.random.default_rng(77), filled, 256)
    foreign = {"shifted by one record": torch.cat([offsets[1:], offsets[-1:]]).contiguous(),
               "of another index list": mem.next_perspectives(other, dtype=dtype)[3],
               "all zeros": torch.zeros_like(offsets)}
    assert not torch.equal(foreign["of another index list"], offsets)
    cap = max([P] + [int(b[-1] - b[0]) for b in foreign.values()]) + 8       # no foreign stack is short of capacity
    raw_t = torch.uint8 if dtype == torch.uint8 else torch.int16 if dtype != torch.float32 else torch.int32
    sent = 0x5A if dtype == torch.uint8 else 0x5A5A
    out = torch.empty((cap + tail, 2, d, d), dtype=dtype, device=DEV)
    opos = torch.empty((out.shape[0], 3), dtype=torch.int32, device=DEV)
    raw = out.view(raw_t)

    def canary():
        raw.fill_(sent)
        opos.fill_(-7)

    # one perspective short: the lattices that fit whole are written, the last one is skipped
    canary()
    _raw_write(mem, idx, offsets, out, opos, P - 1)
    with pytest.raises(T.ToricEnvError, match="capacity"):
        mem.check()
    assert torch.equal(raw[:last], stack.view(raw_t)[:last]) and torch.equal(opos[:last], pos[:last])
    assert bool((raw[last:] == sent).all()) and bool((opos[last:] == -7).all())
    mem.check()
    # offsets that are not the scan of these records' counts
    for name, bad in foreign.items():
        canary()
        _raw_write(mem, idx, bad, out, opos, cap)
        with pytest.raises(ValueError, match="offsets"):
            mem.check()
        stop = min(int(bad[-1] - bad[0]), cap)            # nothing stored outside [0, min(P, capacity)) perspectives
        assert bool((raw[stop:] == sent).all()) and bool((opos[stop:] == -7).all()), name
        mem.check()
    # the handle is as good as new
    again = mem.next_perspectives(idx, dtype=dtype)
    mem.check()
    assert_same(again, (stack, pos, counts, offsets), "after the refused writes")


def torch_target(q, offsets, reward, terminal, discount, lo=-100.0, hi=100.0):
    counts = offsets[1:] - offsets[:-1]
    largest = torch.clamp(counts.max(), min=1).to(torch.int32).reshape(1)
    target = T.segment_max(q, offsets, largest)
    return (reward + (~terminal).type(torch.float) * discount * target).clamp(lo, hi)


@pytest.mark.parametrize("n", [1, 33, 256, 1024, 4096, 20001])
def test_td_target_is_the_torch_expression_bit_for_bit(n):
    g = torch.Generator(device=DEV).manual_seed(n)
    for case in ("mixed", "all negative", "every slice empty", "one long slice"):
        counts = torch.randint(0, 60, (n,), device=DEV, generator=g)
        if case == "every slice empty":
            counts.zero_()
        if case == "one long slice":
            counts[n // 2] = 98
        offsets = torch.zeros(n + 1, dtype=torch.int64, device=DEV)
        offsets[1:] = torch.cumsum(counts, 0)
        P = int(offsets[-1])
        q = torch.randn((P, 3), device=DEV, generator=g) * 40
        if case != "mixed":
            q = -q.abs() - 0.25                           # negative-only slices: the zero-padding quirk decides
        reward = torch.randn(n, device=DEV, generator=g) * 30
        terminal = torch.rand(n, device=DEV, generator=g) < 0.3       # set on non-empty states too
        for discount, lo, hi in ((0.95, -100.0, 100.0), (0.5, -7.0, 3.0)):
            y = T.td_target(q, offsets, reward, terminal, discount, lo, hi)
            want = torch_target(q, offsets, reward, terminal, discount, lo, hi)
            assert y.dtype == torch.float32 and y.shape == (n,)
            assert np.array_equal(y.cpu().numpy(), want.cpu().numpy()), (n, case, discount)
        if case == "all negative" and n > 1:
            live = T.td_target(q, offsets, torch.zeros_like(reward), torch.zeros_like(terminal), 1.0)
            short = (counts > 0) & (counts < counts.max())
            assert bool((live[short] == 0).all()) and bool((live[counts == counts.max()] < 0).all())


def assert_canonical(mem):
    tree = mem.tree().cpu().numpy()
    leaves = mem.leaves().cpu().numpy()
    assert np.array_equal(tree, RO.canonical(leaves, mem.memory_size)), "tree is not the canonical sum of its leaves"


def test_one_learner_step_takes_its_targets_from_the_ring():
    """The set-up of test_sample_batch_is_data_to_batch_and_one_learner_step_runs (tests/test_gpu_replay.py)."""
    d, cap, alpha, beta, B = 7, 4096, 0.6, 0.4, 256
    blk = actor_block(d, 512, 6, 21, 0)
    mem = T.PrioritizedReplayMemory(cap, alpha, d=d, device=DEV, seed=9)
    twin = T.PrioritizedReplayMemory(cap, alpha, d=d, device=DEV, seed=9)
    mem.save_block(blk)
    twin.save_block(blk)
    u = RO.uniforms(9, 0, B)
    state, actions, reward, next_state, terminal, weights, indices = mem.sample_batch(B, beta, uniforms=u)
    lean = twin.sample_batch(B, beta, uniforms=u, next_state=False)
    assert lean[3] is None
    for k in (0, 1, 2, 4, 5, 6):
        assert lean[k].dtype == (state, actions, reward, None, terminal, weights, indices)[k].dtype
        assert torch.equal(lean[k], (state, actions, reward, None, terminal, weights, indices)[k]), k
    assert np.array_equal(twin.leaves().cpu().numpy(), mem.leaves().cpu().numpy())
    twin.check()
    twin.close()
    torch.manual_seed(0)
    net = torch.nn.Sequential(torch.nn.Flatten(), torch.nn.Linear(2 * d * d, 3)).to(DEV)
    out = net(state).gather(1, actions.view(-1, 1)).squeeze(1)
    target = T.predictMaxOptimized(net, next_state, d // 2, d, DEV)
    y_old = (reward + (~terminal).type(torch.float) * 0.95 * target).clamp(-100, 100)
    y = T.learnerTargets(net, mem, indices, reward, terminal, discount=0.95)
    mem.check()
    assert y.dtype == torch.float32 and np.array_equal(y.cpu().numpy(), y_old.cpu().numpy())
    assert bool((y != reward).any())
    loss = weights * torch.nn.functional.mse_loss(y, out, reduction="none")
    pr = loss.abs().detach()
    leaves_before = mem.leaves().cpu().numpy()
    mem.update_priorities(indices, pr)
    want = leaves_before.copy()
    for i, v in zip(indices.cpu().numpy(), pr.cpu().numpy()):
        want[i] = np.float64(v) ** alpha
    got = mem.leaves().cpu().numpy()
    assert np.all(np.abs(got - want) <= np.spacing(np.abs(want)))
    assert_canonical(mem)
    mem.check()
    mem.close()
