"""The two ends of a step that are not the streaming of the stack (on a real MI355X, ``pytest -m gpu``):

* the START of a stack-write launch: a workgroup takes its range from the scan's cut-point table (k_scan_final) -- the
  same bytes as when it finds its cut points itself -- and a table that does not belong to the offsets (the header
  behind the cut points says so) is never followed silently;
* "write(t) is done": the event the two-stream loop waits for is signalled by the write's own dispatch
  (tq_persp_write_signal), and the plain tq_persp_write is still what a HIP graph captures.

Every comparison is byte exact.
"""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

P_OF = {3: 0.1, 5: 0.1, 7: 0.12, 9: 0.15, 21: 0.06}
BIG = 64 << 20            # bytes of stack from which the unequal shares (slot counters) apply: d >= 7, 2- and 4-byte elements


@pytest.fixture(scope="module")
def T():
    import toric_rl_decoder_amd as T
    assert torch.cuda.is_available(), "these tests need the GPU"
    assert os.path.exists(T.LIB_PATH), "libtoricenv.so must be built (no fallback path exists)"
    T.load()
    return T


def make_envs(T, d, n, p=None, seed=99):
    env = T.make("toric-code-v0", {"size": d, "min_qubit_errors": 0, "p_error": P_OF[d] if p is None else p})
    return T.EnvSet(env, n, seed=seed, numpy_io=False)


def write(gpu, offsets, capacity, dtype, fill=7):
    """One stack write into fresh buffers of ``capacity`` + 8 perspectives filled with a sentinel -> (stack, positions)."""
    d = gpu.size
    stack = torch.full((capacity + 8, 2, d, d), fill, dtype=dtype, device=gpu.device)
    pos = torch.full((capacity + 8, 3), -1, dtype=torch.int32, device=gpu.device)
    gpu.writePerspectives(stack[:capacity], pos[:capacity], offsets)
    return stack, pos


# lattices per case: "small" stays below 64 MB of stack (equal shares), "large" is above it -- where, for d >= 7 and f32,
# the workgroups take their shares through the slot counters (bias 5)
N_OF = {(3, "small"): 3000, (3, "large"): 200000, (7, "small"): 2000, (7, "large"): 24576,
        (9, "small"): 800, (9, "large"): 8192, (21, "small"): 40, (21, "large"): 1024}


@pytest.mark.parametrize("dtype", [torch.float32, torch.uint8])
@pytest.mark.parametrize("shape", ["small", "large"])
@pytest.mark.parametrize("d", [3, 7, 9, 21])
def test_range_from_the_scans_tables_equals_the_range_found_by_the_workgroups(T, d, shape, dtype):
    """tq_persp_write with the offsets tensor the scan wrote (the handle's cut-point table) against the same
    offsets cloned into another tensor (no table for that pointer: find_cut): stack, positions and the sentinel behind them
    are equal byte for byte -- also when the stack does not fit the buffer, and when it is empty."""
    L = T._lib.load()
    n, nq = N_OF[(d, shape)], 2 * d * d
    esize = torch.empty((), dtype=dtype).element_size()
    default = L.tq_get_xcd_bias()
    gpu = make_envs(T, d, n)
    try:
        assert L.tq_set_xcd_bias(5) == 0
        gpu.resetAll()
        for _ in range(2):
            gpu.actorStep(None, want_actions=False)
        _, offsets = gpu.perspectiveCounts()
        P = int(offsets[-1].item())
        assert P > 256
        if shape == "small":
            assert P * nq * esize < BIG
        elif d >= 7 and esize == 4:
            assert P * nq * esize >= BIG                     # the slot path
        found = offsets.clone()
        a, apos = write(gpu, offsets, P, dtype)
        gpu.check()
        b, bpos = write(gpu, found, P, dtype)
        gpu.check()
        assert torch.equal(a, b) and torch.equal(apos, bpos)
        assert bool((a[P:] == 7).all()) and bool((apos[P:] == -1).all())
        assert int(apos[:P].min()) >= 0 and int((a[:P] != 0).sum()) > 0      # something was written
        # the stack does not fit: the lattices that fit whole are written, both ways, and the overflow is latched
        cap = P // 2
        a, apos = write(gpu, offsets, cap, dtype)
        with pytest.raises(T.ToricEnvError):
            gpu.check()
        b, bpos = write(gpu, found, cap, dtype)
        with pytest.raises(T.ToricEnvError):
            gpu.check()
        assert torch.equal(a, b) and torch.equal(apos, bpos)
        assert bool((a[cap:] == 7).all()) and bool((apos[cap:] == -1).all())
        # an empty stack: nothing is written and nothing is latched, both ways
        gpu.setQubits(torch.zeros((n, 2, d, d), dtype=torch.uint8, device=gpu.device))
        _, offsets = gpu.perspectiveCounts()
        assert int(offsets[-1].item()) == 0
        a, apos = write(gpu, offsets, 64, dtype)
        b, bpos = write(gpu, offsets.clone(), 64, dtype)
        gpu.check()
        assert bool((a == 7).all()) and bool((b == 7).all()) and bool((apos == -1).all()) and bool((bpos == -1).all())
    finally:
        L.tq_set_xcd_bias(default)
        gpu.close()


def sparse_qubits(n, d, hot, seed):
    rng = np.random.default_rng(seed)
    q = np.zeros((n, 2, d, d), np.uint8)
    where = rng.choice(n, hot, replace=False)
    q[where, rng.integers(0, 2, hot), rng.integers(0, d, hot), rng.integers(0, d, hot)] = rng.integers(1, 4, hot)
    return torch.as_tensor(q, device="cuda")


@pytest.mark.parametrize("d,n", [(7, 24576), (5, 6000)])
def test_a_table_that_does_not_belong_to_the_offsets_is_never_followed_silently(T, d, n):
    """The handle matches a table to the offsets POINTER.  A caller who fills a scanned tensor with another (correct) scan
    hands the write correct offsets and a stale table: all zero (the tensor was scanned for an empty stack), or of an
    earlier stack, larger or smaller.  The write gives the correct stack or TQ_E_INVALID at tq_check -- never an unwritten
    stack without an error (the table's header tells the write that the table is not the one of these offsets, and the
    workgroups find their cut points themselves)."""
    gpu = make_envs(T, d, n)
    try:
        gpu.resetAll()
        gpu.actorStep(None, want_actions=False)
        full = gpu.getQubits().clone()
        x = torch.zeros(n + 1, dtype=torch.int64, device=gpu.device)
        y = torch.zeros(n + 1, dtype=torch.int64, device=gpu.device)

        def correct_or_refused(stale, want_offsets):
            P = int(want_offsets[-1].item())
            ref, rpos = write(gpu, want_offsets.clone(), P, torch.float32)          # no table: the workgroups' own cut points
            gpu.check()
            assert int((ref[:P] != 0).sum()) > 0
            got, gpos = write(gpu, stale, P, torch.float32)
            try:
                gpu.check()
            except ValueError:
                assert bool((got[P:] == 7).all()) and bool((gpos[P:] == -1).all())
                return "refused"
            assert torch.equal(got, ref) and torch.equal(gpos, rpos)
            return "correct"

        # (a) an all-zero table: x was scanned for the empty stack, then receives the scan of the full lattices
        gpu.setQubits(torch.zeros_like(full))
        gpu.perspectiveCounts(x)
        assert int(x[-1].item()) == 0
        gpu.setQubits(full)
        gpu.perspectiveCounts(y)
        x.copy_(y)
        print("all-zero table:", correct_or_refused(x, y))
        # (b) the table of an earlier, larger stack: x scanned for the full lattices, then receives the scan of a sparse state
        gpu.perspectiveCounts(x)
        gpu.setQubits(sparse_qubits(n, d, 700, seed=d))
        gpu.perspectiveCounts(y)
        assert 256 < int(y[-1].item()) < int(x[-1].item())
        x.copy_(y)
        print("table of a larger stack:", correct_or_refused(x, y))
        # ... and of an earlier, smaller one
        gpu.perspectiveCounts(x)
        gpu.setQubits(full)
        gpu.perspectiveCounts(y)
        x.copy_(y)
        print("table of a smaller stack:", correct_or_refused(x, y))
        # the handle is as good as new
        gpu.perspectiveCounts(x)
        P = int(x[-1].item())
        got, gpos = write(gpu, x, P, torch.float32)
        ref, rpos = write(gpu, x.clone(), P, torch.float32)
        gpu.check()
        assert torch.equal(got, ref) and torch.equal(gpos, rpos)
    finally:
        gpu.close()


@pytest.mark.parametrize("d,n,chunks", [(7, 16384, 1), (9, 4096, 4)])
def test_explore_loop_with_the_writes_own_completion_event_equals_the_serial_loop(T, d, n, chunks):
    """T.ExploreLoop(overlap=True) orders step(t+1) behind write(t) by an event that write(t)'s own dispatch signals (for a
    stack written in ranges: the last range's).  160 free-running passes leave, step for step, the same stack and
    positions (integer checksums on the write's stream), the same flushed blocks and the same final lattices and
    counters as the loop on ONE stream."""
    steps, flush, nq = 160, 8, 2 * d * d
    runs = []
    for overlap in (True, False):
        gpu = make_envs(T, d, n, seed=4321)
        gpu.resetAll()
        cap = (n // chunks) * nq
        stack = torch.zeros((cap, 2, d, d), dtype=torch.float32, device=gpu.device)
        pos = torch.zeros((cap, 3), dtype=torch.int32, device=gpu.device)
        offs = torch.zeros((steps + 2, (n + 2) & ~1), dtype=torch.int64, device=gpu.device)
        blocks = [gpu.newTransitionBlock(steps=flush) for _ in range(2)]
        flushed = []
        loop = T.ExploreLoop(gpu, stack, pos, offs, blocks=blocks, flush=flush, chunks=chunks, overlap=overlap,
                             on_flush=lambda b: flushed.append(b.buf.clone()))
        assert loop.overlap == overlap
        if overlap:
            assert all(isinstance(e, T._lib.WriteEvent) for e in loop.written)
        sums = torch.zeros((steps, 2), dtype=torch.int64, device=gpu.device)
        for t in range(steps):
            loop.step()
            sums[t, 0] = stack.view(torch.int32).sum(dtype=torch.int64)      # on the write's stream, behind write(t)
            sums[t, 1] = pos.sum(dtype=torch.int64)
        loop.drain()
        torch.cuda.synchronize()
        gpu.check()
        ep, st = gpu.getCounters()
        runs.append(dict(sums=sums.cpu(), P=offs[:steps, n].cpu(), flushed=[f.cpu() for f in flushed], qubits=gpu.getQubits().cpu(),
                         states=gpu.getStates().cpu(), ep=ep.cpu(), st=st.cpu(), stack=stack.cpu(), pos=pos.cpu()))
        gpu.close()
    a, b = runs
    assert int(a["P"].min()) > 0
    assert torch.equal(a["P"], b["P"]) and torch.equal(a["sums"], b["sums"])
    assert len(a["flushed"]) == len(b["flushed"]) == steps // flush and all(torch.equal(x, y) for x, y in zip(a["flushed"], b["flushed"]))
    for k in ("stack", "pos", "qubits", "states", "ep", "st"):
        assert torch.equal(a[k], b[k]), k


def test_completion_event_orders_a_second_stream_and_capture_keeps_the_plain_write(T):
    """tq_persp_write_signal + tq_stream_wait_event: a second stream that waits for the event reads the finished stack.
    The signalling variant refuses a capturing stream; the plain tq_persp_write is captured and replays (the slot counters
    are left zero by every launch)."""
    from toric_rl_decoder_amd._lib import WriteEvent
    d, n = 7, 24576
    gpu = make_envs(T, d, n, seed=31)
    try:
        gpu.resetAll()
        gpu.actorStep(None, want_actions=False)
        _, offsets = gpu.perspectiveCounts()
        P = int(offsets[-1].item())
        assert P * 2 * d * d * 4 >= BIG
        ref, rpos = write(gpu, offsets, P, torch.float32)
        gpu.check()
        want = int(ref[:P].view(torch.int32).sum(dtype=torch.int64).item())
        ev = WriteEvent(gpu.device)
        side = torch.cuda.Stream(device=gpu.device)
        buf, bpos = torch.zeros_like(ref), torch.zeros_like(rpos)
        torch.cuda.synchronize(gpu.device)
        ev.wait(side)                                        # no write has taken the event yet: returns at once
        for rep in range(3):
            buf.zero_()
            gpu.writePerspectives(buf[:P], bpos[:P], offsets, done=ev)
            ev.wait(side)
            with torch.cuda.stream(side):
                got = buf[:P].view(torch.int32).sum(dtype=torch.int64)
            side.synchronize()
            assert int(got.item()) == want, rep
            torch.cuda.synchronize(gpu.device)
        # a lattice range, and no lattice at all (nothing is launched: the event is still signalled)
        gpu.writePerspectives(buf[:P], bpos[:P], offsets, first=0, count=n // 2, done=ev)
        gpu.writePerspectives(buf[:P], bpos[:P], offsets, first=n // 2, count=0, done=ev)
        ev.wait(side)
        side.synchronize()
        gpu.check()
        L = T._lib.load()
        assert L.tq_stream_wait_event(None, None) == T._lib.TQ_E_INVALID and L.tq_event_destroy(None) == 0
        # capture: the plain write
        bufs = [torch.zeros_like(ref) for _ in range(2)]
        torch.cuda.synchronize(gpu.device)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            with pytest.raises(ValueError, match="captur"):
                gpu.writePerspectives(bufs[0][:P], None, offsets, done=ev)
            for b_ in bufs:
                gpu.writePerspectives(b_[:P], None, offsets)
        for replay in range(3):
            for b_ in bufs:
                b_.zero_()
            g.replay()
            torch.cuda.synchronize(gpu.device)
            gpu.check()
            for b_ in bufs:
                assert torch.equal(b_[:P], ref[:P]), f"replay {replay} wrote another stack"
        ev.close()
    finally:
        gpu.close()
