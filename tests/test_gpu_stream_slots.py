"""The stack write's unequal shares, taken pair by pair (csrc/stream_write.hpp: stream_setup; csrc/stream_range.hpp:
pair_claim): whichever of a pair's two workgroups takes the larger share -- the XCD parity read from the hardware, every
workgroup claiming the same parity (tq_debug_force_xcc_parity 0 / 1: both of a pair prefer the same slot, which a
round-robin dispatcher never produces), the parity inverted -- the stack and the positions are, byte for byte, those of
the same write with equal shares (tq_env_set_xcd_bias(h, 0)); through the scan's table, through a lattice sub-range
(cut points found in the kernel), with a capacity that cuts the stack, with two writes of one handle in flight, and in
a replayed graph.  After every case the handle's pair words read back as zeros and tq_check is clean."""
import pytest
import torch

pytestmark = pytest.mark.gpu

BIAS = 5
# (d, dtype, lattices, p_error, biased): stacks of 64 MiB and more take unequal shares; the last one stays just below
SHAPES = [(7, torch.float32, 6144, 0.10, True), (7, torch.bfloat16, 12288, 0.10, True), (9, torch.float32, 2048, 0.15, True),
          (7, torch.float32, 6143, 0.10, True), (7, torch.float32, 1024, 0.10, False)]


class Case:
    """One shape: the lattices after a reset and a few free steps, their scan, and the equal-share write as the reference."""

    def __init__(self, T, d, dtype, n, p, biased):
        self.T, self.L, self.d, self.dtype, self.n = T, T._lib.load(), d, dtype, n
        env = T.make("toric-code-v0", {"size": d, "min_qubit_errors": 0, "p_error": p})
        self.gpu = gpu = T.EnvSet(env, n, seed=2024 + n, numpy_io=False)
        gpu.resetAll()
        for _ in range(3):
            gpu.actorStep(None)
        _, self.offsets = gpu.perspectiveCounts()
        self.P = P = int(self.offsets[-1].item())
        nbytes = P * 2 * d * d * torch.empty((), dtype=dtype).element_size()
        # the threshold of the unequal shares is really crossed (or, for the last shape, really not)
        assert (nbytes >= 64 << 20) == biased, (P, nbytes)
        self.ref, self.rpos = self.write(0)

    def fresh(self, cap=None):
        cap = self.P + 8 if cap is None else cap
        return (torch.full((cap, 2, self.d, self.d), 7, dtype=self.dtype, device=self.gpu.device),
                torch.full((cap, 3), -1, dtype=torch.int32, device=self.gpu.device))

    def write(self, bias, cap=None, **kw):
        assert self.L.tq_env_set_xcd_bias(self.gpu._h, bias) == 0
        out, pos = self.fresh(cap)
        self.gpu.writePerspectives(out, pos, self.offsets, **kw)
        return out, pos

    def clean(self):
        """The latch is clear and every pair word of the handle's eight sets is zero again."""
        self.gpu.check()
        assert self.L.tq_debug_slot_words_nonzero(self.gpu._h) == 0

    def close(self):
        self.L.tq_debug_force_xcc_parity(-1)
        self.gpu.close()


@pytest.fixture(scope="module", params=SHAPES, ids=lambda s: f"d{s[0]}-{str(s[1]).split('.')[-1]}-{s[2]}")
def case(request):
    import toric_rl_decoder_amd as T
    assert torch.cuda.is_available(), "these tests need the GPU"
    T.load()
    c = Case(T, *request.param)
    c.clean()
    yield c
    c.close()


@pytest.fixture(params=(-1, 0, 1, 2), ids=lambda p: f"parity{p}")
def parity(request, case):
    assert case.L.tq_debug_force_xcc_parity(request.param) == 0
    yield request.param
    assert case.L.tq_debug_force_xcc_parity(-1) == 0


def test_the_hook_is_range_checked(case):
    L = case.L
    assert L.tq_debug_force_xcc_parity(3) < 0 and L.tq_debug_force_xcc_parity(-2) < 0 and b"xcc parity" in L.tq_last_error()
    assert L.tq_debug_force_xcc_parity(-1) == 0


def test_whole_stack_sub_range_and_capacity(case, parity):
    c = case
    out, pos = c.write(BIAS)
    c.clean()
    assert torch.equal(out, c.ref) and torch.equal(pos, c.rpos)
    assert bool((out[c.P:] == 7).all()) and bool((pos[c.P:] == -1).all())
    # a lattice sub-range (first, count): no table, the workgroups find their cut points themselves
    first, count = c.n // 5 + 1, c.n // 2 + 3
    want, wpos = c.write(0, first=first, count=count)
    got, gpos = c.write(BIAS, first=first, count=count)
    c.clean()
    lo, hi = int(c.offsets[first].item()), int(c.offsets[first + count].item())
    assert torch.equal(got, want) and torch.equal(gpos, wpos)
    assert torch.equal(got[:hi - lo], c.ref[lo:hi]) and torch.equal(gpos[:hi - lo], c.rpos[lo:hi]) and bool((got[hi - lo:] == 7).all())
    # a capacity that cuts the stack: the lattices that fit whole are written, the rest is refused and latched
    cap = c.P * 3 // 5 + 1
    cut = []
    for bias in (0, BIAS):
        cut.append(c.write(bias, cap=cap))
        with pytest.raises(c.T.ToricEnvError, match="capacity"):
            c.gpu.check()
    c.clean()
    assert torch.equal(cut[1][0], cut[0][0]) and torch.equal(cut[1][1], cut[0][1])
    written = int((cut[1][1][:, 0] >= 0).sum().item())
    assert 0 < written <= cap and torch.equal(cut[1][0][:written], c.ref[:written]) and bool((cut[1][0][written:] == 7).all())


def test_two_writes_in_flight_and_a_replayed_graph(case, parity):
    c = case
    dev = c.gpu.device
    assert c.L.tq_env_set_xcd_bias(c.gpu._h, BIAS) == 0
    bufs = [c.fresh() for _ in range(2)]
    streams = [torch.cuda.Stream(dev) for _ in range(2)]
    for s, (out, pos) in zip(streams, bufs):
        s.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(s):
            c.gpu.writePerspectives(out, pos, c.offsets)
    for s in streams:
        torch.cuda.current_stream(dev).wait_stream(s)
    c.clean()
    for out, pos in bufs:
        assert torch.equal(out, c.ref) and torch.equal(pos, c.rpos)
    # captured once, replayed three times: every replay finds the captured launch's pair words as the launch before left them
    out, pos = c.fresh()
    torch.cuda.synchronize(dev)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        c.gpu.writePerspectives(out, pos, c.offsets)
    for replay in range(3):
        out.fill_(7)
        pos.fill_(-1)
        g.replay()
        c.clean()
        assert torch.equal(out, c.ref) and torch.equal(pos, c.rpos), f"replay {replay} wrote another stack"
