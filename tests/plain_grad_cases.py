"""Inputs and yardsticks of the plain conv nets' learner step (include/toricenv.h), once for
NN_11 and the wide nets NN_8 / NN_17 (not a test module): cases with one right answer in bits.
tests/nn11_grad_cases.py and tests/nnw_grad_cases.py bind a net each (``GradCases``) and are what the tests import.

  head_contract        loss and dq as the contract writes them, in f32 torch ops
  integer_case         case 1: the net's integer_state_dict with dq in {+-1, +-2}: every gradient of the pre-activations
                       is a small integer, nothing rounds, and torch's own f32 autograd is the reference
  rounding_case        case 2: the same network with dq in +-TIES and small integers: G_L onward holds values bf16
                       cannot hold, ties included; the reference is float64 autograd with a rounding Function
  reference_backward   float64 autograd of the contract (RoundBoth after each ReLU), L = the state_dict's conv layers
  manual_backward      the same backward written out layer by layer: it must equal reference_backward, it asserts that
                       every sum's terms stay below 2^23 in magnitude, and its switches (MUTANTS) are the ways a kernel
                       can be subtly wrong

The integer nets have one or two weights per output channel, so a forward sum has at most two terms and a dgrad sum as
many as the input channel has readers (a handful): the sums do not grow with the width, and the wgrad sums grow with
records x pixels only.  manual_backward asserts it for every case that is drawn."""
from dataclasses import dataclass, field
from typing import Callable, Optional

import numpy as np
import torch
import torch.nn.functional as F

import plain_cases as P

SUM_LIMIT = float(1 << 23)


def tie_records(d):
    """records of the rounding case whose dq is a tie: a wgrad sum runs over records and pixels, and a tie's G is some
    hundred times a small integer's, so their number falls with the lattice size to keep the sums below SUM_LIMIT"""
    return max(1, min(6, 500 // (d * d)))


MUTANT_LAYER = 6                                                       # the layer NN_11 applies a one-layer mutant at

MUTANTS = {
    "G truncated": dict(g_round="trunc"),
    "G rounded half-up": dict(g_round="half_up"),
    "mask taken from the next layer": dict(mask_next=True),
    "taps not flipped": dict(no_flip=MUTANT_LAYER),
    "taps transposed": dict(transpose=MUTANT_LAYER),
    "last output channel dropped in one dgrad": dict(drop_last_cout="alive"),  # the last layer where that channel's G is not 0
    "circular instead of zero padding in one wgrad": dict(circular_wgrad=MUTANT_LAYER),
}


def mutant_switches(name, layer):
    """MUTANTS[name] applied at ``layer`` instead of MUTANT_LAYER"""
    return {k: (layer if v == MUTANT_LAYER and not isinstance(v, bool) else v) for k, v in MUTANTS[name].items()}


def head_contract(q, actions, y, w, n=None):
    """f32 tensors -> (loss (n,), dq (n, 3)): each operation rounded once, left to right."""
    n = q.shape[0] if n is None else n
    qa = q.gather(1, actions.view(-1, 1)).squeeze(1)
    w = torch.ones_like(qa) if w is None else w
    e = y - qa
    loss = w * (e * e)
    g = (((qa - y) * w) * 2.0) / torch.tensor(float(n), dtype=torch.float32)
    return loss, torch.zeros_like(q).scatter(1, actions.view(-1, 1), g.view(-1, 1))


class RoundBoth(torch.autograd.Function):
    """rounds the activation to bf16 on the way forward and the incoming gradient on the way back"""

    @staticmethod
    def forward(ctx, x, mode, exact):
        ctx.mode, ctx.exact = mode, exact
        return P.round_bf16(x, "rne", exact) if x.dtype == torch.float64 else x.bfloat16().float()

    @staticmethod
    def backward(ctx, g):
        if g.dtype == torch.float64:
            return P.round_bf16(g, ctx.mode, ctx.exact), None, None
        return g.bfloat16().float(), None, None


def _rounded_weights(sd, dtype, exact=True):
    if dtype == torch.float64:
        return {k: (P.round_bf16(v.double(), "rne", exact) if k.endswith("weight") else v.double()) for k, v in sd.items()}
    return {k: (v.float().bfloat16().float() if k.endswith("weight") else v.float()) for k, v in sd.items()}


def reference_backward(sd, x, dq, dtype=torch.float64, exact=None, pad_explicitly=False):
    """The contract by autograd: weights rounded to bf16, the activation rounded after each ReLU, the gradient rounded
    where it passes that point on the way back (so G_l = bf16(mask_l * ...), the mask applied by ReLU's own backward to
    the rounded gradient: a rounded value keeps its sign and a zero stays zero, so mask and rounding commute).
    ``x`` (n, 2, d, d), ``dq`` (n, 3) the gradient of the loss with respect to q, or a function of q (detached) that
    gives it -> (q, {parameter name: gradient}).  dtype float32: the same in f32 torch ops, the yardstick for trained
    weights.  ``exact`` (default: float64 only): assert that f32 holds every rounded value.
    pad_explicitly: the zero padding of the inner layers as F.pad before an unpadded conv2d, so that its zeros are terms
    of every sum like any other (0 x NaN = NaN), which is the contract.  torch's padded conv2d has no single answer
    there: its f32 CPU kernels leave the padding's terms out, its f64 ones multiply them -- the NaN tests use this
    switch."""
    L = len(sd) // 2 - 1
    exact = dtype == torch.float64 if exact is None else exact
    p = {k: v.clone().requires_grad_(True) for k, v in _rounded_weights(sd, dtype, exact).items()}
    a = x.to(dtype)
    a = F.pad(P.round_bf16(a, "rne", exact) if dtype == torch.float64 else a.bfloat16().float(), (1, 1, 1, 1), mode="circular")
    for l in range(1, L + 1):
        pad = 0 if l in (1, L) else 1
        if pad and pad_explicitly:
            a, pad = F.pad(a, (1, 1, 1, 1)), 0
        pre = F.conv2d(a, p[f"conv{l}.weight"], p[f"conv{l}.bias"], padding=pad)
        a = RoundBoth.apply(F.relu(pre), "rne", exact)
    q = F.linear(a.flatten(1), p["linear1.weight"], p["linear1.bias"])
    q.backward((dq(q.detach()) if callable(dq) else dq).to(dtype))
    return q.detach(), {k: v.grad for k, v in p.items()}


# ---- NaN and inf in one record of a step (tests/test_gpu_nonfinite.py; the comparisons are plain_cases') ------------------
LEARNER_POISONS = ("y nan", "weight inf", "stack nan")


def poisoned_batch(kind, r, x, y, w):
    """copies of the f32 tensors (x (n, 2, d, d), y (n,), w (n,)) with record ``r`` poisoned: its target a NaN, its
    importance weight +inf, or one element of its stack a NaN"""
    assert kind in LEARNER_POISONS, kind
    x, y, w = x.clone(), y.clone(), w.clone()
    if kind == "y nan":
        y[r] = float("nan")
    elif kind == "weight inf":
        w[r] = float("inf")
    else:
        x[r, 1, x.shape[-1] // 2, 0] = float("nan")
    return x, y, w


def _wgrad(inp, shape, g, padding):
    return torch.nn.grad.conv2d_weight(inp, shape, g, padding=padding)


def _dgrad(shape, w, g, padding):
    return torch.nn.grad.conv2d_input(shape, w, g, padding=padding)


def manual_backward(sd, x, dq, g_round="rne", mask_next=False, no_flip=0, transpose=0, drop_last_cout=0, circular_wgrad=0,
                    limit=SUM_LIMIT):
    """The contract's backward written out in float64, layer by layer, L = the state_dict's conv layers ->
    ({parameter name: gradient}, stats).
    Without a switch it asserts for every dgrad, wgrad, bias and linear sum that the sum of its terms' magnitudes stays
    below ``limit``: every partial sum in any order is then an integer f32 holds, and there is one right answer in bits.
    stats["changed"][l]: share of G_l's non-zero values that RNE changed; stats["g_max"], stats["sum_max"]."""
    L = len(sd) // 2 - 1
    mutant = g_round != "rne" or mask_next or no_flip or transpose or drop_last_cout or circular_wgrad
    exact = not mutant
    p = _rounded_weights(sd, torch.float64)
    acts = [P.round_bf16(x.double())]
    a = F.pad(acts[0], (1, 1, 1, 1), mode="circular")
    for l in range(1, L + 1):
        pad = 0 if l in (1, L) else 1
        a = P.round_bf16(F.relu(F.conv2d(a, p[f"conv{l}.weight"], p[f"conv{l}.bias"], padding=pad)))
        acts.append(a)
    dq = dq.double()
    lw = p["linear1.weight"]
    feat = acts[L].flatten(1)
    grads = {"linear1.weight": dq.T @ feat, "linear1.bias": dq.sum(0)}
    sums = [float((dq.abs().T @ feat.abs()).max()), float(dq.abs().sum(0).max()), float((dq.abs() @ lw.abs()).max())]
    stats = {"changed": {}, "g_max": 0.0}

    def rounded(v, l):
        g = P.round_bf16(v, g_round, exact)
        nz = v != 0
        stats["changed"][l] = float((g != v)[nz].double().mean()) if bool(nz.any()) else 0.0
        stats["g_max"] = max(stats["g_max"], float(g.abs().max()))
        return g

    g = rounded((acts[L] > 0) * (dq @ lw).view_as(acts[L]), L)
    for l in range(L, 0, -1):
        w = p[f"conv{l}.weight"]
        pad = 0 if l in (1, L) else 1
        inp = F.pad(acts[0], (1, 1, 1, 1), mode="circular") if l == 1 else acts[l - 1]
        if circular_wgrad == l:
            inp, wpad = F.pad(inp, (1, 1, 1, 1), mode="circular"), 0
        else:
            wpad = pad
        grads[f"conv{l}.weight"] = _wgrad(inp, w.shape, g, wpad)
        grads[f"conv{l}.bias"] = g.sum((0, 2, 3))
        sums += [float(_wgrad(inp.abs(), w.shape, g.abs(), wpad).max()), float(g.abs().sum((0, 2, 3)).max())]
        if l == 1:
            break
        wd = w
        if no_flip == l:
            wd = wd.flip(2, 3)
        if transpose == l:
            wd = wd.transpose(2, 3)
        if drop_last_cout == l or (drop_last_cout == "alive" and bool(g[:, -1].any())):
            wd, drop_last_cout = wd.clone(), 0
            wd[-1] = 0
        da = _dgrad(acts[l - 1].shape, wd, g, pad)
        sums.append(float(_dgrad(acts[l - 1].shape, wd.abs(), g.abs(), pad).max()))
        mask = acts[l] > 0 if (mask_next and l == 2) else acts[l - 1] > 0       # conv1 and conv2 have as many channels
        g = rounded(mask * da, l - 1)
    stats["sum_max"] = max(sums)
    if exact and limit is not None:
        assert stats["sum_max"] < limit, stats["sum_max"]
    return grads, stats


@dataclass(eq=False)
class GradCases:
    """One net's cases and how they are drawn: what differs between the families is kept as it was first made, so that
    every case stays the one the kernels were pinned on."""
    net: P.Plain                              # the net, as plain_cases binds it
    tag: dict                                 # what a case dict carries ahead of d: {} or {"net": 8}; also its cache key
    seed: Callable                            # (d, kind) -> seed sequence of the case's draws
    row_counts: Callable                      # d -> the sorted record counts a case is stepped at
    g_max: int                                # what |G| of the integer case stays within: the widest layer's channels
    rounding_check: Callable                  # (d, stats) -> None: asserts that RNE changed G in enough layers
    mutant_layer: int                         # the layer a one-layer mutant is applied at
    cache: dict                               # the latest cases, shared by the nets of a family
    keep: int                                 # ... this many
    min_conv_share: Optional[float] = None    # at d >= 5, the least non-zero share of every conv weight gradient
    params: list = field(init=False)          # the 2 (L + 1) gradient tensors, in model.parameters() order

    def __post_init__(self):
        self.params = [f"{n}.{k}" for n in self.net.names for k in ("weight", "bias")]

    def _case(self, d, kind):
        """-> dict(tag, d, sd, x uint8 numpy, actions i64, y f32, t f32, q f32 (rows, 3), dq f32, stats, by_rows) of
        row_counts(d)[-1] records; at_rows gives the step on the first n of them.  Kept per (tag, d, kind)."""
        key = (*self.tag.values(), d, kind)
        if key in self.cache:
            return self.cache[key]
        rows = self.row_counts(d)[-1]
        rng = np.random.default_rng(self.seed(d, kind))
        sd = P.integer_state_dict(self.net, d)
        x = torch.from_numpy(P.dense_rows(d, rows))
        with torch.no_grad():
            q = P.model_of(self.net, sd, d)(x.float())
        assert bool((q == q.round()).all()) and float(q.abs().max()) < 1 << 20
        actions = torch.from_numpy(rng.integers(0, 3, rows))
        if kind == "integer":
            t = rng.choice([-2, -1, 1, 2], rows)
        else:
            t = rng.choice([-3, -2, -1, 1, 2, 3], rows)
            ties = rng.choice(rows, min(rows, tie_records(d)), replace=False)
            t[ties] = rng.choice(P.TIES, ties.size) * rng.choice((-1, 1), ties.size)
            t[0] = 257                                                     # the single record has a tie as well
        t = torch.from_numpy(t.astype(np.float32))
        y = q.gather(1, actions.view(-1, 1)).squeeze(1) - t
        dq = torch.zeros_like(q).scatter(1, actions.view(-1, 1), t.view(-1, 1))
        c = dict(**self.tag, d=d, sd=sd, x=x.numpy(), actions=actions, y=y, t=t, q=q.numpy(), dq=dq, by_rows={})
        _, _, ref = self.at_rows(c, rows, as_f64=True)
        man, c["stats"] = manual_backward(sd, x, dq)
        for k in self.params:
            assert torch.equal(man[k], ref[k]), (k, "the written-out backward is not autograd's")
        while len(self.cache) >= self.keep:
            del self.cache[next(iter(self.cache))]
        self.cache[key] = c
        return c

    def at_rows(self, c, n, as_f64=False):
        """The step on the case's first n records, with w[i] = n / 2 -> (w f32 (n,), loss f32 (n,), {name: f32 numpy
        gradient}).  dq is then exactly t for any n (asserted), and the gradients are float64 autograd's
        (reference_backward), asserted to be values f32 holds."""
        if n not in c["by_rows"] or as_f64:
            w = torch.full((n,), n / 2, dtype=torch.float32)
            q = torch.from_numpy(c["q"][:n])
            loss, dq = head_contract(q, c["actions"][:n], c["y"][:n], w)
            assert torch.equal(dq, c["dq"][:n]), "dq is exactly t for any n"
            q64, ref = reference_backward(c["sd"], torch.from_numpy(c["x"][:n]), dq)
            assert torch.equal(q64.float().double(), q64) and torch.equal(q64.float(), q)
            if as_f64:
                return w, loss, ref
            grads = {}
            for k in self.params:
                g32 = ref[k].float()
                assert torch.equal(g32.double(), ref[k]), k
                grads[k] = g32.numpy()
            c["by_rows"][n] = (w, loss.numpy(), grads)
        return c["by_rows"][n]

    def integer_case(self, d):
        """Case 1.  Asserted: no G rounds, so torch's own f32 autograd gives the same bits; every one of the gradient
        tensors is non-zero (c["nonzero"]: the shares); with min_conv_share, at d >= 5 at least that share of every conv
        weight gradient is."""
        c = self._case(d, "integer")
        if "checked" not in c:
            assert c["stats"]["g_max"] <= self.g_max and not any(c["stats"]["changed"].values()), c["stats"]
            grads = self.at_rows(c, c["x"].shape[0])[2]
            model = P.model_of(self.net, c["sd"], d).train()
            qt = model(torch.from_numpy(c["x"]).float())
            qt.backward(c["dq"])
            for k, p in model.named_parameters():
                assert np.array_equal(p.grad.numpy(), grads[k]), (k, "torch's f32 autograd differs")
            c["nonzero"] = {k: float((grads[k] != 0).mean()) for k in self.params}
            for k in self.params:
                assert c["nonzero"][k] > 0, k
                if self.min_conv_share is not None and d >= 5 and k.startswith("conv") and k.endswith("weight"):
                    assert c["nonzero"][k] >= self.min_conv_share, (k, c["nonzero"][k])
            c["checked"] = True
        return c

    def rounding_case(self, d):
        """Case 2.  Asserted: RNE changed a share of G's non-zero values in enough layers (rounding_check)."""
        c = self._case(d, "rounding")
        self.rounding_check(d, c["stats"])
        return c

    def mutant_grads(self, c, name):
        g, _ = manual_backward(c["sd"], torch.from_numpy(c["x"]), c["dq"], **mutant_switches(name, self.mutant_layer))
        return g


def play_memory(T, d, seed, device="cuda:0"):
    """(GPU tests) a replay memory filled by epsilon = 1 play: 256 lattices, 8 steps"""
    env = T.make("toric-code-v0", {"size": d, "min_qubit_errors": 0, "p_error": 0.1})
    gpu = T.EnvSet(env, 256, device=device, seed=seed, numpy_io=False)
    gpu.resetAll()
    blk = gpu.newTransitionBlock(steps=8)
    for t in range(8):
        gpu.actorStep(None, block=blk, slot=t)
    g = torch.Generator(device=device).manual_seed(seed)
    blk.computePriorities(256, 8, torch.rand((9, 256, 3), generator=g, device=device) * 4 - 2, 0.95)
    gpu.check()
    gpu.close()
    mem = T.PrioritizedReplayMemory(4096, 0.6, d=d, device=device, seed=seed)
    mem.save_block(blk)
    return mem
