"""Inputs and yardsticks shared by tests/test_nnw_grad_host.py and tests/test_gpu_nnw_grad.py (not a test module): the
learner step of the wide nets NN_8 and NN_17 (include/toricenv.h) on the two cases of
tests/nn11_grad_cases.py, restated over a channel tuple and a layer count and bound to nets 8 and 17 through
nnw_cases.BOUND.  The head, the rounding Function, the mutants and the tie records are NN_11's own.

  integer_case         case 1: K.integer_state_dict with dq in {+-1, +-2}: every gradient of the pre-activations is a
                       small integer, nothing rounds, and torch's own f32 autograd is the reference
  rounding_case        case 2: the same network with dq in +-TIES and small integers: G_L onward holds values bf16
                       cannot hold, ties included; the reference is float64 autograd with a rounding Function
  reference_backward   float64 autograd of the contract (RoundBoth after each ReLU), L = the state_dict's conv layers
  manual_backward      the same backward written out layer by layer: it must equal reference_backward, it asserts that
                       every sum's terms stay below 2^23 in magnitude, and its switches (MUTANTS, the one-layer ones at
                       the middle of the net) are the ways a kernel can be subtly wrong

The integer nets have one or two weights per output channel, so a forward sum has at most two terms and a dgrad sum as
many as the input channel has readers (a handful): the sums do not grow with the width, and the wgrad sums grow with
records x pixels only.  manual_backward asserts it for every case that is drawn."""
import numpy as np
import torch
import torch.nn.functional as F

import nnw_cases as K
from nn11_grad_cases import (LEARNER_POISONS, MUTANT_LAYER, MUTANTS, SUM_LIMIT, RoundBoth, head_contract, play_memory,  # noqa: F401
                             _rounded_weights, poisoned_batch, reference_backward, tie_records)

NETS = K.NETS


def layers(net):
    return K.layers(net)


def params(net):
    """the 2 (L + 1) gradient tensors, in model.parameters() order"""
    return [f"{n}.{k}" for n in K.names(net) for k in ("weight", "bias")]


def mutant_layer(net):
    """the layer a one-layer mutant is applied at: the middle of the net"""
    return layers(net) // 2 + 1


def mutant_switches(net, name):
    """MUTANTS[name] with NN_11's mutant layer replaced by this net's"""
    return {k: (mutant_layer(net) if v == MUTANT_LAYER and not isinstance(v, bool) else v) for k, v in MUTANTS[name].items()}


def mutant_is_void(name, net, d):
    """No mutant is void at any (net, d) the tests use -- NN_8 at d = 3, 5, 7 and NN_17 at d = 5: the wide nets' last
    channels stay alive at d = 3 as well, where NN_11's die.  tests/test_nnw_grad_host.py runs every mutant at those
    sizes: one named here must change nothing, any other some gradient tensor."""
    return False


def wgrad_persp(d):
    """records per wgrad workgroup: nnw_wgrad_persp of csrc/nnw_grad.hpp"""
    return max(2, 2048 // (d * d))


def row_counts(d):
    """one record; one more than a conv workgroup's perspectives; one more than a wgrad chunk's records (a two-chunk sum)"""
    return sorted({1, K.group(d) + 1, wgrad_persp(d) + 1})


def _wgrad(inp, shape, g, padding):
    return torch.nn.grad.conv2d_weight(inp, shape, g, padding=padding)


def _dgrad(shape, w, g, padding):
    return torch.nn.grad.conv2d_input(shape, w, g, padding=padding)


def manual_backward(sd, x, dq, g_round="rne", mask_next=False, no_flip=0, transpose=0, drop_last_cout=0, circular_wgrad=0,
                    limit=SUM_LIMIT):
    """nn11_grad_cases.manual_backward with L = the state_dict's conv layers -> ({parameter name: gradient}, stats).
    Without a switch it asserts for every dgrad, wgrad, bias and linear sum that the sum of its terms' magnitudes stays
    below ``limit``: every partial sum in any order is then an integer f32 holds, and there is one right answer in bits.
    stats["changed"][l]: share of G_l's non-zero values that RNE changed; stats["g_max"], stats["sum_max"]."""
    L = len(sd) // 2 - 1
    mutant = g_round != "rne" or mask_next or no_flip or transpose or drop_last_cout or circular_wgrad
    exact = not mutant
    p = _rounded_weights(sd, torch.float64)
    acts = [K.round_bf16(x.double())]
    a = F.pad(acts[0], (1, 1, 1, 1), mode="circular")
    for l in range(1, L + 1):
        pad = 0 if l in (1, L) else 1
        a = K.round_bf16(F.relu(F.conv2d(a, p[f"conv{l}.weight"], p[f"conv{l}.bias"], padding=pad)))
        acts.append(a)
    dq = dq.double()
    lw = p["linear1.weight"]
    feat = acts[L].flatten(1)
    grads = {"linear1.weight": dq.T @ feat, "linear1.bias": dq.sum(0)}
    sums = [float((dq.abs().T @ feat.abs()).max()), float(dq.abs().sum(0).max()), float((dq.abs() @ lw.abs()).max())]
    stats = {"changed": {}, "g_max": 0.0}

    def rounded(v, l):
        g = K.round_bf16(v, g_round, exact)
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
        mask = acts[l] > 0 if (mask_next and l == 2) else acts[l - 1] > 0       # conv1 and conv2 both have 256 channels
        g = rounded(mask * da, l - 1)
    stats["sum_max"] = max(sums)
    if exact and limit is not None:
        assert stats["sum_max"] < limit, stats["sum_max"]
    return grads, stats


_cases = {}


def _case(net, d, kind):
    """-> dict(net, d, sd, x uint8 numpy, actions i64, y f32, t f32, q f32 (rows, 3), dq f32, stats, by_rows) of
    row_counts(d)[-1] records; at_rows gives the step on the first n of them.  Kept per (net, d, kind)."""
    key = (net, d, kind)
    if key in _cases:
        return _cases[key]
    rows = row_counts(d)[-1]
    rng = np.random.default_rng([1108, net, d, kind == "rounding"])
    sd = K.integer_state_dict(net, d)
    x = torch.from_numpy(K.dense_rows(d, rows))
    with torch.no_grad():
        q = K.model_of(sd, d)(x.float())
    assert bool((q == q.round()).all()) and float(q.abs().max()) < 1 << 20
    actions = torch.from_numpy(rng.integers(0, 3, rows))
    if kind == "integer":
        t = rng.choice([-2, -1, 1, 2], rows)
    else:
        t = rng.choice([-3, -2, -1, 1, 2, 3], rows)
        ties = rng.choice(rows, min(rows, tie_records(d)), replace=False)
        t[ties] = rng.choice(K.TIES, ties.size) * rng.choice((-1, 1), ties.size)
        t[0] = 257                                                     # the single record has a tie as well
    t = torch.from_numpy(t.astype(np.float32))
    y = q.gather(1, actions.view(-1, 1)).squeeze(1) - t
    dq = torch.zeros_like(q).scatter(1, actions.view(-1, 1), t.view(-1, 1))
    c = dict(net=net, d=d, sd=sd, x=x.numpy(), actions=actions, y=y, t=t, q=q.numpy(), dq=dq, by_rows={})
    _, _, ref = at_rows(c, rows, as_f64=True)
    man, c["stats"] = manual_backward(sd, x, dq)
    for k in params(net):
        assert torch.equal(man[k], ref[k]), (k, "the written-out backward is not autograd's")
    while len(_cases) >= 6:
        del _cases[next(iter(_cases))]
    _cases[key] = c
    return c


def at_rows(c, n, as_f64=False):
    """The step on the case's first n records, with w[i] = n / 2 -> (w f32 (n,), loss f32 (n,), {name: f32 numpy
    gradient}).  dq is then exactly t for any n (asserted), and the gradients are float64 autograd's (reference_backward),
    asserted to be values f32 holds."""
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
        for k in params(c["net"]):
            g32 = ref[k].float()
            assert torch.equal(g32.double(), ref[k]), k
            grads[k] = g32.numpy()
        c["by_rows"][n] = (w, loss.numpy(), grads)
    return c["by_rows"][n]


def integer_case(net, d):
    """Case 1.  Asserted: no G rounds, so torch's own f32 autograd gives the same bits; every one of the gradient
    tensors is non-zero."""
    c = _case(net, d, "integer")
    if "checked" not in c:
        assert c["stats"]["g_max"] <= 256 and not any(c["stats"]["changed"].values()), c["stats"]
        grads = at_rows(c, c["x"].shape[0])[2]
        model = K.model_of(c["sd"], d).train()
        qt = model(torch.from_numpy(c["x"]).float())
        qt.backward(c["dq"])
        for k, p in model.named_parameters():
            assert np.array_equal(p.grad.numpy(), grads[k]), (k, "torch's f32 autograd differs")
        c["nonzero"] = {k: float((grads[k] != 0).mean()) for k in params(net)}
        for k in params(net):
            assert c["nonzero"][k] > 0, k
        c["checked"] = True
    return c


def rounded_layers(c):
    """the layers whose G the case saw changed by RNE"""
    return [l for l, v in c["stats"]["changed"].items() if v > 0]


def rounding_case(net, d):
    """Case 2.  Asserted: RNE changed a share of G's non-zero values in at least two layers."""
    c = _case(net, d, "rounding")
    assert len(rounded_layers(c)) >= 2, c["stats"]["changed"]
    return c


def mutant_grads(c, name):
    g, _ = manual_backward(c["sd"], torch.from_numpy(c["x"]), c["dq"], **mutant_switches(c["net"], name))
    return g
