"""The learner-step shells of NN_11 and the wide nets on the GPU (tq_nn11_grad_*, tq_nnw_grad_*): every refusal of
*_grad_step and *_grad_load by return code, tq_last_error() text and order -- with two things wrong at once, the one
that is checked first is the one reported -- nothing written by a refused call, a good step after them, and the text of
the action latch.  One small handle per family: d = 3, max_batch = 4."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
INVALID, ACTION = -1, -4                                # TQ_E_INVALID, TQ_E_ACTION
U8, D, B = 3, 3, 4                                      # TQ_U8; the lattice size; max_batch

FAMILIES = {"nn11": ("NN_11", ()), "nnw": ("NN_8", (8,))}      # family -> (the torch module, create's arguments ahead of d)


@pytest.fixture(scope="module")
def T():
    import toric_rl_decoder_amd as T
    assert torch.cuda.is_available()
    T.load()
    return T


def ptr(t):
    return C.c_void_p(None if t is None else t.data_ptr())


def pointers(tensors, hole=None):
    return (C.c_void_p * len(tensors))(*[None if i == hole else t.data_ptr() for i, t in enumerate(tensors)])


@pytest.mark.parametrize("family", sorted(FAMILIES))
def test_step_and_load_refusals_keep_code_text_and_order(T, family):
    L = T.load()
    module, net = FAMILIES[family]
    fn = lambda name: getattr(L, f"tq_{family}_grad_{name}")
    last = lambda: L.tq_last_error().decode()
    torch.manual_seed(3)
    model = getattr(T, module)(D).to(DEV)
    params = dict(model.named_parameters())
    w = [p.detach() for k, p in params.items() if k.endswith("weight")]
    b = [p.detach() for k, p in params.items() if k.endswith("bias")]
    layers = len(w)                                     # the conv layers and the linear one
    x = torch.randint(0, 2, (B + 1, 2, D, D), dtype=torch.uint8, device=DEV)
    a = torch.tensor([0, 1, 2, 1], device=DEV)
    y = torch.tensor([0.5, -1.0, 2.0, 0.25], device=DEV)
    q = torch.full((B, 3), 7.0, device=DEV)
    loss = torch.full((B,), 7.0, device=DEV)
    gw, gb = [torch.full_like(t, 7.0) for t in w], [torch.full_like(t, 7.0) for t in b]
    good = dict(state=x, dtype=U8, n=B, a=a, y=y, loss=loss, gw=pointers(gw), gb=pointers(gb))
    odd = x[1:]                                         # contiguous, 18 bytes past an aligned address
    assert odd.is_contiguous() and odd.data_ptr() % 16 != 0

    h = C.c_void_p(None)
    assert fn("create")(C.byref(h), *net, D, B, 0) == 0 and h.value

    def step(**kw):
        k = dict(good, **kw)
        return fn("step")(h, ptr(k["state"]), k["dtype"], k["n"], ptr(k["a"]), ptr(k["y"]), None, ptr(q), ptr(k["loss"]), k["gw"], k["gb"], None)

    def refused(text, **kw):
        assert step(**kw) == INVALID, kw
        assert last() == text, kw

    # 1. a step before load, ahead of everything else
    before = f"{family} grad step before tq_{family}_grad_load"
    refused(before)
    refused(before, dtype=4, n=0, state=None, gw=None)

    # load's own refusals leave the handle without a network
    assert fn("load")(h, None, pointers(b), None) == INVALID and last() == "weights / biases is NULL"
    assert fn("load")(h, pointers(w), None, None) == INVALID and last() == "weights / biases is NULL"
    assert fn("load")(h, pointers(w, hole=2), pointers(b), None) == INVALID and last() == "weights[2] / biases[2] is NULL"
    assert fn("load")(h, pointers(w), pointers(b, hole=layers - 1), None) == INVALID
    assert last() == f"weights[{layers - 1}] / biases[{layers - 1}] is NULL"
    assert fn("load")(h, pointers(w, hole=1), pointers(b, hole=0), None) == INVALID and last() == "weights[0] / biases[0] is NULL"
    refused(before)
    assert fn("load")(h, pointers(w), pointers(b), None) == 0

    # 2. the dtype
    refused("bad state dtype 4", dtype=4)
    refused("bad state dtype -1", dtype=-1)
    refused("bad state dtype 4", dtype=4, n=B + 1, state=None, gw=None, gb=pointers(gb, hole=0))
    # 3. n
    for n in (B + 1, 0, -3):
        refused(f"n must be in 1..max_batch = {B} (got {n})", n=n)
    refused(f"n must be in 1..max_batch = {B} (got 5)", n=B + 1, a=None, gw=None, state=odd)
    # 4. the four arrays
    null = "state / actions_idx / y / loss is NULL"
    for kw in (dict(state=None), dict(a=None), dict(y=None), dict(loss=None)):
        refused(null, **kw)
    refused(null, y=None, gb=None, gw=pointers(gw, hole=0))
    refused(null, loss=None, state=odd)
    # 5. the two lists
    refused("grad_w / grad_b is NULL", gw=None)
    refused("grad_w / grad_b is NULL", gb=None)
    refused("grad_w / grad_b is NULL", gb=None, gw=pointers(gw, hole=0), state=odd)
    # 6. their entries, the lowest layer first
    refused("grad_w[0] / grad_b[0] is NULL", gw=pointers(gw, hole=0))
    refused(f"grad_w[{layers - 1}] / grad_b[{layers - 1}] is NULL", gb=pointers(gb, hole=layers - 1))
    refused("grad_w[1] / grad_b[1] is NULL", gw=pointers(gw, hole=3), gb=pointers(gb, hole=1))
    refused("grad_w[2] / grad_b[2] is NULL", gw=pointers(gw, hole=2), state=odd)
    # 7. the alignment of the stack
    refused("state must be 16-byte aligned", state=odd)

    # nothing was written
    torch.cuda.synchronize()
    assert bool((loss == 7.0).all()) and bool((q == 7.0).all()) and all(bool((t == 7.0).all()) for t in gw + gb)
    assert fn("check")(h, None) == 0

    # the same call with nothing wrong is taken
    assert step() == 0
    torch.cuda.synchronize()
    assert not bool((loss == 7.0).any()) and not bool((q == 7.0).any()) and not any(bool((t == 7.0).any()) for t in gw + gb)
    assert all(bool(torch.isfinite(t).all()) for t in [loss, q] + gw + gb)
    assert fn("check")(h, None) == 0

    # the latch: an action outside 0..2, reported once
    for bad in (3, -1):
        wrong = a.clone()
        wrong[1] = bad
        assert step(a=wrong) == 0
        assert fn("check")(h, None) == ACTION
        assert last() == f"{family} grad step: an actions_idx outside 0..2 was given"
        assert fn("check")(h, None) == 0
    assert fn("destroy")(h) == 0
