"""The learner-step shells of NN_11 and the wide nets (tq_nn11_grad_*, tq_nnw_grad_*) refuse bad arguments with the same
return code, the same tq_last_error() text and in the same order, whatever code they share underneath; and the Python
handles above them (NN11Grad, NNWideGrad) keep the texts of the ValueErrors they raise before the library is asked.
No GPU: every call here is refused before a device is used (the device argument's own check comes last, and what it
answers depends on whether the machine has one)."""
import ctypes as C
import re

import pytest
import torch

import toric_rl_decoder_amd as T
from toric_rl_decoder_amd import nn11, nnw

INVALID, HIP = -1, -2                                   # TQ_E_INVALID, TQ_E_HIP
BAD_D = "unsupported lattice size d=4 (odd 3..21)"
NET_TEXT = "net must be TQ_NET_NN8 or TQ_NET_NN17 (got 11)"

# family -> (a net the family accepts or None where create takes none, a net it refuses)
FAMILIES = {"nn11": (None, None), "nnw": (8, 11)}


@pytest.fixture(scope="module")
def L():
    T.build()
    return T.load()


def last(L):
    return L.tq_last_error().decode()


def create(L, family, out, net, d, max_batch, device=0):
    fn = getattr(L, f"tq_{family}_grad_create")
    args = (d, max_batch, device) if FAMILIES[family][0] is None else (net, d, max_batch, device)
    return fn(out, *args)


@pytest.mark.parametrize("family", sorted(FAMILIES))
def test_create_refusals_keep_code_text_and_order(L, family):
    good, bad_net = FAMILIES[family]
    h = C.c_void_p(None)

    def refused(out, net, d, max_batch, text, device=0):
        assert create(L, family, out, net, d, max_batch, device) == INVALID, (net, d, max_batch)
        assert last(L) == text
        assert not h.value

    refused(None, good, 3, 4, "out is NULL")
    refused(None, bad_net, 4, 0, "out is NULL", device=-1)                        # ahead of every other refusal
    refused(C.byref(h), good, 4, 4, BAD_D)
    refused(C.byref(h), good, 3, 0, "max_batch must be in 1..4096 (got 0)")
    refused(C.byref(h), good, 3, 4097, "max_batch must be in 1..4096 (got 4097)")
    refused(C.byref(h), good, 3, -5, "max_batch must be in 1..4096 (got -5)")
    refused(C.byref(h), good, 4, 0, BAD_D)                                        # d ahead of max_batch
    refused(C.byref(h), good, 4, 4097, BAD_D, device=-1)
    refused(C.byref(h), good, 3, 0, "max_batch must be in 1..4096 (got 0)", device=-1)       # max_batch ahead of the device
    if bad_net is not None:
        refused(C.byref(h), bad_net, 3, 4, NET_TEXT)
        refused(C.byref(h), bad_net, 4, 4, NET_TEXT)                              # net ahead of d
        refused(C.byref(h), bad_net, 4, 0, NET_TEXT, device=-1)
        refused(C.byref(h), 0, 3, 4, "net must be TQ_NET_NN8 or TQ_NET_NN17 (got 0)")
    # the device, last: with nothing else wrong it is what is refused, by the count of devices or by the failing count
    rc = create(L, family, C.byref(h), good, 3, 4, -1)
    assert rc in (INVALID, HIP) and not h.value
    if rc == INVALID:
        assert re.fullmatch(r"device -1 not available \(\d+ HIP devices\)", last(L)), last(L)
    else:
        assert last(L).startswith("hipGetDeviceCount(&ndev) failed: "), last(L)


@pytest.mark.parametrize("family", sorted(FAMILIES))
def test_a_null_handle_is_refused_by_name(L, family):
    null = f"NULL {family} grad handle"
    h = C.c_void_p(None)
    assert getattr(L, f"tq_{family}_grad_load")(None, None, None, None) == INVALID and last(L) == null
    assert create(L, family, C.byref(h), FAMILIES[family][0], 4, 4) == INVALID and last(L) == BAD_D      # another text in between
    assert getattr(L, f"tq_{family}_grad_step")(None, None, 0, 0, None, None, None, None, None, None, None, None) == INVALID
    assert last(L) == null
    assert create(L, family, C.byref(h), FAMILIES[family][0], 4, 4) == INVALID and last(L) == BAD_D
    assert getattr(L, f"tq_{family}_grad_check")(None, None) == INVALID and last(L) == null
    assert create(L, family, C.byref(h), FAMILIES[family][0], 4, 4) == INVALID and last(L) == BAD_D
    assert getattr(L, f"tq_{family}_grad_destroy")(None) == 0 and last(L) == BAD_D        # NULL is fine and leaves no text
    if family == "nn11":
        assert L.tq_nn11_grad_opt_step(None, 0, 0.0, 0.0, 0.0, 0.0, 0.0, 1, *([None] * 8), None) == INVALID and last(L) == null


# ---- the Python handles: what they refuse by themselves.  A handle's constructor asks for the device first, so the
# checks are reached on an object that was given its attributes by hand, on the CPU.
CPU = torch.device("cpu")


def bare(cls, model, d, **more):
    g = object.__new__(cls)
    g.device, g.system_size, g.max_batch, g.model = CPU, d, 4, model
    for k, v in more.items():
        setattr(g, k, v)
    return g


def message(fn, *args, **kw):
    with pytest.raises(ValueError) as e:
        fn(*args, **kw)
    return str(e.value)


def test_nn11_masters_are_validated_with_the_same_texts():
    d = 3
    model = T.NN_11(d)
    pairs = [(getattr(model, n).weight, getattr(model, n).bias) for n in nn11.NAMES]
    nn11._check_params(pairs, d, CPU)
    assert message(nn11._check_params, pairs, 5, CPU) == (
        "linear1: expected contiguous float32 (3, 576) on cpu, got torch.float32 (3, 64) on cpu")
    model.conv3.double()
    pairs = [(getattr(model, n).weight, getattr(model, n).bias) for n in nn11.NAMES]
    assert message(nn11._check_params, pairs, d, CPU) == (
        "conv3: expected contiguous float32 (120, 128, 3, 3) on cpu, got torch.float64 (120, 128, 3, 3) on cpu")
    wide = T.NN_8(d)
    pairs = [(getattr(wide, n).weight, getattr(wide, n).bias) for n in nn11.NAMES[:8]] + [(wide.linear1.weight, wide.linear1.bias)]
    assert message(nn11._check_params, pairs, d, CPU) == (
        "conv1: expected contiguous float32 (128, 2, 3, 3) on cpu, got torch.float32 (256, 2, 3, 3) on cpu")


def test_wide_masters_are_validated_with_the_same_texts():
    d = 3
    g = bare(T.NNWideGrad, None, d, net=T._lib.TQ_NET_NN8)
    model = T.NN_8(d)
    pairs = g._masters(model)
    assert len(pairs) == 9 and pairs[0][0] is model.conv1.weight and pairs[8][1] is model.linear1.bias
    assert message(g._masters, T.NN_17(d)) == "this handle was made for net 8, the model is net 17's"
    assert message(g._masters, T.NN_11(d)).startswith("state_dict is neither NN_8's nor NN_17's: NN_8: parameter names differ in [")
    assert message(g._masters, T.NN_8(5)) == (
        "state_dict is neither NN_8's nor NN_17's: NN_8 at d=3: linear1.weight has shape (3, 1800), expected (3, 200); "
        "NN_17: parameter names differ in ['conv10.bias', 'conv10.weight', 'conv11.bias', 'conv11.weight', 'conv12.bias', 'conv12.weight']")
    model.conv2.double()
    assert message(g._masters, model) == "conv2: expected a contiguous float32 parameter on cpu, got torch.float64 on cpu"
    # load(model) of another net is refused before the library is asked, and the masters stay
    g._params, g.model = "the masters", "the model"
    assert message(g.load, T.NN_17(d)) == "this handle was made for net 8, the model is net 17's"
    assert g._params == "the masters" and g.model == "the model"


@pytest.mark.parametrize("cls, module", [(T.NN11Grad, T.NN_11), (T.NNWideGrad, T.NN_8)])
def test_backward_refuses_its_arguments_with_the_same_texts(cls, module):
    d = 3
    g = bare(cls, module(d), d, _params=[])
    x = torch.zeros((4, 2, d, d), dtype=torch.uint8)
    a, y = torch.zeros(4, dtype=torch.int64), torch.zeros(4)
    assert message(g.backward, x.to(torch.int32), a, y) == "state dtype torch.int32 not one of float32 / float16 / bfloat16 / uint8"
    assert message(g.backward, x[:, :, :2], a, y) == "expected a (rows, 2, 3, 3) state on cpu, got (4, 2, 2, 3) on cpu"
    assert message(g.backward, x.flatten(1), a, y) == "expected a (rows, 2, 3, 3) state on cpu, got (4, 18) on cpu"
    one_per_record = "actions_idx / y / weights must have one entry per record"
    assert message(g.backward, x, a[:3], y) == one_per_record
    assert message(g.backward, x, a, y[:3]) == one_per_record
    assert message(g.backward, x, a, y, torch.ones(5)) == one_per_record
    assert message(g.backward, x, [0, 1, 2], [0.0, 0.0, 0.0, 0.0]) == one_per_record            # sequences are taken as well
