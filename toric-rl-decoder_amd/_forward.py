"""What the three network families (nn11.py, nnw.py, resnet.py) share above ctypes: the check of a perspective stack,
the C array of a tensor list's pointers, the matcher under both which_net functions, the plain conv net NN_11, NN_8 and
NN_17 are, the base of the forward handles NN11Forward, NNWideForward and ResNetForward, and the base of the learner-step
handles NN11Grad and NNWideGrad."""
import ctypes as C

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _lib
from ._lib import Handle, _ptr, check, require_gpu, to_device

_STACK_DTYPES = {torch.float32: _lib.TQ_F32, torch.float16: _lib.TQ_F16, torch.bfloat16: _lib.TQ_BF16, torch.uint8: _lib.TQ_U8}


def _check_stack(x, d, device, what):
    """A (n, 2, d, d) perspective stack of a dtype the kernels read, on ``device`` -> (contiguous stack, its TQ_* dtype)"""
    if x.dtype not in _STACK_DTYPES:
        raise ValueError(f"{what} dtype {x.dtype} not one of float32 / float16 / bfloat16 / uint8")
    if x.dim() != 4 or tuple(x.shape[1:]) != (2, d, d) or x.device != device:
        raise ValueError(f"expected a (rows, 2, {d}, {d}) {what} on {device}, got {tuple(x.shape)} on {x.device}")
    return x.contiguous(), _STACK_DTYPES[x.dtype]


def _pointers(tensors):
    """tensors (or None) -> the C array of their device pointers (or None)"""
    return None if tensors is None else (C.c_void_p * len(tensors))(*[t.data_ptr() for t in tensors])


def match_net(sd, candidates, names="names", at=""):
    """``candidates``: (net, label, {name: shape}) in turn -> the net whose names and shapes the state_dict ``sd`` has
    exactly; ValueError, with what each candidate differs in, if none."""
    why = []
    for net, label, want in candidates:
        if set(sd.keys()) != set(want):
            why.append(f"{label}: {names} differ in {sorted(set(sd.keys()) ^ set(want))[:6]}")
            continue
        bad = [k for k, s in want.items() if tuple(sd[k].shape) != s]
        if not bad:
            return net
        why.append(f"{label}{at}: {bad[0]} has shape {tuple(sd[bad[0]].shape)}, expected {want[bad[0]]}")
    raise ValueError("state_dict is neither " + " nor ".join(f"{label}'s" for _, label, _ in candidates) + ": " + "; ".join(why))


class PlainConvNet(nn.Module):
    """conv3x3 + ReLU layers of CHANNELS then one linear layer; the first and the last convolution are unpadded after a
    circular pad of 1 (src/nn/torch/util.py:21-26)."""

    CHANNELS = ()

    def __init__(self, system_size, number_of_actions=3, device=None):
        super().__init__()
        ch = self.CHANNELS
        self.layers = len(ch) - 1
        for i in range(self.layers):
            pad = 0 if i in (0, self.layers - 1) else 1
            setattr(self, f"conv{i + 1}", nn.Conv2d(ch[i], ch[i + 1], kernel_size=3, stride=1, padding=pad))
        self.linear1 = nn.Linear(ch[-1] * (system_size - 2) ** 2, number_of_actions)
        self.device = device

    def forward(self, x):
        x = F.pad(x, (1, 1, 1, 1), mode="circular")
        for i in range(self.layers):
            x = F.relu(getattr(self, f"conv{i + 1}")(x))
        return self.linear1(x.flatten(1))


class ForwardHandle(Handle):
    """A network's forward pass behind a library handle, callable like the model it was made from: ``f(persp) -> (rows, 3)``
    float32 tensor on the device.  A subclass names its entry points (``_create``, ``_forward``, ``_destroy``) and has
    ``load(model_or_state_dict)``; what it must refuse before the device is asked for, it refuses before this
    constructor.  ``net``: the arguments of its create call ahead of the lattice size."""

    any_rows = True                 # any row count costs the same per row: _forward_chunked does not pad for it
    gathers = False                 # f(persp, rows) is not offered: a row list goes through _forward_chunked's index_select

    def __init__(self, model_or_state_dict, system_size, device, max_rows, *net):
        self.device = require_gpu(device)
        self.system_size = int(system_size)
        self._L = _lib.load()
        self._h = C.c_void_p(None)
        check(getattr(self._L, self._create)(C.byref(self._h), *net, self.system_size, int(max_rows), self.device.index))
        self.load(model_or_state_dict)

    def _state_dict(self, model_or_state_dict):
        return model_or_state_dict.state_dict() if hasattr(model_or_state_dict, "state_dict") else model_or_state_dict

    def __call__(self, persp):
        persp, dtype = _check_stack(persp, self.system_size, self.device, "stack")
        q = torch.empty((persp.shape[0], 3), dtype=torch.float32, device=self.device)
        self._call(getattr(self._L, self._forward), _ptr(persp), dtype, persp.shape[0], _ptr(q))
        return q

    forward = __call__

    def eval(self):
        return self

    def train(self, mode=True):
        return self

    def to(self, *args, **kwargs):                         # evaluate() moves its model to the device: it is there already
        return self


class GradHandle(Handle):
    """A plain net's learner step behind a library handle: the forward with every layer kept, the gather of Q(s,a), the
    weighted squared error and the backward pass.  ``model``: a torch module on ``device`` whose f32 parameters are the
    masters -- ``backward`` fills their ``.grad`` (written, not accumulated), the caller's optimizer steps them,
    ``load()`` re-reads them.  A subclass names its entry points (``_create``, ``_load``, ``_step``, ``_check``,
    ``_destroy``) and has ``_masters(model)``: the (weight, bias) pairs of its layers, conv1 first and linear1 last, or a
    ValueError for a model it does not take; ``_net(model)`` gives the arguments of its create call ahead of the lattice
    size."""

    def __init__(self, model, system_size, device, max_batch):
        self.device = require_gpu(device)
        self.system_size = int(system_size)
        self.max_batch = int(max_batch)
        self.model = model
        net = self._net(model)                              # a wrong net is refused before the device is asked for
        self._params = self._masters(model)
        self._L = _lib.load()
        self._h = C.c_void_p(None)
        check(getattr(self._L, self._create)(C.byref(self._h), *net, self.system_size, self.max_batch, self.device.index))
        self.load()

    def _net(self, model):
        return ()

    def load(self, model=None):
        """Re-reads the model's parameters (packed on the device, no allocation): after every optimizer step.  ``model``:
        another model that ``_masters`` takes, as the masters from now on."""
        if model is not None:
            self._params, self.model = self._masters(model), model
        self._call(getattr(self._L, self._load), _pointers([w for w, _ in self._params]), _pointers([b for _, b in self._params]))
        return self

    def backward(self, state, actions_idx, y, weights=None):
        """Learner_mp.py:140-160 for one batch: ``state`` (n, 2, d, d) float32 / float16 / bfloat16 / uint8,
        ``actions_idx`` int64 (n,) in 0..2, ``y`` the targets, ``weights`` the importance weights (None: ones) ->
        (loss f32 (n,) = weights * (y - Q(s,a))^2, q f32 (n, 3)); every parameter's ``.grad`` holds the gradient of
        loss.mean().  An action outside 0..2 gets loss 0 and no gradient, and check() raises for it."""
        dev = self.device
        state, dtype = _check_stack(state, self.system_size, dev, "state")
        n = state.shape[0]
        a = to_device(actions_idx, torch.int64, dev).reshape(-1)
        y = to_device(y.detach() if torch.is_tensor(y) else y, torch.float32, dev).reshape(-1)
        w = None if weights is None else to_device(weights, torch.float32, dev).reshape(-1)
        if a.numel() != n or y.numel() != n or (w is not None and w.numel() != n):
            raise ValueError("actions_idx / y / weights must have one entry per record")
        for wt, bt in self._params:
            for p in (wt, bt):
                if p.grad is None or not p.grad.is_contiguous():
                    p.grad = torch.empty_like(p, memory_format=torch.contiguous_format)
        q = torch.empty((n, 3), dtype=torch.float32, device=dev)
        loss = torch.empty(n, dtype=torch.float32, device=dev)
        self._call(getattr(self._L, self._step), _ptr(state), dtype, n, _ptr(a), _ptr(y), _ptr(w), _ptr(q), _ptr(loss),
                   _pointers([wt.grad for wt, _ in self._params]), _pointers([bt.grad for _, bt in self._params]))
        return loss, q

    def check(self):
        """Reads and clears the device error latch (synchronises): ValueError for an action outside 0..2."""
        self._call(getattr(self._L, self._check))
