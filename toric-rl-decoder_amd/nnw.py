"""The reference's two wide Q-networks, NN_8 and NN_17: the torch modules and their hand-written HIP forward behind
tq_nnw_*.

Both are restated as torch modules (same parameter names as the reference, so its state_dicts load unchanged); their
forward also exists as HIP kernels (csrc/nnw.hpp; numerics contract in include/toricenv.h).  Forward only: the learner
step and the optimizer of these nets stay with torch on the f32 parameters.  policy.py re-exports the three classes.

  NN_8           src/nn/torch/NN.py:47-76   8 conv layers, at most 256 channels
  NN_17          src/nn/torch/NN.py:80-133  20 conv layers despite its name, at most 256 channels
  NNWideForward  either one's forward as bf16 MFMA kernels
"""
import ctypes as C

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _lib
from ._lib import Handle, _ptr, check, require_gpu, to_device
from .nn11 import _check_stack

CHANNELS = {
    _lib.TQ_NET_NN8: (2, 256, 256, 240, 224, 220, 215, 205, 200),
    _lib.TQ_NET_NN17: (2, 256, 256, 251, 250, 240, 240, 235, 233, 233, 229, 225, 223, 220, 220, 220, 215, 214, 205, 204, 200),
}


def names(net):
    """The layers of ``net`` (TQ_NET_NN8 / TQ_NET_NN17), in the order of every per-layer list below."""
    return [f"conv{i + 1}" for i in range(len(CHANNELS[net]) - 1)] + ["linear1"]


def shapes(net, d):
    """The weight shapes of names(net) at lattice size ``d`` (a bias has ``shape[:1]``)."""
    ch = CHANNELS[net]
    return [(ch[i + 1], ch[i], 3, 3) for i in range(len(ch) - 1)] + [(3, ch[-1] * (d - 2) ** 2)]


def which_net(sd, d):
    """The net whose parameter names and shapes at size ``d`` the state_dict has exactly; ValueError if neither."""
    why = []
    for net, label in ((_lib.TQ_NET_NN8, "NN_8"), (_lib.TQ_NET_NN17, "NN_17")):
        want = {f"{n}.{k}": s for n, shape in zip(names(net), shapes(net, d)) for k, s in (("weight", shape), ("bias", shape[:1]))}
        if set(sd.keys()) != set(want):
            why.append(f"{label}: parameter names differ in {sorted(set(sd.keys()) ^ set(want))[:6]}")
            continue
        bad = [k for k, s in want.items() if tuple(sd[k].shape) != s]
        if not bad:
            return net
        why.append(f"{label} at d={d}: {bad[0]} has shape {tuple(sd[bad[0]].shape)}, expected {want[bad[0]]}")
    raise ValueError("state_dict is neither NN_8's nor NN_17's: " + "; ".join(why))


class _WideNet(nn.Module):
    """conv3x3 + ReLU layers then one linear layer; the first and the last convolution are unpadded after a circular
    pad of 1 (src/nn/torch/util.py:21-26)."""

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


class NN_8(_WideNet):
    """src/nn/torch/NN.py:47-76."""
    CHANNELS = CHANNELS[_lib.TQ_NET_NN8]


class NN_17(_WideNet):
    """src/nn/torch/NN.py:80-133: twenty conv layers."""
    CHANNELS = CHANNELS[_lib.TQ_NET_NN17]


class NNWideForward(Handle):
    """NN_8's or NN_17's forward pass as HIP kernels (tq_nnw_*; numerics contract in include/toricenv.h): bf16 weights
    and activations, f32 accumulation, f32 Q-values.  Callable like the model it was made from -- ``f(persp) -> (rows, 3)``
    float32 tensor on the device, for a perspective stack (rows, 2, d, d) of float32, float16, bfloat16 or uint8 -- so
    every function of this package that takes ``model`` takes it as well.  ``model_or_state_dict``: an NN_8 / NN_17 (or
    the reference's) or its state_dict; which net it is follows from the parameter names and shapes (``net``), and
    anything else is a ValueError.  ``load()`` refreshes the weights of the same net.  Any row count costs the same per
    row (``any_rows``).  It does not gather: a ``rows`` list goes through _forward_chunked's index_select.
    One handle, one stream: calls share the handle's activation scratch, 2 x max_rows x d^2 x 512 bytes (3.7 GB at
    d = 21 with the default; a larger call is walked in passes of ``max_rows``)."""

    any_rows = True
    gathers = False
    _destroy = "tq_nnw_destroy"

    def __init__(self, model_or_state_dict, system_size, device, max_rows=1 << 13):
        self.system_size = int(system_size)
        sd = self._state_dict(model_or_state_dict)
        self.net = which_net(sd, self.system_size)
        self.device = require_gpu(device)
        self._L = _lib.load()
        self._h = C.c_void_p(None)
        check(self._L.tq_nnw_create(C.byref(self._h), self.net, self.system_size, int(max_rows), self.device.index))
        self.load(sd)

    @staticmethod
    def _state_dict(model_or_state_dict):
        return model_or_state_dict.state_dict() if hasattr(model_or_state_dict, "state_dict") else model_or_state_dict

    def load(self, model_or_state_dict):
        sd = self._state_dict(model_or_state_dict)
        net = which_net(sd, self.system_size)
        if net != self.net:
            raise ValueError(f"this handle was made for net {self.net}, the state_dict is net {net}'s")
        layers = names(net)
        w = [to_device(sd[n + ".weight"].detach(), torch.float32, self.device) for n in layers]
        b = [to_device(sd[n + ".bias"].detach(), torch.float32, self.device) for n in layers]
        ptrs = lambda ts: (C.c_void_p * len(ts))(*[t.data_ptr() for t in ts])
        self._call(self._L.tq_nnw_load, ptrs(w), ptrs(b))           # the pack kernel reads w / b on the current stream,
        return self                                                 # where any copies made above are freed in stream order

    def __call__(self, persp):
        persp, dtype = _check_stack(persp, self.system_size, self.device, "stack")
        q = torch.empty((persp.shape[0], 3), dtype=torch.float32, device=self.device)
        self._call(self._L.tq_nnw_forward, _ptr(persp), dtype, persp.shape[0], _ptr(q))
        return q

    forward = __call__

    def eval(self):
        return self

    def train(self, mode=True):
        return self

    def to(self, *args, **kwargs):                         # evaluate() moves its model to the device: it is there already
        return self
