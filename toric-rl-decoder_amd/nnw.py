"""The reference's two wide Q-networks, NN_8 and NN_17: the torch modules and their hand-written HIP counterparts behind
tq_nnw_*.

Both are restated as torch modules (same parameter names as the reference, so its state_dicts load unchanged); their
forward and their learner step also exist as HIP kernels (csrc/nnw.hpp, csrc/nnw_grad.hpp; numerics contract in
include/toricenv.h).  The optimizer of these nets stays with torch on the f32 parameters.  policy.py re-exports the four
classes.

  NN_8           src/nn/torch/NN.py:47-76   8 conv layers, at most 256 channels
  NN_17          src/nn/torch/NN.py:80-133  20 conv layers despite its name, at most 256 channels
  NNWideForward  either one's forward as bf16 MFMA kernels
  NNWideGrad     src/Learner_mp.py:140-160 for either one (forward, loss head and backward pass as HIP kernels)
"""
import torch

from . import _lib
from ._forward import ForwardHandle, GradHandle, PlainConvNet, _pointers, match_net
from ._lib import to_device

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
    def want(net):
        return {f"{n}.{k}": s for n, shape in zip(names(net), shapes(net, d)) for k, s in (("weight", shape), ("bias", shape[:1]))}
    return match_net(sd, [(net, label, want(net)) for net, label in ((_lib.TQ_NET_NN8, "NN_8"), (_lib.TQ_NET_NN17, "NN_17"))],
                     names="parameter names", at=f" at d={d}")


class NN_8(PlainConvNet):
    """src/nn/torch/NN.py:47-76."""
    CHANNELS = CHANNELS[_lib.TQ_NET_NN8]


class NN_17(PlainConvNet):
    """src/nn/torch/NN.py:80-133: twenty conv layers."""
    CHANNELS = CHANNELS[_lib.TQ_NET_NN17]


class NNWideForward(ForwardHandle):
    """NN_8's or NN_17's forward pass as HIP kernels (tq_nnw_*; numerics contract in include/toricenv.h): bf16 weights
    and activations, f32 accumulation, f32 Q-values.  Callable like the model it was made from -- ``f(persp) -> (rows, 3)``
    float32 tensor on the device, for a perspective stack (rows, 2, d, d) of float32, float16, bfloat16 or uint8 -- so
    every function of this package that takes ``model`` takes it as well.  ``model_or_state_dict``: an NN_8 / NN_17 (or
    the reference's) or its state_dict; which net it is follows from the parameter names and shapes (``net``), and
    anything else is a ValueError.  ``load()`` refreshes the weights of the same net.  Any row count costs the same per
    row (``any_rows``).  It does not gather: a ``rows`` list goes through _forward_chunked's index_select.
    One handle, one stream: calls share the handle's activation scratch, 2 x max_rows x d^2 x 512 bytes (3.7 GB at
    d = 21 with the default; a larger call is walked in passes of ``max_rows``)."""

    _create, _forward, _destroy = "tq_nnw_create", "tq_nnw_forward", "tq_nnw_destroy"

    def __init__(self, model_or_state_dict, system_size, device, max_rows=1 << 13):
        sd = self._state_dict(model_or_state_dict)
        self.net = which_net(sd, int(system_size))              # a wrong net is refused before the device is asked for
        super().__init__(sd, system_size, device, max_rows, self.net)

    def load(self, model_or_state_dict):
        sd = self._state_dict(model_or_state_dict)
        net = which_net(sd, self.system_size)
        if net != self.net:
            raise ValueError(f"this handle was made for net {self.net}, the state_dict is net {net}'s")
        layers = names(net)
        w = [to_device(sd[n + ".weight"].detach(), torch.float32, self.device) for n in layers]
        b = [to_device(sd[n + ".bias"].detach(), torch.float32, self.device) for n in layers]
        self._call(self._L.tq_nnw_load, _pointers(w), _pointers(b))  # the pack kernel reads w / b on the current stream,
        return self                                                  # where any copies made above are freed in stream order


class NNWideGrad(GradHandle):
    """NN_8's or NN_17's learner step as HIP kernels (tq_nnw_grad_*; numerics contract in include/toricenv.h): the
    forward with every layer kept, the gather of Q(s,a), the weighted squared error and the backward pass, bf16 operands
    with f32 accumulation -- NN11Grad's interface, and ``policy.learnerStep`` takes either.  ``model``: a torch NN_8 /
    NN_17 on ``device`` whose f32 parameters are the masters; which net it is follows from its parameter names and shapes
    (``net``).  ``backward`` fills their ``.grad`` (written, not accumulated), the caller's optimizer (torch.optim: these
    nets have no optimizer kernel) steps them, ``load()`` re-reads them.  One handle, one stream; ``max_batch`` (1..4096)
    sizes the scratch: every layer's activation image is kept."""

    _create, _load, _step = "tq_nnw_grad_create", "tq_nnw_grad_load", "tq_nnw_grad_step"
    _check, _destroy = "tq_nnw_grad_check", "tq_nnw_grad_destroy"

    def __init__(self, model, system_size, device, max_batch=256):
        super().__init__(model, system_size, device, max_batch)

    def _net(self, model):
        self.net = which_net(model.state_dict(), self.system_size)
        return (self.net,)

    def _masters(self, model):
        """(weight, bias) per layer of names(net); ValueError unless ``model`` is this handle's net with contiguous float32
        parameters on the device."""
        net = which_net(model.state_dict(), self.system_size)
        if net != self.net:
            raise ValueError(f"this handle was made for net {self.net}, the model is net {net}'s")
        pairs = [(getattr(model, n).weight, getattr(model, n).bias) for n in names(net)]
        for n, pair in zip(names(net), pairs):
            for p in pair:
                if p.dtype != torch.float32 or p.device != self.device or not p.is_contiguous():
                    raise ValueError(f"{n}: expected a contiguous float32 parameter on {self.device}, got {p.dtype} on {p.device}")
        return pairs
