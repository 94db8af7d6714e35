"""The reference launcher's default Q-network, ResNet18, and ResNet34: the torch modules and their hand-written HIP
forward behind tq_resnet_*.

Both are restated as torch modules (same parameter and buffer names as the reference, so its checkpoints load strictly);
their eval-mode forward also exists as HIP kernels (csrc/resnet.hpp; numerics contract in include/toricenv.h).  Forward
only and BatchNorm in inference form only: the learner's ``policy_net.train()`` pass uses batch statistics, and it, the
backward pass and the optimizer stay with torch on the f32 parameters.  policy.py re-exports the three classes.

  ResNet18       src/nn/torch/ResNet.py  ResNet(BasicBlock, [2, 2, 2, 2]), 20 convolutions
  ResNet34       src/nn/torch/ResNet.py  ResNet(BasicBlock, [3, 4, 6, 3]), 36 convolutions
  ResNetForward  either one's eval-mode forward as bf16 MFMA kernels
"""
import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _lib
from ._forward import ForwardHandle, _pointers, match_net
from ._lib import _ptr, to_device

BLOCKS = {_lib.TQ_NET_RESNET18: (2, 2, 2, 2), _lib.TQ_NET_RESNET34: (3, 4, 6, 3)}
PLANES = (64, 128, 256, 512)
STRIDES = (1, 1, 1, 2)                         # of a stage's first block
STEM = 64
BN_KEYS = ("weight", "bias", "running_mean", "running_var")


def convs(net):
    """The convolutions of ``net`` (TQ_NET_RESNET18 / TQ_NET_RESNET34) in state_dict order, the order of tq_resnet_load:
    a list of (conv name, its BatchNorm's name, weight shape)."""
    out = [("conv1", "bn1", (STEM, 2, 3, 3))]
    cin = STEM
    for st, (blocks, planes, stride) in enumerate(zip(BLOCKS[net], PLANES, STRIDES)):
        for b in range(blocks):
            p = f"layer{st + 1}.{b}"
            out.append((f"{p}.conv1", f"{p}.bn1", (planes, cin, 3, 3)))
            out.append((f"{p}.conv2", f"{p}.bn2", (planes, planes, 3, 3)))
            if b == 0 and (stride != 1 or cin != planes):
                out.append((f"{p}.shortcut.0", f"{p}.shortcut.1", (planes, cin, 1, 1)))
            cin = planes
    return out


def shapes(net):
    """name -> shape of every tensor the forward reads (``num_batches_tracked`` is not among them)."""
    want = {}
    for conv, bn, shape in convs(net):
        want[conv + ".weight"] = shape
        for k in BN_KEYS:
            want[f"{bn}.{k}"] = shape[:1]
    want["linear.weight"], want["linear.bias"] = (3, PLANES[-1]), (3,)
    return want


def which_net(sd):
    """The net whose parameter and buffer names and shapes the state_dict has exactly (``num_batches_tracked`` entries
    are ignored); ValueError if neither."""
    read = {k: v for k, v in sd.items() if not k.endswith("num_batches_tracked")}
    return match_net(read, [(net, label, shapes(net)) for net, label in ((_lib.TQ_NET_RESNET18, "ResNet18"), (_lib.TQ_NET_RESNET34, "ResNet34"))])


def _layer_stride(conv):
    """The stride of the convolution ``conv`` of convs(): 2 for the two that leave the full grid."""
    return STRIDES[-1] if conv in ("layer4.0.conv1", "layer4.0.shortcut.0") else 1


def _conv_bn(conv, shape):
    """One entry of convs() as modules: the bias-free convolution, zero padded so that stride 1 keeps the grid, and the
    BatchNorm behind it."""
    cout, cin, k, _ = shape
    return nn.Conv2d(cin, cout, k, _layer_stride(conv), padding=k // 2, bias=False), nn.BatchNorm2d(cout)


class _Block(nn.Module):
    """One residual block from its entries of convs(): two conv + bn pairs, the sum with the block's input -- passed
    through the 1x1 conv + bn of ``shortcut`` where the block has one, an empty container otherwise -- and the ReLU of
    the sum.  Only the attribute names are given: they are the state_dict's keys."""

    def __init__(self, prefix, entries):
        super().__init__()
        cut = []
        for conv, bn, shape in entries:
            mods = _conv_bn(conv, shape)
            if ".shortcut." in conv:
                cut = mods
            else:
                self.add_module(conv[len(prefix) + 1:], mods[0])
                self.add_module(bn[len(prefix) + 1:], mods[1])
        self.shortcut = nn.Sequential(*cut)

    def forward(self, x):
        mid = F.relu(self.bn1(self.conv1(x)))
        return F.relu(self.bn2(self.conv2(mid)) + self.shortcut(x))


class _ResNet(nn.Module):
    """The modules of convs(NET) under the names the state_dict gives them -- the stem's conv + bn, ``layer1`` ..
    ``layer4`` as containers of blocks -- and ``linear`` on the mean over the pixels.  The reference's constructors take
    no argument; the arguments of the other nets are accepted and not needed: the weights do not depend on the lattice
    size."""

    NET = None

    def __init__(self, system_size=None, number_of_actions=3, device=None):
        super().__init__()
        entries = convs(self.NET)
        self.conv1, self.bn1 = _conv_bn(*entries[0][::2])
        blocks = {}                                     # "layer2.0" -> its entries, in convs()'s order
        for e in entries[1:]:
            blocks.setdefault(".".join(e[0].split(".")[:2]), []).append(e)
        for st in range(len(PLANES)):
            mine = [_Block(p, es) for p, es in blocks.items() if p.startswith(f"layer{st + 1}.")]
            setattr(self, f"layer{st + 1}", nn.Sequential(*mine))
        self.linear = nn.Linear(PLANES[-1], number_of_actions)
        self.device = device

    def forward(self, x):
        x = F.relu(self.bn1(self.conv1(x)))
        for st in range(len(PLANES)):
            x = getattr(self, f"layer{st + 1}")(x)
        return self.linear(x.mean((2, 3)))


class ResNet18(_ResNet):
    """src/nn/torch/ResNet.py: ResNet(BasicBlock, [2, 2, 2, 2]), the launcher's default model."""
    NET = _lib.TQ_NET_RESNET18


class ResNet34(_ResNet):
    """src/nn/torch/ResNet.py: ResNet(BasicBlock, [3, 4, 6, 3])."""
    NET = _lib.TQ_NET_RESNET34


class ResNetForward(ForwardHandle):
    """ResNet18's or ResNet34's forward pass as HIP kernels (tq_resnet_*; numerics contract in include/toricenv.h): bf16
    weights and activations, f32 accumulation, BatchNorm folded to an f32 scale and shift, f32 Q-values.  It is the
    EVAL-MODE network -- BatchNorm with its running statistics, what ``model.eval()`` computes under ``no_grad`` in the
    actor, the learner's target network and ``evaluate`` -- and not a training-mode forward: batch statistics, the backward
    pass and the optimizer stay with torch.  Callable like the model it was made from -- ``f(persp) -> (rows, 3)`` float32
    tensor on the device, for a perspective stack (rows, 2, d, d) of float32, float16, bfloat16 or uint8 -- so every
    function of this package that takes ``model`` takes it as well.  ``model_or_state_dict``: a ResNet18 / ResNet34 (or
    the reference's) or its state_dict; which net it is follows from the names and shapes (``net``; ``num_batches_tracked``
    is ignored), and anything else is a ValueError.  ``eps``: the BatchNorm layers' eps; a module's own is taken instead.
    ``load()`` refreshes the weights of the same net.  Any row count costs the same per row (``any_rows``).  It does not
    gather: a ``rows`` list goes through _forward_chunked's index_select.
    One handle, one stream: calls share the handle's activation scratch, 4 x max_rows x d^2 x 512 bytes (0.68 GB at d = 9,
    3.7 GB at d = 21 with the default of 4096 rows; a larger call is walked in passes of ``max_rows``)."""

    _create, _forward, _destroy = "tq_resnet_create", "tq_resnet_forward", "tq_resnet_destroy"

    def __init__(self, model_or_state_dict, system_size, device, max_rows=1 << 12, eps=1e-5):
        self.eps = float(eps)
        self.net = which_net(self._state_dict(model_or_state_dict))  # a wrong net is refused before the device is asked for
        super().__init__(model_or_state_dict, system_size, device, max_rows, self.net)

    def _state_dict(self, model_or_state_dict):
        if not hasattr(model_or_state_dict, "state_dict"):
            return model_or_state_dict
        eps = {m.eps for m in model_or_state_dict.modules() if isinstance(m, nn.modules.batchnorm._BatchNorm)}
        if len(eps) > 1:
            raise ValueError(f"the module's BatchNorm layers have different eps: {sorted(eps)}")
        if eps:
            self.eps = float(eps.pop())
        return model_or_state_dict.state_dict()

    def load(self, model_or_state_dict):
        sd = self._state_dict(model_or_state_dict)
        net = which_net(sd)
        if net != self.net:
            raise ValueError(f"this handle was made for net {self.net}, the state_dict is net {net}'s")
        dev = lambda k: to_device(sd[k].detach(), torch.float32, self.device)
        w = [dev(conv + ".weight") for conv, _, _ in convs(net)]
        bn = [dev(f"{b}.{k}") for _, b, _ in convs(net) for k in BN_KEYS]
        lw, lb = dev("linear.weight"), dev("linear.bias")
        self._call(self._L.tq_resnet_load, _pointers(w), _pointers(bn), _ptr(lw), _ptr(lb), self.eps)   # the pack kernel reads them
        return self                                       # on the current stream, where copies made above are freed in stream order
