"""The Q-network NN_11: the torch module and its hand-written HIP counterparts behind tq_nn11_*.

NN_11 is restated as a torch module (same parameter names as the reference, so its state_dicts load unchanged); its
forward, learner step and optimizer step also exist as HIP kernels (csrc/nn11*.hpp; numerics contract in
include/toricenv.h).  policy.py re-exports the four classes.

  NN_11          src/nn/torch/NN.py:10-45, src/nn/torch/util.py:21-26
  NN11Forward    the same forward as bf16 MFMA kernels
  NN11Grad       src/Learner_mp.py:140-160 (forward, loss head and backward pass as HIP kernels)
  NN11Optimizer  src/Learner_mp.py:81-84 (Adam / RMSprop on the masters and the re-pack, one HIP launch)
"""
import torch

from . import _lib
from ._forward import ForwardHandle, GradHandle, PlainConvNet, _check_stack, _pointers
from ._lib import _ptr, to_device

CHANNELS = (2, 128, 128, 120, 111, 104, 103, 90, 80, 73, 71, 64)
NAMES = [f"conv{i + 1}" for i in range(11)] + ["linear1"]       # the layers, in the order of every list of 12 below


def shapes(d):
    """The weight shapes of NAMES at lattice size ``d`` (a bias has ``shape[:1]``)."""
    return [(CHANNELS[i + 1], CHANNELS[i], 3, 3) for i in range(11)] + [(3, 64 * (d - 2) ** 2)]


def _check_params(pairs, d, device):
    """``pairs``: (weight, bias) per layer of NAMES.  ValueError unless every tensor is contiguous float32 of NN_11's
    shape on ``device``."""
    for n, pair, shape in zip(NAMES, pairs, shapes(d)):
        for p, want in zip(pair, (shape, shape[:1])):
            if tuple(p.shape) != want or p.dtype != torch.float32 or p.device != device or not p.is_contiguous():
                raise ValueError(f"{n}: expected contiguous float32 {want} on {device}, got {p.dtype} {tuple(p.shape)} on {p.device}")


class NN_11(PlainConvNet):
    """11 conv3x3 + ReLU then one linear layer (src/nn/torch/NN.py:10-45); the first and the last
    convolution are unpadded after a circular pad of 1 (src/nn/torch/util.py:21-26)."""

    CHANNELS = CHANNELS


class NN11Forward(ForwardHandle):
    """NN_11's forward pass as HIP kernels (tq_nn11_*; numerics contract in include/toricenv.h): bf16 weights and
    activations, f32 accumulation, f32 Q-values.  Callable like the model it was made from -- ``f(persp) -> (rows, 3)``
    float32 tensor on the device, for a perspective stack (rows, 2, d, d) of float32, float16, bfloat16 or uint8 -- so
    every function of this package that takes ``model`` takes it as well.  ``model_or_state_dict``: an NN_11 (or the
    reference's) or its state_dict, with exactly NN_11's parameter names; ``load()`` refreshes the weights (packed on the
    device, no allocation).  Any row count costs the same per row (``any_rows``): _forward_chunked does not pad for it.
    One handle, one stream: calls share the handle's activation scratch, sized for ``max_rows`` rows per pass."""

    _create, _forward, _destroy = "tq_nn11_create", "tq_nn11_forward", "tq_nn11_destroy"
    gathers = True                  # f(persp, rows) reads the listed rows itself: _forward_chunked makes no copy of them

    def __init__(self, model_or_state_dict, system_size, device, max_rows=1 << 16):
        super().__init__(model_or_state_dict, system_size, device, max_rows)

    def load(self, model_or_state_dict):
        sd = self._state_dict(model_or_state_dict)
        want = {f"{n}.{k}" for n in NAMES for k in ("weight", "bias")}
        if set(sd.keys()) != want:
            raise ValueError(f"state_dict must have exactly NN_11's parameters; differs in {sorted(set(sd.keys()) ^ want)}")
        w = [to_device(sd[n + ".weight"].detach(), torch.float32, self.device) for n in NAMES]
        b = [to_device(sd[n + ".bias"].detach(), torch.float32, self.device) for n in NAMES]
        _check_params(zip(w, b), self.system_size, self.device)
        self._call(self._L.tq_nn11_load, _pointers(w), _pointers(b))   # the pack kernel reads w / b on the current stream,
        return self                                                    # where any copies made above are freed in stream order

    def __call__(self, persp, rows=None):
        """``rows`` (int32 tensor on the device, any order, repeats allowed): the Q-values of ``persp[rows]`` -- the same
        bits as ``f(persp)[rows]`` -- read from the stack in place (tq_nn11_forward_rows).  An index outside the stack
        gives a Q-row of a zero perspective and makes check() raise."""
        if rows is None:
            return super().__call__(persp)
        persp, dtype = _check_stack(persp, self.system_size, self.device, "stack")
        if rows.dtype != torch.int32 or rows.dim() != 1 or rows.device != self.device:
            raise ValueError(f"rows must be a 1-d int32 tensor on {self.device}, got {rows.dtype} {tuple(rows.shape)} on {rows.device}")
        rows = rows.contiguous()
        q = torch.empty((rows.shape[0], 3), dtype=torch.float32, device=self.device)
        self._call(self._L.tq_nn11_forward_rows, _ptr(persp), dtype, persp.shape[0], _ptr(rows), rows.shape[0], _ptr(q))
        return q

    forward = __call__

    def check(self):
        """Reads and clears the device error latch (synchronises): ValueError for a row index outside the stack."""
        self._call(self._L.tq_nn11_check)


class NN11Grad(GradHandle):
    """NN_11's learner step as HIP kernels (tq_nn11_grad_*; numerics contract in include/toricenv.h): the forward with
    every layer kept, the gather of Q(s,a), the weighted squared error and the backward pass, bf16 operands with f32
    accumulation.  ``model``: a torch NN_11 on ``device`` whose f32 parameters are the masters -- ``backward`` fills their
    ``.grad`` (written, not accumulated), the caller's optimizer steps them, ``load()`` re-reads them.  One handle, one
    stream; ``max_batch`` (1..4096) sizes the scratch."""

    _create, _load, _step = "tq_nn11_grad_create", "tq_nn11_grad_load", "tq_nn11_grad_step"
    _check, _destroy = "tq_nn11_grad_check", "tq_nn11_grad_destroy"

    def __init__(self, model, system_size, device, max_batch=256):
        super().__init__(model, system_size, device, max_batch)

    def _masters(self, model):
        pairs = [(getattr(model, n).weight, getattr(model, n).bias) for n in NAMES]
        _check_params(pairs, self.system_size, self.device)
        return pairs

    def load(self):
        """Re-reads the model's parameters (packed on the device, no allocation): after every optimizer step."""
        return super().load()


class NN11Optimizer:
    """NN_11's optimizer step as one HIP launch (tq_nn11_grad_opt_step; numerics contract in include/toricenv.h): Adam or
    RMSprop (Learner_mp.py:81-84) on the f32 masters of ``grad`` (an NN11Grad) from the ``.grad`` its backward wrote, and
    the re-pack of the handle's bf16 images from the same registers, so no ``grad.load()`` follows (``repacks``).  In place
    of ``torch.optim.Adam(model.parameters(), lr=...)`` / ``RMSprop``; torch's other options (weight decay, amsgrad,
    momentum, centered, maximize) are outside the contract.  ``state_dict()`` / ``load_state_dict()`` speak
    torch.optim's format, so the reference's checkpoints (Learner_mp.py:90) carry over in both directions."""

    repacks = True
    KINDS = {"Adam": _lib.TQ_OPT_ADAM, "RMSprop": _lib.TQ_OPT_RMSPROP}

    def __init__(self, grad, kind="Adam", lr=0.00025, betas=(0.9, 0.999), eps=1e-8, alpha=0.99):
        if kind not in self.KINDS:
            raise ValueError(f"kind must be 'Adam' or 'RMSprop', got {kind!r}")
        self.grad, self.kind = grad, kind
        self._set_hyper(lr, betas, eps, alpha)
        self.step_count = 0
        # in model.parameters() order: conv1.weight, conv1.bias, ..., linear1.weight, linear1.bias
        self._flat = [p for pair in grad._params for p in pair]
        zeros = lambda: [torch.zeros_like(p, memory_format=torch.contiguous_format) for p in self._flat]
        self._m = zeros() if kind == "Adam" else None           # exp_avg
        self._v = zeros()                                       # exp_avg_sq / square_avg

    def _set_hyper(self, lr, betas, eps, alpha):
        lr, b1, b2, eps, alpha = float(lr), float(betas[0]), float(betas[1]), float(eps), float(alpha)
        if not lr >= 0.0 or not eps >= 0.0:
            raise ValueError(f"lr and eps must be >= 0, got {lr} and {eps}")
        if self.kind == "Adam" and not (0.0 <= b1 < 1.0 and 0.0 <= b2 < 1.0):
            raise ValueError(f"betas must be in [0, 1), got {(b1, b2)}")
        if self.kind == "RMSprop" and not 0.0 <= alpha < 1.0:
            raise ValueError(f"alpha must be in [0, 1), got {alpha}")
        self.lr, self.betas, self.eps, self.alpha = lr, (b1, b2), eps, alpha

    def step(self):
        """One update, number ``step_count + 1``, on the current stream: masters, state and the handle's images."""
        for p in self._flat:
            if p.grad is None:
                raise ValueError("a master parameter has no .grad: call NN11Grad.backward first")
            if p.grad.dtype != torch.float32 or not p.grad.is_contiguous() or p.grad.device != p.device:
                raise ValueError("every .grad must be a contiguous float32 tensor on the masters' device")
        grads = [p.grad for p in self._flat]
        # of each list of 24, the weights' pointers and then the biases' (Adam's exp_avg is None for RMSprop)
        args = [_pointers(t and t[k::2]) for t in (self._flat, grads, self._m, self._v) for k in (0, 1)]
        self.grad._call(self.grad._L.tq_nn11_grad_opt_step, self.KINDS[self.kind], self.lr, self.betas[0], self.betas[1], self.eps,
                        self.alpha, self.step_count + 1, *args)
        self.step_count += 1

    def zero_grad(self, set_to_none=False):
        """Nothing to do: NN11Grad.backward writes the gradients, it does not accumulate them."""

    def _torch_twin(self):
        """torch's optimizer of this kind and these hyperparameters on the same parameters (it allocates no state)"""
        if self.kind == "Adam":
            return torch.optim.Adam(self._flat, lr=self.lr, betas=self.betas, eps=self.eps)
        return torch.optim.RMSprop(self._flat, lr=self.lr, alpha=self.alpha, eps=self.eps)

    def state_dict(self):
        """What torch.optim.Adam / RMSprop on ``model.parameters()`` would return after ``step_count`` steps: param_groups
        with torch's own keys, and per parameter {'step', 'exp_avg', 'exp_avg_sq'} or {'step', 'square_avg'} (copies; no
        state before the first step, as in torch)."""
        sd = self._torch_twin().state_dict()
        if self.step_count:
            for i in range(len(self._flat)):
                st = {"step": torch.tensor(float(self.step_count), dtype=torch.float32)}
                if self.kind == "Adam":
                    st["exp_avg"], st["exp_avg_sq"] = self._m[i].clone(), self._v[i].clone()
                else:
                    st["square_avg"] = self._v[i].clone()
                sd["state"][i] = st
        return sd

    def load_state_dict(self, sd):
        """Takes a torch.optim.Adam / RMSprop state_dict of NN_11's 24 parameters: the state is copied in, ``step_count``
        and the hyperparameters are taken from it.  ValueError for an option outside the contract, for step counts that
        differ between parameters and for wrong shapes; nothing is changed then."""
        groups = sd["param_groups"]
        if len(groups) != 1 or len(groups[0]["params"]) != len(self._flat):
            raise ValueError("expected one param_group with NN_11's 24 parameters")
        g = groups[0]
        if ("betas" in g) != (self.kind == "Adam") or ("alpha" in g) != (self.kind == "RMSprop"):
            raise ValueError(f"the state_dict is not torch.optim.{self.kind}'s")
        for key in ("weight_decay", "amsgrad", "maximize", "momentum", "centered"):
            if g.get(key, 0):
                raise ValueError(f"{key}={g[key]!r} is outside NN11Optimizer's contract")
        state, keys = sd["state"], (("exp_avg", "exp_avg_sq") if self.kind == "Adam" else ("square_avg",))
        if state and sorted(state.keys()) != sorted(g["params"]):
            raise ValueError("the state must be empty or hold every parameter")
        steps = {float(st["step"]) for st in state.values()}
        if len(steps) > 1 or any(s < 0 or s != int(s) for s in steps):
            raise ValueError(f"per-parameter step counts differ or are not whole numbers: {sorted(steps)}")
        for i, pid in enumerate(g["params"] if state else ()):
            for k in keys:
                if k not in state[pid] or tuple(state[pid][k].shape) != tuple(self._flat[i].shape):
                    raise ValueError(f"state of parameter {i}: {k} missing or not of shape {tuple(self._flat[i].shape)}")
        self._set_hyper(g["lr"], g.get("betas", self.betas), g["eps"], g.get("alpha", self.alpha))
        self.step_count = int(steps.pop()) if steps else 0
        for i in range(len(self._flat)):
            for k, dst in zip(keys, (self._m, self._v) if self.kind == "Adam" else (self._v,)):
                if state:
                    dst[i].copy_(state[g["params"][i]][k])
                else:
                    dst[i].zero_()
