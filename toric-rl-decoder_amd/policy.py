"""Policy-side glue around the env kernels (callers of the hot path).

The Q-network NN_11 is restated here as a torch module (30 lines, same parameter names as the reference so
its state_dicts load unchanged) so that BASELINE configs[2] ("generatePerspective feeding NN_11 policy for
selectAction") and the evaluation loop can run without the reference's Python.  Its forward pass also exists as
hand-written HIP (csrc/nn11.hpp behind tq_nn11_*): NN11Forward wraps a model's weights and is accepted wherever a
``model`` is.

  selectActionBatch    src/numba/util_actor.py:11-53
  predictMaxOptimized  src/util_learner.py:48-111
  learnerTargets       src/Learner_mp.py:146-151 (targets straight from the device replay memory)
  evaluate             src/evaluation.py:10-124
  NN11Forward          src/nn/torch/NN.py:10-45, src/nn/torch/util.py:21-26 (the forward as bf16 MFMA kernels)
  NN11Grad             src/Learner_mp.py:140-160 (forward, loss head and backward pass as HIP kernels)
  NN11Optimizer        src/Learner_mp.py:81-84 (Adam / RMSprop on the masters and the re-pack, one HIP launch)
  learnerStep          src/Learner_mp.py:135-169 (one learner iteration on a device replay memory)
"""
import ctypes as C

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _lib
from ._lib import Handle, _ptr, _stream, check, require_gpu, to_device
from .envset import EnvSet, ToricEnv, generatePerspectiveBatch


class NN_11(nn.Module):
    """11 conv3x3 + ReLU then one linear layer (src/nn/torch/NN.py:10-45); the first and the last
    convolution are unpadded after a circular pad of 1 (src/nn/torch/util.py:21-26)."""

    CHANNELS = (2, 128, 128, 120, 111, 104, 103, 90, 80, 73, 71, 64)

    def __init__(self, system_size, number_of_actions=3, device=None):
        super().__init__()
        ch = self.CHANNELS
        for i in range(11):
            pad = 0 if i in (0, 10) else 1
            setattr(self, f"conv{i + 1}", nn.Conv2d(ch[i], ch[i + 1], kernel_size=3, stride=1, padding=pad))
        self.linear1 = nn.Linear(64 * (system_size - 2) ** 2, number_of_actions)
        self.device = device

    def forward(self, x):
        x = F.pad(x, (1, 1, 1, 1), mode="circular")
        for i in range(11):
            x = F.relu(getattr(self, f"conv{i + 1}")(x))
        return self.linear1(x.flatten(1))


_STACK_DTYPES = {torch.float32: _lib.TQ_F32, torch.float16: _lib.TQ_F16, torch.bfloat16: _lib.TQ_BF16, torch.uint8: _lib.TQ_U8}


class NN11Forward(Handle):
    """NN_11's forward pass as HIP kernels (tq_nn11_*; numerics contract in include/toricenv.h): bf16 weights and
    activations, f32 accumulation, f32 Q-values.  Callable like the model it was made from -- ``f(persp) -> (rows, 3)``
    float32 tensor on the device, for a perspective stack (rows, 2, d, d) of float32, float16, bfloat16 or uint8 -- so
    every function of this package that takes ``model`` takes it as well.  ``model_or_state_dict``: an NN_11 (or the
    reference's) or its state_dict, with exactly NN_11's parameter names; ``load()`` refreshes the weights (packed on the
    device, no allocation).  Any row count costs the same per row (``any_rows``): _forward_chunked does not pad for it.
    One handle, one stream: calls share the handle's activation scratch, sized for ``max_rows`` rows per pass."""

    any_rows = True
    _destroy = "tq_nn11_destroy"

    def __init__(self, model_or_state_dict, system_size, device, max_rows=1 << 16):
        self.device = require_gpu(device)
        self.system_size = int(system_size)
        self._L = _lib.load()
        self._h = C.c_void_p(None)
        check(self._L.tq_nn11_create(C.byref(self._h), self.system_size, int(max_rows), self.device.index))
        self.load(model_or_state_dict)

    def load(self, model_or_state_dict):
        sd = model_or_state_dict.state_dict() if hasattr(model_or_state_dict, "state_dict") else model_or_state_dict
        names = [f"conv{i + 1}" for i in range(11)] + ["linear1"]
        want = {f"{n}.{k}" for n in names for k in ("weight", "bias")}
        if set(sd.keys()) != want:
            raise ValueError(f"state_dict must have exactly NN_11's parameters; differs in {sorted(set(sd.keys()) ^ want)}")
        ch, feats = NN_11.CHANNELS, 64 * (self.system_size - 2) ** 2
        shapes = [(ch[i + 1], ch[i], 3, 3) for i in range(11)] + [(3, feats)]
        w = [to_device(sd[n + ".weight"].detach(), torch.float32, self.device) for n in names]
        b = [to_device(sd[n + ".bias"].detach(), torch.float32, self.device) for n in names]
        for n, wt, bt, shape in zip(names, w, b, shapes):
            if tuple(wt.shape) != shape or tuple(bt.shape) != shape[:1]:
                raise ValueError(f"{n}: weight {tuple(wt.shape)} / bias {tuple(bt.shape)}, expected {shape} / {shape[:1]}")
        wp = (C.c_void_p * 12)(*[t.data_ptr() for t in w])
        bp = (C.c_void_p * 12)(*[t.data_ptr() for t in b])
        self._call(self._L.tq_nn11_load, wp, bp)           # the pack kernel reads w / b on the current stream, where
        return self                                        # any copies made above are freed in stream order

    def __call__(self, persp):
        if persp.dtype not in _STACK_DTYPES:
            raise ValueError(f"stack dtype {persp.dtype} not one of float32 / float16 / bfloat16 / uint8")
        d = self.system_size
        if persp.dim() != 4 or tuple(persp.shape[1:]) != (2, d, d) or persp.device != self.device:
            raise ValueError(f"expected a (rows, 2, {d}, {d}) stack on {self.device}, got {tuple(persp.shape)} on {persp.device}")
        persp = persp.contiguous()
        q = torch.empty((persp.shape[0], 3), dtype=torch.float32, device=self.device)
        self._call(self._L.tq_nn11_forward, _ptr(persp), _STACK_DTYPES[persp.dtype], persp.shape[0], _ptr(q))
        return q

    forward = __call__

    def eval(self):
        return self

    def train(self, mode=True):
        return self

    def to(self, *args, **kwargs):                         # evaluate() moves its model to the device: it is there already
        return self


_NN11_NAMES = [f"conv{i + 1}" for i in range(11)] + ["linear1"]


class NN11Grad(Handle):
    """NN_11's learner step as HIP kernels (tq_nn11_grad_*; numerics contract in include/toricenv.h): the forward with
    every layer kept, the gather of Q(s,a), the weighted squared error and the backward pass, bf16 operands with f32
    accumulation.  ``model``: a torch NN_11 on ``device`` whose f32 parameters are the masters -- ``backward`` fills their
    ``.grad`` (written, not accumulated), the caller's optimizer steps them, ``load()`` re-reads them.  One handle, one
    stream; ``max_batch`` (1..4096) sizes the scratch."""

    _destroy = "tq_nn11_grad_destroy"

    def __init__(self, model, system_size, device, max_batch=256):
        self.device = require_gpu(device)
        self.system_size = int(system_size)
        self.max_batch = int(max_batch)
        self.model = model
        ch, feats = NN_11.CHANNELS, 64 * (self.system_size - 2) ** 2
        shapes = [(ch[i + 1], ch[i], 3, 3) for i in range(11)] + [(3, feats)]
        self._params = []
        for n, shape in zip(_NN11_NAMES, shapes):
            m = getattr(model, n)
            for p, want in ((m.weight, shape), (m.bias, shape[:1])):
                if tuple(p.shape) != want or p.dtype != torch.float32 or p.device != self.device or not p.is_contiguous():
                    raise ValueError(f"{n}: expected contiguous float32 {want} on {self.device}, got {p.dtype} {tuple(p.shape)} on {p.device}")
            self._params.append((m.weight, m.bias))
        self._L = _lib.load()
        self._h = C.c_void_p(None)
        check(self._L.tq_nn11_grad_create(C.byref(self._h), self.system_size, self.max_batch, self.device.index))
        self.load()

    def load(self):
        """Re-reads the model's parameters (packed on the device, no allocation): after every optimizer step."""
        wp = (C.c_void_p * 12)(*[w.data_ptr() for w, _ in self._params])
        bp = (C.c_void_p * 12)(*[b.data_ptr() for _, b in self._params])
        self._call(self._L.tq_nn11_grad_load, wp, bp)
        return self

    def backward(self, state, actions_idx, y, weights=None):
        """Learner_mp.py:140-160 for one batch: ``state`` (n, 2, d, d) float32 / float16 / bfloat16 / uint8,
        ``actions_idx`` int64 (n,) in 0..2, ``y`` the targets, ``weights`` the importance weights (None: ones) ->
        (loss f32 (n,) = weights * (y - Q(s,a))^2, q f32 (n, 3)); every parameter's ``.grad`` holds the gradient of
        loss.mean().  An action outside 0..2 gets loss 0 and no gradient, and check() raises for it."""
        if state.dtype not in _STACK_DTYPES:
            raise ValueError(f"state dtype {state.dtype} not one of float32 / float16 / bfloat16 / uint8")
        d, dev = self.system_size, self.device
        if state.dim() != 4 or tuple(state.shape[1:]) != (2, d, d) or state.device != dev:
            raise ValueError(f"expected a (n, 2, {d}, {d}) state on {dev}, got {tuple(state.shape)} on {state.device}")
        n = state.shape[0]
        state = state.contiguous()
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
        gw = (C.c_void_p * 12)(*[wt.grad.data_ptr() for wt, _ in self._params])
        gb = (C.c_void_p * 12)(*[bt.grad.data_ptr() for _, bt in self._params])
        self._call(self._L.tq_nn11_grad_step, _ptr(state), _STACK_DTYPES[state.dtype], n, _ptr(a), _ptr(y), _ptr(w), _ptr(q),
                   _ptr(loss), gw, gb)
        return loss, q

    def check(self):
        """Reads and clears the device error latch (synchronises): ValueError for an action outside 0..2."""
        self._call(self._L.tq_nn11_grad_check)


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

    @staticmethod
    def _pointers(tensors, which):
        return None if tensors is None else (C.c_void_p * 12)(*[t.data_ptr() for t in tensors[which::2]])

    def step(self):
        """One update, number ``step_count + 1``, on the current stream: masters, state and the handle's images."""
        for p in self._flat:
            if p.grad is None:
                raise ValueError("a master parameter has no .grad: call NN11Grad.backward first")
            if p.grad.dtype != torch.float32 or not p.grad.is_contiguous() or p.grad.device != p.device:
                raise ValueError("every .grad must be a contiguous float32 tensor on the masters' device")
        grads = [p.grad for p in self._flat]
        args = [self._pointers(t, k) for t in (self._flat, grads, self._m, self._v) for k in (0, 1)]
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


def learnerStep(grad, target_model, memory, optimizer, batch_size, beta, discount=0.95, batch=None):
    """One iteration of Learner_mp.py:135-169 on a device PrioritizedReplayMemory: sample_batch -> learnerTargets on
    ``target_model`` (a torch module or an NN11Forward) -> ``grad.backward`` -> ``optimizer.step()`` on the masters ->
    ``grad.load()`` (not after an optimizer that ``repacks``: NN11Optimizer) -> priority_update(indices, |loss|).  ``batch``: a sample_batch result to step on instead of drawing
    one (its next_state is not used).  -> (loss f32 (B,), indices i64 (B,)) device tensors."""
    if batch is None:
        batch = memory.sample_batch(batch_size, beta, next_state=False)
    state, actions, reward, _, terminal, weights, indices = batch
    y = learnerTargets(target_model, memory, indices, reward, terminal, discount=discount)
    loss, _ = grad.backward(state, actions, y, weights)
    optimizer.step()
    if not getattr(optimizer, "repacks", False):
        grad.load()
    memory.update_priorities(indices, loss.abs())
    return loss, indices


def _forward_chunked(model, persp, chunk, pad_to=1024, backing=None, out=None):
    """model(persp) in chunks of `chunk` rows -> (rows, 3) float32.  The number of perspectives changes every step, and
    every new batch size is a new problem for MIOpen's solver search, so the last, ragged chunk is run at a row count
    rounded up to a multiple of `pad_to` (its surplus Q rows are cut off again): a handful of shapes instead of
    thousands.  The surplus rows come from the slack of ``backing`` -- the re-used stack buffer ``persp`` is a view
    of (EnvSet.reusedStackBacking(): rows past P hold earlier perspectives or zeros) -- when it has enough of it, from a
    zero-filled copy otherwise.  Batch rows do not influence each other, but a different row count may select a
    different convolution kernel and summation order: Q-values agree with the unpadded forward to ~1e-6, bit-identity
    needs ``pad_to=1`` (tests/test_gpu_policy.py pins both, and that the greedy choice is the same on the golden
    weights).  ``out``: optional (>= rows, 3) float32 tensor to receive the Q-values (no torch.cat)."""
    n = persp.shape[0]
    if out is None:
        out = torch.empty((n, 3), dtype=torch.float32, device=persp.device)
    with torch.no_grad():
        for i in range(0, n, chunk):
            x = persp[i:i + chunk]
            r = x.shape[0]
            if r < chunk and pad_to > 1 and r % pad_to and not getattr(model, "any_rows", False):
                rows = min(chunk, (r + pad_to - 1) // pad_to * pad_to)
                if backing is not None and backing.data_ptr() == persp.data_ptr() and backing.shape[0] >= i + rows:
                    xp = backing[i:i + rows]
                else:
                    xp = torch.zeros((rows,) + tuple(x.shape[1:]), dtype=x.dtype, device=x.device)
                    xp[:r] = x
                out[i:i + r] = model(xp)[:r]
            else:
                out[i:i + r] = model(x)
    return out[:n]


def selectActionEnvSet(envs, model, epsilon, dtype=torch.float32, chunk=1 << 16):
    """The reference's selectActionBatch for the lattices that live in ``envs`` (an EnvSet), everything
    on the device: perspectives -> model forward (in chunks) -> epsilon-greedy selection keyed by each
    lattice's own (episode, step) counters.
    -> (actions (N,4), q_values (N,3)); numpy with envs.numpy_io, device tensors otherwise."""
    model.eval()
    io = envs.numpy_io
    envs.numpy_io = False
    try:
        persp, pos, _ = envs.generatePerspectiveReused(dtype=dtype)       # consumed at once by the forward pass
        q = _forward_chunked(model, persp, chunk, backing=envs.reusedStackBacking())
        act, qv = envs.selectAction(q, epsilon, positions=pos)
    finally:
        envs.numpy_io = io
    return envs._out(act, np.int64), envs._out(qv)


# The reference's selectActionBatch draws from numpy's global RNG, which nothing ever seeds
# (numba/util_actor.py:49,97-98).  Here the draws are Philox keyed (seed, state index, call number):
# seed_select() fixes the stream; every selectActionBatch call advances the call number.
_select_rng = {"seed": 0, "calls": 0}


def seed_select(seed, calls=0):
    _select_rng["seed"] = int(seed) & 0xFFFFFFFFFFFFFFFF
    _select_rng["calls"] = int(calls)


def _cuda_only(device):
    dev = torch.device(device)
    if dev.type != "cuda":
        raise ValueError("device must be a cuda (ROCm) device: the toric env has no CPU path")
    return dev


def _select_action_launch(n, q, offsets, pos, eps, launch=True):
    """One tq_states_select_action call for ``n`` states: takes the next call number of the Philox stream (taken
    even when ``launch`` is false) -> (actions i32 (n,4), q_values f32 (n,3)) device tensors."""
    actions = torch.empty((n, 4), dtype=torch.int32, device=q.device)
    qv = torch.empty((n, 3), dtype=torch.float32, device=q.device)
    call = _select_rng["calls"]
    _select_rng["calls"] = call + 1
    if launch:
        with torch.cuda.device(q.device):
            check(_lib.load().tq_states_select_action(n, _ptr(q), _ptr(offsets), _ptr(pos), _ptr(eps),
                                                      _select_rng["seed"], call, 0, _ptr(actions), _ptr(qv), _stream()))
    return actions, qv


def selectActionBatch(number_of_actions, epsilon, grid_shift, toric_size, state, model, device, chunk=1 << 16):
    """Drop-in for src/numba/util_actor.py:11-53 -- same argument names, order and return types:
    ``state`` (N,2,d,d) numpy array (or tensor), ``epsilon`` scalar or (N,) array, ``device`` the
    ROCm device the model lives on -> (actions (N,4) int64 numpy, q_values (N,3) float64 numpy).
    Perspective generation, the model forward and the epsilon-greedy selection (greedy iff
    (1-eps) > U; first maximum in row-major order, :93-95; otherwise a uniform perspective and op,
    :97-98) all run on the device; only the (N,4) / (N,3) results come back.  A state without defects
    (the reference would raise on it, :93) gets action op 0 and zero q_values."""
    if int(number_of_actions) != 3:
        raise ValueError("number_of_actions must be 3 (env.action_space.high[-1], Actor_mp.py:58)")
    dev = _cuda_only(device)
    model.eval()
    persp, pos, counts, offsets = generatePerspectiveBatch(grid_shift, toric_size, state, device=dev, return_offsets=True)
    n = int(counts.numel())
    q = _forward_chunked(model, persp, chunk)
    eps = to_device(np.broadcast_to(np.asarray(epsilon, np.float64), (n,)), torch.float64, persp.device)
    actions, qv = _select_action_launch(n, q, offsets, pos, eps)       # zero states: the shell's ValueError
    return actions.cpu().numpy().astype(np.int64), qv.cpu().numpy().astype(np.float64)


def _selectActionBatch_prime(q_values_table, splice_idx, positions, greedy, device=None):
    """Drop-in for src/numba/util_actor.py:69-107 on the device -- same arguments: the (P,3) Q-table of all
    perspectives, ``splice_idx`` = cumsum of the perspectives per state (:31), ``positions`` (P,3), ``greedy`` bool
    (N,) -> (actions (N,4) float64, q_values (N,3) float64) like the reference's np.empty defaults.  greedy[i]: the
    first (perspective, op) attaining the maximum of the state's slice in row-major order (:93-95); otherwise a
    uniform perspective and op (:97-98) from the Philox stream of seed_select() (upstream: numpy's unseeded global
    RNG).  A state with an empty slice (the reference raises on it) gets action op 0 and zero q_values."""
    dev = _cuda_only(torch.device("cuda", torch.cuda.current_device()) if device is None else device)
    q = to_device(q_values_table, torch.float32, dev)
    sp = to_device(splice_idx, torch.int64, dev)
    n = int(sp.numel())
    offsets = torch.zeros(n + 2, dtype=torch.int64, device=dev)[:n + 1]       # even length behind it: 16-byte aligned rows
    offsets[1:] = sp
    pos = to_device(positions, torch.int32, dev)
    if q.shape[0] != pos.shape[0] or (n and int(sp[-1].item()) != q.shape[0]):
        raise ValueError("q_values_table / positions / splice_idx do not describe the same perspectives")
    g = to_device(greedy, torch.bool, dev)
    if g.numel() != n:
        raise ValueError("greedy must have one entry per state")
    eps = (~g).to(torch.float64).contiguous()                 # greedy iff (1 - eps) > U with U in [0,1): eps 0 -> always, 1 -> never
    actions, qv = _select_action_launch(n, q, offsets, pos, eps, launch=n > 0)     # no states: empty arrays, no launch
    return actions.cpu().numpy().astype(np.float64), qv.cpu().numpy().astype(np.float64)


def segment_max(q_table, offsets, largest=None):
    """out[i] = max of q_table[offsets[i]:offsets[i+1]] (0 for an empty slice); with ``largest``
    (device int32[1]) the reference's zero padding is reproduced."""
    n = int(offsets.numel()) - 1
    out = torch.empty(n, dtype=torch.float32, device=q_table.device)
    with torch.cuda.device(q_table.device):
        check(_lib.load().tq_segment_max(_ptr(q_table.contiguous()), _ptr(offsets), n, _ptr(largest), _ptr(out),
                                         _stream()))
    return out


def predictMaxOptimized(model, batch_state, grid_shift, system_size, device, chunk=1 << 16):
    """util_learner.py:48-111: max Q-value of every state of the batch (0 for terminal states),
    perspectives generated and reduced on the device.  -> float32 tensor (n,) on ``device``."""
    model.eval()
    persp, pos, counts, offsets = generatePerspectiveBatch(grid_shift, system_size, batch_state, device=device,
                                                           return_offsets=True)
    q = _forward_chunked(model, persp, chunk)
    # the reference gives a terminal state one dummy perspective (:74-76), which counts for the padding
    largest = torch.clamp(counts.max(), min=1).to(torch.int32).reshape(1)
    return segment_max(q, offsets, largest)


def td_target(q_table, offsets, reward, terminal, discount, lo=-100.0, hi=100.0):
    """y = clamp(reward + (~terminal).float() * discount * m, lo, hi) with m = segment_max(q_table, offsets, largest)
    -- the reference's zero padding included, the longest slice found on the device -- in one launch (tq_td_target),
    bit-identical to that torch expression.  q_table f32 (P,3), offsets i64 (n+1,), reward f32 (n,), terminal bool
    (n,) -> f32 (n,)."""
    n = int(offsets.numel()) - 1
    dev = q_table.device
    q = to_device(q_table, torch.float32, dev)
    r = to_device(reward, torch.float32, dev)
    t = to_device(terminal, torch.bool, dev)
    if r.numel() != n or t.numel() != n:
        raise ValueError("reward / terminal must have one entry per state")
    y = torch.empty(n, dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        check(_lib.load().tq_td_target(_ptr(q), _ptr(offsets), n, _ptr(r), _ptr(t), float(discount), float(lo), float(hi),
                                       _ptr(y), _stream()))
    return y


def learnerTargets(model, memory, indices, reward, terminal, discount=0.95, chunk=1 << 16):
    """The learner's target side (Learner_mp.py:146-151: predictMaxOptimized on the batch's next_state, then
    ``y = (reward + (~terminal) * discount * target).clamp(-100, 100)``) for a batch drawn from a device
    PrioritizedReplayMemory: the next states' perspectives come straight from the ring's packed planes
    (memory.next_perspectives), the target model runs on them in chunks, and tq_td_target does the reduction and the
    arithmetic.  ``indices`` / ``reward`` / ``terminal``: as sample_batch returned them -> y f32 (n,)."""
    model.eval()
    persp, _, _, offsets = memory.next_perspectives(indices)
    q = _forward_chunked(model, persp, chunk)
    return td_target(q, offsets, reward, terminal, discount)


def _greedy_episodes(envs, model, epsilon, num_of_steps, chunk):
    """The inner loop of evaluation.py:78-110 / results/small_p_error_test.py:131-151 for all lattices of ``envs`` side
    by side: select (policy forward + device selection) -> step, until every lattice is solved or ``num_of_steps``
    steps were taken.  -> dict of device tensors: done (syndrome cleared), steps per episode, sum / count of the
    chosen action's Q-value over all live steps."""
    n = envs.no_envs
    done = torch.zeros(n, dtype=torch.bool, device=envs.device)
    n_steps = torch.zeros(n, dtype=torch.int64, device=envs.device)
    q_sum = torch.zeros((), dtype=torch.float64, device=envs.device)
    q_cnt = torch.zeros((), dtype=torch.int64, device=envs.device)
    for _ in range(int(num_of_steps)):
        act, qv = selectActionEnvSet(envs, model, epsilon, chunk=chunk)    # op 0 for solved lattices
        live = ~done
        chosen = torch.gather(qv, 1, (act[:, 3].long() - 1).clamp(min=0).unsqueeze(1)).squeeze(1)
        q_sum += (chosen.double() * live).sum()
        q_cnt += live.sum()
        n_steps += live
        _, _, term, _ = envs.step(act)
        done = done | term.bool()
        if bool(done.all()):
            break
    return dict(done=done, n_steps=n_steps, q_sum=q_sum, q_cnt=q_cnt)


def _close_p_error(envs, r, gs, round_like_reference):
    """The end of one p_error of evaluate / prediction_smart: the error latch is read, the lattices are freed
    -> (share of episodes solved, share in the ground state, mean steps, mean Q of the chosen actions) from the episodes'
    outcome ``r`` (_greedy_episodes) and ``gs`` (evalGroundState, bool tensor)."""
    steps, mean_q = float(r["n_steps"].double().mean()), float(r["q_sum"] / r["q_cnt"].clamp(min=1))
    if round_like_reference:
        steps, mean_q = np.round(steps, 1), np.round(mean_q, 3)
    envs.check()
    envs.close()
    return float(r["done"].double().mean()), float(gs.double().mean()), steps, mean_q


def _eval_setup(model, env_config, grid_shift, device):
    """What evaluate / prediction_smart do first: the model on ``device`` in eval mode -> the lattice size."""
    model.to(device)
    model.eval()
    size = int(env_config["size"])
    if int(grid_shift) != size // 2:
        raise ValueError("grid_shift must be int(size/2)")
    return size


def evaluate(model, env, env_config, grid_shift, device, prediction_list_p_error, num_of_episodes=1,
             num_actions=3, epsilon=0.0, num_of_steps=50, plot_one_episode=False, minimum_nbr_of_qubit_errors=0,
             seed=0, chunk=1 << 16, round_like_reference=True):
    """evaluation.py:10-124 with the episodes of one p_error run side by side as one EnvSet.
    -> (error_corrected_list, ground_state_list, average_number_of_steps_list, mean_q_list, failed_syndroms).
    ``round_like_reference=False`` leaves steps (1 decimal upstream) and mean Q (3 decimals) unrounded."""
    # like upstream, `minimum_nbr_of_qubit_errors` is accepted and unused: the sampler is chosen by
    # env_config["min_qubit_errors"] (evaluation.py:51)
    size = _eval_setup(model, env_config, grid_shift, device)
    k = len(prediction_list_p_error)
    corrected, ground, steps_avg, mean_q = np.zeros(k), np.zeros(k), np.zeros(k), np.zeros(k)
    failed = []
    for i, p in enumerate(prediction_list_p_error):
        cfg = {"size": size, "min_qubit_errors": int(env_config.get("min_qubit_errors", 0)), "p_error": float(p)}
        envs = EnvSet(ToricEnv(cfg, device=device, seed=seed + i), num_of_episodes, device=device, numpy_io=False)
        envs.resetAll()
        init_q = envs.getQubits().clone()
        r = _greedy_episodes(envs, model, epsilon, num_of_steps, chunk)
        done = r["done"]
        gs = envs.evalGroundState().bool()
        bad = (~done) | (~gs)
        if bool(bad.any()):
            fq = envs.getQubits()[bad].cpu().numpy()
            for a, b in zip(init_q[bad].cpu().numpy(), fq):
                failed += [a, b]
        corrected[i], ground[i], steps_avg[i], mean_q[i] = _close_p_error(envs, r, gs, round_like_reference)
    return corrected, ground, steps_avg, mean_q, failed


# ---- the forced-errors sampler of results/small_p_error_test.py (the reference's second recorded accuracy target)
def generateRandomError(matrix, p_error, rng=np.random):
    """results/small_p_error_test.py:22-31: depolarizing errors -- u ~ U(0,1) per qubit, error iff u < p_error,
    Pauli = randint(3) + 1.  ``matrix``: (..., 2, d, d), only its shape is used (as upstream)."""
    u = rng.uniform(0, 1, size=matrix.shape)
    pauli = rng.integers(3, size=matrix.shape) + 1 if hasattr(rng, "integers") else rng.randint(3, size=matrix.shape) + 1
    return ((u < p_error) * pauli).astype(np.int64)


def generateNRandomErrors(matrix, n, rng=np.random):
    """:34-40: exactly n errors on uniformly chosen distinct qubits, Pauli uniform; batched over leading axes."""
    shape = matrix.shape
    nq = 2 * shape[-1] * shape[-1]
    flat = np.zeros((int(np.prod(shape[:-3], dtype=np.int64)), nq), np.int64)
    pauli = rng.integers(3, size=(flat.shape[0], n)) + 1 if hasattr(rng, "integers") else rng.randint(3, size=(flat.shape[0], n)) + 1
    flat[:, :n] = pauli
    # a uniform shuffle of each row: argsort of iid uniforms
    order = np.argsort(rng.uniform(size=flat.shape), axis=1)
    flat = np.take_along_axis(flat, order, axis=1)
    return flat.reshape(shape)


def generateNPlusQRandomErrors(q, p_error, qubit_matrix, rng=np.random):
    """:43-52: q forced errors plus depolarizing noise at p_error on the OTHER qubits.  Batched: qubit_matrix
    (n, 2, d, d) (or (2, d, d)); only its shape is used."""
    forced = generateNRandomErrors(np.zeros(qubit_matrix.shape, np.int64), q, rng)
    noise = generateRandomError(np.zeros(qubit_matrix.shape), p_error, rng)
    noise[forced != 0] = 0
    return forced + noise


def prediction_smart(model, env, env_config, grid_shift, device, prediction_list_p_error, num_of_episodes=1, epsilon=0.0,
                     num_of_steps=50, plot_one_episode=False, show_network=False, show_plot=False, nbr_of_qubit_errors=0,
                     print_Q_values=False, checkpoint=10000, seed=0, chunk=1 << 16, round_like_reference=True):
    """results/small_p_error_test.py:55-196 with the episodes of one p_error side by side on the GPU: every episode
    starts from ``nbr_of_qubit_errors`` forced errors plus depolarizing noise (generateNPlusQRandomErrors), redrawn
    until the syndrome is not empty (:109-120; a stabilizer-shaped draw has none), written into the lattices with
    ``env.qubit_matrix = ...`` (tq_set_qubits), then the greedy loop and evalGroundState.
    -> (error_corrected_list, ground_state_list, average_number_of_steps_list, mean_q_list,
        number_of_failed_syndroms_list, N_fail, P_l_list, failed_syndromes) as upstream."""
    from math import comb
    size = _eval_setup(model, env_config, grid_shift, device)
    k = len(prediction_list_p_error)
    n_ep, q = int(num_of_episodes), int(nbr_of_qubit_errors)
    max_err = size * size
    ground, corrected, steps_avg, mean_q, P_l_list = (np.zeros(k) for _ in range(5))
    failed = []
    table = np.zeros((3, max_err))
    table[0] = np.arange(max_err)
    N_fail = 0.0
    rng = np.random.default_rng(seed)
    for i, p in enumerate(prediction_list_p_error):
        cfg = {"size": size, "min_qubit_errors": int(env_config.get("min_qubit_errors", 0)), "p_error": float(p)}
        envs = EnvSet(ToricEnv(cfg, device=device, seed=seed + i), n_ep, device=device, numpy_io=False)
        qm = generateNPlusQRandomErrors(q, float(p), np.zeros((n_ep, 2, size, size), np.int64), rng)
        for _ in range(1000):                                   # "while terminal_state": redraw the lattices without a defect
            envs.setQubits(qm.astype(np.uint8))
            empty = envs.isTerminal().bool().cpu().numpy()
            if not empty.any():
                break
            qm[empty] = generateNPlusQRandomErrors(q, float(p), np.zeros((int(empty.sum()), 2, size, size), np.int64), rng)
        else:
            raise RuntimeError("the sampler kept producing empty syndromes")
        flips = (qm != 0).reshape(n_ep, -1).sum(1)
        r = _greedy_episodes(envs, model, epsilon, num_of_steps, chunk)
        gs_dev = envs.evalGroundState().bool()
        gs = gs_dev.cpu().numpy()
        inside = flips < max_err
        np.add.at(table[2], flips[inside & ~gs], 1)
        np.add.at(table[1], flips[inside & gs], 1)
        failed.extend(qm[~gs])
        n_fail = np.array([0.0 if j < q else table[2, j] / comb(j, q) for j in range(max_err)])
        N_fail = float(n_fail.sum())
        nq = 2 * size * size
        P_l_list[i] = comb(nq, q) * float(p) ** q * (1 - float(p)) ** (nq - q) * N_fail / n_ep
        corrected[i], ground[i], steps_avg[i], mean_q[i] = _close_p_error(envs, r, gs_dev, round_like_reference)
    return corrected, ground, steps_avg, mean_q, table, N_fail, P_l_list, failed
