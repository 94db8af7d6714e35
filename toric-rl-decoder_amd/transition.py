"""Transition records on the device: the packed block the actor loop fills (layout: include/toricenv.h), the
reference's stateless ``generateTransitionParallel`` and the way from either to the reference's record array."""
import numpy as np
import torch

from . import _lib, wire
from ._lib import _ptr, _stream, check, require_gpu, to_device


def transition_outputs(n, d, device):
    """The output tensors every transition kernel fills: perspective / next_perspective u8 (n,2,d,d), action i32 (n,4)."""
    return dict(perspective=torch.empty((n, 2, d, d), dtype=torch.uint8, device=device),
                next_perspective=torch.empty((n, 2, d, d), dtype=torch.uint8, device=device),
                action=torch.empty((n, 4), dtype=torch.int32, device=device))


class TransitionBlock:
    """Packed transition block on the device (layout: include/toricenv.h)."""

    def __init__(self, d, capacity, device):
        self.d, self.capacity = int(d), int(capacity)
        nbytes = _lib.load().tq_transition_block_bytes(self.d, self.capacity)
        if nbytes < 0:
            raise ValueError("bad transition block shape")
        self.buf = torch.zeros(max(int(nbytes), 8), dtype=torch.uint8, device=device)

    @property
    def nbytes(self):
        return int(self.buf.numel())

    def unpack(self, first=0, count=None, buf=None):
        """-> dict of device tensors (perspective u8, next_perspective u8, action i32[n,4],
        reward f32, terminal u8, priority f32) for slots [first, first+count).  Slots without a
        transition have action op 0 (include/toricenv.h)."""
        buf = self.buf if buf is None else buf
        count = self.capacity - first if count is None else int(count)
        d, dev = self.d, buf.device
        out = dict(transition_outputs(count, d, dev),
                   reward=torch.empty(count, dtype=torch.float32, device=dev),
                   terminal=torch.empty(count, dtype=torch.uint8, device=dev),
                   priority=torch.empty(count, dtype=torch.float32, device=dev))
        with torch.cuda.device(dev):
            check(_lib.load().tq_transition_unpack(d, _ptr(buf), self.capacity, int(first), count,
                                                   _ptr(out["perspective"]), _ptr(out["next_perspective"]),
                                                   _ptr(out["action"]), _ptr(out["reward"]),
                                                   _ptr(out["terminal"]), _ptr(out["priority"]), _stream()))
        return out

    def computePriorities(self, no_envs, steps, q_values=None, discount=0.95):
        """computePrioritiesParallel (util_actor.py:268-287) into the block's priority section for
        the ``steps`` steps of ``no_envs`` lattices it holds (slot t*no_envs + e).  ``q_values``:
        device f32 (steps+1, no_envs, 3) -- the q_values of every step plus the step after -- or
        None for all-zero Q (pure exploration).  No synchronisation."""
        if q_values is not None:
            if (q_values.dtype != torch.float32 or not q_values.is_contiguous()
                    or q_values.numel() != (int(steps) + 1) * int(no_envs) * 3 or q_values.device != self.buf.device):
                raise ValueError("q_values must be a contiguous float32 device tensor of shape (steps+1, no_envs, 3)")
        with torch.cuda.device(self.buf.device):
            check(_lib.load().tq_block_priorities(self.d, _ptr(self.buf), self.capacity, int(no_envs), int(steps),
                                                  _ptr(q_values), float(discount), _stream()))


transition_dtype = wire.transition_type     # the reference's replay record (Actor_mp.py:52-56, util.py:10)


def to_structured(unpacked, size):
    """dict from TransitionBlock.unpack / generateTransition -> numpy array of transition_dtype."""
    n = unpacked["perspective"].shape[0]
    rec = np.empty(n, dtype=transition_dtype(size))
    get = lambda k: unpacked[k].cpu().numpy() if torch.is_tensor(unpacked[k]) else np.asarray(unpacked[k])
    a = get("action")
    rec['perspective'] = get("perspective")
    rec['next_perspective'] = get("next_perspective")
    rec['action']['position'] = a[:, :3]
    rec['action']['op'] = a[:, 3]
    rec['reward'] = get("reward")
    rec['terminal'] = get("terminal").astype(bool)
    return rec


def generateTransitionParallel(action, reward, state, next_state, terminal_state, grid_shift, trans_type=None,
                               device=None):
    """Drop-in for src/util_actor.py:223-264 on the GPU: same arguments, returns a numpy record
    array of ``trans_type`` (default: transition_dtype(size), Actor_mp.py:52-56)."""
    dev = require_gpu(device)
    st, nst = to_device(state, torch.uint8, dev), to_device(next_state, torch.uint8, dev)
    act = to_device(action, torch.int32, dev)
    n, d = int(nst.shape[0]), int(nst.shape[-1])
    if int(grid_shift) != d // 2:
        raise ValueError("grid_shift must be int(toric_size/2) (Actor_mp.py:59)")
    out = transition_outputs(n, d, dev)
    L = _lib.load()
    with torch.cuda.device(dev):
        check(L.tq_states_transition(d, n, _ptr(st), _ptr(nst), _ptr(act), _ptr(out["perspective"]),
                                     _ptr(out["next_perspective"]), _ptr(out["action"]), _stream()))
        check(L.tq_states_check(_stream()))                       # bad action -> ValueError
    out["reward"] = np.asarray(reward, np.float64)
    out["terminal"] = np.asarray(terminal_state, bool)
    rec = to_structured(out, d)
    return rec if trans_type is None else rec.astype(trans_type)
