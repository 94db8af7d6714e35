"""Prioritized replay memory on the device (tq_replay_*, include/toricenv.h).

The reference's PrioritizedReplayMemory / SumTree (src/ReplayMemory.py:45-152, src/SumTree.py) with its methods, plus
a device path: transitions come in as packed TransitionBlocks or gather-ring rows (the wire format) and learner batches
go out as device tensors -- the 7-tuple of dataToBatch (src/util_learner.py:7-46) -- so nothing crosses PCIe between
the actors and the learner.  The sum tree is f64 and canonical (every internal node is fl(left + right)); draws follow
the reference's sequential sampling exactly (the swap in IO_mp.py / Learner_mp.py and the quirks).
"""
import ctypes as C

import numpy as np
import torch

from . import _lib, wire
from ._lib import Handle, _ptr, _stream, check, to_device
from .envset import _DTYPES
from .transition import TransitionBlock

MAX_BATCH = 4096


def block_capacity(d, nbytes):
    """Slots of a packed block of ``nbytes`` bytes (the inverse of wire.block_bytes); ValueError if none fits exactly."""
    lo, hi = 0, max(1, int(nbytes))
    while lo < hi:                                  # block_bytes is strictly increasing in cap
        mid = (lo + hi) // 2
        if wire.block_bytes(d, mid) < nbytes:
            lo = mid + 1
        else:
            hi = mid
    if wire.block_bytes(d, lo) != nbytes:
        raise ValueError(f"{nbytes} bytes is not the size of a packed d={d} block")
    return lo


class PrioritizedReplayMemory(Handle):
    """PrioritizedReplayMemory(memory_size, alpha) (ReplayMemory.py:45-75) held on ``device``.

    ``d``: lattice size of the records; ``seed``: key of the handle's own uniforms (RNG domain 5);
    ``faithful`` (default True) keeps the reference's two exponent quirks -- sample's "revert" sets every picked leaf
    to leaf**alpha, reset_alpha computes (leaf**-alpha_old)**alpha_new; False leaves the tree untouched by a sample and
    inverts the old exponent (leaf**(1/alpha_old))**alpha_new.  One handle, one stream: issue the calls on one stream.
    """

    def __init__(self, memory_size, alpha, d=7, device="cuda", seed=0, faithful=True):
        self._L = _lib.load()
        self.memory_size, self.alpha, self.size = int(memory_size), float(alpha), int(d)
        self.faithful = bool(faithful)
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise ValueError("the replay memory lives on a GPU (device='cuda[:k]')")
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device() if torch.cuda.is_available() else 0)
        self._h = C.c_void_p(None)
        check(self._L.tq_replay_create(C.byref(self._h), self.size, self.memory_size, self.alpha, self.device.index,
                                       int(seed) & ((1 << 64) - 1), int(self.faithful)))

    _destroy = "tq_replay_destroy"

    # ---------------------------------------------------------------- ingest
    def save_block(self, block):
        """``replay_memory.save(t, p)`` for every transition of a packed block (IO_mp.py:60-66): a TransitionBlock, or
        a uint8 device tensor holding one block (a gather-ring row, ``TransitionGather.ring[slot, r]``).  Non-empty
        slots are appended in slot order; leaf = float64(priority_f32)**alpha.  No synchronisation."""
        if isinstance(block, TransitionBlock):
            if block.d != self.size:
                raise ValueError(f"block of d={block.d} for a d={self.size} memory")
            if block.buf.device != self.device:
                raise ValueError(f"block on {block.buf.device} for a memory on {self.device}")
            buf, cap = block.buf, block.capacity
        else:
            buf = block
            if not torch.is_tensor(buf) or buf.dtype != torch.uint8 or buf.device != self.device or buf.dim() != 1:
                raise ValueError("block must be a TransitionBlock or a 1-D uint8 tensor on the memory's device")
            if not buf.is_contiguous():
                raise ValueError("block tensor must be contiguous")
            cap = block_capacity(self.size, buf.numel())
        self._call(self._L.tq_replay_save_block, _ptr(buf), int(cap))

    def save(self, data, priority):
        """PrioritizedReplayMemory.save (ReplayMemory.py:67-77) of one record of the reference's transition type
        (wire.transition_type: perspective, action (position, op), reward, next_perspective, terminal).  One upload and
        one ingest per call -- for parity; production feeds whole blocks to save_block.  The priority travels as f32,
        the wire field's width."""
        rec = np.asarray(data, dtype=wire.transition_type(self.size)).reshape(1)
        op = int(rec['action']['op'][0])
        if not 1 <= op <= 3:
            raise ValueError("a record's op must be in 1..3")
        action = np.concatenate([rec['action']['position'][0], [op]]).reshape(1, 4)
        buf = wire.encode(self.size, rec['perspective'], rec['next_perspective'], action, rec['reward'], rec['terminal'],
                          priority=[priority])
        self.save_block(torch.from_numpy(buf).to(self.device))

    # ---------------------------------------------------------------- queries
    def filled_size(self):
        with torch.cuda.device(self.device):
            n = self._L.tq_replay_filled(self._h, _stream())
        if n < 0:
            check(int(n))
        return int(n)

    def check(self):
        """Reads and clears the device error latch (synchronises): ValueError for an index outside [0, filled), a draw
        that ended on an empty leaf, or offsets next_perspectives' stack write refused; ToricEnvError for a sample of
        more records than are filled, or a stack that did not fit its buffer."""
        self._call(self._L.tq_replay_check)

    def leaves(self):
        out = torch.empty(self.memory_size, dtype=torch.float64, device=self.device)
        self._call(self._L.tq_replay_leaves, _ptr(out))
        return out

    def tree(self):
        out = torch.empty(int(self._L.tq_replay_tree_nodes(self._h)), dtype=torch.float64, device=self.device)
        self._call(self._L.tq_replay_tree, _ptr(out))
        return out

    def _batch_outputs(self, n, next_state=True):
        d, dev = self.size, self.device
        return dict(state=torch.empty((n, 2, d, d), dtype=torch.float32, device=dev),
                    next_state=torch.empty((n, 2, d, d), dtype=torch.float32, device=dev) if next_state else None,
                    actions=torch.empty(n, dtype=torch.int64, device=dev),
                    reward=torch.empty(n, dtype=torch.float32, device=dev),
                    terminal=torch.empty(n, dtype=torch.bool, device=dev),
                    action=torch.empty((n, 4), dtype=torch.int32, device=dev))

    def get(self, indices):
        """Records at ``indices`` (int64 device tensor or sequence) -> dict of device tensors: state / next_state
        f32 (n,2,d,d), actions i64 (op - 1), reward f32, terminal bool, action i32 (n,4) (the raw [layer,row,col,op])."""
        idx = to_device(indices, torch.int64, self.device)
        out = self._batch_outputs(idx.numel())
        self._call(self._L.tq_replay_get, _ptr(idx), int(idx.numel()), _ptr(out["state"]), _ptr(out["next_state"]),
                   _ptr(out["actions"]), _ptr(out["reward"]), _ptr(out["terminal"]), _ptr(out["action"]))
        return out

    def next_perspectives(self, indices, dtype=torch.float32):
        """generatePerspectiveBatch(..., return_offsets=True) of the NEXT states of the records at ``indices`` (int64
        device tensor or sequence, 1..4096 of them), read from the ring's packed planes as they are -- no f32
        next_state, no u8 cast, no re-packing -> (stack (P,2,d,d) ``dtype``, positions (P,3) i32, counts i32 (n,),
        offsets i64 (n+1,)).  An index outside [0, filled) (the -1 of an under-filled sample_batch) counts 0 and latches
        an error for check().  One 8-byte read-back of P, as in generatePerspectiveBatch."""
        idx = to_device(indices, torch.int64, self.device).reshape(-1)
        n, d = int(idx.numel()), self.size
        if not 1 <= n <= MAX_BATCH:
            raise ValueError(f"need 1..{MAX_BATCH} indices")
        if dtype not in _DTYPES:
            raise ValueError(f"unsupported stack dtype {dtype}")
        counts = torch.empty(n, dtype=torch.int32, device=self.device)
        offsets = torch.empty(n + 1, dtype=torch.int64, device=self.device)
        self._call(self._L.tq_replay_next_persp_count, _ptr(idx), n, _ptr(counts), _ptr(offsets))
        P = int(offsets[-1].item())
        out = torch.empty((P, 2, d, d), dtype=dtype, device=self.device)
        pos = torch.empty((P, 3), dtype=torch.int32, device=self.device)
        if P:
            self._call(self._L.tq_replay_next_persp_write, _ptr(idx), n, _ptr(offsets), _ptr(out), _ptr(pos), P,
                       _DTYPES[dtype])
        return out, pos, counts, offsets

    # ---------------------------------------------------------------- sampling
    def _uniforms(self, u, n):
        u = to_device(u, torch.float64, self.device)
        if u is not None and u.numel() != n:
            raise ValueError("need one uniform per draw")
        return u

    def _sample(self, batch_size, beta, uniforms, records, next_state=True):
        n = int(batch_size)
        if not 1 <= n <= MAX_BATCH:
            raise ValueError(f"batch_size must be in 1..{MAX_BATCH}")
        u = self._uniforms(uniforms, n)
        idx = torch.empty(n, dtype=torch.int64, device=self.device)
        prio = torch.empty(n, dtype=torch.float64, device=self.device)
        w = torch.empty(n, dtype=torch.float64, device=self.device)
        out = self._batch_outputs(n, next_state) if records else {}
        g = lambda k: _ptr(out.get(k))
        self._call(self._L.tq_replay_sample, n, float(beta), _ptr(u), _ptr(idx), _ptr(prio), _ptr(w), g("state"),
                   g("next_state"), g("actions"), g("reward"), g("terminal"), g("action"))
        return idx, prio, w, out

    def sample(self, batch_size, beta, uniforms=None):
        """PrioritizedReplayMemory.sample (ReplayMemory.py:85-124) -> (records, weights, indices, priorities) on the
        host: records of wire.transition_type, weights / priorities float64, indices int64; (None, None, None) when
        fewer than ``batch_size`` records are held, as upstream.  ``uniforms``: the B values random.random() would have
        given, else the handle's own stream.  Synchronises."""
        if self.filled_size() < int(batch_size):
            return None, None, None
        idx, prio, w, out = self._sample(batch_size, beta, uniforms, True)
        self.check()
        a = out["action"].cpu().numpy()
        dec = dict(perspective=out["state"].cpu().numpy().astype(np.uint8),
                   next_perspective=out["next_state"].cpu().numpy().astype(np.uint8), action=a,
                   reward=out["reward"].cpu().numpy(), terminal=out["terminal"].cpu().numpy(),
                   priority=np.zeros(a.shape[0], np.float32))
        records, _ = wire.to_records(dec, self.size)
        return records, w.cpu().numpy(), idx.cpu().numpy(), prio.cpu().numpy()

    def sample_batch(self, batch_size, beta, uniforms=None, next_state=True):
        """sample + dataToBatch (util_learner.py:7-46) without leaving the device -> (state f32 (B,2,d,d), actions i64
        (op - 1), reward f32, next_state f32 (B,2,d,d), terminal bool, weights f32, indices i64), all device tensors.
        ``next_state=False``: the f32 next_state is neither allocated nor written and None stands in its place (a
        learner that takes its targets from policy.learnerTargets reads the next states from the ring by index).
        No synchronisation: an under-filled memory latches an error that check() reports."""
        idx, _, w, out = self._sample(batch_size, beta, uniforms, True, next_state)
        return out["state"], out["actions"], out["reward"], out["next_state"], out["terminal"], w.to(torch.float32), idx

    # ---------------------------------------------------------------- priorities
    def update_priorities(self, indices, priorities):
        """priority_update on device tensors (Learner_mp.py:160-169 -> IO_mp.py): leaf = priority**alpha, last
        occurrence of an index wins."""
        idx = to_device(indices, torch.int64, self.device).reshape(-1)
        p = to_device(priorities, torch.float64, self.device).reshape(-1)
        if idx.numel() != p.numel():
            raise ValueError("indices and priorities differ in length")
        self._call(self._L.tq_replay_update, _ptr(idx), _ptr(p), int(idx.numel()))

    def priority_update(self, indices, priorities):
        """PrioritizedReplayMemory.priority_update (ReplayMemory.py:126-133)."""
        self.update_priorities(np.asarray(indices, np.int64), np.asarray(priorities, np.float64))

    def reset_alpha(self, alpha):
        """PrioritizedReplayMemory.reset_alpha (ReplayMemory.py:135-145); a zero leaf stays 0 (the reference raises)."""
        self._call(self._L.tq_replay_reset_alpha, float(alpha))
        self.alpha = float(alpha)
