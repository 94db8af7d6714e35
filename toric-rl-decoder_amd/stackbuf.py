"""Which device buffer a perspective stack is written to.

On MI355X the rate of a write stream into a buffer depends on the buffer AND on the stream's shape (5.2-6.9 TB/s for
the stack write, from allocation to allocation: profiles/r04_stream_tune_d7_all.txt), and a caller writes the same
buffer every step.  So this module owns the two kinds of allocation a stack can come from (torch.empty, and
tq_stack_alloc's 2 MiB chunks: :func:`alloc_chunked`), and the set-up probe behind ``EnvSet.pickStackBuffer`` that times
the write on several candidates and keeps the fastest.  The probe is split into its decisions -- plain functions of
numbers, checked without a GPU by tests/test_stack_probe_host.py -- and its device steps (allocate, time, check the
workgroup shares); ``EnvSet.pickStackBuffer`` is the sequence of them.
"""
import ctypes as C

import numpy as np
import torch

from . import _lib
from ._lib import check, require_gpu

# All candidates exist at once while the timing runs: never more of them than this share of the free device memory holds.
FREE_MEMORY_SHARE = 0.5
# "Nobody stands out": every candidate's median within 7 % of candidate 0's.  On some boxes the first tens of GB a
# process allocates ALL write at the slow rate and faster buffers only turn up behind them (profiles/README.md, round 4:
# 24 x 2.5 GB at 0.358-0.368 ms, then, for the next leg, candidates 12 and 16-20 of 24 x 5 GB at 0.57 against 0.71 ms),
# so the search then goes on once, with as many candidates again, WHILE the first ones stay allocated.
EXTEND_WITHIN = 0.93
EXTEND_MIN_MS = 0.1             # ... but a write of under 0.1 ms is not about bandwidth
# The "uniform" note of the report: no candidate more than 10 % faster than candidate 0 -- on some boxes every buffer,
# and every write stream, runs at one rate (profiles/r03_stack_write_ab.txt).
UNIFORM_WITHIN = 0.9
UNIFORM_NOTE = ("no candidate writes more than 10 % faster than candidate 0: on some boxes every buffer -- and "
                "every write stream, hipMemset included -- runs at one rate (profiles/r03_stack_write_ab.txt)")
# Unequal workgroup shares (toricenv.h: tq_set_xcd_bias) are only ever used by the write of d >= 7 stacks that are not u8.
SHARES_MIN_SIZE = 7
TORCH_EMPTY, CHUNKED, REPROBED = "torch.empty", "alloc_stack (2 MiB chunks)", "re-probed"      # report["kinds"]


# ---------------------------------------------------------------------- the two kinds of allocation
class _ChunkedBuffer:
    """Device memory from tq_stack_alloc, exposed through __cuda_array_interface__ and freed with the last tensor
    that views it."""

    def __init__(self, nbytes, device):
        self.ptr = C.c_void_p(None)
        self.nbytes = int(nbytes)
        self._L = _lib.load()
        check(self._L.tq_stack_alloc(device.index, self.nbytes, C.byref(self.ptr)))
        self.__cuda_array_interface__ = {"shape": (self.nbytes,), "typestr": "|u1", "data": (self.ptr.value, False), "version": 2}

    def __del__(self):
        try:
            if self.ptr.value:
                self._L.tq_stack_free(self.ptr)
                self.ptr = C.c_void_p(None)
        except Exception:
            pass


def alloc_chunked(shape, dtype=torch.float32, device=None):
    """A device tensor of ``shape`` / ``dtype`` in tq_stack_alloc memory: 2 MiB physical chunks behind one virtual
    range, zero-filled, every page verified to be reached through its own address (include/toricenv.h).  The kind of
    allocation the stack write ran fastest on in most processes of round 3 (6.5-6.8 TB/s against 5.1-5.5 into
    torch.empty buffers; on some boxes no kind is faster than another).  The memory is released when the returned
    tensor (and every view of it) is gone."""
    dev = require_gpu(device)
    shape = tuple(int(x) for x in (shape if isinstance(shape, (tuple, list, torch.Size)) else (shape,)))
    nbytes = int(np.prod(shape, dtype=np.int64)) * torch.empty((), dtype=dtype).element_size()
    holder = _ChunkedBuffer(max(nbytes, 16), dev)
    with torch.cuda.device(dev):
        flat = torch.as_tensor(holder, device=dev)            # zero-copy view; keeps `holder` alive
    return flat[:nbytes].view(dtype).view(shape)


def alloc_stack(capacity, size, dtype=torch.float32, device=None):
    """A stack buffer (capacity, 2, d, d) of ``dtype`` from alloc_chunked (tq_stack_alloc)."""
    return alloc_chunked((int(capacity), 2, int(size), int(size)), dtype, device)


def alloc_kind(kind, shape, dtype, device):
    """A buffer of ``kind``: "chunked" = alloc_chunked -- torch.empty where the driver has no virtual-memory API (or no
    memory for the chunks) --, any other = torch.empty.  -> (tensor, the kind it came from)."""
    if kind == "chunked":
        try:
            return alloc_chunked(shape, dtype, device), kind
        except _lib.ToricEnvError:
            kind = "torch"
    return torch.empty(shape, dtype=dtype, device=device), kind


# ---------------------------------------------------------------------- the workgroup-share setting
def configured_xcd_bias():
    """The process-wide workgroup-share setting (toricenv.h: tq_set_xcd_bias; the library's default or TORICENV_XCD_BIAS).
    pickStackBuffer's check decides per EnvSet (tq_env_set_xcd_bias) and leaves this alone."""
    return int(_lib.load().tq_get_xcd_bias())


def set_xcd_bias(bias):
    """tq_set_xcd_bias for this process."""
    check(_lib.load().tq_set_xcd_bias(int(bias)))


# ---------------------------------------------------------------------- the probe's decisions (host arithmetic only)
def candidate_kind(kinds, k):
    """Where candidate ``k`` comes from: kinds[0] for candidate 0, the rest cyclically for the others."""
    return kinds[0] if k == 0 or len(kinds) == 1 else kinds[1 + (k - 1) % (len(kinds) - 1)]


def candidates_that_fit(free_bytes, candidate_bytes, asked):
    """-> (room: candidates that may exist at once, fit: how many to allocate first -- at least one is tried)."""
    room = int(FREE_MEMORY_SHARE * free_bytes // max(candidate_bytes, 1))
    return room, max(1, min(max(1, int(asked)), room))


def medians(samples):
    return [float(np.median(x)) for x in samples]


def candidates_to_add(ms, room, reprobe):
    """The extension rule: how many more candidates to allocate and time after the first ``len(ms)`` gave the medians
    ``ms`` -- as many again (bounded by ``room``) when three or more of them were timed and nobody stands out, none
    otherwise or on a re-probe (``among``)."""
    n = len(ms)
    nobody_stands_out = min(ms) > EXTEND_WITHIN * ms[0] and ms[0] >= EXTEND_MIN_MS
    if reprobe or not 3 <= n < room or not nobody_stands_out:
        return 0
    return min(n, room - n)


def verdict(samples):
    """-> (median ms, min ms of every candidate, chosen).  The MEDIAN decides (one fast outlier does not make a
    buffer fast); ties go to the lower index."""
    ms = medians(samples)
    return ms, [float(min(x)) for x in samples], int(np.argmin(ms))


def share_check_applies(size, dtype):
    return size >= SHARES_MIN_SIZE and dtype != torch.uint8


def shares_outcome(bias, biased_ms=None, equal_ms=None):
    """report["xcd_bias"] for a kept buffer whose write took ``biased_ms`` with the process-wide ``bias`` and
    ``equal_ms`` with equal shares: the bias is kept unless equal shares are faster.  bias 0: nothing to compare."""
    if bias <= 0:
        return {"bias": 0}
    return {"bias": bias if biased_ms <= equal_ms else 0, "write_ms_biased": biased_ms, "write_ms_equal_shares": equal_ms}


def probe_report(samples, asked, added, kinds_used, addresses, shares=None):
    """The report of pickStackBuffer.  ``shares``: shares_outcome(...) when the share check applied, else None."""
    ms, ms_min, chosen = verdict(samples)
    report = {"candidates": len(ms), "candidates_asked": asked, "candidates_added_because_uniform": added, "write_ms": ms,
              "write_ms_min": ms_min, "chosen": chosen, "probe_ms_chosen": ms[chosen],
              "writes_per_candidate": len(samples[0]), "kinds": kinds_used, "addresses": addresses}
    if shares is not None:
        report["xcd_bias"] = shares
        if "write_ms_biased" in shares:
            report["probe_ms_chosen"] = min(shares["write_ms_biased"], shares["write_ms_equal_shares"])
    if len(ms) > 2 and min(ms) > UNIFORM_WITHIN * ms[0]:
        report["uniform"] = UNIFORM_NOTE
    return report


# ---------------------------------------------------------------------- the probe's device steps
def allocate_candidates(keep, used, count, kinds, shape, dtype, device):
    """``count`` more candidates appended to ``keep``, what they came from to ``used``.  Stops quietly when the device
    runs out of memory (the candidates that exist will do) unless there is none at all."""
    for _ in range(count):
        try:
            c, kind = alloc_kind(candidate_kind(kinds, len(keep)), shape, dtype, device)
        except torch.OutOfMemoryError:
            if not keep:
                raise
            return
        used.append(TORCH_EMPTY if kind == "torch" else CHUNKED)
        keep.append(c)


def default_timer(envs, positions):
    """-> timer(stack, k): k times of scan + write of ``envs``' current lattices, back to back, after one untimed write."""
    off = envs.perspectiveCounts()[1].clone()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def timer(stack, k):
        out = []
        for _ in range(k + 1):
            e0.record()
            envs.writePerspectives(stack, positions, off)
            e1.record()
            e1.synchronize()
            out.append(e0.elapsed_time(e1))
        return out[1:]
    return timer


def time_candidates(timer, stacks, passes, per_pass):
    """Every stack timed ``passes`` times in turn, ``per_pass`` writes each time -> one list of ms per stack."""
    samples = [[] for _ in stacks]
    for _ in range(passes):
        for i, c in enumerate(stacks):
            samples[i] += list(timer(c, per_pass))
    return samples


def check_shares(envs, timer, stack, per_pass, dtype):
    """The shares of the write's workgroups (tq_set_xcd_bias: the even XCDs' workgroups take more of the stack) against
    equal shares, on the buffer that was kept: the setting rests on a measured asymmetry of MI355X, so it is checked
    where it is used.  The outcome is set on this EnvSet's handle only (-1 = follow the process-wide setting, which is
    left alone).  -> report["xcd_bias"], None where unequal shares are never used."""
    if not share_check_applies(envs.size, dtype):
        return None
    bias = configured_xcd_bias()
    if bias <= 0:
        return shares_outcome(bias)

    def timed(handle_bias):
        check(envs._L.tq_env_set_xcd_bias(envs._h, handle_bias))
        return medians(time_candidates(timer, [stack], 2, per_pass))[0]
    equal_ms, biased_ms = timed(0), timed(bias)
    outcome = shares_outcome(bias, biased_ms, equal_ms)
    check(envs._L.tq_env_set_xcd_bias(envs._h, -1 if outcome["bias"] else 0))
    return outcome
