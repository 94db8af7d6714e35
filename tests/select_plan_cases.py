"""What tests/test_select_plan_host.py and tests/test_gpu_select_sparse.py share (not a test module): the g++ shim over
csrc/select_plan.hpp, the reference's epsilon schedule, and what the oracle's selection reads."""
import ctypes as C

import numpy as np

from host_build import build_shim
from oracle import toric_oracle as O

_P = C.c_void_p


def load_shim(tmp_path_factory):
    lib = build_shim(tmp_path_factory, "host_select_plan_shim.cpp")
    lib.shim_need.restype, lib.shim_need.argtypes = C.c_int, [C.c_int, C.c_int]
    lib.shim_greedy.restype, lib.shim_greedy.argtypes = C.c_int, [C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32, C.c_double]
    lib.shim_plan.restype = C.c_int64
    lib.shim_plan.argtypes = [C.c_int64, _P, _P, _P, _P, C.c_uint64, C.c_int64, _P, _P, _P, C.c_int64]
    lib.shim_select_planned.restype = C.c_int64
    lib.shim_select_planned.argtypes = [C.c_int64, _P, _P, _P, _P, _P, _P, _P, C.c_uint64, C.c_int64, _P, _P]
    return lib


def _p(a):
    return a.ctypes.data_as(_P)


def _eps(eps, n):
    return np.ascontiguousarray(np.broadcast_to(np.asarray(eps, np.float64), (n,)))


def reference_eps(n, eps=0.8, alpha=7.0):
    """calculateEpsilon(0.8, 7, n) (src/util_actor.py:294-312): actor i of n explores with eps ** (1 + alpha i / (n - 1))."""
    if n == 1:
        return np.array([eps])
    return eps ** (1.0 + alpha * np.arange(n) / (n - 1))


ROWS_UNWRITTEN = -7


def host_plan(lib, offsets, eps, episodes, steps, seed, first_env=0, rows_cap=None):
    """-> (need i32 (N,), plan_offsets i64 (N+1,), rows i32 (rows_cap,) with ROWS_UNWRITTEN where nothing was written, R)"""
    offsets = np.ascontiguousarray(offsets, np.int64)
    n = offsets.size - 1
    cap = int(offsets[-1]) if rows_cap is None else int(rows_cap)
    need, poff = np.zeros(n, np.int32), np.zeros(n + 1, np.int64)
    rows = np.full(max(cap, 1), ROWS_UNWRITTEN, np.int32)
    ep, st = np.ascontiguousarray(episodes, np.uint32), np.ascontiguousarray(steps, np.uint32)
    R = lib.shim_plan(n, _p(offsets), _p(_eps(eps, n)), _p(ep), _p(st), int(seed), int(first_env), _p(need), _p(poff), _p(rows), cap)
    return need, poff, rows[:cap], int(R)


def host_select_planned(lib, q_rows, offsets, plan_offsets, positions, eps, episodes, steps, seed, first_env=0):
    """-> (actions i32 (N,4), q_values f32 (N,3), number of lattices whose slice of the plan does not fit)"""
    offsets = np.ascontiguousarray(offsets, np.int64)
    n = offsets.size - 1
    q = np.ascontiguousarray(q_rows, np.float32).reshape(-1, 3)
    if q.shape[0] == 0:
        q = np.zeros((1, 3), np.float32)
    pos = np.ascontiguousarray(positions, np.int32)
    act, qv = np.full((n, 4), -1, np.int32), np.full((n, 3), np.nan, np.float32)
    ep, st = np.ascontiguousarray(episodes, np.uint32), np.ascontiguousarray(steps, np.uint32)
    bad = lib.shim_select_planned(n, _p(q), _p(offsets), _p(np.ascontiguousarray(plan_offsets, np.int64)), _p(pos),
                                  _p(_eps(eps, n)), _p(ep), _p(st), int(seed), int(first_env), _p(act), _p(qv))
    return act, qv, int(bad)


def oracle_greedy(eps, seed, env_ids, episodes, steps):
    """the oracle's greedy decision (toric_oracle.select_action_batch: greedy iff (1 - eps) > U of the lattice's draw)"""
    k0, k1 = O._key(seed)
    w0, _, _, _ = O.philox4x32(np.asarray(env_ids, np.uint64), np.asarray(episodes, np.uint64), np.asarray(steps, np.uint64),
                               np.uint64(O.DOMAIN_SEL << 24), k0, k1)
    n = len(env_ids)
    return (1.0 - _eps(eps, n)) > O._u01(np.broadcast_to(w0, (n,)))


def oracle_reads(q_table, offsets, positions, eps, seed, env_ids, episodes, steps):
    """The oracle's selection on the full table -> (actions, q_values, the rows of the table it reads: every row of a
    greedy lattice -- its argmax runs over the whole slice -- and the chosen row of another; none of an empty one)."""
    act, qv, chosen = O.select_action_batch(q_table, offsets, positions, eps, seed, env_ids, episodes, steps)
    greedy = oracle_greedy(eps, seed, env_ids, episodes, steps)
    reads = []
    for i in range(len(offsets) - 1):
        lo, hi = int(offsets[i]), int(offsets[i + 1])
        if hi > lo:
            reads += list(range(lo, hi)) if greedy[i] else [int(chosen[i])]
    return act, qv, np.array(reads, np.int64)


# ---- slices with NaN and inf (tests/test_nonfinite_host.py, tests/test_gpu_nonfinite.py) ---------------------------------
SLICE_LENGTHS = (1, 21, 22, 43)                # 3 cnt = 3, 63, 66, 129: below, at and beyond one and two rounds of 64 lanes


def nonfinite_slices():
    """-> (q (P,3) f32, offsets): for every length the finite slice, a NaN at each of the flat positions 0, 63, 64 and the
    last that the slice has, NaNs at two of them (the first wins), all NaN, all -inf, and NaN with +inf on either side."""
    rng = np.random.default_rng(404)
    slices = []
    for cnt in SLICE_LENGTHS:
        base = rng.normal(size=3 * cnt).astype(np.float32)
        base[rng.integers(0, 3 * cnt, 2)] = base.max()                          # a tie of maxima: the first one counts
        at = sorted({p for p in (0, 63, 64, 3 * cnt - 1) if p < 3 * cnt})
        slices.append(base.copy())
        for p in at:
            s = base.copy()
            s[p] = np.float32(np.nan)
            slices.append(s)
        s = base.copy()
        s[[at[-1], at[len(at) // 2]]] = np.float32(np.nan)
        slices.append(s)
        slices.append(np.full(3 * cnt, np.float32(np.nan)))
        slices.append(np.full(3 * cnt, -np.float32(np.inf)))
        for nan_at, inf_at in ((at[-1], 0), (0, at[-1])) if cnt > 1 else ((2, 0), (0, 2)):
            s = base.copy()
            s[nan_at], s[inf_at] = np.float32(np.nan), np.float32(np.inf)
            slices.append(s)
    off = np.concatenate([[0], np.cumsum([s.size // 3 for s in slices])]).astype(np.int64)
    return np.concatenate(slices).reshape(-1, 3), off
