"""Host-side mirror of the reference's env surface over libtoricenv (HIP).

Replaces, with the same names / argument order / return shapes:
  * ``gym.make('toric-code-v0', config=...)``  -> :func:`make` / :class:`ToricEnv`
    (gym_ToricCode is an absent submodule upstream; API census in SURVEY.md 8(b))
  * ``src/EnvSet.py:4-51``                      -> :class:`EnvSet`
  * ``generatePerspectiveBatch`` + concatenate (``src/numba/util_actor.py:33-39,56-67``)
                                                -> :meth:`EnvSet.generatePerspective`
  * ``_selectActionBatch_prime`` (``src/numba/util_actor.py:69-107``) -> :meth:`EnvSet.selectAction`
  * ``generateTransitionParallel`` (``src/util_actor.py:223-264``)    -> :meth:`EnvSet.generateTransition`
  * the body of the actor loop after the policy (``src/Actor_mp.py:116-183``) -> :meth:`EnvSet.actorStep`

PyTorch-ROCm is only the device-memory container and stream provider; all lattice work
happens in the HIP kernels behind the C-ABI.  With ``numpy_io=True`` (default) the methods
take/return numpy arrays with the reference's dtypes, so ``Actor_mp``-style loops run
unchanged; with ``numpy_io=False`` they take/return device tensors and never synchronise.
"""
import ctypes as C

import numpy as np
import torch

from . import _lib, stackbuf
from ._lib import TQ_BF16, TQ_F16, TQ_F32, TQ_U8, Handle, _ptr, _stream, check, require_gpu, to_device
from .stackbuf import alloc_chunked, alloc_stack, configured_xcd_bias, set_xcd_bias  # noqa: F401
from .transition import TransitionBlock, generateTransitionParallel, to_structured, transition_dtype, transition_outputs  # noqa: F401

_DTYPES = {torch.float32: TQ_F32, torch.float16: TQ_F16, torch.bfloat16: TQ_BF16, torch.uint8: TQ_U8}
_STRATEGY = {None: 0, "fixed": 0, "linear": 1, "random": 2}
SUPPORTED_SIZES = (3, 5, 7, 9, 11, 13, 15, 17, 19, 21)


class _ActionSpace:
    """``env.action_space.high[-1] == 3`` (Actor_mp.py:58)."""

    def __init__(self, d):
        self.low = np.array([0, 0, 0, 1])
        self.high = np.array([1, d - 1, d - 1, 3])


class ToricEnv:
    """Single-lattice facade with the attributes the reference touches on a gym env:
    system_size, action_space, reset, step, qubit_matrix, state, createSyndromOpt,
    isTerminalState, evalGroundState.  Backed by an EnvSet of one lattice on the GPU,
    created on first use."""

    def __init__(self, config=None, device=None, seed=0):
        config = dict(config or {})
        self.config = config
        self.system_size = int(config.get("size", 3))
        if self.system_size not in SUPPORTED_SIZES:
            raise ValueError(f"size must be odd in {SUPPORTED_SIZES}, got {self.system_size}")
        self.min_qubit_errors = int(config.get("min_qubit_errors", 0))
        if not 0 <= self.min_qubit_errors <= 2 * self.system_size ** 2:
            raise ValueError("min_qubit_errors must be in [0, 2*size*size]")
        self.p_error = float(config.get("p_error", 0.1))
        self.terminal_reward = float(config.get("terminal_reward", 100.0))
        self.action_space = _ActionSpace(self.system_size)
        self.device = device
        self.seed = int(seed)
        self._set = None
        self._scratch = None

    def _envs(self):
        if self._set is None:
            self._set = EnvSet(self, 1, device=self.device, seed=self.seed)
        return self._set

    def reset(self, p_error=None):
        return self._envs().resetAll(None if p_error is None else [p_error])[0]

    def step(self, action):
        s, r, t, info = self._envs().step(np.asarray(action).reshape(1, 4))
        return s[0], float(r[0]), bool(t[0]), info

    @property
    def state(self):
        return self._envs().getStates()[0]

    @property
    def qubit_matrix(self):
        return self._envs().getQubits()[0]

    @qubit_matrix.setter
    def qubit_matrix(self, q):
        self._envs().setQubits(np.asarray(q).reshape(1, 2, self.system_size, self.system_size))

    def createSyndromOpt(self, qubit_matrix):
        d = self.system_size
        if self._scratch is None:                              # one scratch lattice, created once (11 hipMallocs)
            self._scratch = EnvSet(self, 1, device=self.device, seed=self.seed)
        self._scratch.setQubits(np.asarray(qubit_matrix).reshape(1, 2, d, d))
        return self._scratch.getStates()[0]

    @staticmethod
    def isTerminalState(state):
        return bool(np.all(np.asarray(state) == 0))

    def evalGroundState(self):
        return bool(self._envs().evalGroundState()[0])


def make(env_id, config=None, device=None, seed=0):
    """Stand-in for ``gym.make('toric-code-v0', config=...)`` (Distributed_mp.py:72-76)."""
    if env_id != "toric-code-v0":
        raise ValueError(f"unknown env id {env_id!r} (only 'toric-code-v0')")
    return ToricEnv(config, device=device, seed=seed)


class SelectPlan:
    """What EnvSet.selectPlan returns: ``rows`` int32 (R,), the perspectives (rows of the stack / the Q-table) the
    epsilon-greedy selection of the current step reads, strictly increasing; ``plan_offsets`` int64 (N+1,), lattice e's
    slice of them; ``R`` their number.  Views of buffers the EnvSet re-uses: valid until its next selectPlan."""

    __slots__ = ("rows", "plan_offsets", "R")

    def __init__(self, rows, plan_offsets, R):
        self.rows, self.plan_offsets, self.R = rows, plan_offsets, R


class EnvSet(Handle):
    """Batch of N toric-code lattices resident on one MI355X (reference: src/EnvSet.py:4-51).

    ``env`` is a :class:`ToricEnv` (or anything with ``system_size`` and optionally
    ``p_error`` / ``terminal_reward``).  ``first_env_id`` is the shard offset of this handle's
    lattices in the global env numbering (RNG is keyed by global id, so any partition over
    GPUs yields identical lattices).
    """

    def __init__(self, env, no_envs, device=None, seed=None, first_env_id=0, numpy_io=True,
                 max_steps_per_episode=75):
        self._parked = []               # candidates pickStackBuffer(park=True) rejected, until releaseParked() / close()
        self._stack_cache = None        # generatePerspectiveReused's buffer: dict(dtype, capacity, buf, pos, probe)
        self._positions = None          # positions of the last stack written: selectAction's default
        self._plan_rows = None          # selectPlan's row list (grown when a step needs more) and plan offsets
        self._plan_offsets = None
        self._h = C.c_void_p(None)
        self.size = int(env.system_size)
        self.no_envs = int(no_envs)
        self.numpy_io = bool(numpy_io)
        self.device = require_gpu(device if device is not None else getattr(env, "device", None))
        self.seed = int(getattr(env, "seed", 0) if seed is None else seed)
        self.first_env_id = int(first_env_id)
        self.p_error = float(getattr(env, "p_error", 0.1))
        self.terminal_reward = float(getattr(env, "terminal_reward", 100.0))
        self.max_steps_per_episode = int(max_steps_per_episode)
        self._L = _lib.load()
        with torch.cuda.device(self.device):
            check(self._L.tq_create(C.byref(self._h), self.no_envs, self.size, self.device.index,
                                    C.c_uint64(self.seed & 0xFFFFFFFFFFFFFFFF), self.first_env_id))
        # gym config "min_qubit_errors" (always 0 in the reference's own configs): n > 0 = fixed-n sampler,
        # which does not use p_error -- set first, so that {min_qubit_errors: n, p_error: 0} is a valid config
        self.min_qubit_errors = int(getattr(env, "min_qubit_errors", 0))
        if self.min_qubit_errors > 0:
            check(self._L.tq_set_min_qubit_errors(self._h, self.min_qubit_errors))
        check(self._L.tq_set_params(self._h, self.p_error, self.terminal_reward, self.max_steps_per_episode))
        n, d, dev = self.no_envs, self.size, self.device
        self._state_u8 = torch.zeros((n, 2, d, d), dtype=torch.uint8, device=dev)
        self._rewards = torch.zeros(n, dtype=torch.float32, device=dev)
        self._terminals = torch.zeros(n, dtype=torch.uint8, device=dev)
        self._actions = torch.zeros((n, 4), dtype=torch.int32, device=dev)
        self._qv = torch.zeros((n, 3), dtype=torch.float32, device=dev)
        self._counts = torch.zeros(n, dtype=torch.int32, device=dev)
        self._offsets = torch.zeros(n + 1, dtype=torch.int64, device=dev)
        # attributes of the reference class (EnvSet.py:9-11)
        self.states = np.zeros((n, 2, d, d), dtype=np.int64)
        self.rewards = np.zeros(n)
        self.terminals = np.zeros(n, dtype=bool)

    # ------------------------------------------------------------------ plumbing
    _destroy = "tq_destroy"

    def close(self):
        self._parked = []
        self._stack_cache = None
        self._plan_rows = self._plan_offsets = None
        super().close()

    def _out(self, x, dtype=None):
        """The numpy_io return convention: the device tensor itself, or its host copy (as ``dtype``, the reference's)."""
        if not self.numpy_io:
            return x
        x = x.cpu().numpy()
        return x if dtype is None else x.astype(dtype)

    def check(self):
        """Raise if a kernel latched an error (bad action / capacity).  Synchronises."""
        self._call(self._L.tq_check)

    def set_perror_schedule(self, strategy, p_start, p_final, p_delta):
        """Reset policy of the actor (Actor_mp.py:41-46,176-180) used by actorStep."""
        with torch.cuda.device(self.device):
            check(self._L.tq_set_perror_schedule(self._h, _STRATEGY[strategy], float(p_start), float(p_final),
                                                 float(p_delta)))

    # ------------------------------------------------------------------ reference surface
    def resetAll(self, p_errors=None):
        """EnvSet.py:29-36 -> states (N,2,d,d) (int64 numpy / uint8 tensor)."""
        p = to_device(p_errors, torch.float64, self.device)
        if p is not None and p.numel() != self.no_envs:
            raise ValueError("p_errors must have one entry per env")
        self._call(self._L.tq_reset_all, _ptr(p))
        return self.getStates()

    def resetTerminalEnvs(self, idx, p_errors=None):
        """EnvSet.py:19-27 -> states of the reset lattices (len(idx),2,d,d) (float64 numpy)."""
        idx_t = to_device(idx, torch.int32, self.device)
        k = int(idx_t.numel())
        p = to_device(p_errors, torch.float64, self.device)
        if p is not None and p.numel() != k:
            raise ValueError("p_errors must have one entry per idx")
        if self.numpy_io and k:
            idx_np = idx_t.cpu().numpy()
            if idx_np.min() < 0 or idx_np.max() >= self.no_envs or np.unique(idx_np).size != k:
                raise ValueError("idx must be distinct env indices in range")
        out = torch.empty((k, 2, self.size, self.size), dtype=torch.uint8, device=self.device)
        if k:
            # the device checks idx as well (range, duplicates) and latches TQ_E_INDEX for check()
            self._call(self._L.tq_reset_idx, _ptr(idx_t), k, _ptr(p))
            self._call(self._L.tq_get_state_idx, _ptr(idx_t), k, _ptr(out))
        return self._out(out, np.float64)

    def step(self, actions):
        """EnvSet.py:38-47 -> (states, rewards, terminals, info)."""
        a = to_device(actions, torch.int32, self.device)
        if a.numel() != 4 * self.no_envs:
            raise ValueError("actions must be (no_envs, 4)")
        self._actions.copy_(a.reshape(self.no_envs, 4))
        self._call(self._L.tq_step, _ptr(self._actions), _ptr(self._rewards), _ptr(self._terminals))
        states = self.getStates()
        if self.numpy_io:
            self.check()
            self.rewards, self.terminals = self._out(self._rewards, np.float64), self._out(self._terminals, bool)
            return states, self.rewards, self.terminals, {}
        return states, self._rewards, self._terminals, {}

    def getStates(self):
        self._call(self._L.tq_get_state, _ptr(self._state_u8))
        if self.numpy_io:
            self.states = self._out(self._state_u8, np.int64)
            return self.states
        return self._state_u8

    def getQubits(self):
        q = torch.empty((self.no_envs, 2, self.size, self.size), dtype=torch.uint8, device=self.device)
        self._call(self._L.tq_get_qubits, _ptr(q))
        return self._out(q, np.int64)

    def setQubits(self, qubits):
        q = to_device(qubits, torch.uint8, self.device)
        if q.numel() != self.no_envs * 2 * self.size * self.size:
            raise ValueError("qubits must be (no_envs, 2, d, d)")
        self._call(self._L.tq_set_qubits, _ptr(q))

    def getCounters(self):
        ep = torch.empty(self.no_envs, dtype=torch.int32, device=self.device)
        st = torch.empty(self.no_envs, dtype=torch.int32, device=self.device)
        self._call(self._L.tq_get_counters, _ptr(ep), _ptr(st))
        return self._out(ep), self._out(st)

    def evalGroundState(self):
        out = torch.empty(self.no_envs, dtype=torch.uint8, device=self.device)
        self._call(self._L.tq_eval_ground_state, _ptr(out))
        return self._out(out, bool)

    def isTerminal(self):
        out = torch.empty(self.no_envs, dtype=torch.uint8, device=self.device)
        self._call(self._L.tq_is_terminal, _ptr(out))
        return self._out(out, bool)

    # ------------------------------------------------------------------ perspectives
    def perspectiveCounts(self, offsets=None):
        """-> (counts i32[N], offsets i64[N+1]) device tensors; no synchronisation.  ``offsets``:
        optional caller-owned int64[N+1] tensor to receive the scan instead of the internal one."""
        if offsets is not None:
            if offsets.dtype != torch.int64 or offsets.numel() != self.no_envs + 1 or not offsets.is_contiguous():
                raise ValueError("offsets must be a contiguous int64 tensor of no_envs + 1 elements")
            self._offsets = offsets
        self._call(self._L.tq_persp_count, _ptr(self._counts), _ptr(self._offsets))
        return self._counts, self._offsets

    def writePerspectives(self, out, positions=None, offsets=None, first=0, count=None, done=None):
        """Write the stack for ``offsets`` (default: the last perspectiveCounts) into the
        caller's tensor ``out`` (capacity = out.shape[0] perspectives).  No synchronisation.
        ``first`` / ``count``: only the lattices [first, first+count), their first perspective at
        out[0] -- for consumers that walk the batch in chunks.
        ``done``: a _lib.WriteEvent the write's own dispatch signals when it has finished (not under graph capture)."""
        if out.dtype not in _DTYPES or not out.is_contiguous():
            raise ValueError("out must be a contiguous float32/float16/bfloat16/uint8 tensor")
        nq = 2 * self.size * self.size
        cap = out.numel() // nq
        if positions is not None and (positions.dtype != torch.int32 or positions.numel() < 3 * cap):
            raise ValueError("positions must be int32 with at least 3*capacity elements")
        off = self._offsets if offsets is None else offsets
        whole = first == 0 and count is None
        count = self.no_envs - int(first) if count is None else int(count)
        if done is not None:
            self._call(self._L.tq_persp_write_range_signal, _ptr(off), int(first), count, _ptr(out), _ptr(positions), cap,
                       _DTYPES[out.dtype], done._h)
        elif whole:
            self._call(self._L.tq_persp_write, _ptr(off), _ptr(out), _ptr(positions), cap, _DTYPES[out.dtype])
        else:
            self._call(self._L.tq_persp_write_range, _ptr(off), int(first), count, _ptr(out), _ptr(positions), cap,
                       _DTYPES[out.dtype])
        self._positions = positions

    def pickStackBuffer(self, candidates=4, dtype=torch.float32, capacity=None, positions=None, launches=10,
                        kinds=("torch", "chunked"), park=False, timer=None, passes=2, among=None):
        """Set-up helper: allocate ``candidates`` stack buffers (``capacity`` perspectives each, default the worst
        case no_envs * 2*d*d), time the stack write on each of them and keep the fastest.  On MI355X the rate of a
        write stream into a buffer depends on the buffer AND on the stream's shape (5.2-6.9 TB/s for this kernel,
        from allocation to allocation; a buffer that is fast for the f32 stack can be slow for the bf16 stack of the
        same lattices: profiles/r04_stream_tune_d7_all.txt), and a caller writes the same buffer every step, so the
        choice is worth a few dozen launches at set-up -- per dtype.  The steps (stackbuf.py has each of them):
        1. ALL candidates are allocated first, as many as half of the free memory holds, and stay allocated while the
           timing runs.  ``kinds``: where they come from -- kinds[0] for candidate 0, the rest cyclically for the
           others: "torch" = torch.empty (candidate 0 by default: what a caller has without this helper), "chunked" =
           alloc_stack (2 MiB physical chunks).  ``among``: time these tensors instead of allocating (a re-probe of
           parked candidates).
        2. Every candidate is timed ``passes`` times in turn, ``launches`` writes in all.  ``timer(stack, k)`` -> list
           of k write times in ms: what is timed -- default: scan + write of the current lattices, back to back;
           ExploreLoop.time_writes times the write inside the caller's loop, the env kernels beside it.
        3. When no candidate writes 7 % faster than candidate 0, as many candidates again are allocated and timed (the
           first ones stay allocated) -- once.
        4. The MEDIAN decides.  ``park``: keep the rejected candidates allocated until releaseParked() / close()
           instead of freeing them here -- the driver wipes freed device memory in the background, tens of GB of it
           take HBM bandwidth away from whatever runs in the next tens of milliseconds (a benchmark's timed region, say).
        5. The kept buffer is timed with equal shares per workgroup against the library's unequal ones (toricenv.h:
           tq_set_xcd_bias) and the faster setting is kept for this EnvSet (report["xcd_bias"]).
        -> (stack tensor (capacity,2,d,d), report dict: median / min ms and kind of every candidate, which was kept).
        Synchronises; never call it in the step loop."""
        d, nq = self.size, 2 * self.size * self.size
        cap = self.no_envs * nq if capacity is None else int(capacity)
        if positions is None:
            positions = torch.empty((cap, 3), dtype=torch.int32, device=self.device)
        shape, passes = (cap, 2, d, d), max(1, int(passes))
        per_pass = max(1, int(launches) // passes)
        if among is not None:
            keep, used, room = list(among), [stackbuf.REPROBED] * len(among), 0
        else:
            keep, used = [], []
            with torch.cuda.device(self.device):
                free = torch.cuda.mem_get_info()[0]
            room, fit = stackbuf.candidates_that_fit(free, cap * nq * torch.empty((), dtype=dtype).element_size(), candidates)
            stackbuf.allocate_candidates(keep, used, fit, kinds, shape, dtype, self.device)
        if timer is None:
            timer = stackbuf.default_timer(self, positions)
        torch.cuda.synchronize(self.device)
        samples = stackbuf.time_candidates(timer, keep, passes, per_pass)
        first, more = len(keep), stackbuf.candidates_to_add(stackbuf.medians(samples), room, among is not None)
        if more:
            stackbuf.allocate_candidates(keep, used, more, kinds, shape, dtype, self.device)
            torch.cuda.synchronize(self.device)
            samples += stackbuf.time_candidates(timer, keep[first:], passes, per_pass)
        self.check()
        best = keep[stackbuf.verdict(samples)[2]]
        if park:
            self._parked = [x for x in self._parked if all(x is not y for y in keep)] + [x for x in keep if x is not best]
        shares = stackbuf.check_shares(self, timer, best, per_pass, dtype)
        report = stackbuf.probe_report(samples, int(candidates) if among is None else len(keep), len(keep) - first, used,
                                       [hex(x.data_ptr()) for x in keep], shares)
        del keep
        if not park:
            torch.cuda.empty_cache()
        return best, report

    def releaseParked(self):
        """Free the candidates pickStackBuffer(park=True) kept."""
        self._parked = []
        torch.cuda.empty_cache()

    REUSED_PROBE_CANDIDATES = 4     # candidates of the one-off probe behind generatePerspectiveReused (0 / 1 = no probe)
    REUSED_HEADROOM = 1.5           # capacity of the re-used buffer = observed perspectives x this (grown when exceeded)

    def generatePerspectiveReused(self, dtype=torch.float32, capacity=None):
        """generatePerspective for the current states into ONE stack buffer this EnvSet keeps and re-uses, for loops that
        consume the stack at once (the policy's forward pass: numba/util_actor.py:39-46) -- no allocation per step, and
        the buffer comes from the same probe bench.py uses: at first use (and again when the dtype changes or the
        buffer has to grow) ``REUSED_PROBE_CANDIDATES`` candidates (one torch.empty, the rest tq_stack_alloc) are timed
        with the stack write of the current lattices and the fastest is kept (pickStackBuffer; ~0.1-1 s, once).
        ``capacity`` (perspectives; default: the observed count x REUSED_HEADROOM, at most the worst case
        no_envs * 2*d*d): 1.0 GB instead of 2.5 GB at 65 536 lattices of d=7 in f32.  When a later step has more
        perspectives than the buffer holds it is re-allocated larger (the count is read back before the write anyway).
        -> (perspectives (P,2,d,d), positions (P,3), counts (N,)) as VIEWS of that buffer: valid until the next call."""
        d, nq = self.size, 2 * self.size * self.size
        counts, offsets = self.perspectiveCounts()
        P = int(offsets[-1].item())
        worst = self.no_envs * nq
        cache = self._stack_cache
        if cache is None or cache["dtype"] != dtype or cache["capacity"] < P or (capacity is not None and cache["capacity"] < min(int(capacity), worst)):
            want = min(worst, max(int(capacity) if capacity is not None else int(P * self.REUSED_HEADROOM) + 1024, P, 1024))
            cache = self._stack_cache = None
            torch.cuda.empty_cache()
            pos = stackbuf.alloc_kind("chunked", (want, 3), torch.int32, self.device)[0]
            k = int(self.REUSED_PROBE_CANDIDATES)
            if k > 1 and P > 0:
                buf, report = self.pickStackBuffer(k, dtype=dtype, capacity=want, positions=pos, launches=6, passes=2)
            else:
                buf, report = stackbuf.alloc_kind("chunked", (want, 2, d, d), dtype, self.device)[0], None
            cache = self._stack_cache = {"dtype": dtype, "capacity": want, "buf": buf, "pos": pos, "probe": report}
        buf, pos = cache["buf"], cache["pos"]
        if P:
            self.writePerspectives(buf, pos, offsets)
        self._positions = pos[:P]
        return buf[:P], pos[:P], counts

    def reusedStackBacking(self):
        """The whole buffer behind the last generatePerspectiveReused result (rows past P are slack)."""
        return None if self._stack_cache is None else self._stack_cache["buf"]

    def generatePerspective(self, states=None, dtype=torch.float32):
        """generatePerspectiveBatch + concatenate (numba/util_actor.py:33-39,56-67) for the current
        states, or for an explicit ``states`` array (n,2,d,d) like the reference's function
        -> (perspectives (P,2,d,d), positions (P,3), counts (N,)).
        Reads P back from the device (one 8-byte copy), like the reference's data-dependent shape."""
        if states is not None:
            out, pos, counts = generatePerspectiveBatch(self.size // 2, self.size, states, dtype=dtype, device=self.device)
        else:
            counts, offsets = self.perspectiveCounts()
            P = int(offsets[-1].item())
            out = torch.empty((P, 2, self.size, self.size), dtype=dtype, device=self.device)
            pos = torch.empty((P, 3), dtype=torch.int32, device=self.device)
            if P:
                self.writePerspectives(out, pos, offsets)
            self._positions = pos
        return self._out(out), self._out(pos, np.int64), self._out(counts, np.int64)

    # ------------------------------------------------------------------ policy glue
    def _eps(self, eps):
        """a scalar or (N,) epsilon -> float64 (N,) on the device"""
        if not torch.is_tensor(eps):
            eps = np.broadcast_to(np.asarray(eps, np.float64), (self.no_envs,))
        e = to_device(eps, torch.float64, self.device)
        if e.numel() != self.no_envs:
            raise ValueError("eps must be a scalar or have one entry per env")
        return e

    def selectPlan(self, eps, offsets=None):
        """Which rows of the Q-table selectAction(q, eps) would read, decided before any Q-value exists (tq_select_plan):
        all n of a lattice that will act greedily, the one row of a lattice that will not, none of a lattice without
        perspectives -> a SelectPlan.  The forward pass then runs on ``plan.rows`` alone and
        ``selectAction(q_rows, eps, plan=plan)`` selects from its (R, 3) output, with the same result in bits.  No step or
        reset may lie between the plan and that selection, and ``eps`` must be the same (check() raises otherwise).
        ``offsets``: default the last perspectiveCounts.  Reads R back (one 8-byte copy: the row count is data dependent)."""
        off = self._offsets if offsets is None else to_device(offsets, torch.int64, self.device)
        e = self._eps(eps)
        n = self.no_envs
        cap = self._positions.shape[0] if self._positions is not None else n * 2 * self.size * self.size
        if self._plan_rows is None or self._plan_rows.numel() < cap:
            self._plan_rows = torch.empty(max(cap, 1024), dtype=torch.int32, device=self.device)
        if self._plan_offsets is None:
            self._plan_offsets = torch.zeros(n + 2, dtype=torch.int64, device=self.device)[:n + 1]
        rows, poff = self._plan_rows, self._plan_offsets
        self._call(self._L.tq_select_plan, _ptr(off), _ptr(e), _ptr(poff), _ptr(rows), rows.numel())
        R = int(poff[-1].item())
        return SelectPlan(rows[:R], poff, R)

    def selectAction(self, q_table, eps, positions=None, offsets=None, plan=None):
        """_selectActionBatch_prime on the device -> (actions (N,4), q_values (N,3)).
        q_table None = pure exploration (every eps must be 1).
        ``plan`` (a SelectPlan of this step and this eps): ``q_table`` is the compact (R, 3) table of ``plan.rows``."""
        pos = self._positions if positions is None else positions
        if pos is None:
            raise ValueError("call generatePerspective / writePerspectives (with positions) first")
        pos = to_device(pos, torch.int32, self.device)
        off = self._offsets if offsets is None else to_device(offsets, torch.int64, self.device)
        q = to_device(q_table, torch.float32, self.device)
        if plan is not None:
            if q is None or q.numel() != 3 * plan.R:
                raise ValueError("with a plan, q_table must be the (plan.R, 3) table of plan.rows")
            if plan.R == 0:                                     # no lattice has a perspective: nothing of q is read
                q = torch.zeros((1, 3), dtype=torch.float32, device=self.device)
            self._call(self._L.tq_select_action_planned, _ptr(q), _ptr(off), _ptr(plan.plan_offsets), _ptr(pos),
                       _ptr(self._eps(eps)), _ptr(self._actions), _ptr(self._qv))
            return self._out(self._actions, np.int64), self._out(self._qv)
        if q is not None and not torch.is_tensor(eps):
            eps = np.broadcast_to(np.asarray(eps, np.float64), (self.no_envs,))
        e = None if q is None else to_device(eps, torch.float64, self.device)
        self._call(self._L.tq_select_action, _ptr(q), _ptr(off), _ptr(pos), _ptr(e), _ptr(self._actions), _ptr(self._qv))
        return self._out(self._actions, np.int64), self._out(self._qv)

    def generateTransition(self, actions):
        """generateTransitionParallel for the last step() (util_actor.py:223-264)
        -> dict(perspective u8, next_perspective u8, action i32[N,4]) of device tensors
        (numpy arrays with numpy_io)."""
        a = to_device(actions, torch.int32, self.device)
        out = transition_outputs(self.no_envs, self.size, self.device)
        self._call(self._L.tq_transition_write, _ptr(a), _ptr(out["perspective"]), _ptr(out["next_perspective"]),
                   _ptr(out["action"]))
        if self.numpy_io:
            self.check()
            return {k: self._out(v) for k, v in out.items()}
        return out

    def newTransitionBlock(self, steps=1):
        return TransitionBlock(self.size, self.no_envs * int(steps), self.device)

    def actorStep(self, actions=None, block=None, slot=0, want_actions=True):
        """Fused step -> transition -> auto-reset -> counts (Actor_mp.py:116-183).
        actions None = pure exploration drawn in-kernel.  ``block``/``slot``: lattice e writes
        transition slot ``slot*no_envs + e`` of the TransitionBlock.
        -> (actions_taken i32[N,4], rewards f32[N], terminals u8[N]) device tensors."""
        a = to_device(actions, torch.int32, self.device)
        blk_ptr, cap, base = C.c_void_p(0), 0, 0
        if block is not None:
            blk_ptr, cap, base = _ptr(block.buf), block.capacity, int(slot) * self.no_envs
        self._call(self._L.tq_actor_step, _ptr(a), _ptr(self._actions) if want_actions else C.c_void_p(0),
                   _ptr(self._rewards), _ptr(self._terminals), blk_ptr, cap, base)
        if self.numpy_io:
            self.check()
            return self._out(self._actions, np.int64), self._out(self._rewards, np.float64), self._out(self._terminals, bool)
        return self._actions, self._rewards, self._terminals


_reserved = {}      # (device index, d) -> states the device's stateless scratch is sized for


def _reserve_states(dev, d, n):
    """tq_states_reserve is a set-up call (allocates, synchronises): issue it only when a larger
    batch than ever before arrives on this device; the tq_states_* calls themselves never allocate."""
    key = (dev.index, d)
    if _reserved.get(key, 0) < n:
        with torch.cuda.device(dev):
            check(_lib.load().tq_states_reserve(d, n))
        _reserved[key] = n                                # the scratch only ever grows


def generatePerspectiveBatch(grid_shift, toric_size, states, dtype=torch.float32, device=None, return_offsets=False):
    """numba/util_actor.py:56-67 for syndromes that do not live in an EnvSet (e.g. the learner's
    next_state batch, util_learner.py:48-111).  states: (n,2,d,d) numpy / tensor.
    -> (perspectives (P,2,d,d) tensor, positions (P,3) i32 tensor, counts (n,) i32 tensor)
    [+ offsets (n+1,) i64 tensor, the exclusive scan the kernels produced, with ``return_offsets``].
    One 8-byte read-back of P (the output shape is data dependent, as upstream)."""
    dev = require_gpu(device)
    if int(grid_shift) != int(toric_size) // 2:
        raise ValueError("grid_shift must be int(toric_size/2) (Actor_mp.py:59)")
    L = _lib.load()
    st = to_device(states, torch.uint8, dev)
    n, d = int(st.shape[0]), int(toric_size)
    counts = torch.empty(n, dtype=torch.int32, device=dev)
    offsets = torch.empty(n + 1, dtype=torch.int64, device=dev)
    _reserve_states(dev, d, n)
    with torch.cuda.device(dev):
        rc = L.tq_states_persp_count(d, n, _ptr(st), _ptr(counts), _ptr(offsets), _stream())
        if rc == _lib.TQ_E_CAPACITY:                           # the python-side record of the scratch size was stale
            _reserved.pop((dev.index, d), None)
            _reserve_states(dev, d, n)
            rc = L.tq_states_persp_count(d, n, _ptr(st), _ptr(counts), _ptr(offsets), _stream())
        check(rc)
        P = int(offsets[-1].item())
        out = torch.empty((P, 2, d, d), dtype=dtype, device=dev)
        pos = torch.empty((P, 3), dtype=torch.int32, device=dev)
        if P:
            check(L.tq_states_persp_write(d, n, _ptr(st), _ptr(offsets), _ptr(out), _ptr(pos), P, _DTYPES[dtype],
                                          _stream()))
    return (out, pos, counts, offsets) if return_offsets else (out, pos, counts)
