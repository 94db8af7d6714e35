"""ctypes binding of libtoricenv.so (include/toricenv.h).

There is no CPU fallback: if the library is missing or no HIP device is usable the
functions raise -- a GPU box must never pass silently on some other path.
"""
import ctypes as C
import glob
import os
import subprocess

import numpy as np
import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libtoricenv.so")
CSRC = os.path.join(_HERE, "csrc")

TQ_F32, TQ_F16, TQ_BF16, TQ_U8 = 0, 1, 2, 3
TQ_PERR_FIXED, TQ_PERR_LINEAR, TQ_PERR_RANDOM = 0, 1, 2
TQ_OPT_ADAM, TQ_OPT_RMSPROP = 0, 1
TQ_NET_NN8, TQ_NET_NN17 = 8, 17
TQ_NET_RESNET18, TQ_NET_RESNET34 = 18, 34
TQ_E_INVALID, TQ_E_HIP, TQ_E_CAPACITY, TQ_E_ACTION, TQ_E_INDEX, TQ_E_RESET = -1, -2, -3, -4, -5, -6

# every symbol include/toricenv.h declares: (name, restype, argtypes)
_vp, _i, _i64, _u64, _d = C.c_void_p, C.c_int, C.c_int64, C.c_uint64, C.c_double
SYMBOLS = [
    ("tq_version", _i, []),
    ("tq_last_error", C.c_char_p, []),
    ("tq_create", _i, [C.POINTER(_vp), _i, _i, _i, _u64, _i64]),
    ("tq_destroy", _i, [_vp]),
    ("tq_set_params", _i, [_vp, _d, _d, _i]),
    ("tq_set_min_qubit_errors", _i, [_vp, _i]),
    ("tq_set_perror_schedule", _i, [_vp, _i, _d, _d, _d]),
    ("tq_stack_alloc", _i, [_i, _u64, C.POINTER(_vp)]),
    ("tq_stack_free", _i, [_vp]),
    ("tq_set_xcd_bias", _i, [_i]),
    ("tq_get_xcd_bias", _i, []),
    ("tq_env_set_xcd_bias", _i, [_vp, _i]),
    ("tq_env_get_xcd_bias", _i, [_vp]),
    ("tq_debug_force_xcc_parity", _i, [_i]),
    ("tq_debug_slot_words_nonzero", _i, [_vp]),
    ("tq_num_envs", _i, [_vp]),
    ("tq_size", _i, [_vp]),
    ("tq_reset_all", _i, [_vp, _vp, _vp]),
    ("tq_reset_idx", _i, [_vp, _vp, _i, _vp, _vp]),
    ("tq_step", _i, [_vp, _vp, _vp, _vp, _vp]),
    ("tq_get_state", _i, [_vp, _vp, _vp]),
    ("tq_get_state_idx", _i, [_vp, _vp, _i, _vp, _vp]),
    ("tq_get_qubits", _i, [_vp, _vp, _vp]),
    ("tq_set_qubits", _i, [_vp, _vp, _vp]),
    ("tq_get_counters", _i, [_vp, _vp, _vp, _vp]),
    ("tq_eval_ground_state", _i, [_vp, _vp, _vp]),
    ("tq_is_terminal", _i, [_vp, _vp, _vp]),
    ("tq_persp_count", _i, [_vp, _vp, _vp, _vp]),
    ("tq_persp_write", _i, [_vp, _vp, _vp, _vp, _i64, _i, _vp]),
    ("tq_persp_write_range", _i, [_vp, _vp, _i, _i, _vp, _vp, _i64, _i, _vp]),
    ("tq_event_create", _i, [C.POINTER(_vp), _i]),
    ("tq_event_destroy", _i, [_vp]),
    ("tq_persp_write_signal", _i, [_vp, _vp, _vp, _vp, _i64, _i, _vp, _vp]),
    ("tq_persp_write_range_signal", _i, [_vp, _vp, _i, _i, _vp, _vp, _i64, _i, _vp, _vp]),
    ("tq_stream_wait_event", _i, [_vp, _vp]),
    ("tq_states_reserve", _i, [_i, _i]),
    ("tq_states_persp_count", _i, [_i, _i, _vp, _vp, _vp, _vp]),
    ("tq_states_persp_write", _i, [_i, _i, _vp, _vp, _vp, _vp, _i64, _i, _vp]),
    ("tq_select_action", _i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    ("tq_states_select_action", _i, [_i, _vp, _vp, _vp, _vp, _u64, _u64, _i64, _vp, _vp, _vp]),
    ("tq_select_plan", _i, [_vp, _vp, _vp, _vp, _vp, _i64, _vp]),
    ("tq_select_action_planned", _i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    ("tq_states_check", _i, [_vp]),
    ("tq_segment_max", _i, [_vp, _vp, _i, _vp, _vp, _vp]),
    ("tq_td_target", _i, [_vp, _vp, _i, _vp, _vp, C.c_float, C.c_float, C.c_float, _vp, _vp]),
    ("tq_transition_write", _i, [_vp, _vp, _vp, _vp, _vp, _vp]),
    ("tq_states_transition", _i, [_i, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    ("tq_transition_block_bytes", _i64, [_i, _i64]),
    ("tq_transition_unpack", _i, [_i, _vp, _i64, _i64, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    ("tq_block_priorities", _i, [_i, _vp, _i64, _i, _i, _vp, _d, _vp]),
    ("tq_actor_step", _i, [_vp, _vp, _vp, _vp, _vp, _vp, _i64, _i64, _vp]),
    ("tq_check", _i, [_vp, _vp]),
    ("tq_replay_create", _i, [C.POINTER(_vp), _i, _i64, _d, _i, _u64, _i]),
    ("tq_replay_destroy", _i, [_vp]),
    ("tq_replay_save_block", _i, [_vp, _vp, _i64, _vp]),
    ("tq_replay_filled", _i64, [_vp, _vp]),
    ("tq_replay_sample", _i, [_vp, _i, _d, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    ("tq_replay_get", _i, [_vp, _vp, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    ("tq_replay_next_persp_count", _i, [_vp, _vp, _i, _vp, _vp, _vp]),
    ("tq_replay_next_persp_write", _i, [_vp, _vp, _i, _vp, _vp, _vp, _i64, _i, _vp]),
    ("tq_replay_update", _i, [_vp, _vp, _vp, _i, _vp]),
    ("tq_replay_reset_alpha", _i, [_vp, _d, _vp]),
    ("tq_replay_leaves", _i, [_vp, _vp, _vp]),
    ("tq_replay_tree_nodes", _i64, [_vp]),
    ("tq_replay_tree", _i, [_vp, _vp, _vp]),
    ("tq_replay_check", _i, [_vp, _vp]),
    ("tq_nn11_create", _i, [C.POINTER(_vp), _i, _i64, _i]),
    ("tq_nn11_destroy", _i, [_vp]),
    ("tq_nn11_load", _i, [_vp, C.POINTER(_vp), C.POINTER(_vp), _vp]),
    ("tq_nn11_forward", _i, [_vp, _vp, _i, _i64, _vp, _vp]),
    ("tq_nn11_forward_rows", _i, [_vp, _vp, _i, _i64, _vp, _i64, _vp, _vp]),
    ("tq_nn11_check", _i, [_vp, _vp]),
    ("tq_nn11_grad_create", _i, [C.POINTER(_vp), _i, _i, _i]),
    ("tq_nn11_grad_destroy", _i, [_vp]),
    ("tq_nn11_grad_load", _i, [_vp, C.POINTER(_vp), C.POINTER(_vp), _vp]),
    ("tq_nn11_grad_step", _i, [_vp, _vp, _i, _i, _vp, _vp, _vp, _vp, _vp, C.POINTER(_vp), C.POINTER(_vp), _vp]),
    ("tq_nn11_grad_check", _i, [_vp, _vp]),
    ("tq_nn11_grad_opt_step", _i, [_vp, _i, _d, _d, _d, _d, _d, _i64] + [C.POINTER(_vp)] * 8 + [_vp]),
    ("tq_nnw_create", _i, [C.POINTER(_vp), _i, _i, _i64, _i]),
    ("tq_nnw_destroy", _i, [_vp]),
    ("tq_nnw_load", _i, [_vp, C.POINTER(_vp), C.POINTER(_vp), _vp]),
    ("tq_nnw_forward", _i, [_vp, _vp, _i, _i64, _vp, _vp]),
    ("tq_nnw_grad_create", _i, [C.POINTER(_vp), _i, _i, _i, _i]),
    ("tq_nnw_grad_destroy", _i, [_vp]),
    ("tq_nnw_grad_load", _i, [_vp, C.POINTER(_vp), C.POINTER(_vp), _vp]),
    ("tq_nnw_grad_step", _i, [_vp, _vp, _i, _i, _vp, _vp, _vp, _vp, _vp, C.POINTER(_vp), C.POINTER(_vp), _vp]),
    ("tq_nnw_grad_check", _i, [_vp, _vp]),
    ("tq_resnet_create", _i, [C.POINTER(_vp), _i, _i, _i64, _i]),
    ("tq_resnet_destroy", _i, [_vp]),
    ("tq_resnet_load", _i, [_vp, C.POINTER(_vp), C.POINTER(_vp), _vp, _vp, _d, _vp]),
    ("tq_resnet_forward", _i, [_vp, _vp, _i, _i64, _vp, _vp]),
]

_lib = None


class ToricEnvError(RuntimeError):
    pass


def build(force=False, verbose=False):
    """Compile libtoricenv.so for gfx950 with hipcc (cross-compiles without a GPU)."""
    srcs = glob.glob(os.path.join(CSRC, "*.hip")) + glob.glob(os.path.join(CSRC, "*.hpp"))
    srcs += [os.path.join(CSRC, "Makefile"), os.path.join(_HERE, "..", "include", "toricenv.h")]
    stale = (not os.path.exists(LIB_PATH)) or any(os.path.getmtime(s) > os.path.getmtime(LIB_PATH) for s in srcs)
    if force or stale:
        cmd = ["make", "-C", CSRC] + (["-B"] if force else [])
        out = None if verbose else subprocess.DEVNULL
        subprocess.check_call(cmd, stdout=out)
    return LIB_PATH


def load():
    """dlopen the library and bind every symbol of the header.  Raises if it is missing."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ToricEnvError(
                f"{LIB_PATH} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                "(hipcc --offload-arch=gfx950).  There is no CPU fallback.")
        lib = C.CDLL(LIB_PATH)
        for name, res, args in SYMBOLS:
            fn = getattr(lib, name)           # AttributeError if the .so lacks a declared symbol
            fn.restype = res
            fn.argtypes = args
        _lib = lib
    return _lib


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _ptr(t):
    return C.c_void_p(0 if t is None else t.data_ptr())


def check(rc):
    if rc != 0:
        msg = load().tq_last_error().decode("utf-8", "replace")
        if rc in (TQ_E_INVALID, TQ_E_ACTION, TQ_E_INDEX):
            raise ValueError(f"libtoricenv: {msg}")
        raise ToricEnvError(f"libtoricenv error {rc}: {msg}")


def require_gpu(device):
    """The ``device`` argument of the env surface (None = the current one) -> an indexed cuda device."""
    if not torch.cuda.is_available():
        raise ToricEnvError("no HIP device visible to PyTorch-ROCm: the toric env has no CPU fallback")
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    if dev.type != "cuda":
        raise ValueError(f"device must be a cuda (ROCm) device, got {dev}")
    return torch.device("cuda", dev.index if dev.index is not None else torch.cuda.current_device())


def to_device(x, dtype, device):
    """numpy array / sequence / tensor (or None) -> contiguous ``dtype`` tensor on ``device`` (or None).  A read-only
    numpy array (np.broadcast_to, a memory-mapped file) is copied first: torch would alias it as writable."""
    if x is None:
        return None
    if not torch.is_tensor(x):
        x = torch.as_tensor(np.array(x, copy=True) if isinstance(x, np.ndarray) and not x.flags.writeable else np.ascontiguousarray(x))
    return x.to(device=device, dtype=dtype).contiguous()


class Handle:
    """An object that owns one library handle ``_h`` on ``device`` (bound library ``_L``): how its calls are issued
    and how it is destroyed.  ``_h`` is None (or a null pointer) unless a create call succeeded and close() has not run,
    so close() is safe on a half-constructed object and when called twice."""

    _h = None                       # subclasses also name the symbol that frees it: _destroy

    def _call(self, fn, *args):
        with torch.cuda.device(self.device):
            check(fn(self._h, *args, _stream()))

    def close(self):
        if self._h is not None and self._h.value:
            getattr(self._L, self._destroy)(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class WriteEvent:
    """A library-owned event that a stack write signals with its own dispatch (tq_persp_write_signal: no packet of its
    own on the write's stream) and another stream waits for: ``EnvSet.writePerspectives(..., done=ev)``, then
    ``ev.wait(stream)``."""

    def __init__(self, device):
        self.device = require_gpu(device)
        self._L = load()
        self._h = C.c_void_p(None)
        check(self._L.tq_event_create(C.byref(self._h), self.device.index))

    def wait(self, stream=None):
        """Order ``stream`` (default: the current one) behind the last write this event was passed to."""
        s = _stream() if stream is None else C.c_void_p(stream.cuda_stream)
        check(self._L.tq_stream_wait_event(self._h, s))

    def close(self):
        if self._h is not None and self._h.value:
            self._L.tq_event_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
