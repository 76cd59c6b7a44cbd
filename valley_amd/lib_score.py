"""ctypes binding of libvalley_hip_score.so (include/valley_hip_score.h): token log-probabilities, top-n alternatives, the
decode step's per-token record and the forward-only cross-entropy.

A companion of libvalley_hip.so with its own ABI version; it reads fp32 logits and int32 ids only, so the same library
serves every precision.  Loaded on first use only: a run that never asks for scores never maps it.  Missing or stale, it
fails loudly: the scores have no non-HIP path."""
from __future__ import annotations

import ctypes
import os
import threading
from ctypes import c_char_p, c_int, c_void_p

from . import build as _build
from .lib import ValleyHipError

_P = c_void_p
SIGS = {
    "vly_score_abi_version": (c_int, []),
    "vly_score_last_error": (c_char_p, []),
    "vly_score_rows": (c_int, [_P, c_int, c_int, c_int, _P, _P, _P, c_int, _P, _P, _P, c_int, _P]),
    "vly_score_record": (c_int, [_P, c_int, c_int, c_int, _P, _P, _P, c_int, c_int, _P, c_int, c_int, _P, _P, _P, _P, _P]),
    "vly_score_loss": (c_int, [_P, _P, c_int, c_int, _P, _P, _P]),
}
EXPORTS = tuple(SIGS)
ABI_VERSION = 1
MAX_TOP = 20             # VLY_SCORE_MAX_TOP

_LIB = None
_LOCK = threading.Lock()


def lib_path() -> str:
    return os.environ.get("VALLEY_HIP_SCORE_LIB", _build.LIB_SCORE)


def load_score():
    """Load (once) and type libvalley_hip_score.so.  Raises if it is absent, incomplete or of another ABI version."""
    global _LIB
    if _LIB is not None:
        return _LIB
    with _LOCK:
        if _LIB is not None:
            return _LIB
        path = lib_path()
        if not os.path.exists(path):
            raise ValleyHipError(f"{path} not found: build it with `python -m valley_amd.build` (hipcc --offload-arch=gfx950). "
                                 "Token log-probabilities and the loss have no non-HIP path.")
        lib = ctypes.CDLL(path)
        for name, (res, args) in SIGS.items():
            try:
                fn = getattr(lib, name)
            except AttributeError as e:
                raise ValleyHipError(f"{path} does not export {name}") from e
            fn.restype = res
            fn.argtypes = args
        if lib.vly_score_abi_version() != ABI_VERSION:
            raise ValleyHipError(f"score ABI mismatch: library {lib.vly_score_abi_version()} vs binding {ABI_VERSION}")
        _LIB = lib
        return lib


def check(rc: int, what: str):
    if rc != 0:
        msg = load_score().vly_score_last_error().decode(errors="replace")
        raise ValleyHipError(f"{what} failed (rc={rc}): {msg}")
