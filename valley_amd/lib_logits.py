"""ctypes binding of libvalley_hip_logits.so (include/valley_hip_logits.h): HF's logits processors on the device.

A companion of libvalley_hip.so with its own ABI version; it reads fp32 logits and int32 ids only, so the same library
serves every precision.  Missing or stale, it fails loudly: the processors have no non-HIP path."""
from __future__ import annotations

import ctypes
import os
import threading
from ctypes import c_char_p, c_int, c_size_t, c_void_p

from . import build as _build
from .lib import ValleyHipError

_P = c_void_p
SIGS = {
    "vly_logits_abi_version": (c_int, []),
    "vly_logits_last_error": (c_char_p, []),
    "vly_logits_process": (c_int, [_P, c_int, c_int, c_int, _P, _P, c_int, _P, c_int, c_int, _P, _P, c_int, c_int, _P]),
    "vly_logits_history_gather": (c_int, [_P, c_int, c_int, _P, c_int, _P, c_int, _P]),
    "vly_logits_beam_scratch_bytes": (c_size_t, [c_int, c_int, c_int]),
    "vly_logits_beam_candidates": (c_int, [_P, c_int, c_int, c_int, c_int, _P, c_int, _P, c_int, _P, _P, _P, _P, _P, _P]),
}
EXPORTS = tuple(SIGS)
ABI_VERSION = 1

_LIB = None
_LOCK = threading.Lock()


def lib_path() -> str:
    return os.environ.get("VALLEY_HIP_LOGITS_LIB", _build.LIB_LOGITS)


def load_logits():
    """Load (once) and type libvalley_hip_logits.so.  Raises if it is absent, incomplete or of another ABI version."""
    global _LIB
    if _LIB is not None:
        return _LIB
    with _LOCK:
        if _LIB is not None:
            return _LIB
        path = lib_path()
        if not os.path.exists(path):
            raise ValleyHipError(f"{path} not found: build it with `python -m valley_amd.build` (hipcc --offload-arch=gfx950). "
                                 "The logits processors have no non-HIP path.")
        lib = ctypes.CDLL(path)
        for name, (res, args) in SIGS.items():
            try:
                fn = getattr(lib, name)
            except AttributeError as e:
                raise ValleyHipError(f"{path} does not export {name}") from e
            fn.restype = res
            fn.argtypes = args
        if lib.vly_logits_abi_version() != ABI_VERSION:
            raise ValleyHipError(f"logits ABI mismatch: library {lib.vly_logits_abi_version()} vs binding {ABI_VERSION}")
        _LIB = lib
        return lib


def check(rc: int, what: str):
    if rc != 0:
        msg = load_logits().vly_logits_last_error().decode(errors="replace")
        raise ValleyHipError(f"{what} failed (rc={rc}): {msg}")
