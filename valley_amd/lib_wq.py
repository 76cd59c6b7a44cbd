"""ctypes binding of libvalley_hip_wq.so (include/valley_hip_wq.h): weight-only INT8 decode — the per-row quantizer and the
int8 weight-streaming GEMVs.

A companion of libvalley_hip.so with its own ABI version; every compute entry takes the 16-bit storage type as an argument,
so the same library serves the bf16 and the fp16 engine.  Loaded only by an engine that quantized its weights.  Missing or
stale, it fails loudly: the int8 path has no non-HIP form."""
from __future__ import annotations

import ctypes
import os
import threading
from ctypes import c_char_p, c_float, c_int, c_void_p

from . import build as _build
from .lib import ValleyHipError

_P = c_void_p
SIGS = {
    "vly_wq_abi_version": (c_int, []),
    "vly_wq_last_error": (c_char_p, []),
    "vly_wq_quantize_rows": (c_int, [_P, c_int, c_int, c_int, c_int, _P, _P, _P]),
    "vly_wq_gemv": (c_int, [_P, c_int, _P, c_int, _P, _P, c_int, _P, c_int, c_int, c_int, c_int, c_int, c_int, c_int, _P]),
    "vly_wq_gemv_rmsnorm": (c_int, [_P, c_int, _P, c_float, _P, c_int, _P, _P, c_int, _P, c_int, c_int, c_int, c_int, c_int, c_int,
                                    c_int, _P]),
    "vly_wq_gemv_rmsnorm_supported": (c_int, [c_int, c_int]),
}
EXPORTS = tuple(SIGS)
ABI_VERSION = 1

_LIB = None
_LOCK = threading.Lock()


def lib_path() -> str:
    return os.environ.get("VALLEY_HIP_WQ_LIB", _build.LIB_WQ)


def load_wq():
    """Load (once) and type libvalley_hip_wq.so.  Raises if it is absent, incomplete or of another ABI version."""
    global _LIB
    if _LIB is not None:
        return _LIB
    with _LOCK:
        if _LIB is not None:
            return _LIB
        path = lib_path()
        if not os.path.exists(path):
            raise ValleyHipError(f"{path} not found: build it with `python -m valley_amd.build` (hipcc --offload-arch=gfx950). "
                                 "INT8 weight-only decode has no non-HIP path.")
        lib = ctypes.CDLL(path)
        for name, (res, args) in SIGS.items():
            try:
                fn = getattr(lib, name)
            except AttributeError as e:
                raise ValleyHipError(f"{path} does not export {name}") from e
            fn.restype = res
            fn.argtypes = args
        if lib.vly_wq_abi_version() != ABI_VERSION:
            raise ValleyHipError(f"wq ABI mismatch: library {lib.vly_wq_abi_version()} vs binding {ABI_VERSION}")
        _LIB = lib
        return lib


def check(rc: int, what: str):
    if rc != 0:
        msg = load_wq().vly_wq_last_error().decode(errors="replace")
        raise ValleyHipError(f"{what} failed (rc={rc}): {msg}")
