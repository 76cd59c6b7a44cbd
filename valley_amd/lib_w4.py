"""ctypes binding of libvalley_hip_w4.so (include/valley_hip_w4.h): weight-only INT4 decode — the group quantizer (one fp32
scale per 128 weights of a row) and the 4-bit weight-streaming GEMVs.

A companion of libvalley_hip.so with its own ABI version; every compute entry takes the 16-bit storage type as an argument,
so the same library serves the bf16 and the fp16 engine.  Loaded only by an engine that quantized its weights.  Missing or
stale, it fails loudly: the int4 path has no non-HIP form."""
from __future__ import annotations

import ctypes
import os
import threading
from ctypes import c_char_p, c_float, c_int, c_void_p

from . import build as _build
from .lib import ValleyHipError

_P = c_void_p
SIGS = {
    "vly_w4_abi_version": (c_int, []),
    "vly_w4_last_error": (c_char_p, []),
    "vly_w4_quantize_rows": (c_int, [_P, c_int, c_int, c_int, c_int, _P, _P, _P]),
    "vly_w4_gemv": (c_int, [_P, c_int, _P, c_int, _P, _P, c_int, _P, c_int, c_int, c_int, c_int, c_int, c_int, c_int, _P]),
    "vly_w4_gemv_rmsnorm": (c_int, [_P, c_int, _P, c_float, _P, c_int, _P, _P, c_int, _P, c_int, c_int, c_int, c_int, c_int, c_int,
                                    c_int, _P]),
    "vly_w4_gemv_rmsnorm_supported": (c_int, [c_int, c_int]),
}
EXPORTS = tuple(SIGS)
ABI_VERSION = 1

_LIB = None
_LOCK = threading.Lock()


def lib_path() -> str:
    return os.environ.get("VALLEY_HIP_W4_LIB", _build.LIB_W4)


def load_w4():
    """Load (once) and type libvalley_hip_w4.so.  Raises if it is absent, incomplete or of another ABI version."""
    global _LIB
    if _LIB is not None:
        return _LIB
    with _LOCK:
        if _LIB is not None:
            return _LIB
        path = lib_path()
        if not os.path.exists(path):
            raise ValleyHipError(f"{path} not found: build it with `python -m valley_amd.build` (hipcc --offload-arch=gfx950). "
                                 "INT4 weight-only decode has no non-HIP path.")
        lib = ctypes.CDLL(path)
        for name, (res, args) in SIGS.items():
            try:
                fn = getattr(lib, name)
            except AttributeError as e:
                raise ValleyHipError(f"{path} does not export {name}") from e
            fn.restype = res
            fn.argtypes = args
        if lib.vly_w4_abi_version() != ABI_VERSION:
            raise ValleyHipError(f"w4 ABI mismatch: library {lib.vly_w4_abi_version()} vs binding {ABI_VERSION}")
        _LIB = lib
        return lib


def check(rc: int, what: str):
    if rc != 0:
        msg = load_w4().vly_w4_last_error().decode(errors="replace")
        raise ValleyHipError(f"{what} failed (rc={rc}): {msg}")
