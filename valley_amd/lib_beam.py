"""ctypes binding of libvalley_hip_beam.so (include/valley_hip_beam.h): the beam-search kernels.

A companion of libvalley_hip.so with its own ABI version; it does not depend on the 16-bit storage type, so the same
library serves every precision.  Missing or stale, it fails loudly: beam search has no non-HIP path."""
from __future__ import annotations

import ctypes
import os
import threading
from ctypes import c_char_p, c_int, c_size_t, c_void_p

from . import build as _build
from .lib import ValleyHipError

_P = c_void_p
SIGS = {
    "vly_beam_abi_version": (c_int, []),
    "vly_beam_last_error": (c_char_p, []),
    "vly_beam_scratch_bytes": (c_size_t, [c_int, c_int, c_int]),
    "vly_beam_candidates": (c_int, [_P, c_int, c_int, c_int, c_int, _P, c_int, _P, c_int, _P, _P, _P, _P, _P, _P]),
    "vly_beam_select": (c_int, [_P, _P, _P, _P, c_int, c_int, c_int, _P, _P, _P, _P]),
    "vly_kv_beam_reorder": (c_int, [_P, c_int, c_int, c_int, c_int, c_int, _P, c_int, _P, c_int, _P]),
}
EXPORTS = tuple(SIGS)
ABI_VERSION = 1

_LIB = None
_LOCK = threading.Lock()


def lib_path() -> str:
    return os.environ.get("VALLEY_HIP_BEAM_LIB", _build.LIB_BEAM)


def load_beam():
    """Load (once) and type libvalley_hip_beam.so.  Raises if it is absent, incomplete or of another ABI version."""
    global _LIB
    if _LIB is not None:
        return _LIB
    with _LOCK:
        if _LIB is not None:
            return _LIB
        path = lib_path()
        if not os.path.exists(path):
            raise ValleyHipError(f"{path} not found: build it with `python -m valley_amd.build` (hipcc --offload-arch=gfx950). "
                                 "Beam search has no non-HIP path.")
        lib = ctypes.CDLL(path)
        for name, (res, args) in SIGS.items():
            try:
                fn = getattr(lib, name)
            except AttributeError as e:
                raise ValleyHipError(f"{path} does not export {name}") from e
            fn.restype = res
            fn.argtypes = args
        if lib.vly_beam_abi_version() != ABI_VERSION:
            raise ValleyHipError(f"beam ABI mismatch: library {lib.vly_beam_abi_version()} vs binding {ABI_VERSION}")
        _LIB = lib
        return lib


def check(rc: int, what: str):
    if rc != 0:
        msg = load_beam().vly_beam_last_error().decode(errors="replace")
        raise ValleyHipError(f"{what} failed (rc={rc}): {msg}")
