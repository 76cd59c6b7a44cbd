"""ctypes binding of libvalley_hip_spec.so (include/valley_hip_spec.h): prompt-lookup speculative decoding — the split
attention of the verify step's k + 1 queries, the draft lookup and the acceptance.

A companion of libvalley_hip.so with its own ABI version; one build serves both 16-bit storage types (the attention takes
the dtype code).  Loaded on first use only: a run that never speculates never maps it.  Missing or stale, it fails loudly:
speculative decoding has no non-HIP path."""
from __future__ import annotations

import ctypes
import os
import threading
from ctypes import c_char_p, c_int, c_void_p

from . import build as _build
from .lib import ValleyHipError

_P = c_void_p
SIGS = {
    "vly_spec_abi_version": (c_int, []),
    "vly_spec_last_error": (c_char_p, []),
    "vly_spec_attention": (c_int, [_P, _P, _P, _P, c_int, _P, c_int, c_int, c_int, c_int, _P, c_int, _P, _P, c_int, _P]),
    "vly_spec_draft": (c_int, [_P, c_int, _P, c_int, c_int, c_int, _P, c_int, c_int, c_int, _P, _P, _P, _P]),
    "vly_spec_accept": (c_int, [_P, _P, _P, c_int, _P, c_int, _P, _P, _P, _P, _P]),
}
EXPORTS = tuple(SIGS)
ABI_VERSION = 1
MAX_QUERIES = 8          # VLY_SPEC_MAX_QUERIES
MAX_DRAFT = 7            # VLY_SPEC_MAX_DRAFT
MAX_NGRAM = 8            # VLY_SPEC_MAX_NGRAM
SPLITS = 4               # VLY_SPEC_SPLITS
PARTIAL = 132            # VLY_SPEC_PARTIAL

_LIB = None
_LOCK = threading.Lock()


def lib_path() -> str:
    return os.environ.get("VALLEY_HIP_SPEC_LIB", _build.LIB_SPEC)


def load_spec():
    """Load (once) and type libvalley_hip_spec.so.  Raises if it is absent, incomplete or of another ABI version."""
    global _LIB
    if _LIB is not None:
        return _LIB
    with _LOCK:
        if _LIB is not None:
            return _LIB
        path = lib_path()
        if not os.path.exists(path):
            raise ValleyHipError(f"{path} not found: build it with `python -m valley_amd.build` (hipcc --offload-arch=gfx950). "
                                 "Speculative decoding has no non-HIP path.")
        lib = ctypes.CDLL(path)
        for name, (res, args) in SIGS.items():
            try:
                fn = getattr(lib, name)
            except AttributeError as e:
                raise ValleyHipError(f"{path} does not export {name}") from e
            fn.restype = res
            fn.argtypes = args
        if lib.vly_spec_abi_version() != ABI_VERSION:
            raise ValleyHipError(f"spec ABI mismatch: library {lib.vly_spec_abi_version()} vs binding {ABI_VERSION}")
        _LIB = lib
        return lib


def check(rc: int, what: str):
    if rc != 0:
        msg = load_spec().vly_spec_last_error().decode(errors="replace")
        raise ValleyHipError(f"{what} failed (rc={rc}): {msg}")
