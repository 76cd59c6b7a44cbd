"""ctypes binding of libvalley_hip_spec_sample.so (include/valley_hip_spec_sample.h): the draw counters of a speculative
verify step under seeded sampling.

A companion of libvalley_hip_spec.so with its own ABI version, int32 only.  Loaded on first use: a greedy speculative
generation never maps it.  Missing or stale, it fails loudly: the sampled verify step has no non-HIP path."""
from __future__ import annotations

import ctypes
import os
import threading
from ctypes import c_char_p, c_int, c_void_p

from . import build as _build
from .lib import ValleyHipError

_P = c_void_p
SIGS = {
    "vly_spec_sample_abi_version": (c_int, []),
    "vly_spec_sample_last_error": (c_char_p, []),
    "vly_spec_counters": (c_int, [_P, c_int, c_int, _P, _P]),
}
EXPORTS = tuple(SIGS)
ABI_VERSION = 1
MAX_DRAFT = 7            # VLY_SPEC_SAMPLE_MAX_DRAFT

_LIB = None
_LOCK = threading.Lock()


def lib_path() -> str:
    return os.environ.get("VALLEY_HIP_SPEC_SAMPLE_LIB", _build.LIB_SPEC_SAMPLE)


def load_spec_sample():
    """Load (once) and type libvalley_hip_spec_sample.so.  Raises if it is absent, incomplete or of another ABI version."""
    global _LIB
    if _LIB is not None:
        return _LIB
    with _LOCK:
        if _LIB is not None:
            return _LIB
        path = lib_path()
        if not os.path.exists(path):
            raise ValleyHipError(f"{path} not found: build it with `python -m valley_amd.build` (hipcc --offload-arch=gfx950). "
                                 "Speculative decoding under sampling has no non-HIP path.")
        lib = ctypes.CDLL(path)
        for name, (res, args) in SIGS.items():
            try:
                fn = getattr(lib, name)
            except AttributeError as e:
                raise ValleyHipError(f"{path} does not export {name}") from e
            fn.restype = res
            fn.argtypes = args
        if lib.vly_spec_sample_abi_version() != ABI_VERSION:
            raise ValleyHipError(f"spec-sample ABI mismatch: library {lib.vly_spec_sample_abi_version()} vs binding {ABI_VERSION}")
        _LIB = lib
        return lib


def check(rc: int, what: str):
    if rc != 0:
        msg = load_spec_sample().vly_spec_sample_last_error().decode(errors="replace")
        raise ValleyHipError(f"{what} failed (rc={rc}): {msg}")
