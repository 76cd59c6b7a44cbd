"""ctypes binding of libvalley_hip_stop.so (include/valley_hip_stop.h): EOS and HF's stop strings decided on the device.

A companion of libvalley_hip.so with its own ABI version; it reads int32 only, so the same library serves every precision.
Missing or stale, it fails loudly: stop strings on the device have no non-HIP path."""
from __future__ import annotations

from ctypes import c_char_p, c_int, c_void_p

from . import build as _build
from .companion import Companion

_P = c_void_p
SIGS = {
    "vly_stop_abi_version": (c_int, []),
    "vly_stop_last_error": (c_char_p, []),
    "vly_stop_apply": (c_int, [_P, _P, c_int, _P, c_int, c_int, _P, _P, _P, c_int, _P, c_int, c_int, _P]),
}
EXPORTS = tuple(SIGS)
ABI_VERSION = 1

COMPANION = Companion("stop", SIGS, ABI_VERSION, _build.LIB_STOP, "Stop strings on the device have no non-HIP path.")
load, loaded, check, lib_path, reset = COMPANION.load, COMPANION.loaded, COMPANION.check, COMPANION.lib_path, COMPANION.reset
