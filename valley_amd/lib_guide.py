"""ctypes binding of libvalley_hip_guide.so (include/valley_hip_guide.h): classifier-free guidance on the device.

A companion of libvalley_hip.so with its own ABI version; it reads fp32 logits and int32 only, so the same library
serves every precision.  Missing or stale, it fails loudly: guidance has no non-HIP path."""
from __future__ import annotations

from ctypes import c_char_p, c_int, c_void_p

from . import build as _build
from .companion import Companion

_P = c_void_p
SIGS = {
    "vly_guide_abi_version": (c_int, []),
    "vly_guide_last_error": (c_char_p, []),
    "vly_guide_apply": (c_int, [_P, c_int, c_int, c_int, _P, _P]),
    "vly_guide_follow": (c_int, [_P, c_int, _P, _P]),
}
EXPORTS = tuple(SIGS)
ABI_VERSION = 1
NEUTRAL, COND, UNCOND = 0, 1, 2      # VLY_GUIDE_<role>

COMPANION = Companion("guide", SIGS, ABI_VERSION, _build.LIB_GUIDE, "Classifier-free guidance has no non-HIP path.")
load, loaded, check, lib_path, reset = COMPANION.load, COMPANION.loaded, COMPANION.check, COMPANION.lib_path, COMPANION.reset
