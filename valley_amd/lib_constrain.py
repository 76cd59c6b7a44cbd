"""ctypes binding of libvalley_hip_constrain.so (include/valley_hip_constrain.h): token constraints on the device.

A companion of libvalley_hip.so with its own ABI version; it reads fp32 logits and int32 ids only, so the same library
serves every precision.  Missing or stale, it fails loudly: the constraints have no non-HIP path."""
from __future__ import annotations

from ctypes import c_char_p, c_int, c_void_p

from . import build as _build
from .companion import Companion

_P = c_void_p
SIGS = {
    "vly_constrain_abi_version": (c_int, []),
    "vly_constrain_last_error": (c_char_p, []),
    "vly_constrain_apply": (c_int, [_P, c_int, c_int, c_int, _P, _P, c_int, _P, c_int, _P, c_int, c_int, _P]),
}
EXPORTS = tuple(SIGS)
ABI_VERSION = 1
MAX_WORD = 64        # VLY_CONSTRAIN_MAX_WORD
MAX_DEPTH = 64       # VLY_CONSTRAIN_MAX_DEPTH
HEADER = 16          # VLY_CONSTRAIN_HEADER
BAD_WORDS, TRIE, FORCED_EOS, SUPPRESS, BEGIN_SUPPRESS = 1, 2, 4, 8, 16     # VLY_CONSTRAIN_<rule>: the bits of a row's flags

COMPANION = Companion("constrain", SIGS, ABI_VERSION, _build.LIB_CONSTRAIN, "Token constraints have no non-HIP path.")
load, loaded, check, lib_path, reset = COMPANION.load, COMPANION.loaded, COMPANION.check, COMPANION.lib_path, COMPANION.reset
