"""ctypes binding of libvalley_hip_logits.so (include/valley_hip_logits.h): HF's logits processors on the device.

A companion of libvalley_hip.so with its own ABI version; it reads fp32 logits and int32 ids only, so the same library
serves every precision.  Missing or stale, it fails loudly: the processors have no non-HIP path."""
from __future__ import annotations

from ctypes import c_char_p, c_int, c_size_t, c_void_p

from . import build as _build
from .companion import Companion

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

COMPANION = Companion("logits", SIGS, ABI_VERSION, _build.LIB_LOGITS, "The logits processors have no non-HIP path.")
load, loaded, check, lib_path, reset = COMPANION.load, COMPANION.loaded, COMPANION.check, COMPANION.lib_path, COMPANION.reset
