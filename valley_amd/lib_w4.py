"""ctypes binding of libvalley_hip_w4.so (include/valley_hip_w4.h): weight-only INT4 decode — the group quantizer (one fp32
scale per 128 weights of a row) and the 4-bit weight-streaming GEMVs.

A companion of libvalley_hip.so with its own ABI version; every compute entry takes the 16-bit storage type as an argument,
so the same library serves the bf16 and the fp16 engine.  Loaded only by an engine that quantized its weights.  Missing or
stale, it fails loudly: the int4 path has no non-HIP form."""
from __future__ import annotations

from ctypes import c_char_p, c_float, c_int, c_void_p

from . import build as _build
from .companion import Companion

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

COMPANION = Companion("w4", SIGS, ABI_VERSION, _build.LIB_W4, "INT4 weight-only decode has no non-HIP path.")
load, loaded, check, lib_path, reset = COMPANION.load, COMPANION.loaded, COMPANION.check, COMPANION.lib_path, COMPANION.reset
