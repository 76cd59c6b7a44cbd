"""ctypes binding of libvalley_hip_wq.so (include/valley_hip_wq.h): weight-only INT8 decode — the per-row quantizer and the
int8 weight-streaming GEMVs.

A companion of libvalley_hip.so with its own ABI version; every compute entry takes the 16-bit storage type as an argument,
so the same library serves the bf16 and the fp16 engine.  Loaded only by an engine that quantized its weights.  Missing or
stale, it fails loudly: the int8 path has no non-HIP form."""
from __future__ import annotations

from ctypes import c_char_p, c_float, c_int, c_void_p

from . import build as _build
from .companion import Companion

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

COMPANION = Companion("wq", SIGS, ABI_VERSION, _build.LIB_WQ, "INT8 weight-only decode has no non-HIP path.")
load, loaded, check, lib_path, reset = COMPANION.load, COMPANION.loaded, COMPANION.check, COMPANION.lib_path, COMPANION.reset
