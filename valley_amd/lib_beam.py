"""ctypes binding of libvalley_hip_beam.so (include/valley_hip_beam.h): the beam-search kernels.

A companion of libvalley_hip.so with its own ABI version; it does not depend on the 16-bit storage type, so the same
library serves every precision.  Missing or stale, it fails loudly: beam search has no non-HIP path."""
from __future__ import annotations

from ctypes import c_char_p, c_int, c_size_t, c_void_p

from . import build as _build
from .companion import Companion

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

COMPANION = Companion("beam", SIGS, ABI_VERSION, _build.LIB_BEAM, "Beam search has no non-HIP path.")
load, loaded, check, lib_path, reset = COMPANION.load, COMPANION.loaded, COMPANION.check, COMPANION.lib_path, COMPANION.reset
