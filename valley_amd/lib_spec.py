"""ctypes binding of libvalley_hip_spec.so (include/valley_hip_spec.h): prompt-lookup speculative decoding — the split
attention of the verify step's k + 1 queries, the draft lookup and the acceptance.

A companion of libvalley_hip.so with its own ABI version; one build serves both 16-bit storage types (the attention takes
the dtype code).  Loaded on first use only: a run that never speculates never maps it.  Missing or stale, it fails loudly:
speculative decoding has no non-HIP path."""
from __future__ import annotations

from ctypes import c_char_p, c_int, c_void_p

from . import build as _build
from .companion import Companion

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

COMPANION = Companion("spec", SIGS, ABI_VERSION, _build.LIB_SPEC, "Speculative decoding has no non-HIP path.")
load, loaded, check, lib_path, reset = COMPANION.load, COMPANION.loaded, COMPANION.check, COMPANION.lib_path, COMPANION.reset
