"""ctypes binding of libvalley_hip_spec_rows.so (include/valley_hip_spec_rows.h): prompt-lookup speculative decoding for
several sequences in one verify step — RoPE and KV append, split attention, draft lookup, acceptance and draw counters, every
sequence at its own device-side position.

A companion of libvalley_hip.so with its own ABI version; one build serves both 16-bit storage types (the dtype code).  Loaded
on first use only: a run that never speculates over a batch never maps it.  Missing or stale, it fails loudly: batched
speculative decoding has no non-HIP path."""
from __future__ import annotations

from ctypes import c_char_p, c_int, c_void_p

from . import build as _build
from .companion import Companion

_P = c_void_p
SIGS = {
    "vly_spec_rows_abi_version": (c_int, []),
    "vly_spec_rows_last_error": (c_char_p, []),
    "vly_spec_rows_rope_kv": (c_int, [_P, _P, _P, _P, _P, c_int, c_int, c_int, _P, c_int, c_int, _P]),
    "vly_spec_rows_attention": (c_int, [_P, _P, _P, _P, c_int, _P, c_int, c_int, c_int, _P, c_int, _P, _P, c_int, _P]),
    "vly_spec_rows_draft": (c_int, [_P, c_int, _P, c_int, _P, c_int, c_int, c_int, _P, c_int, c_int, c_int, _P, _P, _P, _P]),
    "vly_spec_rows_accept": (c_int, [_P, _P, _P, _P, c_int, c_int, _P, c_int, _P, _P, _P, _P, _P]),
    "vly_spec_rows_counters": (c_int, [_P, c_int, c_int, c_int, _P, _P]),
}
EXPORTS = tuple(SIGS)
ABI_VERSION = 1
MAX_QUERIES = 8          # VLY_SPEC_ROWS_MAX_QUERIES
MAX_DRAFT = 7            # VLY_SPEC_ROWS_MAX_DRAFT
MAX_NGRAM = 8            # VLY_SPEC_ROWS_MAX_NGRAM
SPLITS = 4               # VLY_SPEC_ROWS_SPLITS
PARTIAL = 132            # VLY_SPEC_ROWS_PARTIAL

COMPANION = Companion("spec_rows", SIGS, ABI_VERSION, _build.LIB_SPEC_ROWS, "Batched speculative decoding has no non-HIP path.")
load, loaded, check, lib_path, reset = COMPANION.load, COMPANION.loaded, COMPANION.check, COMPANION.lib_path, COMPANION.reset
