"""ctypes binding of libvalley_hip_suffix.so (include/valley_hip_suffix.h): the split attention of 1..64 new queries over a
cached prefix — the launch of a conversation's next turn when the earlier turns' K / V are still in the cache.

A companion of libvalley_hip.so with its own ABI version; one build serves both 16-bit storage types (the attention takes
the dtype code).  Loaded on first use only: a run without a prefix session never maps it.  Missing or stale, it fails loudly:
the split suffix attention has no non-HIP path."""
from __future__ import annotations

from ctypes import c_char_p, c_int, c_size_t, c_void_p

from . import build as _build
from .companion import Companion

_P = c_void_p
SIGS = {
    "vly_suffix_abi_version": (c_int, []),
    "vly_suffix_last_error": (c_char_p, []),
    "vly_suffix_scratch_bytes": (c_size_t, [c_int, c_int, c_int]),
    "vly_suffix_attention": (c_int, [_P, _P, _P, _P, c_int, _P, c_int, c_int, c_int, c_int, _P, c_int, c_int, _P, _P]),
}
EXPORTS = tuple(SIGS)
ABI_VERSION = 1
MAX_QUERIES = 64         # VLY_SUFFIX_MAX_QUERIES
MAX_SPLITS = 16          # VLY_SUFFIX_MAX_SPLITS
PARTIAL = 132            # VLY_SUFFIX_PARTIAL

COMPANION = Companion("suffix", SIGS, ABI_VERSION, _build.LIB_SUFFIX, "The split suffix attention has no non-HIP path.")
load, loaded, check, lib_path, reset = COMPANION.load, COMPANION.loaded, COMPANION.check, COMPANION.lib_path, COMPANION.reset
