"""ctypes binding of libvalley_hip_spec_sample.so (include/valley_hip_spec_sample.h): the draw counters of a speculative
verify step under seeded sampling.

A companion of libvalley_hip_spec.so with its own ABI version, int32 only.  Loaded on first use: a greedy speculative
generation never maps it.  Missing or stale, it fails loudly: the sampled verify step has no non-HIP path."""
from __future__ import annotations

from ctypes import c_char_p, c_int, c_void_p

from . import build as _build
from .companion import Companion

_P = c_void_p
SIGS = {
    "vly_spec_sample_abi_version": (c_int, []),
    "vly_spec_sample_last_error": (c_char_p, []),
    "vly_spec_counters": (c_int, [_P, c_int, c_int, _P, _P]),
}
EXPORTS = tuple(SIGS)
ABI_VERSION = 1
MAX_DRAFT = 7            # VLY_SPEC_SAMPLE_MAX_DRAFT

COMPANION = Companion("spec_sample", SIGS, ABI_VERSION, _build.LIB_SPEC_SAMPLE,
                      "Speculative decoding under sampling has no non-HIP path.", label="spec-sample")
load, loaded, check, lib_path, reset = COMPANION.load, COMPANION.loaded, COMPANION.check, COMPANION.lib_path, COMPANION.reset
