"""ctypes binding of libvalley_hip_score.so (include/valley_hip_score.h): token log-probabilities, top-n alternatives, the
decode step's per-token record and the forward-only cross-entropy.

A companion of libvalley_hip.so with its own ABI version; it reads fp32 logits and int32 ids only, so the same library
serves every precision.  Loaded on first use only: a run that never asks for scores never maps it.  Missing or stale, it
fails loudly: the scores have no non-HIP path."""
from __future__ import annotations

from ctypes import c_char_p, c_int, c_void_p

from . import build as _build
from .companion import Companion

_P = c_void_p
SIGS = {
    "vly_score_abi_version": (c_int, []),
    "vly_score_last_error": (c_char_p, []),
    "vly_score_rows": (c_int, [_P, c_int, c_int, c_int, _P, _P, _P, c_int, _P, _P, _P, c_int, _P]),
    "vly_score_record": (c_int, [_P, c_int, c_int, c_int, _P, _P, _P, c_int, c_int, _P, c_int, c_int, _P, _P, _P, _P, _P]),
    "vly_score_loss": (c_int, [_P, _P, c_int, c_int, _P, _P, _P]),
}
EXPORTS = tuple(SIGS)
ABI_VERSION = 1
MAX_TOP = 20             # VLY_SCORE_MAX_TOP

COMPANION = Companion("score", SIGS, ABI_VERSION, _build.LIB_SCORE, "Token log-probabilities and the loss have no non-HIP path.")
load, loaded, check, lib_path, reset = COMPANION.load, COMPANION.loaded, COMPANION.check, COMPANION.lib_path, COMPANION.reset
