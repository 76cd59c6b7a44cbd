"""Conversation KV reuse without a GPU (include/valley_hip_suffix.h, valley_amd/prefix.py): the third build table and the
library's four exports, the refusals of ops.suffix_attention before the library is loaded, the host logic of
``common_prefix``, the oracle's own conditions on the kernel cases of tests/suffix_cases.py (gap, rounds, the fp64 reference
passes, every mask mutation is caught), and the turn-2 prompt's unambiguous greedy tokens."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import attention_oracle as AO
from tests import golden_cfg as G
from tests import suffix_cases as SC
from tests.test_companions_cpu import exported, header_macro, header_symbols, header_text
from valley_amd import build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["vly_suffix_abi_version", "vly_suffix_attention", "vly_suffix_last_error", "vly_suffix_scratch_bytes"]


# ---- the build table, the exports, the lazy load ------------------------------------------------------------------------------
def test_the_third_table_is_the_suffix_companion():
    assert [c.name for c in build.COMPANIONS_SUFFIX] == ["suffix"]
    others = {c.name for c in (*build.COMPANIONS, *build.COMPANIONS_ROWS)}
    assert "suffix" not in others and len(build.COMPANIONS) == 7 and [c.name for c in build.COMPANIONS_ROWS] == ["spec_rows"]
    c = build.COMPANIONS_SUFFIX[0]
    assert c.lib == build.LIB_SUFFIX == os.path.join(build.LIBDIR, "libvalley_hip_suffix.so") and c.header == "valley_hip_suffix.h"
    assert c.lib not in {o.lib for o in (*build.COMPANIONS, *build.COMPANIONS_ROWS)}
    src = open(os.path.join(build.CSRC, c.sources[0])).read()
    assert set(re.findall(r'#include "([a-z0-9_]+\.(?:hpp|inc))"', src)) <= set(c.deps) | set(build.COMPANION_SHARED)


def test_header_binding_and_library_agree():
    build.build(verbose=False)
    from valley_amd import lib_suffix, ops
    assert header_symbols("valley_hip_suffix.h") == NAMES == sorted(lib_suffix.EXPORTS) == exported(build.LIB_SUFFIX)
    assert re.search(r"#define VLY_SUFFIX_ABI_VERSION 1\b", header_text("valley_hip_suffix.h")) and lib_suffix.ABI_VERSION == 1
    assert lib_suffix.load().vly_suffix_abi_version() == 1
    assert header_macro("valley_hip_suffix.h", "VLY_SUFFIX_MAX_QUERIES") == 64 == lib_suffix.MAX_QUERIES == ops.SUFFIX_MAX_QUERIES
    assert header_macro("valley_hip_suffix.h", "VLY_SUFFIX_MAX_SPLITS") == lib_suffix.MAX_SPLITS == ops.SUFFIX_MAX_SPLITS
    assert header_macro("valley_hip_suffix.h", "VLY_SUFFIX_PARTIAL") == lib_suffix.PARTIAL == ops.SUFFIX_PARTIAL
    # the host-side size rule is the library's (no device needed), and out-of-range arguments give 0
    sb = lib_suffix.load().vly_suffix_scratch_bytes
    for B, S, heads in ((1, 1, 2), (1, 64, 40), (3, 20, 2)):
        assert sb(B, S, heads) == 4 * ops._suffix_scratch_words(B, S, heads)
    assert sb(1, 65, 2) == 0 and sb(0, 1, 2) == 0 and sb(1, 0, 2) == 0
    # the other libraries are what they were
    assert len(exported(build.LIB)) == 52 and not [n for n in exported(build.LIB) if "suffix" in n]
    for c in (*build.COMPANIONS, *build.COMPANIONS_ROWS):
        assert not [n for n in exported(c.lib) if "suffix" in n], c.name


def test_bad_arguments_to_the_entry_point_return_einval():
    """No launch is made for bad arguments: -22 and a message (checked with NULL pointers, which are themselves refused)."""
    build.build(verbose=False)
    from valley_amd import lib_suffix
    lib = lib_suffix.load()
    assert lib.vly_suffix_attention(None, None, None, None, 0, None, 1, 65, 2, 0, None, 128, 0, None, None) == -22
    assert b"S=65" in lib.vly_suffix_last_error()
    assert lib.vly_suffix_attention(None, None, None, None, 0, None, 1, 4, 2, 126, None, 128, 0, None, None) == -22


def test_importing_ops_does_not_load_the_library():
    code = ("import sys; import valley_amd.ops as ops; from valley_amd import lib_suffix; "
            "assert not lib_suffix.loaded() and 'valley_amd.prefix' not in sys.modules; print('ok')")
    p = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, cwd=ROOT)
    assert p.returncode == 0 and p.stdout.strip() == "ok", p.stderr[-2000:]


# ---- ops.suffix_attention refuses before the library is loaded ----------------------------------------------------------------
def _args(S=4, past=10, heads=2, ctx=64, B=1):
    from valley_amd.runtime import HALF
    return dict(qkv=torch.zeros((B * S, 3 * heads * 128), dtype=HALF), k=torch.zeros((B, heads, ctx, 128), dtype=HALF),
                v=torch.zeros((B, heads, ctx, 128), dtype=HALF), key_valid=None, B=B, S=S, heads=heads, past=past,
                scratch=torch.zeros((B * heads * S * 16 * 132 + B * heads,), dtype=torch.int32))


@pytest.mark.parametrize("what", ["S0", "S65", "cpu", "qkv_dtype", "k_dtype", "scratch_dtype", "qkv_shape", "k_shape", "v_shape", "past_room",
                                  "scratch_small", "valid_narrow", "valid_dtype", "out_shape"])
def test_suffix_attention_refuses_without_a_device(what):
    from valley_amd import lib_suffix, ops
    from valley_amd.runtime import HALF
    lib_suffix.reset()
    a = _args()
    if what == "S0":
        a = _args(S=1)
        a["S"] = 0
    elif what == "S65":
        a = _args(S=65, ctx=128)
    elif what == "cpu":
        pass                                                 # well-formed host tensors: the device check refuses them
    elif what == "qkv_dtype":
        a["qkv"] = a["qkv"].float()
    elif what == "k_dtype":
        a["k"] = a["k"].to(torch.float16 if HALF == torch.bfloat16 else torch.bfloat16)
    elif what == "scratch_dtype":
        a["scratch"] = a["scratch"].float()
    elif what == "qkv_shape":
        a["qkv"] = a["qkv"][:, :-128].contiguous()
    elif what == "k_shape":
        a["k"] = a["k"][:, :, :, :64].contiguous()
    elif what == "v_shape":
        a["v"] = a["v"][:, :, :32].contiguous()
    elif what == "past_room":
        a["past"] = 61
    elif what == "scratch_small":
        a["scratch"] = a["scratch"][:100].contiguous()
    elif what == "valid_narrow":
        a["key_valid"] = torch.ones((1, 13), dtype=torch.uint8)
    elif what == "valid_dtype":
        a["key_valid"] = torch.ones((1, 64), dtype=torch.bool)
    elif what == "out_shape":
        a["out"] = torch.zeros((4, 128), dtype=HALF)
    with pytest.raises(ValueError):
        ops.suffix_attention(**a)
    assert not lib_suffix.loaded()


# ---- common_prefix ------------------------------------------------------------------------------------------------------------
def test_common_prefix():
    from valley_amd.prefix import common_prefix, same_frames
    vis = [300, 301, 302]
    prompt = [1, 5, 300, 301, 301, 302, 7, 8]
    ans = [20, 21, 22, 23]
    cached = prompt + ans
    assert common_prefix(cached, cached, vis, True) == len(cached) - 1                        # identical ids: one position is computed
    assert common_prefix(cached, cached[:5], vis, True) == 0                                  # ... and here it is a placeholder
    assert common_prefix(cached, cached + [9, 9], vis, True) == len(cached)
    assert common_prefix(cached, prompt + ans[:2] + [99, 98], vis, True) == len(prompt) + 2   # divergence inside the previous answer
    assert common_prefix(cached, prompt + ans[:2], vis, True) == len(prompt) + 1              # cap at len - 1
    assert common_prefix(cached, [1, 5, 300, 301, 301, 302, 7, 9, 300], vis, True) == 0       # a placeholder in the suffix
    assert common_prefix(cached, [1, 6] + prompt[2:], vis, True) == 0                         # ... the whole visual block is
    assert common_prefix(cached, cached + [9], vis, False) == 0                               # changed frames
    assert common_prefix([], cached, vis, True) == 0 and common_prefix([], [4], [], True) == 0   # an empty session
    assert common_prefix(cached, [], vis, True) == 0
    a = torch.zeros((2, 3))
    ver = (a._version,)
    assert same_frames(a, ver, a) and same_frames(a, ver, a.clone()) and not same_frames(a, ver, a + 1)
    assert same_frames(None, (), None) and not same_frames(a, ver, None) and not same_frames(None, (), a)
    assert same_frames([a, a], (a._version,) * 2, [a, a.clone()]) and not same_frames([a, a], (a._version,) * 2, [a])
    a.add_(1)                                                                                 # the same object, written since
    assert not same_frames(a, ver, a)


def test_attention_arm_is_resolved_from_the_argument_then_the_environment(monkeypatch):
    from valley_amd import prefix
    monkeypatch.delenv("VALLEY_SUFFIX_ATTN", raising=False)
    assert prefix.resolve_attention(None) == prefix.DEFAULT_ATTENTION and prefix.DEFAULT_ATTENTION in prefix.ATTENTION_ARMS
    monkeypatch.setenv("VALLEY_SUFFIX_ATTN", "split")
    assert prefix.resolve_attention(None) == "split" and prefix.resolve_attention("prefill") == "prefill"
    with pytest.raises(ValueError):
        prefix.resolve_attention("fast")


def test_truncate_sets_the_length_and_refuses_growth():
    from valley_amd.llama import HipKVCache
    c = HipKVCache.__new__(HipKVCache)
    c.seq_len = 40
    c.truncate(12)
    assert c.seq_len == 12 and c.get_seq_length() == 12
    c.truncate(12)
    for bad in (13, -1):
        with pytest.raises(ValueError):
            c.truncate(bad)


# ---- the kernel cases satisfy the oracle's own conditions ---------------------------------------------------------------------
def test_the_cases_are_the_issues():
    assert len(SC.CASES) == 14 and len(SC.BY_NAME) == 14 and set(SC.DENSE) <= set(SC.BY_NAME) and SC.FP16_CASE in SC.BY_NAME
    assert all(1 <= c.S <= 64 for c in SC.CASES) and {c.S for c in SC.CASES} >= {1, 15, 16, 17, 33, 48, 63, 64}
    assert any(c.past + c.S == c.ctx_max for c in SC.CASES) and any(c.heads == 40 for c in SC.CASES) and any(c.B == 3 for c in SC.CASES)


@pytest.mark.parametrize("case", SC.CASES, ids=lambda c: c.name)
def test_gap_and_rounds_of_every_case(case):
    """check (a)'s condition on the case as the GPU runs it: build_pointer asserts G >= 160 in every round, on both storage
    types; the smallest gap over the list is 310 log2 units, no case needs more than 9 rounds."""
    assert case.ctx_max <= AO.code_table(AO.D).shape[0]
    rounds = AO.pointer_rounds(case)
    assert rounds <= 9
    for dtype in (torch.bfloat16, torch.float16):
        for rnd in range(rounds):
            inp = AO.build_pointer(case, dtype, "cpu", rnd)
            assert AO.assert_gap(inp) >= 310.0
    assert bool(case.live_rows().all())                     # no dead query row in the list: every row is checked


def _cpu(case):
    return AO.Case(**{**case.__dict__, "heads": min(case.heads, 2)})


def _checks(case, dtype, vis=None):
    run = lambda inp: AO.reference(inp, vis).to(dtype)      # noqa: E731
    res = {}
    for name, fn in (("pointer", lambda: AO.check_pointer(case, run, dtype, rounds=1)),
                     ("invisible", lambda: AO.check_invisible(case, run, dtype, cuts=AO.thin_cuts(case.S))),
                     ("count", lambda: AO.check_count(case, run, dtype))):
        try:
            fn()
            res[name] = None
        except AssertionError as e:
            res[name] = str(e)
    return res


@pytest.mark.parametrize("n", range(len(SC.CASES)), ids=[c.name for c in SC.CASES])
def test_reference_passes_and_every_mutation_is_caught(n):
    c = _cpu(SC.CASES[n])
    for dtype in (torch.bfloat16, torch.float16):
        res = _checks(c, dtype)
        assert all(v is None for v in res.values()), res
    dtype = torch.float16 if n % 2 else torch.bfloat16
    muts = AO.mutations(c)
    assert "newest_key_dropped" in muts and "causal_plus_one" in muts
    for name, vis in muts.items():
        caught = [k for k, v in _checks(c, dtype, vis).items() if v is not None]
        assert caught, f"{c.name}: mutation {name} passed all three checks"


# ---- the turn-2 prompt --------------------------------------------------------------------------------------------------------
def test_turn2_prompt_is_unambiguous():
    from oracle import valley_oracle as O
    g = np.load(os.path.join(ROOT, "tests", "golden", "g5_decode2.npz"))
    c = G.GCFG
    ids1 = G.golden_ids("decode2")[0]
    assert ids1.shape == (1, 283)
    assert ids1[0, 272] == G.special()["vi_end_token"] and not set(G.special().values()) & set(ids1[0, 273:].tolist())
    ids2 = SC.turn2_ids(ids1[0].tolist(), g["tokens"][0].tolist())
    assert len(ids2) == 329 and ids2[:283] == ids1[0].tolist() and ids2[283:289] == g["tokens"][0, :6].tolist()
    lcfg = O.LlamaCfg(hidden=c["H"], heads=c["heads"], intermediate=c["I"], layers=c["L"], vocab=c["vocab"], eps=c["eps"])
    vcfg = O.VisionCfg(intermediate=c["VI"], layers=c["VL"])
    px = torch.from_numpy(G.golden_pixels(c["T"], "mixed")).view(1, c["T"], 3, 224, 224)
    with torch.no_grad():
        toks, lasts = O.greedy_decode(torch.tensor([ids2]), px, G.llama_state(), G.vision_state(), lcfg, vcfg,
                                      O.TokenIds(**G.special()), len(SC.TURN2_TOKENS))
    assert toks[0].tolist() == SC.TURN2_TOKENS
    srt = np.sort(np.asarray(lasts)[0], -1)
    assert float((srt[:, -1] - srt[:, -2]).min()) >= SC.TURN2_MIN_GAP
