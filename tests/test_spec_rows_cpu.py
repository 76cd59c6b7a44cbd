"""CPU-side checks of batched prompt-lookup speculation: the companion contract of tests/test_companions_cpu.py applied to
valley_amd.build.COMPANIONS_ROWS, the argument refusals of the five ops.spec_rows_* wrappers and of
ContinuousBatcher(prompt_lookup_num_tokens=...) before anything is touched, and tests/spec_rows_ref.py against tests/spec_ref.py."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import spec_ref as SR
from tests import spec_rows_ref as RR
from tests.test_companions_cpu import exported, header_macro, header_symbols, header_text, stub_library
from valley_amd import build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENTENCE = "Batched speculative decoding has no non-HIP path."
NAMES = ["vly_spec_rows_abi_version", "vly_spec_rows_accept", "vly_spec_rows_attention", "vly_spec_rows_counters", "vly_spec_rows_draft",
         "vly_spec_rows_last_error", "vly_spec_rows_rope_kv"]


@pytest.fixture(scope="module")
def built():
    build.build(verbose=False)


# ---- the companion contract ---------------------------------------------------------------------------------------------------
def test_the_rows_table_sits_beside_the_seven():
    assert len(build.COMPANIONS) == 7 and [c.name for c in build.COMPANIONS_ROWS] == ["spec_rows"]
    assert not {c.name for c in build.COMPANIONS} & {c.name for c in build.COMPANIONS_ROWS}
    from valley_amd import lib_spec_rows
    c = build.COMPANIONS_ROWS[0]
    assert c.lib == build.LIB_SPEC_ROWS == os.path.join(build.LIBDIR, "libvalley_hip_spec_rows.so") == lib_spec_rows.lib_path()
    assert c.header == "valley_hip_spec_rows.h" and c.sources == ("spec_rows.hip",)
    # editing anything the unit includes recompiles it; the shared attention is a dependency of both libraries that instantiate it
    src = open(os.path.join(build.CSRC, "spec_rows.hip")).read()
    included = set(re.findall(r'#include "([a-z0-9_]+\.(?:hpp|inc))"', src))
    assert included <= set(c.deps) | set(build.COMPANION_SHARED) and {"spec_attn.inc", "spec_lookup.inc"} <= included
    spec = next(x for x in build.COMPANIONS if x.name == "spec")
    for inc in ("spec_attn.inc", "spec_lookup.inc"):             # ... and the draft and acceptance rules likewise
        assert inc in spec.deps and inc in c.deps and f'#include "{inc}"' in open(os.path.join(build.CSRC, "spec.hip")).read()
    # objects land under lib/spec_rows/, which .gitignore covers with the rest of the library directory
    assert "valley_amd/lib/" in open(os.path.join(ROOT, ".gitignore")).read().split()


def test_the_library_exports_exactly_its_header(built):
    from valley_amd import lib_spec_rows
    names = header_symbols("valley_hip_spec_rows.h")
    assert names == NAMES and len(names) == 7
    assert exported(build.LIB_SPEC_ROWS) == names == sorted(lib_spec_rows.EXPORTS)
    assert lib_spec_rows.load().vly_spec_rows_abi_version() == lib_spec_rows.ABI_VERSION == 1
    assert re.search(r"#define VLY_SPEC_ROWS_ABI_VERSION 1\b", header_text("valley_hip_spec_rows.h"))

def test_mirrored_constants(built):
    from valley_amd import lib_spec, lib_spec_rows, ops
    for macro, a, b in (("MAX_QUERIES", lib_spec_rows.MAX_QUERIES, ops.SPEC_MAX_QUERIES), ("MAX_DRAFT", lib_spec_rows.MAX_DRAFT, ops.SPEC_MAX_DRAFT),
                        ("MAX_NGRAM", lib_spec_rows.MAX_NGRAM, ops.SPEC_MAX_NGRAM), ("SPLITS", lib_spec_rows.SPLITS, lib_spec.SPLITS),
                        ("PARTIAL", lib_spec_rows.PARTIAL, lib_spec.PARTIAL)):
        assert header_macro("valley_hip_spec_rows.h", f"VLY_SPEC_ROWS_{macro}") == a == b, macro


def test_no_existing_library_gained_a_rows_name(built):
    libs = [build.LIB, build.LIB_F16, build.LIB_EXP, build.LIB_EXP_F16] + [c.lib for c in build.COMPANIONS]
    for path in libs:
        got = exported(path)
        assert not [n for n in got if n.startswith("vly_spec_rows_")] and not set(got) & set(NAMES), path
    # ... and the new library carries nobody else's
    others = {n for c in build.COMPANIONS for n in header_symbols(c.header)}
    assert not set(exported(build.LIB_SPEC_ROWS)) & others
    assert len(exported(build.LIB_SPEC)) == 5 and len(exported(build.LIB_SPEC_SAMPLE)) == 3


def test_missing_library_fails_loudly(monkeypatch, tmp_path):
    from valley_amd import lib, lib_spec_rows
    lib_spec_rows.reset()
    monkeypatch.setenv("VALLEY_HIP_SPEC_ROWS_LIB", str(tmp_path / "nope.so"))
    with pytest.raises(lib.ValleyHipError) as e:
        lib_spec_rows.load()
    assert str(e.value) == (f"{tmp_path / 'nope.so'} not found: build it with `python -m valley_amd.build` (hipcc --offload-arch=gfx950). "
                            f"{SENTENCE}")
    assert not lib_spec_rows.loaded()


def test_incomplete_and_mis_versioned_libraries_fail_loudly(monkeypatch, tmp_path):
    from valley_amd import lib, lib_spec_rows
    from valley_amd.companion import Companion

    def fresh():
        return Companion("spec_rows", lib_spec_rows.SIGS, lib_spec_rows.ABI_VERSION, build.LIB_SPEC_ROWS, SENTENCE)

    full = {n: 0 for n in NAMES}
    short = stub_library(tmp_path, "short", {n: v for n, v in dict(full, vly_spec_rows_abi_version=1).items() if n != "vly_spec_rows_draft"})
    monkeypatch.setenv("VALLEY_HIP_SPEC_ROWS_LIB", short)
    c = fresh()
    with pytest.raises(lib.ValleyHipError) as e:
        c.load()
    assert str(e.value) == f"{short} does not export vly_spec_rows_draft" and not c.loaded()
    stale = stub_library(tmp_path, "stale", dict(full, vly_spec_rows_abi_version=2))
    monkeypatch.setenv("VALLEY_HIP_SPEC_ROWS_LIB", stale)
    c = fresh()
    with pytest.raises(lib.ValleyHipError) as e:
        c.load()
    assert str(e.value) == "spec_rows ABI mismatch: library 2 vs binding 1" and not c.loaded()
    assert lib_spec_rows.COMPANION.label == "spec_rows" and lib_spec_rows.COMPANION.no_fallback == SENTENCE


def test_the_library_loads_once_and_not_on_import(built):
    from valley_amd import lib, lib_spec_rows
    h = lib_spec_rows.load()
    assert lib_spec_rows.load() is h and lib_spec_rows.loaded()
    lib_spec_rows.check(0, "nothing")
    with pytest.raises(lib.ValleyHipError, match=r"probe failed \(rc=-22\): "):
        lib_spec_rows.check(-22, "probe")
    code = ("import valley_amd, valley_amd.ops, valley_amd.spec, valley_amd.serving, valley_amd.lib_spec_rows as m\n"
            "assert not m.loaded()\n"
            "assert 'libvalley_hip_spec_rows.so' not in open('/proc/self/maps').read()\n"
            "print('lazy')\n")
    out = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.strip().endswith("lazy"), out.stderr[-2000:]


def test_bad_arguments_are_refused_by_the_library(built):
    from valley_amd import lib_spec_rows
    h = lib_spec_rows.load()
    ok = 4096

    def refused(fn, args, name):
        assert fn(*args) == -22, (name, args)
        assert name.encode() in h.vly_spec_rows_last_error()

    for args in ((None, ok, ok, ok, ok, 2, 4, 2, ok, 64, 0, None), (ok, ok, ok, ok, ok, 0, 4, 2, ok, 64, 0, None),
                 (ok, ok, ok, ok, ok, 2, 9, 2, ok, 64, 0, None), (ok, ok, ok, ok, ok, 2, 4, 2, None, 64, 0, None),
                 (ok, ok, ok, ok, ok, 2, 4, 2, ok, 0, 0, None), (ok, ok, ok, ok, ok, 2, 4, 2, ok, 64, 2, None),
                 (ok + 8, ok, ok, ok, ok, 2, 4, 2, ok, 64, 0, None)):
        refused(h.vly_spec_rows_rope_kv, args, "vly_spec_rows_rope_kv")
    for args in ((ok, ok, ok, None, 0, ok, 2, 0, 2, ok, 64, ok, ok, 0, None), (ok, ok, ok, None, 0, ok, 2, 9, 2, ok, 64, ok, ok, 0, None),
                 (ok, ok, ok, None, 0, ok, 2, 4, 2, None, 64, ok, ok, 0, None), (ok, ok, ok, ok, 63, ok, 2, 4, 2, ok, 64, ok, ok, 0, None),
                 (ok, ok, ok, None, 0, ok, 2, 4, 2, ok, 64, ok, None, 0, None), (ok, ok, ok, None, 0, ok, 2, 4, 2, ok, 64, None, ok, 0, None)):
        refused(h.vly_spec_rows_attention, args, "vly_spec_rows_attention")
    for args in ((None, 64, ok, 1, None, 2, 3, 2, None, 0, 0, 1, ok, ok, ok, None), (ok, 64, None, 1, None, 2, 3, 2, None, 0, 0, 1, ok, ok, ok, None),
                 (ok, 64, ok, 1, None, 0, 3, 2, None, 0, 0, 1, ok, ok, ok, None), (ok, 64, ok, 1, None, 2, 0, 2, None, 0, 0, 1, ok, ok, ok, None),
                 (ok, 64, ok, 1, None, 2, 8, 2, None, 0, 0, 1, ok, ok, ok, None), (ok, 64, ok, 1, None, 2, 3, 9, None, 0, 0, 1, ok, ok, ok, None),
                 (ok, 64, ok, 1, None, 2, 3, 2, None, 1, 0, 1, ok, ok, ok, None), (ok, 64, ok, 1, None, 2, 3, 2, None, 0, 0, 1, ok, ok, None, None)):
        refused(h.vly_spec_rows_draft, args, "vly_spec_rows_draft")
    for args in ((None, ok, ok, None, 2, 3, ok, 64, ok, ok, ok, ok, None), (ok, ok, ok, None, 0, 3, ok, 64, ok, ok, ok, ok, None),
                 (ok, ok, ok, None, 2, 8, ok, 64, ok, ok, ok, ok, None), (ok, ok, ok, None, 2, 3, ok, 0, ok, ok, ok, ok, None),
                 (ok, ok, ok, None, 2, 3, ok, 64, None, ok, ok, ok, None), (ok, ok, ok, None, 2, 3, ok, 64, ok, ok, ok, None, None)):
        refused(h.vly_spec_rows_accept, args, "vly_spec_rows_accept")
    for args in ((None, 2, 3, 64, ok, None), (ok, 0, 3, 64, ok, None), (ok, 2, 0, 64, ok, None), (ok, 2, 8, 64, ok, None),
                 (ok, 2, 3, 0, ok, None), (ok, 2, 3, 64, None, None), (ok + 2, 2, 3, 64, ok, None)):
        refused(h.vly_spec_rows_counters, args, "vly_spec_rows_counters")


# ---- the wrappers' refusals -----------------------------------------------------------------------------------------------------
def i32(*s):
    return torch.zeros(s, dtype=torch.int32)


def half(*s):
    from valley_amd.runtime import HALF
    return torch.zeros(s, dtype=HALF)


def test_the_ops_check_their_arguments_before_any_launch():
    from valley_amd import lib, ops
    B, S, heads, ctx = 2, 4, 2, 64
    qkv, kc, vc = half(B * S, 3 * heads * 128), half(B, heads, ctx, 128), half(B, heads, ctx, 128)
    cos = sin = torch.zeros((ctx, 64), dtype=torch.float32)
    scratch = (torch.zeros((B * heads * S * 4 * 132,)), i32(B * heads))
    for fn, tail in ((ops.spec_rows_rope_kv, lambda s, p: (cos, sin, B, s, heads, p)),
                     (ops.spec_rows_attention, lambda s, p: (None, B, s, heads, p, scratch))):
        name = fn.__name__
        for s in (0, 9):
            with pytest.raises(ValueError, match=rf"{name}: S must be in \[1, 8\]"):
                fn(half(B * max(s, 1), 3 * heads * 128), kc, vc, *tail(s, i32(B)))
        with pytest.raises(ValueError, match=f"{name}: kcache / vcache"):
            fn(qkv, half(1, heads, ctx, 128), half(1, heads, ctx, 128), *tail(S, i32(B)))
        with pytest.raises(ValueError, match=f"{name}: qkv"):
            fn(half(B * S + 1, 3 * heads * 128), kc, vc, *tail(S, i32(B)))
        for pos in (i32(1), i32(B, 1), torch.zeros((B,), dtype=torch.int64), 5):
            with pytest.raises(ValueError, match=f"{name}: pos must be int32"):
                fn(qkv, kc, vc, *tail(S, pos))
        with pytest.raises(lib.ValleyHipError):                  # all fine: no CPU compute path
            fn(qkv, kc, vc, *tail(S, i32(B)))
    with pytest.raises(ValueError, match="spec_rows_rope_kv: cos fp32"):
        ops.spec_rows_rope_kv(qkv, kc, vc, torch.zeros((ctx - 1, 64)), sin, B, S, heads, i32(B))
    with pytest.raises(ValueError, match="spec_rows_attention: key_valid"):
        ops.spec_rows_attention(qkv, kc, vc, torch.ones((B, ctx - 1), dtype=torch.uint8), B, S, heads, i32(B), scratch)
    with pytest.raises(ValueError, match="spec_rows_attention: scratch too small"):
        ops.spec_rows_attention(qkv, kc, vc, None, B, S, heads, i32(B), (torch.zeros((8,)), i32(B * heads)))
    with pytest.raises(ValueError, match="spec_rows_attention: out"):
        ops.spec_rows_attention(qkv, kc, vc, None, B, S, heads, i32(B), scratch, out=half(B * S, 128))

    k = 3
    hist, draft, dl, tok = i32(B, ctx), i32(B, k), i32(B), i32(B * (k + 1))
    for bad in (0, 8, -1):
        with pytest.raises(ValueError, match=r"spec_rows_draft: k must be in \[1, 7\]"):
            ops.spec_rows_draft(hist, i32(B), 1, bad, 2, draft, dl, tok)
        with pytest.raises(ValueError, match=r"spec_rows_accept: k must be in \[1, 7\]"):
            ops.spec_rows_accept(i32(B * (k + 1)), draft, dl, bad, hist, i32(B), i32(B, k + 2), tok, i32(B, 3))
        with pytest.raises(ValueError, match=r"spec_rows_counters: k must be in \[1, 7\]"):
            ops.spec_rows_counters(i32(B), bad, ctx, i32(B * (k + 1)))
    for bad in (0, 9):
        with pytest.raises(ValueError, match=r"spec_rows_draft: max_ngram must be in \[1, 8\]"):
            ops.spec_rows_draft(hist, i32(B), 1, k, bad, draft, dl, tok)
    with pytest.raises(ValueError, match="spec_rows_draft: hist"):
        ops.spec_rows_draft(i32(ctx), i32(1), 1, k, 2, draft, dl, tok)
    with pytest.raises(ValueError, match="spec_rows_draft: draft"):
        ops.spec_rows_draft(hist, i32(B), 1, k, 2, i32(B, k + 1), dl, tok)
    with pytest.raises(ValueError, match="spec_rows_draft: draft"):
        ops.spec_rows_draft(hist, i32(B), 1, k, 2, draft, i32(1), tok)
    with pytest.raises(ValueError, match="spec_rows_draft: pos must be int32"):
        ops.spec_rows_draft(hist, i32(1), 1, k, 2, draft, dl, tok)
    with pytest.raises(ValueError, match="spec_rows_draft: live must be uint8"):
        ops.spec_rows_draft(hist, i32(B), 1, k, 2, draft, dl, tok, live=i32(B))
    with pytest.raises(lib.ValleyHipError):
        ops.spec_rows_draft(hist, i32(B), 1, k, 2, draft, dl, tok, live=torch.ones((B,), dtype=torch.uint8))
    with pytest.raises(ValueError, match="spec_rows_accept: am"):
        ops.spec_rows_accept(i32(k + 1), draft, dl, k, hist, i32(B), i32(B, k + 2), tok, i32(B, 3))
    with pytest.raises(ValueError, match="spec_rows_accept: am"):
        ops.spec_rows_accept(i32(B * (k + 1)), draft, dl, k, hist, i32(B), i32(B, k + 1), tok, i32(B, 3))
    with pytest.raises(ValueError, match="spec_rows_accept: am"):
        ops.spec_rows_accept(i32(B * (k + 1)), draft, dl, k, hist, i32(B), i32(B, k + 2), tok, i32(3))
    with pytest.raises(ValueError, match="spec_rows_accept: live must be uint8"):
        ops.spec_rows_accept(i32(B * (k + 1)), draft, dl, k, hist, i32(B), i32(B, k + 2), tok, i32(B, 3), live=torch.ones((1,), dtype=torch.uint8))
    with pytest.raises(lib.ValleyHipError):
        ops.spec_rows_accept(i32(B * (k + 1)), draft, dl, k, hist, i32(B), i32(B, k + 2), tok, i32(B, 3))
    with pytest.raises(ValueError, match="spec_rows_counters: out must be int32"):
        ops.spec_rows_counters(i32(B), k, ctx, i32(k + 1))
    with pytest.raises(ValueError, match="spec_rows_counters: out must be int32"):
        ops.spec_rows_counters(i32(B), k, ctx, torch.zeros((B * (k + 1),), dtype=torch.int64))
    with pytest.raises(ValueError, match="spec_rows_counters: pos must be int32"):
        ops.spec_rows_counters(7, k, ctx, i32(B * (k + 1)))
    with pytest.raises(ValueError, match="spec_rows_counters: ctx_max"):
        ops.spec_rows_counters(i32(B), k, 0, i32(B * (k + 1)))
    with pytest.raises(lib.ValleyHipError):
        ops.spec_rows_counters(i32(B), k, ctx, i32(B * (k + 1)))
    part, arr = ops.spec_rows_scratch(2, 4, 3, "cpu")
    assert part.numel() == 2 * 3 * 4 * 4 * 132 and part.dtype == torch.float32 and arr.tolist() == [0] * 6 and arr.dtype == torch.int32


class Reached(Exception):
    pass


class StubModel:
    """The batcher's refusals come before the model is touched: touching it raises."""

    def __init__(self):
        self.reached = 0

    def get_model(self):
        self.reached += 1
        raise Reached("the model was touched")


def test_the_batcher_refuses_before_the_model_is_touched(monkeypatch):
    from valley_amd import decode, runtime
    from valley_amd.serving import ContinuousBatcher
    m = StubModel()
    for kw, msg in ((dict(slots=2, prompt_lookup_num_tokens=4), r"2 slots x \(k \+ 1 = 5\) = 10 rows"),
                    (dict(slots=4, prompt_lookup_num_tokens=2), r"4 slots x \(k \+ 1 = 3\) = 12 rows"),
                    (dict(slots=8, prompt_lookup_num_tokens=1), r"8 slots x \(k \+ 1 = 2\) = 16 rows"),
                    (dict(slots=2, prompt_lookup_num_tokens=3, processors=True), "processors"),
                    (dict(slots=2, prompt_lookup_num_tokens=3, logprobs=0), "logprobs"),
                    (dict(slots=2, max_matching_ngram_size=2), "max_matching_ngram_size needs prompt_lookup_num_tokens"),
                    (dict(slots=1, prompt_lookup_num_tokens=0), r"prompt_lookup_num_tokens must be an int in \[1, 7\]"),
                    (dict(slots=1, prompt_lookup_num_tokens=8), r"prompt_lookup_num_tokens must be an int in \[1, 7\]"),
                    (dict(slots=1, prompt_lookup_num_tokens=True), r"prompt_lookup_num_tokens must be an int in \[1, 7\]"),
                    (dict(slots=1, prompt_lookup_num_tokens=2.0), r"prompt_lookup_num_tokens must be an int in \[1, 7\]"),
                    (dict(slots=2, prompt_lookup_num_tokens=3, max_matching_ngram_size=0), r"max_matching_ngram_size must be an int in \[1, 8\]"),
                    (dict(slots=2, prompt_lookup_num_tokens=3, max_matching_ngram_size=9), r"max_matching_ngram_size must be an int in \[1, 8\]")):
        with pytest.raises(ValueError, match=msg):
            ContinuousBatcher(m, **kw)
    assert m.reached == 0
    # the engine refusals of spec.refuse_engine()
    monkeypatch.setattr(runtime, "PRECISION", "fp32")
    with pytest.raises(ValueError, match="16-bit engine"):
        ContinuousBatcher(m, slots=2, prompt_lookup_num_tokens=3)
    monkeypatch.undo()
    monkeypatch.setattr(decode, "PERSISTENT", True)
    with pytest.raises(ValueError, match="VALLEY_DECODE_PERSISTENT"):
        ContinuousBatcher(m, slots=2, prompt_lookup_num_tokens=3)
    monkeypatch.undo()
    monkeypatch.setattr(decode, "MERGE_IN", "oproj")
    with pytest.raises(ValueError, match="VALLEY_DECODE_MERGE"):
        ContinuousBatcher(m, slots=2, prompt_lookup_num_tokens=3)
    monkeypatch.undo()
    assert m.reached == 0
    # every admitted geometry gets as far as the model
    for slots, k in ((1, 7), (2, 3), (2, 1), (4, 1), (1, 1)):
        with pytest.raises(Reached):
            ContinuousBatcher(m, slots=slots, prompt_lookup_num_tokens=k, max_matching_ngram_size=8)
    with pytest.raises(Reached):                                 # ... and so does the batcher without the arguments
        ContinuousBatcher(m, slots=8)
    assert m.reached == 6


def test_the_session_refuses_too_many_rows():
    from valley_amd.spec import SpecRowsSession

    class Cache:
        batch, ctx_max, generation = 3, 64, 0

    class LL:
        heads, H = 2, 256

    with pytest.raises(ValueError, match=r"3 sequences x \(k \+ 1 = 3\) = 9 rows"):
        SpecRowsSession(LL(), Cache(), 2)
    for k in (0, 8):
        with pytest.raises(ValueError, match="prompt_lookup_num_tokens"):
            SpecRowsSession(LL(), Cache(), k)
    with pytest.raises(ValueError, match="max_matching_ngram_size"):
        SpecRowsSession(LL(), Cache(), 1, max_ngram=9)


# ---- the per-sequence rules against tests/spec_ref.py ----------------------------------------------------------------------------
def test_rows_reference_is_spec_ref_per_sequence():
    g = np.random.default_rng(7)
    for _ in range(300):
        B = int(g.integers(1, 5))
        ctx = 44
        cases = [SR.random_case(g) for _ in range(B)]
        k, n, eos = cases[0][1], cases[0][2], cases[0][3]
        hist = np.full((B, ctx), -1, dtype=np.int64)
        lengths = []
        for b, (h, _k, _n, _e) in enumerate(cases):
            hist[b, :len(h)] = h
            lengths.append(len(h))
        live = [int(x) for x in g.integers(0, 2, size=B)]
        before = g.integers(50, 60, size=(B, k))
        d, dl, tok = RR.draft_rows(hist, lengths, k, n, eos, live=live, draft=before, draft_len=[9] * B)
        for b in range(B):
            if live[b]:
                assert (d[b], dl[b], tok[b]) == SR.draft_outputs(hist[b], lengths[b], k, n, eos, ctx_max=ctx)
            else:
                assert d[b] == before[b].tolist() and dl[b] == 0 and tok[b] == [0] * (k + 1)
        # forced drafts: the caller's draft and length stay, the rows are built from the clamped length
        d2, dl2, tok2 = RR.draft_rows(hist, lengths, k, n, eos, lookup=False, draft=before, draft_len=[k] * B)
        assert d2 == before.tolist() and dl2 == [k] * B
        for b in range(B):
            last, cap = int(hist[b, lengths[b] - 1]), min(k, ctx - lengths[b])
            assert tok2[b] == [last] + before[b, :cap].tolist() + [last] * (k - cap)
        # acceptance
        am = g.integers(0, 3, size=B * (k + 1))
        drafted = g.integers(0, 3, size=(B, k))
        dls = g.integers(0, k + 2, size=B)
        pos = [length - 1 for length in lengths]
        stats = g.integers(0, 9, size=(B, 3))
        emit0 = np.full((B, k + 2), -3)
        tok0 = [-3] * (B * (k + 1))
        ns, h2, emit, tk, st, p2 = RR.accept_rows(am, drafted, dls, k, hist, pos, stats, live=live, emit=emit0, tok=tok0)
        for b in range(B):
            rest = [t for i, t in enumerate(tk[b * (k + 1):(b + 1) * (k + 1)]) if i]
            assert rest == [-3] * k
            if not live[b]:
                assert ns[b] is None and emit[b] == [0] + [-3] * (k + 1) and p2[b] == pos[b] and st[b] == stats[b].tolist()
                assert (h2[b] == hist[b]).all() and tk[b * (k + 1)] == -3
                continue
            want = SR.accept(am[b * (k + 1):(b + 1) * (k + 1)].tolist(), drafted[b].tolist(), int(dls[b]), k, hist[b], pos[b], stats[b].tolist())
            assert ns[b] == want[0] and (h2[b] == want[1]).all() and emit[b] == want[2] and tk[b * (k + 1)] == want[3]
            assert st[b] == want[4] and p2[b] == want[5]
    assert RR.counters([0, 5, 63, 64, -2], 2, 64) == [0, 1, 2, 5, 6, 7, 63, 64, 65, 63, 64, 65, 0, 1, 2]
    assert [RR.dead(62, j, 64) for j in range(4)] == [False, False, True, True] and RR.dead(99, 0, 64) is False and RR.dead(99, 1, 64)
