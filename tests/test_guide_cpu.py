"""Classifier-free guidance without a GPU (include/valley_hip_guide.h): the reference of tests/guide_ref.py pinned to transformers'
UnbatchedClassifierFreeGuidanceLogitsProcessor, per call and end to end through ``LlamaForCausalLM.generate`` on a tiny CPU
Llama; the table packer of valley_amd.ops and every refusal with its message; the companion contract of the fifth build table."""
import inspect
import math
import os
import re
import subprocess
import sys
from ctypes import c_char_p, c_int, c_void_p
from types import SimpleNamespace

import pytest
import torch

from tests import guide_ref as GR
from tests import logits_ref
from tests.test_companions_cpu import exported, header_macro, header_symbols, header_text
from valley_amd import build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["vly_guide_abi_version", "vly_guide_apply", "vly_guide_follow", "vly_guide_last_error"]
EOS = 7
NEG_INF = float("-inf")


# ---- the build table, the exports, the lazy load ------------------------------------------------------------------------------
def test_the_fifth_table_is_the_guide_companion():
    assert [c.name for c in build.COMPANIONS_GUIDE] == ["guide"]
    assert build.EVERY_COMPANION == (*build.ALL_COMPANIONS, *build.COMPANIONS_GUIDE)
    assert len(build.COMPANIONS) == 7 and [c.name for c in build.COMPANIONS_CONSTRAIN] == ["constrain"]
    c = build.COMPANIONS_GUIDE[0]
    assert c.lib == build.LIB_GUIDE == os.path.join(build.LIBDIR, "libvalley_hip_guide.so")
    assert c.header == "valley_hip_guide.h" and c.sources == ("guide.hip",) and c.deps == ("beam_rows.inc",)
    assert c.lib not in {o.lib for o in build.ALL_COMPANIONS}
    src = open(os.path.join(build.CSRC, c.sources[0])).read()
    assert set(re.findall(r'#include "([a-z0-9_]+\.(?:hpp|inc))"', src)) == set(c.deps) | set(build.COMPANION_SHARED)
    # the build walks it: a missing library makes the tree stale
    assert "EVERY_COMPANION" in inspect.getsource(build.needs_build) and "EVERY_COMPANION" in inspect.getsource(build.build)


def prototypes(header):
    """{name: (return ctype, [argument ctypes])} of a header's vly_* prototypes: pointers are c_void_p (const char * returned:
    c_char_p), everything else here is int."""
    txt = re.sub(r"/\*.*?\*/", "", header_text(header), flags=re.S)
    out = {}
    for ret, name, args in re.findall(r"^((?:const\s+)?\w+\s*\*?)\s*(vly_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", txt, flags=re.M):
        kinds = []
        for a in [a.strip() for a in args.split(",") if a.strip() != "void"]:
            assert "*" in a or re.fullmatch(r"int \w+", a), a
            kinds.append(c_void_p if "*" in a else c_int)
        out[name] = (c_char_p if "char" in ret else c_int, kinds)
    return out


def test_header_binding_and_library_agree():
    build.build(verbose=False)
    from valley_amd import lib_guide, ops
    assert header_symbols("valley_hip_guide.h") == NAMES == sorted(lib_guide.EXPORTS) == exported(build.LIB_GUIDE)
    assert prototypes("valley_hip_guide.h") == {k: (r, list(a)) for k, (r, a) in lib_guide.SIGS.items()}
    assert header_macro("valley_hip_guide.h", "VLY_GUIDE_ABI_VERSION") == lib_guide.ABI_VERSION == 1
    assert lib_guide.load().vly_guide_abi_version() == 1 and lib_guide.lib_path() == build.LIB_GUIDE
    for macro, a, b, c in (("NEUTRAL", lib_guide.NEUTRAL, ops.GUIDE_NEUTRAL, GR.NEUTRAL), ("COND", lib_guide.COND, ops.GUIDE_COND, GR.COND),
                           ("UNCOND", lib_guide.UNCOND, ops.GUIDE_UNCOND, GR.UNCOND)):
        assert header_macro("valley_hip_guide.h", f"VLY_GUIDE_{macro}") == a == b == c, macro
    # the other libraries are what they were, and none carries the new names
    assert len(exported(build.LIB)) == 52 and not [n for n in exported(build.LIB) if "guide" in n]
    for c in build.ALL_COMPANIONS:
        got = exported(c.lib)
        assert not [n for n in got if "guide" in n], c.name
        assert got == header_symbols(c.header), c.name
        assert not [n for n in exported(build.LIB_GUIDE) if n.startswith(f"vly_{c.name}_")], c.name


def test_bad_arguments_to_the_entry_points_return_einval():
    """No launch is made for bad arguments: -22 and a message."""
    build.build(verbose=False)
    from valley_amd import lib_guide
    h = lib_guide.load()
    # apply(logits, ld, V, R, rows, stream); follow(tok, R, rows, stream)
    assert h.vly_guide_apply(None, 10, 10, 2, 64, None) == -22
    assert b"vly_guide_apply" in h.vly_guide_last_error()
    assert h.vly_guide_apply(64, 10, 10, 2, None, None) == -22
    assert h.vly_guide_apply(64, 10, 11, 2, 64, None) == -22                   # ld < V
    assert b"V=11 ld=10" in h.vly_guide_last_error()
    assert h.vly_guide_apply(64, 1 << 24, 1 << 24, 2, 64, None) == -22         # V too wide
    assert h.vly_guide_apply(64, 10, 10, 0, 64, None) == -22                   # no rows
    assert h.vly_guide_apply(64, 10, 10, 65536, 64, None) == -22
    assert h.vly_guide_apply(66, 10, 10, 2, 64, None) == -22                   # misaligned
    assert h.vly_guide_follow(None, 2, 64, None) == -22
    assert b"vly_guide_follow" in h.vly_guide_last_error()
    assert h.vly_guide_follow(64, 2, None, None) == -22 and h.vly_guide_follow(64, 0, 64, None) == -22
    assert h.vly_guide_follow(64, 2, 66, None) == -22


def test_a_default_generation_and_batcher_never_import_the_binding():
    """In a fresh process: the package, the model, the sessions and the batcher are imported, a generation's and a request's
    guidance arguments are checked at their defaults (and at a scale of 1), and the binding's module is not even imported (the GPU
    suite runs a real default ``generate`` under the same assertion)."""
    code = ("import sys, torch; import valley_amd.ops, valley_amd.valley_model, valley_amd.decode, valley_amd.serving, valley_amd.cli\n"
            "from valley_amd import generation\n"
            "ids = torch.zeros((1, 4), dtype=torch.long)\n"
            "assert generation.guidance_args(None, ids, None, None, None, None, 0.0, 1, None, None, False, True) is None\n"
            "assert generation.guidance_args(None, ids, 1.0, ids, None, None, 0.5, 4, 3, object(), True, None) is None\n"
            "assert generation.guidance_scalars(None, 0.0) is None and generation.guidance_scalars(1, 0.3) is None\n"
            "assert valley_amd.cli.guidance_kwargs(None) == {}\n"
            "assert 'valley_amd.lib_guide' not in sys.modules\n"
            "from valley_amd import lib_guide\n"
            "assert not lib_guide.loaded() and 'libvalley_hip_guide' not in open('/proc/self/maps').read(); print('ok')")
    p = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, cwd=ROOT)
    assert p.returncode == 0 and p.stdout.strip() == "ok", p.stderr[-2000:]


def test_generate_completion_batcher_and_cli_name_the_arguments():
    from valley_amd import cli, generation
    from valley_amd.serving import ContinuousBatcher
    from valley_amd.valley_model import ValleyLlamaForCausalLM
    keys = ("guidance_scale", "negative_prompt_ids", "negative_prompt_attention_mask", "negative_images", "guidance_plausibility")
    assert generation.GUIDANCE_KEYS == keys and "generation.GUIDANCE_KEYS" in inspect.getsource(ValleyLlamaForCausalLM.completion)
    for fn in (ValleyLlamaForCausalLM.generate, ContinuousBatcher.add):
        sig = inspect.signature(fn).parameters
        assert [sig[k].default for k in keys] == [None, None, None, None, 0.0]
    assert inspect.signature(ContinuousBatcher.__init__).parameters["guidance"].default is False
    from valley_amd.decode import DecodeSession
    assert inspect.signature(DecodeSession.__init__).parameters["guidance"].default is False
    a = cli.parse_args([])
    assert a.guidance_scale is None and a.negative_prompt is None
    a = cli.parse_args(["--guidance-scale", "1.5", "--negative-prompt", "a photo"])
    tok = lambda texts: SimpleNamespace(input_ids=[[1, 5, 6]])    # noqa: E731
    kw = cli.guidance_kwargs(tok, a.guidance_scale, a.negative_prompt)
    assert kw["guidance_scale"] == 1.5 and kw["negative_prompt_ids"].tolist() == [[1, 5, 6]] and len(kw) == 2
    assert cli.guidance_kwargs(tok, 2.0) == {"guidance_scale": 2.0}
    with pytest.raises(ValueError, match="--negative-prompt needs --guidance-scale"):
        cli.guidance_kwargs(tok, None, "x")


# ---- the table packer -----------------------------------------------------------------------------------------------------------
def message(fn, kind=ValueError):
    with pytest.raises(kind) as e:
        fn()
    return str(e.value)


def test_guidance_rows_packing():
    from valley_amd import ops
    bits = lambda v: torch.tensor(v, dtype=torch.float32).view(torch.int32).item()    # noqa: E731
    t = ops.guidance_rows(5, [(3, 0, 1.5, 0.1), (1, 4, -1, 0), (2, 2, 1.0, 0.0)][:2])
    assert t.dtype == torch.int32 and tuple(t.shape) == (5, 4)
    one, ninf = bits(1.0), bits(NEG_INF)
    assert t.tolist() == [[2, 3, one, ninf], [1, 4, bits(-1.0), ninf], [0, -1, one, ninf], [1, 0, bits(1.5), bits(math.log(0.1))],
                          [2, 1, one, ninf]]
    assert torch.equal(t, GR.table_of(5, [(3, 0, 1.5, 0.1), (1, 4, -1, 0)]))
    assert ops.guidance_rows(3).tolist() == [[0, -1, one, ninf]] * 3          # neutral rows
    assert ops.guidance_rows(2, [(0, 1, 2, 1)]).tolist() == [[1, 1, bits(2.0), bits(0.0)], [2, 0, one, ninf]]   # beta = 1: log 0


def test_guidance_rows_refusals():
    from valley_amd import ops
    g = ops.guidance_rows
    assert message(lambda: g(0)) == "guidance_rows: R must be an int >= 1, got 0"
    assert message(lambda: g(True)) == "guidance_rows: R must be an int >= 1, got True"
    assert message(lambda: g(2, [(0, 1, 1.5)])) == "guidance_rows: a pair is (cond_row, uncond_row, scale, plausibility), got (0, 1, 1.5)"
    assert message(lambda: g(2, [(0, 2, 1.5, 0)])) == "guidance_rows: uncond_row must be an int in [0, 2), got 2"
    assert message(lambda: g(2, [(-1, 1, 1.5, 0)])) == "guidance_rows: cond_row must be an int in [0, 2), got -1"
    assert message(lambda: g(2, [(0.0, 1, 1.5, 0)])) == "guidance_rows: cond_row must be an int in [0, 2), got 0.0"
    assert message(lambda: g(2, [(1, 1, 1.5, 0)])) == "guidance_rows: the rows of all pairs must be distinct, got (1, 1) behind []"
    assert message(lambda: g(4, [(0, 1, 1.5, 0), (2, 1, 1.5, 0)])) == \
        "guidance_rows: the rows of all pairs must be distinct, got (2, 1) behind [0, 1]"
    for bad in (float("nan"), float("inf"), None, "2", True):
        assert message(lambda: g(2, [(0, 1, bad, 0)])) == f"guidance_rows: the scale must be a finite float, got {bad!r}"
    for bad in (-0.1, 1.5, float("nan"), None, True):
        assert message(lambda: g(2, [(0, 1, 2.0, bad)])) == f"guidance_rows: the plausibility must lie in [0, 1], got {bad!r}"


def test_ops_wrappers_reject_cpu_tensors_and_shapes():
    from valley_amd import lib, lib_guide, ops
    lib_guide.reset()
    rows = ops.guidance_rows(2, [(0, 1, 1.5, 0)])
    with pytest.raises(lib.ValleyHipError):
        ops.guide(torch.zeros((2, 16)), rows)
    with pytest.raises(lib.ValleyHipError):
        ops.guide_follow(torch.zeros(2, dtype=torch.int32), rows)
    assert not lib_guide.loaded()


# ---- refusals of generate and the batcher: before any launch, before the library is loaded ---------------------------------------
def test_generate_and_batcher_refusals():
    from valley_amd import lib_guide
    from valley_amd.serving import ContinuousBatcher
    from valley_amd.valley_model import ValleyLlamaForCausalLM
    lib_guide.reset()
    launched = []

    class Model(SimpleNamespace):                             # anything a refused call touched would show here
        def forward(self, *a, **kw):
            launched.append("forward")
            raise AssertionError("a refused generate reached the forward")

    stub = Model(model=SimpleNamespace(precision="bf16"), device="cpu", config=SimpleNamespace())
    ids = torch.zeros((1, 6), dtype=torch.long)
    gen = lambda ids=ids, model=stub, **kw: ValleyLlamaForCausalLM.generate(model, ids, **kw)    # noqa: E731
    assert "at most 4 prompt rows, got input_ids (5, 6)" in message(lambda: gen(ids=ids.expand(5, 6), guidance_scale=2.0))
    assert message(lambda: gen(guidance_scale=2.0, num_beams=2)) == "guidance_scale is not supported with num_beams > 1"
    assert "not supported with prompt_lookup_num_tokens" in message(lambda: gen(guidance_scale=2.0, prompt_lookup_num_tokens=3))
    assert "not supported with prefix=" in message(lambda: gen(guidance_scale=2.0, prefix=object()))
    assert message(lambda: gen(guidance_scale=2.0, output_logprobs=True, return_dict_in_generate=True)) == \
        "guidance_scale is not supported with output_logprobs"
    assert "use_graph True (captured) or False (eager), not None" in message(lambda: gen(guidance_scale=2.0, use_graph=None))
    fp32 = Model(model=SimpleNamespace(precision="fp32"), device="cpu", config=SimpleNamespace())
    assert "not fp32" in message(lambda: gen(model=fp32, guidance_scale=2.0))
    for bad in (float("nan"), float("inf"), "2"):
        assert message(lambda: gen(guidance_scale=bad)) == f"guidance_scale must be a finite float, got {bad!r}"
    for bad in (-0.5, 1.01, float("nan")):
        assert message(lambda: gen(guidance_scale=2.0, guidance_plausibility=bad)) == f"guidance_plausibility must lie in [0, 1], got {bad!r}"
    assert message(lambda: gen(guidance_plausibility=0.3)) == "guidance_plausibility needs a guidance_scale"
    want = "negative_prompt_ids / negative_prompt_attention_mask / negative_images need a guidance_scale"
    for kw in (dict(negative_prompt_ids=ids), dict(negative_prompt_attention_mask=ids), dict(negative_images=ids)):
        assert message(lambda: gen(**kw)) == want
    assert "must be [1, S_neg] (one negative prompt per prompt row), got (2, 6)" in \
        message(lambda: gen(guidance_scale=2.0, negative_prompt_ids=ids.expand(2, 6)))
    assert "must have negative_prompt_ids' shape (1, 6), got (1, 5)" in \
        message(lambda: gen(guidance_scale=2.0, negative_prompt_ids=ids, negative_prompt_attention_mask=ids[:, :5]))
    assert message(lambda: gen(guidance_scale=2.0, negative_prompt_attention_mask=ids)) == "negative_prompt_attention_mask needs negative_prompt_ids"
    # the batcher: in the constructor, and in add() of a batcher built without guidance
    assert message(lambda: ContinuousBatcher(None, slots=2, guidance=True, prompt_lookup_num_tokens=2)) == \
        "guidance=True does not combine with prompt_lookup_num_tokens or logprobs"
    assert message(lambda: ContinuousBatcher(None, slots=2, guidance=True, logprobs=0)) == \
        "guidance=True does not combine with prompt_lookup_num_tokens or logprobs"
    plain = SimpleNamespace(guidance=False, sampling=False)
    add = lambda **kw: ContinuousBatcher.add(plain, ids, **kw)    # noqa: E731
    assert message(lambda: add(guidance_scale=2.0)) == "add(guidance_scale=) needs ContinuousBatcher(..., guidance=True)"
    assert message(lambda: add(negative_prompt_ids=ids)) == want
    assert message(lambda: add(guidance_scale=float("inf"))) == "guidance_scale must be a finite float, got inf"
    # a session: per-row positions only, no beams, no logprobs
    from valley_amd.decode import DecodeSession
    src = inspect.getsource(DecodeSession.__init__)
    assert "DecodeSession(guidance=True) needs per_row_positions=True" in src and "takes no beams and no logprobs" in src
    assert not launched and not lib_guide.loaded()


# ---- the reference equals transformers' processor ------------------------------------------------------------------------------
class FixedModel:
    """What UnbatchedClassifierFreeGuidanceLogitsProcessor calls: returns the same unconditional logits at every call."""

    def __init__(self, logits):
        self.logits, self.calls = logits, []

    def __call__(self, input_ids, attention_mask=None, use_cache=None, past_key_values=None):
        from transformers.modeling_outputs import CausalLMOutputWithPast
        self.calls.append((input_ids.clone(), attention_mask.clone()))
        return CausalLMOutputWithPast(logits=self.logits[:, None, :])


@pytest.mark.parametrize("scale", [1.5, 3.0, 0.5, -1.0, 0.0])
def test_reference_equals_transformers_per_call(scale):
    """Finite inputs, beta = 0.  transformers takes torch's log_softmax; with the same function the reference gives HF's bits, and
    its own log-softmax (the header's m + log sum exp) stays within a few ulp of torch's."""
    from transformers.generation.logits_process import UnbatchedClassifierFreeGuidanceLogitsProcessor
    g = torch.Generator().manual_seed(int(scale * 10) + 20)
    for V in (1, 7, 101, 1000):
        xc, xu = torch.randn((3, V), generator=g) * 4, torch.randn((3, V), generator=g) * 4
        ids = torch.randint(0, max(V, 2), (3, 5), generator=g)
        m = FixedModel(xu)
        want = UnbatchedClassifierFreeGuidanceLogitsProcessor(scale, m)(ids, xc.clone())
        assert torch.equal(m.calls[0][0], ids[:, -1:])        # HF's default negative prompt: the last prompt token
        table = GR.table_of(6, [(b, 3 + b, scale, 0.0) for b in range(3)])
        got = GR.apply(torch.cat([xc, xu]), table, lsm=lambda t: torch.log_softmax(t, -1))
        assert GR.same_bits(got[:3], want) and GR.same_bits(got[3:], xu)
        own = GR.apply(torch.cat([xc, xu]), table)
        bound = (abs(scale) + abs(scale - 1) + 1) * 1e-6 * max(1.0, float(want.abs().max()))
        assert float((own[:3] - want).abs().max()) <= bound
    assert UnbatchedClassifierFreeGuidanceLogitsProcessor(1, None)(ids, xc).equal(torch.log_softmax(xc, -1))   # 1 is off in HF: no model call


def test_reference_edges():
    x = torch.tensor([[2.0, 1.0, NEG_INF, float("nan"), 0.5, 2.0, -3.0],
                      [0.0, NEG_INF, 1.0, 2.0, float("nan"), 1.0, 0.0]])
    t = GR.table_of(2, [(0, 1, 3.0, 0.0)])
    lc, lu = GR.log_softmax_row(x[0]), GR.log_softmax_row(x[1])
    assert math.isclose(float(torch.exp(lc[~lc.isnan()]).sum()), 1.0, rel_tol=1e-6)      # NaN is left out of the sum
    out = GR.apply(x, t)
    assert GR.same_bits(out[1], x[1]) and not out[0].isnan().any()
    assert out[0, 2] == NEG_INF and out[0, 3] == NEG_INF      # x_c -inf / NaN
    assert out[0, 1] == lc[1] and out[0, 4] == lc[4]          # x_u -inf / NaN: no guidance for that column
    assert out[0, 0] == 3.0 * (lc[0] - lu[0]) + lu[0]
    # the cut-off: beta = 1 keeps the columns tied at the maximum, beta = 0.1 those within log(0.1) of it
    keep = lambda beta: torch.isfinite(GR.apply(x, GR.table_of(2, [(0, 1, 3.0, beta)]))[0]).nonzero().view(-1).tolist()    # noqa: E731
    assert keep(1.0) == [0, 5] and keep(0.1) == [0, 1, 4, 5] and keep(0.0) == [0, 1, 4, 5, 6]
    # a conditional row of -inf stays -inf; +inf never makes a NaN
    dead = GR.apply(torch.tensor([[NEG_INF] * 3, [0.0, 1.0, 2.0]]), t)
    assert dead[0].tolist() == [NEG_INF] * 3
    hot = GR.apply(torch.tensor([[float("inf"), 1.0, 2.0], [float("inf"), 1.0, 0.0]]), GR.table_of(2, [(0, 1, 0.0, 0.0)]))
    assert not hot.isnan().any() and hot[0, 0] == float("inf")
    # malformed partners: out of range, the row itself, a row that is not unconditional
    for bad in ([[1, 2, 0, 0], [2, 0, 0, 0]], [[1, -1, 0, 0], [2, 0, 0, 0]], [[1, 0, 0, 0], [2, 0, 0, 0]], [[1, 1, 0, 0], [0, 0, 0, 0]],
                [[1, 1, 0, 0], [1, 0, 0, 0]]):
        assert GR.same_bits(GR.apply(x, torch.tensor(bad, dtype=torch.int32)), x)
    tok = torch.tensor([5, 6, 7, 8], dtype=torch.int32)
    assert GR.follow(tok, GR.table_of(4, [(2, 0, 1.5, 0)])).tolist() == [7, 6, 7, 8]
    assert GR.follow(tok, torch.tensor([[2, 1, 0, 0], [0, 0, 0, 0], [2, 2, 0, 0], [2, 9, 0, 0]], dtype=torch.int32)).tolist() == [5, 6, 7, 8]


# ---- the reference loop against transformers' generate ------------------------------------------------------------------------
@pytest.fixture(scope="module")
def model():
    from tests.test_logits_process_cpu import tiny_llama
    return tiny_llama()


@pytest.mark.parametrize("scale,neg_len,procs", [(1.5, 0, {}), (3.0, 3, {}), (0.5, 12, {}), (-1.0, 5, {}),
                                                 (2.0, 4, dict(repetition_penalty=1.3, no_repeat_ngram_size=2))])
@pytest.mark.parametrize("B,padded", [(1, False), (2, True)])
def test_reference_loop_matches_hf_generate(model, scale, neg_len, procs, B, padded):
    """``guided_loop`` over two cached HF forwards returns what ``generate(guidance_scale=, negative_prompt_ids=)`` returns: the
    guidance in front of the other processors, both rows fed the chosen token, the default negative prompt (neg_len 0)."""
    from tests.test_logits_process_cpu import V, hf_stepper, make_inputs
    ids, mask = make_inputs(B, 8, padded, seed=B * 3 + neg_len)
    new = 8
    neg = None if not neg_len else torch.randint(8, V, (B, neg_len), generator=torch.Generator().manual_seed(neg_len))
    ref = model.generate(input_ids=ids, attention_mask=mask, do_sample=False, num_beams=1, max_new_tokens=new, eos_token_id=EOS,
                         pad_token_id=0, guidance_scale=scale, negative_prompt_ids=neg, **procs)
    plain = model.generate(input_ids=ids, attention_mask=mask, do_sample=False, num_beams=1, max_new_tokens=new, eos_token_id=EOS,
                           pad_token_id=0, **procs)
    cstep, _ = hf_stepper(model, ids, mask)
    nids = ids[:, -1:] if neg is None else neg
    ustep, _ = hf_stepper(model, nids, torch.ones_like(nids))
    back = logits_ref.hf_processors(procs.get("repetition_penalty"), procs.get("no_repeat_ngram_size"), prompt_len=ids.shape[1], eos=EOS)
    got, margins = GR.guided_loop(cstep, ustep, ids, new, scale, 0.0, back, eos=EOS, pad=0)
    assert torch.equal(got, ref), (got, ref)
    assert tuple(margins.shape) == (B, got.shape[1] - ids.shape[1]) and bool((margins >= 0).all())
    if abs(scale - 1) >= 1:                                   # a strong scale changes this model's output (a weak one may not)
        assert not torch.equal(ref[:, :plain.shape[1]], plain[:, :ref.shape[1]])
