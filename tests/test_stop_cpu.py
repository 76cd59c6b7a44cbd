"""Stop strings without a GPU (include/valley_hip_stop.h): the scalar walk of tests/stop_ref.py pinned to transformers'
StopStringCriteria — over every sequence of one to four of eleven chosen tokens, and as a ``stopping_criteria`` callback of
``LlamaForCausalLM.generate`` on a tiny CPU Llama against ``generate(stop_strings=, tokenizer=)`` —, the table packer of
valley_amd.ops, every refusal with its message, and the companion contract of the sixth build table."""
import inspect
import itertools
import os
import re
import subprocess
import sys
from types import SimpleNamespace

import pytest
import torch

from tests import stop_ref as SR
from tests import stop_tokenizer as ST
from tests.test_companions_cpu import exported, header_macro, header_symbols
from tests.test_guide_cpu import message, prototypes
from valley_amd import build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["vly_stop_abi_version", "vly_stop_apply", "vly_stop_last_error"]
STRINGS = ["###", "stop"]
CHOSEN = ("#", "##", "###", "####", "a#", "#b", "x###y", "st", "op", "stop", "a")


def hf(tokenizer, strings):
    from transformers.generation.stopping_criteria import StopStringCriteria
    return StopStringCriteria(tokenizer, strings)


# ---- the build table, the exports, the lazy load ------------------------------------------------------------------------------
def test_the_sixth_table_is_the_stop_companion():
    assert [c.name for c in build.COMPANIONS_STOP] == ["stop"]
    assert build.EVERY_COMPANION == (*build.ALL_COMPANIONS, *build.COMPANIONS_GUIDE)       # as it was: the build walks both
    c = build.COMPANIONS_STOP[0]
    assert c.lib == build.LIB_STOP == os.path.join(build.LIBDIR, "libvalley_hip_stop.so")
    assert c.header == "valley_hip_stop.h" and c.sources == ("stop.hip",) and c.deps == ()
    assert c.lib not in {o.lib for o in build.EVERY_COMPANION}
    src = open(os.path.join(build.CSRC, c.sources[0])).read()
    assert set(re.findall(r'#include "([a-z0-9_]+\.(?:hpp|inc))"', src)) == set(build.COMPANION_SHARED)
    for fn in (build.needs_build, build.build):                    # a missing library makes the tree stale; it is compiled and audited
        assert "(*EVERY_COMPANION, *COMPANIONS_STOP)" in inspect.getsource(fn)
    assert inspect.getsource(build.build).count("in EVERY_COMPANION") == 0


def test_header_binding_and_library_agree():
    build.build(verbose=False)
    from valley_amd import lib_stop, ops
    assert header_symbols("valley_hip_stop.h") == NAMES == sorted(lib_stop.EXPORTS) == exported(build.LIB_STOP)
    assert prototypes("valley_hip_stop.h") == {k: (r, list(a)) for k, (r, a) in lib_stop.SIGS.items()}
    assert header_macro("valley_hip_stop.h", "VLY_STOP_ABI_VERSION") == lib_stop.ABI_VERSION == 1
    assert lib_stop.load().vly_stop_abi_version() == 1 and lib_stop.lib_path() == build.LIB_STOP
    for macro, a in (("MAX_STRINGS", ops.STOP_MAX_STRINGS), ("MAX_LEN", ops.STOP_MAX_LEN), ("MAX_WIDTH", ops.STOP_MAX_WIDTH),
                     ("HEADER", ops.STOP_HEADER), ("WATCH", ops.STOP_WATCH), ("PAD_AFTER", ops.STOP_PAD_AFTER)):
        assert header_macro("valley_hip_stop.h", f"VLY_STOP_{macro}") == a, macro
    assert (SR.WATCH, SR.PAD_AFTER) == (ops.STOP_WATCH, ops.STOP_PAD_AFTER) and not hasattr(lib_stop, "WATCH")    # one Python home
    # the other libraries are what they were, and none carries the new names
    assert len(exported(build.LIB)) == 52 and not [n for n in exported(build.LIB) if "vly_stop" in n]
    for c in build.EVERY_COMPANION:
        got = exported(c.lib)
        assert not [n for n in got if "vly_stop" in n], c.name
        assert got == header_symbols(c.header), c.name
        assert not [n for n in exported(build.LIB_STOP) if n.startswith(f"vly_{c.name}_")], c.name


def test_bad_arguments_to_the_entry_point_return_einval():
    """No launch is made for bad arguments: -22 and a message."""
    build.build(verbose=False)
    from valley_amd import lib_stop
    h = lib_stop.load()
    # apply(tok, hist, ld, pos, per_row, pos_add, rows, state, tables, table_words, eos, n_eos, R, stream)
    ok = [64, 64, 8, 64, 0, 0, 64, 64, 64, 16, None, 0, 2, None]

    def call(**kw):
        a = list(ok)
        for k, v in kw.items():
            a[int(k[1:])] = v
        return h.vly_stop_apply(*a)
    assert call(a0=None) == -22 and b"vly_stop_apply" in h.vly_stop_last_error()
    for bad in (dict(a1=None), dict(a6=None), dict(a7=None), dict(a8=None), dict(a2=0), dict(a9=15), dict(a12=0), dict(a12=65536),
                dict(a11=1), dict(a11=-1), dict(a10=64, a11=65), dict(a3=None, a4=1), dict(a0=66), dict(a3=62), dict(a10=6, a11=1)):
        assert call(**bad) == -22, bad
    assert b"R=2 ld=8 table_words=16 n_eos=1" in h.vly_stop_last_error()


def test_a_default_generation_and_batcher_never_import_the_binding():
    code = ("import sys, torch; import valley_amd.ops, valley_amd.valley_model, valley_amd.decode, valley_amd.serving, valley_amd.cli\n"
            "from valley_amd import generation\n"
            "ids = torch.zeros((1, 4), dtype=torch.long)\n"
            "a = (None, ids, None, None, 'sequence', 1, 1, None, False, None, False, 1.0, None, None, None, False, True, None)\n"
            "assert generation.stop_args(*a) is None\n"
            "assert generation.stop_args(*a[:3], object(), *a[4:]) is None\n"
            "assert valley_amd.cli.stop_kwargs() == {}\n"
            "assert 'valley_amd.lib_stop' not in sys.modules\n"
            "t = valley_amd.ops.stop_tables(None, [])\n"
            "assert 'valley_amd.lib_stop' not in sys.modules\n"
            "from valley_amd import lib_stop\n"
            "assert not lib_stop.loaded() and 'libvalley_hip_stop' not in open('/proc/self/maps').read(); print('ok')")
    p = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, cwd=ROOT)
    assert p.returncode == 0 and p.stdout.strip() == "ok", p.stderr[-2000:]


def test_generate_completion_batcher_session_and_cli_name_the_arguments():
    from valley_amd import cli, generation
    from valley_amd.decode import DecodeSession
    from valley_amd.serving import ContinuousBatcher
    from valley_amd.valley_model import ValleyLlamaForCausalLM
    sig = inspect.signature(ValleyLlamaForCausalLM.generate).parameters
    assert [sig[k].default for k in ("stop_strings", "tokenizer", "stop_begin", "sync_every")] == [None, None, "sequence", 1]
    assert generation.STOP_KEYS == ("stop_strings", "stop_begin", "sync_every")
    sig = inspect.signature(ContinuousBatcher.__init__).parameters
    assert sig["stop_strings"].default is None and sig["tokenizer"].default is None and "eos_token_id" in sig
    sig = inspect.signature(DecodeSession.__init__).parameters
    assert sig["stop"].default is None and sig["stop_eos"].default is None
    a = cli.parse_args([])
    assert a.stop_on_device is False and a.sync_every is None and cli.stop_kwargs(a.stop_on_device, a.sync_every) == {}
    a = cli.parse_args(["--stop-on-device", "--sync-every", "8"])
    assert cli.stop_kwargs(a.stop_on_device, a.sync_every) == {"stop_strings": ["###"], "sync_every": 8}
    assert cli.stop_kwargs(True) == {"stop_strings": ["###"]}
    assert message(lambda: cli.stop_kwargs(False, 4)) == "--sync-every needs --stop-on-device"
    with pytest.raises(SystemExit):                                # refused where the arguments are parsed, before a model is loaded
        cli.parse_args(["--sync-every", "4"])


def test_completion_passes_the_keys_and_drops_the_keyword_criterion(monkeypatch):
    from tests.fake_tokenizer import FakeTokenizer
    from tests.test_spec_cpu import stub_model
    from valley_amd.video import KeywordsStoppingCriteria
    m, seen = stub_model(), []

    def fake_generate(input_ids=None, **kw):
        seen.append(kw)
        return torch.cat([input_ids, torch.full((1, 2), 7, dtype=input_ids.dtype)], dim=1)

    tok = FakeTokenizer(300)
    monkeypatch.setattr(type(m), "device", property(lambda self: torch.device("cpu")), raising=False)
    monkeypatch.setattr(m, "build_inputs", lambda tokenizer, message: type("I", (), {"input_ids": [[1, 5, 6, 7]]})(), raising=False)
    monkeypatch.setattr(m, "generate", fake_generate, raising=False)
    monkeypatch.setattr(m, "process_response", lambda outs: outs, raising=False)
    video = torch.zeros((3, 2, 224, 224))
    m.completion(tok, video, [], {"max_new_tokens": 4})
    m.completion(tok, video, [], {"max_new_tokens": 4, "sync_every": 4, "stop_begin": "sequence", "tokenizer": 1})     # no stop_strings: as ever
    m.completion(tok, video, [], {"max_new_tokens": 4, "stop_strings": ["###"], "sync_every": 4, "stop_begin": "sequence"})
    for kw in seen[:2]:                                            # exactly today's arguments
        assert sorted(kw) == ["images", "max_new_tokens", "stopping_criteria"]
        assert len(kw["stopping_criteria"]) == 1 and isinstance(kw["stopping_criteria"][0], KeywordsStoppingCriteria)
    kw = seen[2]
    assert kw["stopping_criteria"] is None and kw["stop_strings"] == ["###"] and kw["sync_every"] == 4
    assert kw["tokenizer"] is tok and kw["stop_begin"] == "generated"


# ---- the reference equals transformers' criterion -----------------------------------------------------------------------------
@pytest.fixture(scope="module")
def small():
    tk = ST.small()
    assert len(tk.pieces) == 27 and set("abcdef") <= set(tk.pieces)
    crit = hf(tk, STRINGS)
    assert crit._stop_string_matching_mode is None
    return tk, crit, SR.tables_of(crit)


def test_reference_equals_hf_on_every_sequence_of_one_to_four_tokens(small):
    tk, crit, t = small
    ids = [tk.vocab[p] for p in CHOSEN]
    total = fired = 0
    for n in range(1, 5):
        seqs = list(itertools.product(ids, repeat=n))
        want = crit(torch.tensor(seqs), None).tolist()
        assert [SR.fires(t, list(s)) for s in seqs] == want, n
        total, fired = total + len(seqs), fired + sum(want)
    assert total == 11 + 11 ** 2 + 11 ** 3 + 11 ** 4 and 0 < fired < total


def test_reference_clamps_ids_as_hf_does(small):
    tk, crit, t = small
    h, T = tk.vocab["#"], len(t.emb)
    assert T == len(tk.pieces) + 1 and set(t.emb[-1]) == {-1}
    ids = [h, tk.vocab["##"], tk.vocab["a"], 999, -3, T - 1]
    for n in (2, 3, 4):
        for s in itertools.product(ids, repeat=n):
            as_hf = [i if i >= 0 else 10 ** 6 for i in s]          # HF clamps from above only: a negative id stands for a huge one
            assert SR.fires(t, list(s)) == bool(crit(torch.tensor([as_hf]), None)[0]), s
    assert SR.fires(t, [h, h, h]) and not SR.fires(t, [h, 999, h, h]) and not SR.fires(t, [h, -3, h, h]) and not SR.fires(t, [h, h, -1])


def test_begin_is_equivalent_to_cutting_the_sequence(small):
    tk, crit, t = small
    ids = [tk.vocab[p] for p in ("#", "##", "st", "op", "a")]
    differs = 0
    for s in itertools.product(ids, repeat=5):
        for b in (0, 2, 4, 5, 9):
            cut = list(s[b:]) if b < len(s) else list(s[-1:])      # the newest token is always tested
            assert SR.fires(t, list(s), b) == SR.fires(t, cut) == bool(crit(torch.tensor([cut]), None)[0])
            differs += SR.fires(t, list(s), b) != SR.fires(t, list(s))
    assert differs
    # the launch's reference: pad rule, EOS, unwatched rows, positions outside the history
    tok, state = [ids[0], 5, 99, ids[0], 99], [[0, -1], [1, 3], [0, -1], [0, -1], [0, -1]]
    SR.apply(t, tok, [[ids[0]] * 4] * 5, [3, 3, 3, 9, 2], [[1, 0, 0, 0], [3, 0, 44, 0], [0, 0, 0, 0], [1, 0, 0, 0], [1, 0, 0, 0]], state,
             eos=[99])
    assert tok == [ids[0], 44, 99, ids[0], 99] and state == [[1, 4], [1, 3], [0, -1], [0, -1], [1, 3]]


def test_the_generated_vocabulary():
    tk = ST.generated(306)
    assert len(tk.get_vocab()) == 306 and all(1 <= len(p) <= 3 and set(p) <= set(ST.ALPHABET) for p in tk.pieces)
    assert [tk.pieces[i] for i in range(7)] == list("abc#def") and tk(ST.ALPHABET)["input_ids"] == tk.encode("abc#def")
    crit = hf(tk, ["c#a", "#"])
    t = SR.tables_of(crit)
    g = torch.Generator().manual_seed(1)
    seqs = torch.randint(0, 306, (4000, 5), generator=g)
    want = crit(seqs, None).tolist()
    assert [SR.fires(t, s) for s in seqs.tolist()] == want and 0 < sum(want) < len(want)
    # what the criterion means (no matching mode): a stop string ends inside the newest token
    text = lambda s: "".join(tk.pieces[i] for i in s)              # noqa: E731
    assert want == [any(text(s)[:len(text(s)) - k].endswith(("c#a", "#")) for k in range(len(tk.pieces[s[-1]]))) for s in seqs.tolist()]


# ---- the packer ---------------------------------------------------------------------------------------------------------------
def test_the_packers_tables_are_hfs(small):
    from valley_amd import ops
    tk, crit, t = small
    p = ops.stop_tables(tk, STRINGS)
    T, W = crit.embedding_vec.shape
    assert p.buf.dtype == torch.int32 and p.buf.numel() == ops.STOP_HEADER + T * W and p.strings == ("###", "stop") and p.maximum_token_len == 4
    assert p.buf[:ops.STOP_HEADER].tolist() == [2, crit.max_valid_positions, crit.max_valid_end_lens, crit.maximum_token_len, T, W, 0, 0,
                                                3, 4, 0, 0, 0, 0, 0, 0]
    assert torch.equal(p.buf[ops.STOP_HEADER:].view(T, W), crit.embedding_vec.to(torch.int32))
    assert W == 2 * (crit.max_valid_positions + crit.max_valid_end_lens) + 1
    one = ops.stop_tables(tk, "###")
    assert one.strings == ("###",) and int(one.buf[0]) == 1
    empty = ops.stop_tables(None, [])
    assert empty.buf.tolist() == [0] * ops.STOP_HEADER and empty.strings == ()
    assert ops.stop_rows(3, begin=[0, 5, 7], pad=9, watch=[True, False, True], pad_after=[False, True, True]).tolist() == \
        [[1, 0, 9, 0], [2, 5, 9, 0], [3, 7, 9, 0]]
    assert ops.stop_rows(2).tolist() == [[1, 0, 0, 0]] * 2 and ops.stop_state(2).tolist() == [[0, -1]] * 2


def test_packer_refusals(small, monkeypatch):
    from valley_amd import ops
    tk = small[0]
    assert message(lambda: ops.stop_tables(tk, ["a"] * 9)) == "stop_strings: at most 8 stop strings, got 9"
    assert message(lambda: ops.stop_tables(tk, ["a", ""])) == "stop_strings: an empty stop string matches everywhere"
    assert message(lambda: ops.stop_tables(tk, ["a" * 65])) == "stop_strings: a stop string holds at most 64 characters, got 65"
    assert message(lambda: ops.stop_tables(tk, [3])) == "stop_strings must be a string or a list of strings, got [3]"
    assert "unable to identify tokens" in message(lambda: ops.stop_tables(tk, ["zzz"]))        # HF's own error passes through
    # a table row wider than the limit.  8 strings of 64 characters stay below 1024 ints (at most 63 positions and 64 end
    # overlaps each: 1017), so the limit itself is lowered to show the refusal
    wide = ST.ToyTokenizer(list("abcdefgh") + [c * n for c in "abcdefgh" for n in range(2, 6)])
    assert int(ops.stop_tables(wide, [c * 64 for c in "abcdefgh"]).buf[5]) == 8 * (63 + 5) + 1
    monkeypatch.setattr(ops, "STOP_MAX_WIDTH", 544)
    assert message(lambda: ops.stop_tables(wide, [c * 64 for c in "abcdefgh"])) == \
        "stop_strings: a table row of 545 ints (the strings' valid positions and end overlaps per token) exceeds 544"
    assert int(ops.stop_tables(tk, ["#" * 64]).buf[3]) == 64
    assert message(lambda: ops.stop_rows(0)) == "stop_rows: R must be an int >= 1, got 0"
    assert message(lambda: ops.stop_rows(2, begin=[1])) == "stop_rows: begin must be an int or 2 ints, got [1]"
    assert message(lambda: ops.stop_rows(2, begin=-1)) == "stop_rows: begin >= 0 expected, got [-1, -1]"
    assert message(lambda: ops.stop_state(True)) == "stop_state: R must be an int >= 1, got True"


def test_ops_wrapper_rejects_cpu_tensors(small):
    from valley_amd import lib, lib_stop, ops
    lib_stop.reset()
    t = ops.stop_tables(small[0], STRINGS)
    with pytest.raises(lib.ValleyHipError):
        ops.stop(torch.zeros(2, dtype=torch.int32), ops.stop_rows(2), ops.stop_state(2), t, torch.zeros((2, 8), dtype=torch.int32))
    assert not lib_stop.loaded()


# ---- refusals of generate, the session and the batcher: before any launch, before the library is loaded -----------------------
def test_generate_session_and_batcher_refusals(small):
    from valley_amd import generation, lib_stop, ops
    from valley_amd.decode import DecodeSession
    from valley_amd.serving import ContinuousBatcher
    from valley_amd.valley_model import ValleyLlamaForCausalLM
    lib_stop.reset()
    tk, launched = small[0], []

    class Model(SimpleNamespace):
        def forward(self, *a, **kw):
            launched.append("forward")
            raise AssertionError("a refused generate reached the forward")

    stub = Model(model=SimpleNamespace(precision="bf16"), device="cpu", config=SimpleNamespace())
    ids = torch.zeros((1, 6), dtype=torch.long)
    gen = lambda ids=ids, model=stub, **kw: ValleyLlamaForCausalLM.generate(model, ids, **kw)    # noqa: E731
    on = dict(stop_strings=["###"], tokenizer=tk)
    assert message(lambda: gen(stop_strings="###")) == generation.NO_TOKENIZER
    assert "we could not locate a tokenizer" in generation.NO_TOKENIZER
    assert message(lambda: gen(num_beams=2, **on)) == "stop_strings is not supported with num_beams > 1"
    assert message(lambda: gen(prompt_lookup_num_tokens=2, **on)) == "stop_strings is not supported with prompt_lookup_num_tokens"
    assert message(lambda: gen(guidance_scale=2.0, **on)) == "stop_strings is not supported with guidance_scale"
    assert message(lambda: gen(stop_begin="prompt", **on)) == 'stop_begin must be "sequence" or "generated", got \'prompt\''
    for bad in (0, -1, 2.0, True, None, "2"):
        assert message(lambda: gen(sync_every=bad, **on)) == f"sync_every must be an int >= 1, got {bad!r}"
    assert "sync_every > 1 is not supported with stopping_criteria" in message(lambda: gen(sync_every=2, stopping_criteria=[len], **on))
    assert "sync_every > 1 is not supported with do_sample without top_k / top_p / seed" in message(lambda: gen(sync_every=2, do_sample=True, **on))
    assert message(lambda: gen(sync_every=2, output_logprobs=True, return_dict_in_generate=True, **on)) == \
        "sync_every > 1 is not supported with output_logprobs"
    want = "sync_every > 1 needs the decode session: use_graph True (captured) or False (eager), not None, at most 8 rows, not the fp32 engine"
    assert message(lambda: gen(sync_every=2, use_graph=None, **on)) == want
    assert message(lambda: gen(ids=ids.expand(9, 6), sync_every=2, **on)) == want
    fp32 = Model(model=SimpleNamespace(precision="fp32"), device="cpu", config=SimpleNamespace())
    assert message(lambda: gen(model=fp32, sync_every=2, **on)) == want
    assert "sync_every > 1 needs stop_strings or an eos_token_id" in message(lambda: gen(sync_every=2))
    assert message(lambda: gen(sync_every=2, eos_token_id=2, num_beams=2)) == "sync_every > 1 is not supported with num_beams > 1"
    assert message(lambda: gen(sync_every=2, eos_token_id=2, guidance_scale=2.0)) == "sync_every > 1 is not supported with guidance_scale"
    assert message(lambda: gen(stop_strings=["a"] * 9, tokenizer=tk)) == "stop_strings: at most 8 stop strings, got 9"
    assert message(lambda: gen(stop_strings=[""], tokenizer=tk)) == "stop_strings: an empty stop string matches everywhere"
    assert "at most 64 characters" in message(lambda: gen(stop_strings=["#" * 65], tokenizer=tk))
    assert "unable to identify tokens" in message(lambda: gen(stop_strings=["zzz"], tokenizer=tk))
    # the batcher, in its constructor; the session, in its
    assert message(lambda: ContinuousBatcher(None, slots=2, stop_strings=["###"], tokenizer=tk, prompt_lookup_num_tokens=2)) == \
        "stop_strings does not combine with prompt_lookup_num_tokens or guidance=True"
    assert message(lambda: ContinuousBatcher(None, slots=2, stop_strings=["###"], tokenizer=tk, guidance=True)) == \
        "stop_strings does not combine with prompt_lookup_num_tokens or guidance=True"
    assert message(lambda: ContinuousBatcher(None, slots=2, stop_strings=["###"])) == generation.NO_TOKENIZER
    tables = ops.stop_tables(tk, ["###"])
    for kw in (dict(beams=(1, 2, 4, [2])), dict(guidance=True, per_row_positions=True), dict(beams=(1, 2, 4, [2]), guidance=True)):
        assert message(lambda: DecodeSession(Model(), Model(), stop=tables, **kw)) == "DecodeSession(stop=) takes no beams and no guidance"
    assert not launched and not lib_stop.loaded()


# ---- the reference as a callback against transformers' generate ---------------------------------------------------------------
@pytest.mark.parametrize("B,padded", [(1, False), (3, True)])
def test_reference_as_a_criterion_matches_hf_generate(B, padded):
    """``generate(stop_strings=, tokenizer=)`` of a tiny CPU Llama returns what the reference returns as a per-row
    ``stopping_criteria`` callback: strings chosen from the text that came out, so that every row stops inside its answer."""
    from transformers import StoppingCriteriaList
    from tests.test_logits_process_cpu import V, make_inputs, tiny_llama
    model, tk = tiny_llama(), ST.generated(V)
    ids, mask = make_inputs(B, 8, padded, seed=B)
    S, new = ids.shape[1], 12
    kw = dict(input_ids=ids, attention_mask=mask, do_sample=False, num_beams=1, max_new_tokens=new, eos_token_id=None, pad_token_id=0,
              repetition_penalty=1.3)
    plain = model.generate(**kw)
    assert plain.shape[1] == S + new
    strings = sorted({tk.pieces[int(plain[r, S + 1 + 2 * r])][-1] + tk.pieces[int(plain[r, S + 2 + 2 * r])] for r in range(B)})
    want = model.generate(stop_strings=strings, tokenizer=tk, **kw)
    got = model.generate(stopping_criteria=StoppingCriteriaList([SR.AsCriterion(hf(tk, strings))]), **kw)
    assert torch.equal(got, want) and S + 1 < want.shape[1] < S + new
    cut = model.generate(stopping_criteria=StoppingCriteriaList([SR.AsCriterion(hf(tk, strings), begin=S)]), **kw)
    assert cut.shape[1] >= want.shape[1]
