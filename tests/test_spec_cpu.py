"""CPU-side checks of prompt-lookup speculative decoding: the plain-Python draft rule (tests/spec_ref.py) equals transformers'
PromptLookupCandidateGenerator, the acceptance rule is stated on all 36 (draft length, first mismatch) pairs of k = 7, and
the library, the wrappers and generate() refuse what they do not cover before any launch."""
import numpy as np
import pytest
import torch

from tests import spec_ref as SR


def hf_draft(hist, k, n, eos):
    from transformers.generation.candidate_generator import PromptLookupCandidateGenerator
    gen = PromptLookupCandidateGenerator(eos_token_id=torch.tensor(eos) if eos else None, num_output_tokens=k, max_matching_ngram_size=n,
                                         max_length=10 ** 6)
    ids = torch.tensor([hist])
    cand, _ = gen.get_candidates(ids)
    return cand[0, len(hist):].tolist()


def test_reference_draft_is_transformers_prompt_lookup():
    g = np.random.default_rng(20240917)
    nonempty = 0
    for _ in range(2500):
        hist, k, n, eos = SR.random_case(g)
        want = hf_draft(hist, k, n, eos)
        got = SR.draft(hist, len(hist), k, n, eos)
        assert got == want, (hist, k, n, eos, got, want)
        # tokens behind `length` are not part of the sequence
        assert SR.draft(hist + hist[-n:] + [0, 1], len(hist), k, n, eos) == want
        nonempty += bool(want)
    assert nonempty > 1000                                   # the cases do draft


def test_reference_draft_rule_by_hand():
    #        0  1  2  3  4  5  6  7  8
    h = [5, 6, 7, 5, 6, 8, 9, 5, 6]
    assert SR.draft(h, 9, 3, 2) == [7, 5, 6]                 # the EARLIEST (5, 6), not the latest
    assert SR.draft(h, 9, 7, 2) == [7, 5, 6, 8, 9, 5, 6]     # cropped at the sequence's end
    assert SR.draft(h, 9, 3, 2, eos=[5]) == [7]              # in front of the first EOS
    assert SR.draft(h, 9, 3, 2, eos=[7]) == []               # an empty crop ends the search: no fall-back to n = 1
    assert SR.draft([1, 2, 3, 4, 2], 5, 2, 2) == [3, 4]      # no 2-gram match: n = 1
    assert SR.draft([1, 2, 3], 3, 2, 2) == [] and SR.draft([4], 1, 3, 2) == []
    assert SR.draft(h, 9, 3, 2, ctx_max=10) == [7] and SR.draft(h, 9, 3, 2, ctx_max=9) == []
    assert SR.draft_outputs(h, 9, 4, 2, eos=[6]) == ([7, 5, 6, 6], 2, [6, 7, 5, 6, 6])


def test_reference_accept_on_all_36_pairs():
    k = 7
    pairs = [(dl, m) for dl in range(k + 1) for m in range(dl + 1)]
    assert len(pairs) == 36
    am = [10, 11, 12, 13, 14, 15, 16, 17]
    for dl, m in pairs:                                      # m: the first draft that differs (m == dl: none does)
        d = [am[i] if i != m else 99 for i in range(k)]
        hist = np.full((64,), -7, dtype=np.int32)
        n, h, emit, tok0, stats, pos = SR.accept(am, d, dl, k, hist, 20, [3, 4, 5])
        assert n == m and pos == 21 + m and tok0 == am[m]
        assert emit == [m + 1] + am[:m + 1] + [-1] * (k - m) and len(emit) == k + 2
        assert h[21:22 + m].tolist() == am[:m + 1] and (np.delete(h, np.arange(21, 22 + m)) == -7).all()
        assert stats == [4, 4 + dl, 5 + m]
    # the end of the cache: what fits is written, the position still advances
    hist = np.full((24,), -7, dtype=np.int32)
    # (only the drafts whose rows fit the cache were fed to the step — the draft kernel's clamp — so only those are compared)
    n, h, emit, tok0, stats, pos = SR.accept(am, am[:7], 7, k, hist, 21, [0, 0, 0])
    assert n == 2 and h[22:].tolist() == am[:2] and (h[:22] == -7).all() and pos == 24 and emit[:4] == [3] + am[:3]
    assert stats == [1, 2, 2]
    n, h, emit, tok0, stats, pos = SR.accept(am, am[:7], 7, k, hist, 23, [0, 0, 0])
    assert n == 0 and (h == -7).all() and pos == 24 and emit[:2] == [1, am[0]] and stats == [1, 0, 0]
    n, *_ = SR.accept(am, am[:7], 99, k, hist, 0, [0, 0, 0])  # a draft length beyond k counts as k
    assert n == 7


def test_bad_arguments_are_refused_by_the_library():
    from valley_amd import lib_spec
    h = lib_spec.load()
    ok = 4096
    assert h.vly_spec_attention(None, ok, ok, None, 0, ok, 1, 2, 2, 0, None, 64, ok, ok, 0, None) == -22
    assert b"vly_spec_attention" in h.vly_spec_last_error()
    assert h.vly_spec_attention(ok, ok, ok, None, 0, ok, 1, 9, 2, 0, None, 64, ok, ok, 0, None) == -22       # S > 8
    assert h.vly_spec_attention(ok, ok, ok, None, 0, ok, 1, 0, 2, 0, None, 64, ok, ok, 0, None) == -22       # S < 1
    assert h.vly_spec_attention(ok, ok, ok, None, 0, ok, 1, 4, 2, 61, None, 64, ok, ok, 0, None) == -22      # past + S > ctx_max
    assert h.vly_spec_attention(ok, ok, ok, None, 0, ok, 1, 4, 2, 0, None, 64, ok, ok, 2, None) == -22       # dtype code
    assert h.vly_spec_attention(ok, ok, ok, None, 0, ok, 1, 4, 2, 0, None, 64, None, ok, 0, None) == -22     # no scratch
    assert h.vly_spec_attention(ok + 2, ok, ok, None, 0, ok, 1, 4, 2, 0, None, 64, ok, ok, 0, None) == -22   # alignment
    assert h.vly_spec_attention(ok, ok, ok, ok, 3, ok, 1, 4, 2, 0, None, 64, ok, ok, 0, None) == -22         # key_valid stride < kv_len
    assert h.vly_spec_attention(ok, ok, ok, ok, 63, ok, 1, 4, 2, 0, ok, 64, ok, ok, 0, None) == -22         # ... < ctx_max, device position
    assert h.vly_spec_draft(None, 64, ok, 1, 3, 2, None, 0, 0, 1, ok, ok, ok, None) == -22
    assert b"vly_spec_draft" in h.vly_spec_last_error()
    assert h.vly_spec_draft(ok, 64, ok, 1, 0, 2, None, 0, 0, 1, ok, ok, ok, None) == -22                      # k < 1
    assert h.vly_spec_draft(ok, 64, ok, 1, 8, 2, None, 0, 0, 1, ok, ok, ok, None) == -22                      # k > 7
    assert h.vly_spec_draft(ok, 64, ok, 1, 3, 9, None, 0, 0, 1, ok, ok, ok, None) == -22                      # max_ngram > 8
    assert h.vly_spec_draft(ok, 64, ok, 1, 3, 0, None, 0, 0, 1, ok, ok, ok, None) == -22
    assert h.vly_spec_draft(ok, 64, ok, 1, 3, 2, None, 2, 0, 1, ok, ok, ok, None) == -22                      # n_eos without eos
    assert h.vly_spec_draft(ok, 64, None, 0, 3, 2, None, 0, 0, 1, ok, ok, ok, None) == -22                    # no length at all
    assert h.vly_spec_accept(ok, ok, ok, 8, ok, 64, ok, ok, ok, ok, None) == -22
    assert h.vly_spec_accept(ok, ok, ok, 3, ok, 64, None, ok, ok, ok, None) == -22
    assert b"vly_spec_accept" in h.vly_spec_last_error()


def test_spec_ops_check_their_arguments_before_any_launch():
    from valley_amd import lib, ops
    from valley_amd.runtime import HALF
    i32 = lambda *s: torch.zeros(s, dtype=torch.int32)           # noqa: E731
    kc = torch.zeros((1, 2, 64, 128), dtype=HALF)
    qkv = torch.zeros((4, 3 * 256), dtype=HALF)
    scratch = (torch.zeros((2 * 4 * 4 * 132,)), i32(2))
    with pytest.raises(ValueError, match=r"S must be in \[1, 8\]"):
        ops.spec_attention(qkv, kc, kc, None, 1, 9, 2, 0, scratch)
    with pytest.raises(ValueError, match="exceeds the cache"):
        ops.spec_attention(qkv, kc, kc, None, 1, 4, 2, 61, scratch)
    with pytest.raises(ValueError, match="qkv"):
        ops.spec_attention(qkv[:3], kc, kc, None, 1, 4, 2, 0, scratch)
    with pytest.raises(ValueError, match="kcache"):
        ops.spec_attention(qkv, kc[:, :1], kc, None, 1, 4, 2, 0, scratch)
    with pytest.raises(ValueError, match="scratch too small"):
        ops.spec_attention(qkv, kc, kc, None, 1, 4, 2, 0, (scratch[0][:100], scratch[1]))
    with pytest.raises(ValueError, match="key_valid"):
        ops.spec_attention(qkv, kc, kc, torch.ones((1, 3), dtype=torch.uint8), 1, 4, 2, 0, scratch)
    with pytest.raises(ValueError, match="ctx_max columns"):
        ops.spec_attention(qkv, kc, kc, torch.ones((1, 10), dtype=torch.uint8), 1, 4, 2, 0, scratch, past_dev=i32(1))
    with pytest.raises(lib.ValleyHipError):                              # all shapes fine: no CPU compute path
        ops.spec_attention(qkv, kc, kc, None, 1, 4, 2, 0, scratch)
    with pytest.raises(ValueError, match=r"k must be in \[1, 7\]"):
        ops.spec_draft(i32(64), i32(1), 1, 8, 2, i32(8), i32(1), i32(9))
    with pytest.raises(ValueError, match=r"max_ngram must be in \[1, 8\]"):
        ops.spec_draft(i32(64), i32(1), 1, 3, 9, i32(3), i32(1), i32(4))
    with pytest.raises(ValueError, match="tok"):
        ops.spec_draft(i32(64), i32(1), 1, 3, 2, i32(3), i32(1), i32(3))
    with pytest.raises(ValueError, match="one sequence"):
        ops.spec_draft(i32(2, 64), i32(1), 1, 3, 2, i32(3), i32(1), i32(4))
    with pytest.raises(lib.ValleyHipError):
        ops.spec_draft(i32(64), i32(1), 1, 3, 2, i32(3), i32(1), i32(4))
    with pytest.raises(ValueError, match=r"k must be in \[1, 7\]"):
        ops.spec_accept(i32(1), i32(0), i32(1), 0, i32(64), i32(1), i32(2), i32(1), i32(3))
    with pytest.raises(ValueError, match="emit"):
        ops.spec_accept(i32(4), i32(3), i32(1), 3, i32(64), i32(1), i32(4), i32(4), i32(3))
    with pytest.raises(lib.ValleyHipError):
        ops.spec_accept(i32(4), i32(3), i32(1), 3, i32(64), i32(1), i32(5), i32(4), i32(3))


def stub_model():
    from valley_amd import valley_model as vm

    class Stub(vm.ValleyLlamaForCausalLM):
        def __init__(self):                                             # the checks come before the model is touched
            pass

    return Stub()


def test_generate_refuses_what_speculation_does_not_cover(monkeypatch):
    from valley_amd import decode, runtime, spec
    m = stub_model()
    ids = torch.zeros((1, 4), dtype=torch.long)
    for bad in (0, 8, -1, 2.0, True):
        with pytest.raises(ValueError, match="prompt_lookup_num_tokens must be"):
            m.generate(ids, prompt_lookup_num_tokens=bad)
    for bad in (0, 9, 1.5):
        with pytest.raises(ValueError, match="max_matching_ngram_size must be"):
            m.generate(ids, prompt_lookup_num_tokens=3, max_matching_ngram_size=bad)
    with pytest.raises(ValueError, match="needs prompt_lookup_num_tokens"):
        m.generate(ids, max_matching_ngram_size=2)
    with pytest.raises(ValueError, match="one prompt row"):
        m.generate(torch.zeros((2, 4), dtype=torch.long), prompt_lookup_num_tokens=3)
    with pytest.raises(ValueError, match="do_sample"):
        m.generate(ids, prompt_lookup_num_tokens=3, do_sample=True)
    with pytest.raises(ValueError, match="num_beams"):
        m.generate(ids, prompt_lookup_num_tokens=3, num_beams=2)
    for proc in ({"repetition_penalty": 1.2}, {"no_repeat_ngram_size": 2}, {"min_length": 5}, {"min_new_tokens": 2}):
        with pytest.raises(ValueError, match="logits processors"):
            m.generate(ids, prompt_lookup_num_tokens=3, **proc)
    with pytest.raises(ValueError, match="output_logprobs"):
        m.generate(ids, prompt_lookup_num_tokens=3, output_logprobs=True, return_dict_in_generate=True)
    with pytest.raises(ValueError, match="use_graph"):
        m.generate(ids, prompt_lookup_num_tokens=3, use_graph=None)
    monkeypatch.setattr(runtime, "PRECISION", "fp32")
    with pytest.raises(ValueError, match="fp32"):
        m.generate(ids, prompt_lookup_num_tokens=3)
    with pytest.raises(ValueError, match="fp32"):
        spec.refuse_engine()
    monkeypatch.setattr(runtime, "PRECISION", "bf16")
    monkeypatch.setattr(decode, "PERSISTENT", True)
    with pytest.raises(ValueError, match="VALLEY_DECODE_PERSISTENT"):
        spec.refuse_engine()
    monkeypatch.setattr(decode, "PERSISTENT", False)
    monkeypatch.setattr(decode, "MERGE_IN", "oproj")
    with pytest.raises(ValueError, match="VALLEY_DECODE_MERGE"):
        spec.refuse_engine()


def test_completion_and_cli_pass_the_arguments_through(monkeypatch):
    from tests.fake_tokenizer import FakeTokenizer
    from valley_amd import cli
    m = stub_model()
    seen = {}

    def fake_generate(input_ids=None, **kw):
        seen.update(kw)
        return torch.cat([input_ids, torch.full((1, 2), 7, dtype=input_ids.dtype)], dim=1)

    tok = FakeTokenizer(300)
    monkeypatch.setattr(type(m), "device", property(lambda self: torch.device("cpu")), raising=False)
    monkeypatch.setattr(m, "build_inputs", lambda tokenizer, message: type("I", (), {"input_ids": [[1, 5, 6, 7]]})(), raising=False)
    monkeypatch.setattr(m, "generate", fake_generate, raising=False)
    monkeypatch.setattr(m, "process_response", lambda outs: outs, raising=False)
    video = torch.zeros((3, 2, 224, 224))
    m.completion(tok, video, [], {"max_new_tokens": 4, "prompt_lookup_num_tokens": 3, "max_matching_ngram_size": 4, "unknown": 1})
    assert seen["prompt_lookup_num_tokens"] == 3 and seen["max_matching_ngram_size"] == 4 and seen["max_new_tokens"] == 4
    assert "unknown" not in seen
    assert cli.parse_args(["--prompt-lookup", "5"]).prompt_lookup == 5 and cli.parse_args([]).prompt_lookup is None
    calls = {}

    class M:
        def completion(self, tokenizer, video, turns, gen, device):
            calls.update(gen)
            return ["ok"]

    monkeypatch.setattr(cli, "load", lambda *a, **k: (M(), None))
    monkeypatch.setattr(cli, "_require_gpu", lambda: torch.device("cpu"))
    cli.main(cli.parse_args(["--prompt-lookup", "5"]))
    assert calls["prompt_lookup_num_tokens"] == 5
    calls.clear()
    cli.main(cli.parse_args([]))
    assert "prompt_lookup_num_tokens" not in calls
