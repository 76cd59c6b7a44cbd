"""GPU checks of conversation KV reuse (valley_amd/prefix.py, generate(prefix=)) on the golden model.

The conversation: turn 1 is the "decode2" fixture (283 tokens; its 8 greedy tokens are pinned by g5_decode2.npz), turn 2
appends the first 6 of them and 40 text tokens (329 tokens; tests/suffix_cases.py, its greedy tokens pinned on the CPU oracle
by tests/test_suffix_cpu.py), further turns append more text.

The "prefill" arm launches exactly what a forward over a filled cache launches, so everything through a session on that arm
is compared BIT FOR BIT with the same continuation made by hand: rows [0, P) of the session's cache copied into a fresh cache,
``model(input_ids=ids[:, P:], past_key_values=copy)``, then a DecodeSession (or, for the combinations, generate()'s own loop
over that hand-continued cache).  The "split" arm differs from it by the attention kernel's rounding only: within 2e-2, the
project's bound for "same kernels, different chunking" (tests/test_model_gpu.py).  Measured figures are printed before they
are asserted."""
import numpy as np
import pytest
import torch

from tests import golden_cfg as G
from tests import suffix_cases as SC
from tests.test_model_gpu import GOLD, build_golden_model

pytestmark = pytest.mark.gpu
TOL = 2e-2


@pytest.fixture(scope="module")
def golden():
    import os
    model = build_golden_model()
    T = G.GCFG["T"]
    img = torch.from_numpy(G.golden_pixels(T, "mixed")).view(1, T, 3, 224, 224).cuda()
    ids1 = torch.from_numpy(G.golden_ids("decode2")[0]).cuda()
    tokens1 = np.load(os.path.join(GOLD, "g5_decode2.npz"))["tokens"][0].tolist()
    ids2 = torch.tensor([SC.turn2_ids(ids1[0].tolist(), tokens1)], device=ids1.device)
    assert ids1.shape[1] == 283 and ids2.shape[1] == 329
    return model, img, ids1, ids2, tokens1


def session(model, arm, **kw):
    from valley_amd.prefix import PrefixSession
    return PrefixSession(model, attention=arm, **kw)


def book(s, seq):
    """The bookkeeping after every call: the session holds a prefix of the returned sequence, one cache row per token."""
    n = len(s.ids)
    assert s.ids == seq[0, :n].tolist() and s.cache.seq_len == n and n >= seq.shape[1] - 1, (n, seq.shape, s.cache.seq_len)


def after_turn1(golden, arm, **kw):
    model, img, ids1, _, tokens1 = golden
    s = session(model, arm, **kw)
    seq = model.generate(ids1, images=img, prefix=s, max_new_tokens=SC.TURN1_NEW)
    assert seq[0, 283:].tolist() == tokens1
    book(s, seq)
    return s


def copy_rows(model, s, P, ctx=640):
    """A fresh cache holding rows [0, P) of the session's."""
    c = model.get_model().llama.new_cache(1, ctx)
    for dst, src in ((c.k, s.cache.k), (c.v, s.cache.v)):
        for d, t in zip(dst, src):
            d[:, :, :P] = t[:, :, :P]
    c.seq_len = P
    return c


class HandPrefix:
    """generate()'s hooks over a hand-continued cache: the forward is the plain model call on ``ids[:, P:]``.  What the
    combinations are compared with — the same loops, none of PrefixSession's logic."""

    def __init__(self, model, cache, P):
        self.model, self.cache, self.P = model, cache, P

    def refuse(self, *a, **k):
        pass

    def forward(self, input_ids, images=None):
        assert self.cache.seq_len == self.P
        return self.model(input_ids=input_ids[:, self.P:], past_key_values=self.cache, use_cache=True)

    def reserve(self, n):
        self.cache.reserve(n)

    def settle(self, seq):
        pass


def by_hand(model, cache, ids, P, n_new):
    """-> (last logits of the suffix forward, n_new greedy tokens) from a cache that holds rows [0, P)."""
    from valley_amd.decode import DecodeSession
    o = model(input_ids=ids[:, P:], past_key_values=cache, use_cache=True)
    last = o.logits[:, -1, :].clone()
    sess = DecodeSession(model.get_model().llama, cache, use_graph=True)
    sess.begin(last.argmax(-1))
    toks = [int(sess.tok[0])]
    for _ in range(n_new - 1):
        toks.append(int(sess.step()[0]))
    sess.check()
    return last, toks


# ---- the three scenes of the issue ----------------------------------------------------------------------------------------------
def test_turn1_through_a_session_is_the_plain_call(golden):
    model, img, ids1, _, tokens1 = golden
    want = model.generate(ids1, images=img, max_new_tokens=SC.TURN1_NEW)
    for arm in ("split", "prefill"):
        s = session(model, arm)
        got = model.generate(ids1, images=img, prefix=s, max_new_tokens=SC.TURN1_NEW)
        assert torch.equal(got, want) and got[0, 283:].tolist() == tokens1
        assert s.stats == {"turns": 1, "reused": 0, "prefilled": 283, "tower_runs": 1}
        book(s, got)


def test_warm_then_ask(golden):
    from valley_amd import lib_suffix
    model, img, ids1, _, tokens1 = golden
    for arm in ("split", "prefill"):
        s = session(model, arm)
        s.prefill(ids1[:, :273], img)                        # the prompt through the visual block's end
        assert s.stats["tower_runs"] == 1 and len(s.ids) == 273 and s.cache.seq_len == 273
        got = model.generate(ids1, images=img, prefix=s, max_new_tokens=SC.TURN1_NEW)
        assert got[0, 283:].tolist() == tokens1
        assert s.stats == {"turns": 2, "reused": 273, "prefilled": 283, "tower_runs": 1}
        book(s, got)
    assert lib_suffix.loaded()


def test_turn2(golden):
    model, img, ids1, ids2, _ = golden
    n2 = len(SC.TURN2_TOKENS)
    plain = model.generate(ids2, images=img, max_new_tokens=n2)
    assert plain[0, 329:].tolist() == SC.TURN2_TOKENS
    full = model(input_ids=ids2, images=img).logits[:, -1].float().cpu()
    for arm in ("split", "prefill"):
        s = after_turn1(golden, arm)
        got = model.generate(ids2, images=img, prefix=s, max_new_tokens=n2)
        assert got[0, 329:].tolist() == SC.TURN2_TOKENS and torch.equal(got, plain)
        assert s.stats["reused"] == 289 and s.stats["prefilled"] == 283 + 40 and s.stats["tower_runs"] == 1
        book(s, got)
        s = after_turn1(golden, arm)
        err = float((s.prefill(ids2, img).float().cpu() - full).abs().max())
        print(f"turn 2, {arm}: last logits of the 40-token suffix vs the one-shot forward: max-abs {err:.3e}")
        assert err <= TOL


# ---- exact host logic -------------------------------------------------------------------------------------------------------------
def turn3(kind, seq2):
    """The third turn's prompt from the second's result (ids2 + 6 tokens) -> (ids, P)."""
    n = seq2.shape[1]
    if kind == "long":                                       # a 70-token suffix behind the cached n - 1 rows: S = 71 > 64
        tail = G._text("turn3.long", 70)
        return torch.cat([seq2, torch.tensor([tail], device=seq2.device)], 1), n - 1
    tail = G._text("turn3.other", 20)                        # diverges inside the previous answer, after 3 of its tokens
    while tail[0] == int(seq2[0, 329 + 3]):
        tail = tail[1:]
    return torch.cat([seq2[:, :329 + 3], torch.tensor([tail], device=seq2.device)], 1), 329 + 3


@pytest.mark.parametrize("scene", ["turn2", "long", "diverge"])
def test_session_equals_the_hand_continued_cache(golden, scene):
    model, img, ids1, ids2, _ = golden
    n_new = 6

    def prepared(arm):
        s = after_turn1(golden, arm)
        if scene == "turn2":
            return s, ids2, 289
        seq2 = model.generate(ids2, images=img, prefix=s, max_new_tokens=n_new)
        book(s, seq2)
        ids, P = turn3(scene, seq2)
        return s, ids, P

    s, ids, P = prepared("prefill")
    want_last, want_toks = by_hand(model, copy_rows(model, s, P), ids, P, n_new)
    reused = s.stats["reused"]
    last = s.prefill(ids, img)
    assert s.stats["reused"] - reused == P and s.cache.seq_len == ids.shape[1] == len(s.ids)
    assert torch.equal(last, want_last), float((last - want_last).abs().max())
    s, ids, P = prepared("prefill")
    got = model.generate(ids, images=img, prefix=s, max_new_tokens=n_new)
    assert got[0, ids.shape[1]:].tolist() == want_toks
    book(s, got)
    # the split arm: the same turns within the chunking bound (its earlier turns left rows of the split kernel's rounding)
    s, ids, P = prepared("split")
    last = s.prefill(ids, img)
    err = float((last - want_last).abs().max())
    print(f"{scene}: P = {P}, suffix {ids.shape[1] - P}; split arm vs hand-continued prefill arm: max-abs {err:.3e}")
    assert err <= TOL
    if ids.shape[1] - P > 64:                                # the fallback: bit for bit a hand continuation of THIS session's rows
        s, ids, P = prepared("split")
        want2, _ = by_hand(model, copy_rows(model, s, P), ids, P, 1)
        assert torch.equal(s.prefill(ids, img), want2)


# ---- combinations on turn 2 -------------------------------------------------------------------------------------------------------
COMBOS = {
    "seeded_sampling": dict(do_sample=True, temperature=1.0, top_k=50, seed=1234),
    "processors": dict(repetition_penalty=1.3, no_repeat_ngram_size=2),
    "logprobs": dict(output_logprobs=True, top_logprobs=3, return_dict_in_generate=True),
    "lookup_graph": dict(prompt_lookup_num_tokens=3, use_graph=True),
    "lookup_eager": dict(prompt_lookup_num_tokens=3, use_graph=False),
    "generic_forward": dict(use_graph=None),
    "eager": dict(use_graph=False),
}


def _combo(golden, model, kw, n_new=10):
    _, img, ids1, ids2, tokens1 = golden
    s = session(model, "prefill")
    seq1 = model.generate(ids1, images=img, prefix=s, max_new_tokens=SC.TURN1_NEW)
    book(s, seq1)
    hand = HandPrefix(model, copy_rows(model, s, 289), 289)
    want = model.generate(ids2, images=img, prefix=hand, max_new_tokens=n_new, **kw)
    got = model.generate(ids2, images=img, prefix=s, max_new_tokens=n_new, **kw)
    assert s.stats["reused"] == 289
    return s, got, want


@pytest.mark.parametrize("name", list(COMBOS))
def test_combinations_on_turn2(golden, name):
    model = golden[0]
    kw = COMBOS[name]
    s, got, want = _combo(golden, model, kw)
    if kw.get("return_dict_in_generate"):
        assert torch.equal(got.sequences, want.sequences)
        for f in ("token_logprobs", "top_tokens", "top_logprobs"):
            a, b = getattr(got, f), getattr(want, f)
            assert torch.equal(a.view(torch.int32), b.view(torch.int32)), f
        book(s, got.sequences)
    else:
        assert torch.equal(got, want), (got[0, 329:].tolist(), want[0, 329:].tolist())
        book(s, got)
    if name in ("generic_forward", "eager"):                 # greedy: the pinned tokens
        assert got[0, 329:329 + 6].tolist() == SC.TURN2_TOKENS


def test_turn2_on_the_int8_engine(golden):
    model = build_golden_model()
    model.quantize_decode_weights("int8")
    s, got, want = _combo(golden, model, {})
    assert torch.equal(got, want)
    book(s, got)
    plain = model.generate(golden[3], images=golden[1], max_new_tokens=10)
    print(f"int8 engine, turn 2: session {got[0, 329:].tolist()} plain {plain[0, 329:].tolist()}")


def test_speculative_call_stopped_by_eos_mid_step(golden):
    """A verify step may have stored rows behind the stop: the session keeps the rows of the returned sequence only."""
    model, img, ids1, ids2, _ = golden
    for arm in ("prefill", "split"):
        s = after_turn1(golden, arm)
        eos = SC.TURN2_TOKENS[3]
        out = model.generate(ids2, images=img, prefix=s, max_new_tokens=12, prompt_lookup_num_tokens=7, eos_token_id=eos,
                             return_dict_in_generate=True)
        seq = out.sequences
        assert seq[0, 329:].tolist() == SC.TURN2_TOKENS[:4], out.speculation
        book(s, seq)
        # ... and goes on from there: the next turn reuses every row it kept (332 or 333: the stop's own row only if a draft fed it)
        ids3 = torch.cat([seq, torch.tensor([G._text("turn3.eos", 12)], device=seq.device)], 1)
        kept, reused = len(s.ids), s.stats["reused"]
        assert kept in (332, 333)
        hand = HandPrefix(model, copy_rows(model, s, kept), kept)
        want = model.generate(ids3, images=img, prefix=hand, max_new_tokens=4)
        got = model.generate(ids3, images=img, prefix=s, max_new_tokens=4)
        assert s.stats["reused"] - reused == kept
        if arm == "prefill":
            assert torch.equal(got, want)
        book(s, got)


# ---- further cases ----------------------------------------------------------------------------------------------------------------
def test_changed_frames_or_a_placeholder_in_the_suffix_prefill_everything(golden):
    model, img, ids1, ids2, _ = golden
    s = after_turn1(golden, "split")
    img2 = img.clone()
    img2[0, 0, 0, :8, :8] += 1.0
    want = model.generate(ids2, images=img2, max_new_tokens=6)
    got = model.generate(ids2, images=img2, prefix=s, max_new_tokens=6)
    assert torch.equal(got, want) and s.stats["tower_runs"] == 2 and s.stats["reused"] == 0
    book(s, got)
    # equal contents in another tensor: reused
    got = model.generate(ids2, images=img2.clone(), prefix=s, max_new_tokens=6)
    assert torch.equal(got, want) and s.stats["tower_runs"] == 2 and s.stats["reused"] == 328
    # the same tensor object, written in place since: everything again
    img2[0, 1, 0, :8, :8] -= 1.0
    want = model.generate(ids2, images=img2, max_new_tokens=6)
    got = model.generate(ids2, images=img2, prefix=s, max_new_tokens=6)
    assert torch.equal(got, want) and s.stats["tower_runs"] == 3
    # a second visual block behind the common prefix: a full prefill with the tower
    sp = G.special()
    s = after_turn1(golden, "split")
    moved = torch.cat([ids1[:, :5], torch.tensor([G._text("moved", 3)], device=ids1.device), ids1[:, 5:]], 1)   # the block moves: it lies in the suffix
    assert sp["im_patch_token"] in moved[0, 5:].tolist()
    want = model.generate(moved, images=img, max_new_tokens=4)
    got = model.generate(moved, images=img, prefix=s, max_new_tokens=4)
    assert torch.equal(got, want) and s.stats["tower_runs"] == 2 and s.stats["reused"] == 0
    book(s, got)
    s.reset()
    assert s.ids == [] and s.cache.seq_len == 0 and s.frames is None


def test_a_session_that_outgrows_its_cache(golden):
    model, img, ids1, _, tokens1 = golden
    want = model.generate(ids1, images=img, max_new_tokens=40)
    s = session(model, "split", initial_ctx=300)
    s.prefill(ids1[:, :273], img)
    assert s.cache.ctx_max == 300 and s.cache.generation == 0
    got = model.generate(ids1, images=img, prefix=s, max_new_tokens=40)
    assert s.cache.generation >= 1 and s.cache.ctx_max >= 323
    assert torch.equal(got, want) and got[0, 283:291].tolist() == tokens1
    book(s, got)


def test_refusals_come_before_any_launch(golden):
    from valley_amd import ops
    from valley_amd.prefix import PrefixSession
    model, img, ids1, _, _ = golden
    s = session(model, "split")
    launches = []                                            # (receives every MFMA GEMM launch: the first thing any forward does)
    ops.set_recorder(launches)
    try:
        two = torch.cat([ids1, ids1], 0)
        for kw in (dict(input_ids=two), dict(input_ids=ids1, num_beams=2),
                   dict(input_ids=ids1, attention_mask=torch.cat([torch.zeros((1, 3)), torch.ones((1, 280))], 1).long())):
            with pytest.raises(ValueError):
                model.generate(images=img, prefix=s, max_new_tokens=2, **kw)
        with pytest.raises(ValueError):
            s.prefill(two, img)
        with pytest.raises(ValueError):
            s.prefill(ids1, img, attention_mask=torch.zeros((1, 283)).long())
        with pytest.raises(ValueError):
            PrefixSession(model, attention="fast")
        other = session(build_golden_model(), "split")
        with pytest.raises(ValueError):
            model.generate(ids1, images=img, prefix=other, max_new_tokens=2)
    finally:
        ops.set_recorder(None)
    assert not launches and s.cache is None and s.stats["turns"] == 0
    # a mask of ones is no padding
    got = model.generate(ids1, images=img, prefix=s, max_new_tokens=2, attention_mask=torch.ones((1, 283)).long().cuda())
    book(s, got)


def test_fp32_engine_is_refused():
    import subprocess
    import sys
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = ("import sys; sys.path.insert(0, %r)\n"
            "from tests.test_model_gpu import build_golden_model\n"
            "from valley_amd.prefix import PrefixSession\n"
            "m = build_golden_model()\n"
            "assert m.get_model().precision == 'fp32'\n"
            "try:\n    PrefixSession(m)\nexcept ValueError as e:\n    print('refused')\n" % root)
    env = dict(os.environ, VALLEY_PRECISION="fp32")
    p = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env, timeout=300)
    assert p.returncode == 0 and p.stdout.strip().endswith("refused"), p.stdout[-1000:] + p.stderr[-3000:]


def test_conv_inference_reuse_kv_prints_the_same_answers(monkeypatch):
    """The interactive loop scripted through ``read_line`` / ``emit`` with the fake tokenizer: two turns with --reuse-kv on
    the "prefill" arm print what they print without it; the second turn reuses the first one's prompt, visual block included,
    and the tower runs once.  (The fake tokenizer re-encodes an answer's text to other ids, so the common prefix ends at the
    first turn's prompt; every fifth id decodes to the separator, so that answers end.)"""
    import re
    from types import SimpleNamespace

    import transformers

    from tests.fake_tokenizer import SPECIALS, FakeTokenizer
    from valley_amd import cli, prefix, video
    model = build_golden_model()                             # its own: the loop binds the tokenizer's ids onto the tower's config
    model.config.mm_use_im_start_end = True
    T = G.GCFG["T"]
    clip = torch.from_numpy(G.golden_pixels(T, "mixed")).view(T, 3, 224, 224).permute(1, 0, 2, 3).contiguous()      # load_video's layout

    class Tok(FakeTokenizer):
        def batch_decode(self, ids, skip_special_tokens=True):
            return [" ".join("###" if int(i) % 5 == 0 else f"w{int(i)}" for i in row
                             if not (skip_special_tokens and int(i) >= self.vocab_text)) for row in ids]

    def tokenizer(*a, **k):
        t = Tok(G.GCFG["vocab_text"])
        t.add_tokens(SPECIALS, special_tokens=True)
        return t

    made = []

    class Recorded(prefix.PrefixSession):
        def __init__(self, *a, **k):
            super().__init__(*a, **k)
            made.append(self)

    monkeypatch.setattr(transformers, "LlamaTokenizer", SimpleNamespace(from_pretrained=tokenizer), raising=False)
    monkeypatch.setattr(cli, "ValleyLlamaForCausalLM", SimpleNamespace(from_pretrained=lambda *a, **k: model))
    monkeypatch.setattr(video, "load_video", lambda path: clip)
    monkeypatch.setattr(prefix, "PrefixSession", Recorded)
    monkeypatch.setenv("VALLEY_SUFFIX_ATTN", "prefill")

    def run(flags):
        lines = iter(["", "what happens in the video", "and what happens after that", "quit"])
        out = []
        args = cli.conv_parse_args(["--model-name", "golden", "--video_file", "clip.mp4", "--seed", "7"] + flags)
        cli.conv_inference(args, read_line=lambda prompt="": next(lines), emit=out.append)
        return out

    plain = run([])
    assert not made and len(plain) == 2 and all(re.fullmatch(r"Assistant:( w\d+)*\n", a) for a in plain), plain     # (answers, not errors)
    assert any("w" in a for a in plain)
    reuse = run(["--reuse-kv"])
    print(f"conv_inference: {plain}; session {made[0].stats if made else None}")
    assert reuse == plain
    assert len(made) == 1 and made[0].attention == "prefill"
    s = made[0].stats
    assert s["turns"] == 2 and s["tower_runs"] == 1 and s["reused"] >= 273


def test_split_arm_over_a_context_of_several_splits(golden):
    """The golden conversation stays below 512 keys, where the split kernel is one workgroup per head and bit for bit the prefill
    kernel.  Here the context is 583 tokens and the turn 20: two splits and their merge inside the model, against the
    hand-continued prefill arm."""
    model, img, ids1, _, _ = golden
    ctx = torch.cat([ids1, torch.tensor([G._text("long.ctx", 300)], device=ids1.device)], 1)
    ids = torch.cat([ctx, torch.tensor([G._text("long.turn", 20)], device=ids1.device)], 1)
    P = ctx.shape[1]
    s = session(model, "prefill")
    s.prefill(ctx, img)
    want, _ = by_hand(model, copy_rows(model, s, P, ctx=1024), ids, P, 1)
    assert torch.equal(s.prefill(ids, img), want) and s.stats["reused"] == P == 583
    s = session(model, "split")
    s.prefill(ctx, img)
    last = s.prefill(ids, img)
    err = float((last - want).abs().max())
    print(f"583 + 20 tokens: split arm (two splits) vs hand-continued prefill arm: max-abs {err:.3e}")
    assert 0.0 < err <= TOL and s.stats == {"turns": 2, "reused": 583, "prefilled": 603, "tower_runs": 1}
