"""GPU checks of prompt-lookup speculative decoding (include/valley_hip_spec.h, valley_amd/spec.py, generate()):

* vly_spec_attention through the three exact checks of tests/attention_oracle.py, its position invariance bit for bit, and
  its agreement with vly_rope_kv + vly_llama_attention within the bound tests/test_kernels_gpu.py holds the split decode
  kernel to (max |d| <= 2.56 EPS, relative error < 0.512 EPS);
* vly_spec_draft and vly_spec_accept against tests/spec_ref.py, exactly;
* SpecDecodeSession with forced drafts and generate(prompt_lookup_num_tokens=k) against plain greedy decoding, token for token.

Measured figures are printed before they are asserted."""
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import attention_oracle as AO
from tests import golden_cfg as G
from tests import spec_ref as SR
from valley_amd.runtime import HALF

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = torch.finfo(HALF).eps
DEV = "cuda:0"


# ---- vly_spec_attention -----------------------------------------------------------------------------------------------------
def C(B, S, pasts, heads, ctx_max, **kw):
    return AO.Case(f"spec-B{B}-S{S}-past{pasts[0]}-h{heads}-ctx{ctx_max}", B, S, pasts, heads, ctx_max, **kw)


ATTN_CASES = [C(1, 2, [0], 2, 64), C(1, 1, [336], 2, 600), C(1, 4, [61], 2, 128), C(1, 8, [249], 2, 320), C(1, 8, [255], 2, 320),
              C(1, 8, [256], 2, 320), C(1, 5, [1020], 2, 1100), C(2, 3, [700, 700], 2, 1024, pads=[300, 0], holes=True, full_valid=True),
              C(1, 8, [592], 2, 600), C(1, 8, [2040], 40, 2048)]


class SpecRun:
    """``run(inp)`` of the oracle's checks: packs inp.q into a q|k|v buffer (the k and v thirds hold data the kernel must not
    read), launches, and checks after EVERY launch that the caches are bit-unchanged and the tickets are back at zero.  The
    position goes in through the device (every other launch through the host argument) where key_valid spans the cache."""

    def __init__(self):
        self.launches = 0
        self.scratch = {}

    def __call__(self, inp, S=None, past=None, q=None):
        from valley_amd import ops
        case = inp.case
        B, heads = case.B, case.heads
        S = case.S if S is None else S
        past = case.past if past is None else past
        q = inp.q if q is None else q
        Hq = heads * 128
        qkv = torch.full((B * S, 3 * Hq), 3.0, dtype=HALF, device=DEV)
        qkv[:, :Hq] = q.to(DEV).reshape(B * S, Hq)
        k0, v0 = inp.k.to(DEV).contiguous(), inp.v.to(DEV).contiguous()
        k, v = k0.clone(), v0.clone()
        valid = None if inp.valid is None else inp.valid.to(DEV)
        key = (B, S, heads)
        if key not in self.scratch:
            self.scratch[key] = ops.spec_scratch(B, S, heads, DEV)
        scratch = self.scratch[key]
        on_device = (valid is None or valid.shape[1] >= case.ctx_max) and self.launches % 2 == 0
        self.launches += 1
        if on_device:                                        # the host argument is then ignored: a wrong one must not matter
            out = ops.spec_attention(qkv, k, v, valid, B, S, heads, 0, scratch, past_dev=torch.tensor([past], dtype=torch.int32, device=DEV))
        else:
            out = ops.spec_attention(qkv, k, v, valid, B, S, heads, past, scratch)
        assert torch.equal(AO.bits(k), AO.bits(k0)) and torch.equal(AO.bits(v), AO.bits(v0)), "the caches are read-only"
        assert int(scratch[1].abs().sum()) == 0, "ticket counters not back at zero"
        return out.view(B, S, heads, 128)


def attention_checks(case):
    run = SpecRun()
    AO.check_pointer(case, run, HALF, DEV)
    AO.check_count(case, run, HALF, DEV)
    AO.check_invisible(case, run, HALF, DEV)
    inp = AO.build_dense(case, HALF, DEV)
    a, b = run(inp), run(inp)                                # (one through the device-side position, one through the host's)
    assert torch.equal(AO.bits(a), AO.bits(b)), "two launches differ"
    return run.launches


@pytest.mark.parametrize("case", ATTN_CASES, ids=lambda c: c.name)
def test_spec_attention_exact(case):
    n = attention_checks(case)
    print(f"{case.name}: {n} launches")
    assert AO.pointer_rounds(case) <= 17


def test_spec_attention_cases_cover_what_they_claim():
    assert max(AO.pointer_rounds(c) for c in ATTN_CASES) == 17
    assert {i for c in ATTN_CASES for i in range(c.S)} == set(range(8))
    spans = [(c.past, c.past + c.S - 1) for c in ATTN_CASES]
    assert any(lo // 64 != hi // 64 for lo, hi in spans) and any(lo // 256 != hi // 256 for lo, hi in spans)
    assert any(hi // 64 >= 8 for lo, hi in spans)            # a second round for every split
    assert any(c.past + c.S == c.ctx_max for c in ATTN_CASES) and any(c.heads == 40 for c in ATTN_CASES)


@pytest.mark.parametrize("past", [60, 250])
def test_spec_attention_position_invariance(past):
    """The row of the query at absolute position P: the same bits from S = 8 (index i), S = 1 (index 0) and S = 3 (index 1)."""
    case = C(1, 8, [past], 2, 320)
    inp = AO.build_dense(case, HALF, DEV)
    run = SpecRun()
    full = run(inp)
    for i in range(8):
        one = run(inp, S=1, past=past + i, q=inp.q[:, i:i + 1])
        assert torch.equal(AO.bits(one[0, 0]), AO.bits(full[0, i])), (past, i, "S = 1")
        three = run(inp, S=3, past=past + i - 1, q=inp.q[:, [(i - 1) % 8, i, (i + 1) % 8]])
        assert torch.equal(AO.bits(three[0, 1]), AO.bits(full[0, i])), (past, i, "S = 3")


def relerr(got, ref):
    got, ref = got.float().cpu(), ref.float().cpu()
    return float((got - ref).norm() / (ref.norm() + 1e-30))


def maxabs(got, ref):
    return float((got.float().cpu() - ref.float().cpu()).abs().max())


@pytest.mark.parametrize("past", [60, 250])
def test_spec_attention_agrees_with_rope_kv_and_llama_attention(past):
    from valley_amd import ops
    case = C(1, 8, [past], 2, 320)
    inp = AO.build_dense(case, HALF, DEV)
    Hq = 256
    g = torch.Generator().manual_seed(past)
    qkv = torch.randn((8, 3 * Hq), generator=g).to(HALF).to(DEV)
    qkv[:, :Hq] = inp.q.reshape(8, Hq)
    cos, sin = (t.to(DEV) for t in AO.rope_tables(320))
    k, v = inp.k.clone(), inp.v.clone()
    pos = torch.tensor([past], dtype=torch.int32, device=DEV)
    ops.rope_kv(qkv, k, v, cos, sin, 1, 8, 2, 0, past_dev=pos)
    want = ops.llama_attention(qkv, k, v, None, 1, 8, 2, 0, past_dev=pos)
    got = ops.spec_attention(qkv, k, v, None, 1, 8, 2, 0, ops.spec_scratch(1, 8, 2, DEV), past_dev=pos)
    print(f"past {past}: max |d| = {maxabs(got, want) / EPS:.3f} EPS, relative error = {relerr(got, want) / EPS:.4f} EPS")
    assert maxabs(got, want) <= 2.56 * EPS and relerr(got, want) < 0.512 * EPS


# ---- vly_spec_draft ---------------------------------------------------------------------------------------------------------
CTX = 4200
LENGTHS = [1, 2, 3, 255, 256, 257, 1500, 4097, CTX]


def run_draft(hist_dev, length, k, n, eos, lookup=True, draft=None, draft_len=None, vocab=0):
    from valley_amd import ops
    d = torch.full((k,), -5, dtype=torch.int32, device=DEV) if draft is None else torch.tensor(draft, dtype=torch.int32, device=DEV)
    dl = torch.full((1,), -5, dtype=torch.int32, device=DEV) if draft_len is None else torch.tensor([draft_len], dtype=torch.int32, device=DEV)
    tok = torch.full((k + 1,), -5, dtype=torch.int32, device=DEV)
    e = torch.tensor(eos, dtype=torch.int32, device=DEV) if eos else None
    # the length arrives half through the device word, half through the host's addend
    ops.spec_draft(hist_dev, torch.tensor([length - length // 2], dtype=torch.int32, device=DEV), length // 2, k, n, d, dl, tok, eos=e,
                   vocab=vocab, lookup=lookup)
    return d.tolist(), int(dl), tok.tolist()


def draft_history(length, seed):
    """A small-vocabulary history of ``length`` tokens in a CTX-wide table whose columns behind ``length`` are poisoned: they
    repeat the sequence's last 8 tokens (a scan that ran past the end would match there) and then hold ids no draft may show."""
    g = np.random.default_rng(seed)
    V = int(g.integers(2, 7))
    h = np.full((CTX,), 7777, dtype=np.int32)
    h[:length] = g.integers(0, V, size=length)
    tail = h[max(0, length - 8):length]
    room = min(CTX - length, 2 * len(tail))
    h[length:length + room] = np.tile(tail, 2)[:room]
    return h, V


@pytest.mark.parametrize("length", LENGTHS)
def test_spec_draft_matches_the_reference(length):
    for seed in range(2):
        h, V = draft_history(length, 1000 * seed + length)
        hd = torch.from_numpy(h).to(DEV)
        for k in range(1, 8):
            for n in (1, 2, 3, 4, 8):
                for eos in ([], [V - 1], [0, V - 1]):
                    want = SR.draft_outputs(h, length, k, n, eos, ctx_max=CTX)
                    got = run_draft(hd, length, k, n, eos)
                    assert got == want, (length, seed, k, n, eos, got, want)


def planted(length, at, ngram, cont, fill_from=100):
    """Distinct tokens everywhere except ``ngram`` planted at the starts ``at`` (each followed by its continuation) and as the
    sequence's last tokens."""
    h = np.full((CTX,), 7777, dtype=np.int32)
    h[:length] = np.arange(fill_from, fill_from + length)
    for a, c in zip(at, cont):
        h[a:a + len(ngram)] = ngram
        h[a + len(ngram):a + len(ngram) + len(c)] = c
    h[length - len(ngram):length] = ngram
    return h


def test_spec_draft_planted_matches():
    ng = [11, 12, 13]
    # only a late match, behind a whole stride of the workgroup
    h = planted(1500, [1400], ng, [[21, 22, 23, 24, 25, 26, 27]])
    for k in (1, 4, 7):
        want = SR.draft_outputs(h, 1500, k, 3, [], ctx_max=CTX)
        assert want[1] == k and want[0][:k] == [21, 22, 23, 24, 25, 26, 27][:k]
        assert run_draft(torch.from_numpy(h).to(DEV), 1500, k, 3, []) == want
    # two matches one workgroup stride (1024 starts) apart, seen by the SAME thread: the earlier wins
    h = planted(3000, [301, 1325], ng, [[31, 32, 33], [41, 42, 43]])
    want = SR.draft_outputs(h, 3000, 3, 3, [], ctx_max=CTX)
    assert want[0] == [31, 32, 33]
    assert run_draft(torch.from_numpy(h).to(DEV), 3000, 3, 3, []) == want
    # ... and seen by different threads, the later thread's match lower
    h = planted(3000, [1030, 900], ng, [[41, 42, 43], [31, 32, 33]])
    want = SR.draft_outputs(h, 3000, 3, 3, [], ctx_max=CTX)
    assert want[0] == [31, 32, 33]
    assert run_draft(torch.from_numpy(h).to(DEV), 3000, 3, 3, []) == want
    # the longer n-gram decides even where a shorter one matches earlier
    h = planted(2000, [1200], ng, [[51, 52]])
    h[5] = 13
    h[6] = 61
    want = SR.draft_outputs(h, 2000, 2, 3, [], ctx_max=CTX)
    assert want[0] == [51, 52] and SR.draft_outputs(h, 2000, 2, 1, [], ctx_max=CTX)[0] == [61, 107]
    assert run_draft(torch.from_numpy(h).to(DEV), 2000, 2, 3, []) == want
    assert run_draft(torch.from_numpy(h).to(DEV), 2000, 2, 1, []) == SR.draft_outputs(h, 2000, 2, 1, [], ctx_max=CTX)
    # a continuation shorter than k: the match sits right in front of the trailing n-gram
    h = planted(600, [600 - 3 - 2 - 3], ng, [[71, 72]])
    want = SR.draft_outputs(h, 600, 7, 3, [], ctx_max=CTX)
    assert want[1] == 5 and want[0][:5] == [71, 72, 11, 12, 13]
    assert run_draft(torch.from_numpy(h).to(DEV), 600, 7, 3, []) == want
    # an id outside the vocabulary ends a draft like an EOS
    h = planted(600, [200], ng, [[81, 82, 999, 83]])
    assert run_draft(torch.from_numpy(h).to(DEV), 600, 4, 3, [], vocab=900) == SR.draft_outputs(h, 600, 4, 3, [], ctx_max=CTX, vocab=900)
    assert SR.draft_outputs(h, 600, 4, 3, [], ctx_max=CTX, vocab=900)[1] == 2


def test_spec_draft_context_cap_and_forced_drafts():
    ng = [11, 12]
    for length, cap in ((CTX - 2, 2), (CTX - 1, 1), (CTX, 0)):
        h = planted(length, [50], ng, [[21, 22, 23, 24, 25]])
        want = SR.draft_outputs(h, length, 5, 2, [], ctx_max=CTX)
        assert want[1] == cap
        assert run_draft(torch.from_numpy(h).to(DEV), length, 5, 2, []) == want
    # lookup = 0: the caller's draft and length stay, tok is built from them (and a match in the history is ignored)
    h = planted(500, [50], ng, [[21, 22, 23, 24, 25]])
    hd = torch.from_numpy(h).to(DEV)
    last = int(h[499])
    assert run_draft(hd, 500, 4, 2, [], lookup=False, draft=[5, 6, 7, 8], draft_len=2) == ([5, 6, 7, 8], 2, [last, 5, 6, last, last])
    assert run_draft(hd, 500, 4, 2, [], lookup=False, draft=[5, 6, 7, 8], draft_len=0) == ([5, 6, 7, 8], 0, [last] * 5)
    assert run_draft(hd, 500, 4, 2, [], lookup=False, draft=[5, 6, 7, 8], draft_len=9) == ([5, 6, 7, 8], 9, [last, 5, 6, 7, 8])
    h2 = planted(CTX - 1, [50], ng, [[21]])
    assert run_draft(torch.from_numpy(h2).to(DEV), CTX - 1, 4, 2, [], lookup=False, draft=[5, 6, 7, 8], draft_len=4)[2] == \
        [12, 5, 12, 12, 12]


# ---- vly_spec_accept --------------------------------------------------------------------------------------------------------
GUARD = 12


def run_accept(am, draft, dl, k, hist, pos, stats):
    """Every table sits in the middle of a guarded buffer; returns what the kernel left, guards checked."""
    from valley_amd import ops

    def guarded(values):
        t = torch.full((len(values) + 2 * GUARD,), -99, dtype=torch.int32)
        t[GUARD:GUARD + len(values)] = torch.as_tensor(values, dtype=torch.int32)
        return t.to(DEV)

    bufs = {"am": guarded(am), "draft": guarded(draft), "dl": guarded([dl]), "hist": guarded(hist), "pos": guarded([pos]),
            "emit": guarded([-3] * (k + 2)), "tok": guarded([-3] * (k + 1)), "stats": guarded(stats)}
    view = {name: t[GUARD:t.numel() - GUARD] for name, t in bufs.items()}
    ops.spec_accept(view["am"], view["draft"], view["dl"], k, view["hist"], view["pos"], view["emit"], view["tok"], view["stats"])
    for name, t in bufs.items():
        assert bool((t[:GUARD] == -99).all()) and bool((t[-GUARD:] == -99).all()), f"{name}: a guard word changed"
    for name, src in (("am", am), ("draft", draft), ("dl", [dl])):
        assert view[name].tolist() == list(src), f"{name} is an input"
    return {name: view[name].tolist() for name in ("hist", "pos", "emit", "tok", "stats")}


def test_spec_accept_all_36_pairs():
    k = 7
    am = [10, 11, 12, 13, 14, 15, 16, 17]
    for dl in range(k + 1):
        for m in range(dl + 1):
            d = [am[i] if i != m else 99 for i in range(k)]
            hist = np.full((64,), -7, dtype=np.int32)
            n, h, emit, tok0, stats, pos = SR.accept(am, d, dl, k, hist, 20, [3, 4, 5])
            assert n == m
            got = run_accept(am, d, dl, k, hist.tolist(), 20, [3, 4, 5])
            assert got["hist"] == h.tolist() and got["emit"] == emit and got["pos"] == [pos] and got["stats"] == stats, (dl, m, got)
            assert got["tok"] == [tok0] + [-3] * k, (dl, m, got["tok"])           # only tok[0] is written


@pytest.mark.parametrize("k", [1, 3])
def test_spec_accept_smaller_k_and_the_end_of_the_cache(k):
    am = list(range(30, 31 + k))
    for pos in (21, 20, 23 - k, 23):                         # hist has 24 columns: partly, wholly (k = 1, 3), and not at all inside
        for dl in range(k + 1):
            hist = np.full((24,), -7, dtype=np.int32)
            n, h, emit, tok0, stats, p = SR.accept(am, am[:k], dl, k, hist, pos, [0, 0, 0])
            got = run_accept(am, am[:k], dl, k, hist.tolist(), pos, [0, 0, 0])
            assert got["hist"] == h.tolist() and got["emit"] == emit and got["pos"] == [p] and got["stats"] == stats
            assert got["tok"][0] == tok0 and n == min(dl, max(0, 24 - (pos + 1)))      # the drafts whose rows fit the cache
    assert run_accept(am, am[:k], 50, k, [-7] * 24, 2, [0, 0, 0])["emit"][0] == k + 1     # a draft length beyond k counts as k


# ---- the session and generate() ---------------------------------------------------------------------------------------------
NEW = 24
TRUTH = 40


@pytest.fixture(scope="module")
def golden():
    """The golden model, the prompts and plain greedy decoding's tokens — computed once, shared, never modified."""
    from tests.test_model_gpu import build_golden_model
    model = build_golden_model()
    T = G.GCFG["T"]
    img = torch.from_numpy(G.golden_pixels(T, "mixed")).view(1, T, 3, 224, 224).cuda()
    prompts = {}
    for case in ("decode", "decode2"):
        prompts[case] = (torch.from_numpy(G.golden_ids(case)[0]).cuda(), None)
    ids, mask = G.golden_ids("main")                         # row 1 of "main" is left-padded
    prompts["main1"] = (torch.from_numpy(ids[1:2]).cuda(), torch.from_numpy(mask[1:2]).cuda())
    truth = {}
    for name, (ids_t, m) in prompts.items():
        seq = model.generate(ids_t, images=img, attention_mask=m, max_new_tokens=TRUTH, use_graph=True)
        truth[name] = seq[0, ids_t.shape[1]:].tolist()
        assert len(truth[name]) == TRUTH
    return model, img, prompts, truth


def forced_session(golden, name, k, use_graph):
    from valley_amd import ops
    from valley_amd.spec import SpecDecodeSession
    model, img, prompts, truth = golden
    ids, mask = prompts[name]
    ll = model.get_model().llama
    cache = ll.new_cache(1, ids.shape[1] + TRUTH + 8)
    out = model(input_ids=ids, images=img, attention_mask=mask, past_key_values=cache, use_cache=True)
    first = ops.argmax(out.logits[:, -1, :].contiguous())
    sess = SpecDecodeSession(ll, cache, k, use_graph=use_graph, lookup=False)
    sess.begin(first, prompt_ids=ids[0])
    return sess, [int(first[0])]


def forced_run(golden, name, k, m, use_graph):
    """Every step drafts k tokens: the first m are the true greedy continuation, the others are wrong (truth + 1 mod vocab)."""
    truth = golden[3][name]
    V = G.GCFG["vocab"]
    sess, new = forced_session(golden, name, k, use_graph)
    steps = 0
    while len(new) < NEW:
        nxt = truth[len(new):len(new) + k]
        sess.draft.copy_(torch.tensor([t if i < m else (t + 1) % V for i, t in enumerate(nxt)], dtype=torch.int32))
        sess.draft_len.fill_(k)
        before = sess.stats.tolist()
        got = sess.step()
        after = sess.stats.tolist()
        assert len(got) == m + 1 and after == [before[0] + 1, before[1] + k, before[2] + m], (name, k, m, steps, got, before, after)
        new += got
        steps += 1
        assert sess.cache.seq_len == sess.pos.item() == golden[2][name][0].shape[1] + len(new) - 1
    sess.check()
    assert new[:NEW] == truth[:NEW], (name, k, m, new[:NEW], truth[:NEW])
    assert steps == math.ceil((NEW - 1) / (m + 1))
    return steps


@pytest.mark.parametrize("use_graph", [True, False], ids=["graph", "eager"])
@pytest.mark.parametrize("k", [1, 3, 7])
@pytest.mark.parametrize("name", ["decode", "decode2"])
def test_session_forced_drafts(golden, name, k, use_graph):
    """m = k: every step accepts k (ceil(23 / (k + 1)) steps); m = 0: nothing is accepted (23 steps); in between the rows of
    the rejected drafts are stale K / V at and behind the new position — invisible, then overwritten."""
    for m in range(k + 1):
        forced_run(golden, name, k, m, use_graph)


def test_session_prefill_attention_arm_and_refusals(golden, monkeypatch):
    from valley_amd.spec import SpecDecodeSession
    monkeypatch.setenv("VALLEY_SPEC_ATTN", "prefill")
    forced_run(golden, "decode2", 3, 2, True)
    monkeypatch.setenv("VALLEY_SPEC_ATTN", "other")
    ll = golden[0].get_model().llama
    with pytest.raises(ValueError, match="VALLEY_SPEC_ATTN"):
        SpecDecodeSession(ll, ll.new_cache(1, 64), 3)
    monkeypatch.delenv("VALLEY_SPEC_ATTN")
    with pytest.raises(ValueError, match="cache.batch == 1"):
        SpecDecodeSession(ll, ll.new_cache(2, 64), 3)
    for k in (0, 8):
        with pytest.raises(ValueError, match="prompt_lookup_num_tokens"):
            SpecDecodeSession(ll, ll.new_cache(1, 64), k)
    # a cache that cannot grow with fewer than k + 1 positions left
    sess, new = forced_session(golden, "decode", 7, False)
    sess.cache.seq_len = sess.cache.ctx_max - 7
    assert not sess.room()
    with pytest.raises(ValueError, match="fewer than k"):
        sess.step()


def kv_bits(cache, n):
    return [AO.bits(t[:, :, :n].clone()) for t in cache.k + cache.v]


@pytest.mark.parametrize("use_graph", [True, False], ids=["graph", "eager"])
def test_session_on_a_nearly_full_cache_leaves_the_cache_alone(golden, use_graph):
    """begin() on a cache with fewer than k + 1 positions left must not warm a step up: the kernels clamp the position to
    ctx_max - (k + 1), below the prompt's end, and the step's rope_kv would overwrite K / V rows of real positions."""
    from valley_amd import ops
    from valley_amd.spec import SpecDecodeSession
    model, img, prompts, _ = golden
    ids, mask = prompts["decode"]
    ll = model.get_model().llama
    S = ids.shape[1]
    for free in (1, 4, 7):
        cache = ll.new_cache(1, S + free)
        out = model(input_ids=ids, images=img, attention_mask=mask, past_key_values=cache, use_cache=True)
        first = ops.argmax(out.logits[:, -1, :].contiguous())
        before = kv_bits(cache, cache.ctx_max)
        sess = SpecDecodeSession(ll, cache, 7, use_graph=use_graph)
        sess.begin(first, prompt_ids=ids[0])
        assert sess.graph is None and not sess.room()
        with pytest.raises(ValueError, match="fewer than k"):
            sess.step()
        torch.cuda.synchronize()
        assert all(torch.equal(a, b) for a, b in zip(kv_bits(cache, cache.ctx_max), before)), free
        assert cache.seq_len == S and sess.stats.tolist() == [0, 0, 0]


@pytest.mark.parametrize("use_graph", [True, False], ids=["graph", "eager"])
def test_generate_with_fewer_new_tokens_than_drafts_keeps_the_prompt_rows(golden, monkeypatch, use_graph):
    """max_new_tokens <= k: the cache (S + max_new_tokens deep) never has room for a verify step.  No speculative session is
    made, every token comes from the one-token route, and the prompt's K / V rows are bit for bit the plain call's."""
    model, img, prompts, truth = golden
    ll = model.get_model().llama
    made = []
    new_cache = ll.new_cache
    monkeypatch.setattr(ll, "new_cache", lambda *a, **kw: made.append(new_cache(*a, **kw)) or made[-1])
    for name in ("decode", "main1"):
        ids, mask = prompts[name]
        S = ids.shape[1]
        for k in (3, 7):
            for n in range(1, k + 1):
                del made[:]
                want = model.generate(ids, images=img, attention_mask=mask, max_new_tokens=n, use_graph=use_graph)
                out = model.generate(ids, images=img, attention_mask=mask, max_new_tokens=n, use_graph=use_graph,
                                     prompt_lookup_num_tokens=k, return_dict_in_generate=True)
                assert len(made) == 2 and made[0].ctx_max == made[1].ctx_max == S + n
                assert torch.equal(out.sequences, want) and want[0, S:].tolist() == truth[name][:n], (name, k, n)
                # rows [0, S + n - 1): the prompt and every token that was fed
                assert all(torch.equal(a, b) for a, b in zip(kv_bits(made[1], S + n - 1), kv_bits(made[0], S + n - 1))), (name, k, n)
                assert out.speculation == {"steps": n - 1, "drafted": 0, "accepted": 0}
    assert "valley_amd.spec" in sys.modules                  # (the arguments were checked, no session was made)


@pytest.mark.parametrize("use_graph", [True, False], ids=["graph", "eager"])
@pytest.mark.parametrize("k", [1, 3, 7])
def test_generate_prompt_lookup_is_plain_greedy(golden, k, use_graph):
    model, img, prompts, truth = golden
    for name, (ids, mask) in prompts.items():
        out = model.generate(ids, images=img, attention_mask=mask, max_new_tokens=NEW, use_graph=use_graph, prompt_lookup_num_tokens=k,
                             return_dict_in_generate=True)
        new = out.sequences[0, ids.shape[1]:].tolist()
        assert torch.equal(out.sequences[:, :ids.shape[1]], ids) and new == truth[name][:NEW], (name, k, new, truth[name][:NEW])
        s = out.speculation
        print(f"{name} k={k}: {s}")
        assert set(s) == {"steps", "drafted", "accepted"} and s["accepted"] <= s["drafted"] <= k * s["steps"]
        assert s["steps"] <= NEW - 1 <= s["steps"] + s["accepted"]
        assert out.sequences_scores is None


def test_generate_prompt_lookup_stops_like_plain_greedy(golden):
    from transformers import StoppingCriteria

    class AtLength(StoppingCriteria):
        def __init__(self, n):
            self.n = n

        def __call__(self, input_ids, scores, **kw):
            return input_ids.shape[1] >= self.n

    model, img, prompts, truth = golden
    for name, (ids, mask) in prompts.items():
        kw = dict(images=img, attention_mask=mask)
        n_in = ids.shape[1]
        for k in (3, 7):
            eos = truth[name][5]
            want = model.generate(ids, max_new_tokens=NEW, eos_token_id=eos, **kw)
            got = model.generate(ids, max_new_tokens=NEW, eos_token_id=eos, prompt_lookup_num_tokens=k, **kw)
            assert torch.equal(got, want) and want.shape[1] <= n_in + 6 and int(want[0, -1]) == eos, (name, k)
            got = model.generate(ids, max_new_tokens=NEW, eos_token_id=[eos, 1], pad_token_id=0, prompt_lookup_num_tokens=k,
                                 max_matching_ngram_size=3, **kw)
            assert torch.equal(got, want)
            want = model.generate(ids, max_new_tokens=NEW, stopping_criteria=[AtLength(n_in + 7)], **kw)
            got = model.generate(ids, max_new_tokens=NEW, stopping_criteria=[AtLength(n_in + 7)], prompt_lookup_num_tokens=k, **kw)
            assert torch.equal(got, want) and want.shape[1] == n_in + 7, (name, k)
    ids, mask = prompts["decode2"]
    for n in range(1, 11):
        got = model.generate(ids, images=img, max_new_tokens=n, prompt_lookup_num_tokens=7)
        assert got.shape[1] == ids.shape[1] + n and got[0, ids.shape[1]:].tolist() == truth["decode2"][:n], n


def test_generate_prompt_lookup_long_run_and_cache_growth(golden):
    """270 new tokens at k = 3: generate() against the plain call, and the session on a cache that grows under it (a
    model-sized cache doubles when it fills up: new storage, a new history table, a new graph)."""
    from valley_amd import ops
    from valley_amd.spec import SpecDecodeSession
    model, img, prompts, _ = golden
    ids, mask = prompts["decode"]
    want = model.generate(ids, images=img, max_new_tokens=270)
    out = model.generate(ids, images=img, max_new_tokens=270, prompt_lookup_num_tokens=3, return_dict_in_generate=True)
    print(f"270 tokens, k = 3: {out.speculation}")
    assert torch.equal(out.sequences, want)
    ll = model.get_model().llama
    cache = ll.new_cache(1, ids.shape[1] + 40)
    cache.growable, cache.limit = True, 2048                 # what the model sets on a cache it sized itself
    o = model(input_ids=ids, images=img, past_key_values=cache, use_cache=True)
    first = ops.argmax(o.logits[:, -1, :].contiguous())
    sess = SpecDecodeSession(ll, cache, 3, use_graph=True)
    sess.begin(first, prompt_ids=ids[0])
    new, gen0 = [int(first[0])], cache.generation
    while len(new) < 270:
        new += sess.step()
    sess.check()
    assert cache.generation > gen0 and cache.ctx_max >= ids.shape[1] + 270 and sess.hist.numel() == cache.ctx_max
    assert new[:270] == want[0, ids.shape[1]:].tolist()
    assert sess.hist[:ids.shape[1]].tolist() == ids[0].tolist() and sess.hist[ids.shape[1]:ids.shape[1] + len(new)].tolist() == new


def test_generate_prompt_lookup_on_the_int8_engine():
    from tests.test_model_gpu import build_golden_model
    model = build_golden_model()
    model.quantize_decode_weights("int8")
    T = G.GCFG["T"]
    img = torch.from_numpy(G.golden_pixels(T, "mixed")).view(1, T, 3, 224, 224).cuda()
    ids = torch.from_numpy(G.golden_ids("decode2")[0]).cuda()
    want = model.generate(ids, images=img, max_new_tokens=NEW)
    for k in (1, 3):
        out = model.generate(ids, images=img, max_new_tokens=NEW, prompt_lookup_num_tokens=k, return_dict_in_generate=True)
        assert torch.equal(out.sequences, want), (k, out.sequences[0, ids.shape[1]:].tolist(), want[0, ids.shape[1]:].tolist())
        assert out.speculation["steps"] >= 1


# ---- the fp16 storage type, and a run that never speculates -------------------------------------------------------------------
def _worker(mode, env_extra):
    env = {k: v for k, v in os.environ.items() if k not in ("VALLEY_PRECISION", "VALLEY_SPEC_ATTN")}
    env.update(env_extra)
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "spec_worker.py"), mode], capture_output=True, text=True, env=env,
                       timeout=600)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    return json.loads(p.stdout.strip().splitlines()[-1])


def test_spec_on_the_fp16_library():
    res = _worker("fp16", {"VALLEY_PRECISION": "fp16"})
    assert res["ok"] and res["storage"] == 1 and res["tokens_equal"]


def test_plain_generate_never_loads_the_spec_library():
    res = _worker("off", {})
    assert res["ok"] and res["new_tokens"] == 4 and res["spec_lib_loaded"] is False
