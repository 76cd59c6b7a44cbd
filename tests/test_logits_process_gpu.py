"""Logits processors on the MI355X: vly_logits_process against transformers' own processor classes applied to the same
device tensors, the beam history gather against index_select, the scored beam candidates against vly_beam_candidates, a
captured launch replayed with new inputs, and generate() / ContinuousBatcher end to end on the golden model against the
reference loops of tests/logits_ref.py (pinned to transformers by tests/test_logits_process_cpu.py)."""
import json
import os
import subprocess
import sys

import pytest
import torch

from tests import golden_cfg as G
from tests import logits_ref

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def dev():
    return torch.device("cuda:0")


def same_bits(a, b):
    """Equal values, NaN where NaN (torch.equal treats NaN as unequal)."""
    return torch.equal(a.isnan(), b.isnan()) and torch.equal(torch.where(a.isnan(), 0.0, a), torch.where(b.isnan(), 0.0, b))


def random_case(R, V, ld, hist_ld, seed, nan=True):
    """Per-row parameters, histories with duplicate ids (small alphabets make n-grams repeat), lengths, logits with -inf /
    NaN entries, sentinels in the padding columns."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn((R, ld), generator=g) * 3.0
    x[:, V:] = 12345.0
    hist = torch.zeros((R, hist_ld), dtype=torch.int32)
    lens, rows = [], []
    pens, ns = [1.0, 0.7, 1.3, 2.0], [0, 1, 2, 3, 5]
    for r in range(R):
        alpha = [4, 8, V][r % 3]
        hist[r] = torch.randint(0, alpha, (hist_ld,), generator=g, dtype=torch.int32)
        L = int(torch.randint(1, hist_ld + 1, (1,), generator=g))
        if r % 4 == 3:
            L = 2                                                                  # len < n for most n
        lens.append(L)
        if r % 6 == 0:
            rows.append((1.0, 0, 0))                                               # neutral
        else:
            rows.append((pens[r % 4] if r % 4 else 1.3, ns[r % 5], [0, L - 1, L + 3][r % 3]))
        x[r, int(hist[r, L - 1]) % V] = float("-inf")
        if nan and r % 7 == 2:
            x[r, int(hist[r, 0]) % V] = float("nan")
            x[r, 5] = float("nan")
    return x, hist, lens, rows


def expected_row(x_row, ids, pen, n, m, eos, log_softmax=False):
    """transformers' processors on the host copy of the row.  (On the device, torch divides a tensor by a Python scalar as a
    multiplication by its reciprocal, one rounding more than the IEEE division HF's penalty specifies and the kernel does;
    on the host torch divides.)"""
    procs = logits_ref.hf_processors(pen, n, m, None, eos=eos)
    x_row = x_row.cpu()
    s = torch.log_softmax(x_row, -1) if log_softmax else x_row.clone()
    return (procs(ids.cpu().long()[None], s[None])[0] if len(procs) else s).to(dev())


@pytest.mark.parametrize("R,V,ld", [(1, 32000, 32000), (16, 32000, 32000), (5, 1000, 1003), (16, 306, 320)])
@pytest.mark.parametrize("append", [False, True])
def test_process_matches_transformers_logit_mode(R, V, ld, append):
    from valley_amd import ops
    x, hist, lens, rows = random_case(R, V, ld, 96, seed=R * 1000 + V + append)
    eos = [2, V - 1, 2]                                                            # a duplicate EOS id too
    xd, hd = x.to(dev()), hist.to(dev())
    tok = torch.randint(0, V, (R,), dtype=torch.int32)
    params = ops.processor_rows([p for p, _, _ in rows], [n for _, n, _ in rows], [m for _, _, m in rows], device=dev())
    length = torch.tensor(lens, dtype=torch.int32, device=dev()) - (1 if append else 0)
    orig = xd.clone()
    ops.logits_process(xd[:, :V], params, hd, length, 1 if append else 0, tok=tok.to(dev()) if append else None,
                       eos=torch.tensor(eos, dtype=torch.int32, device=dev()))
    want_hist = hist.clone()
    if append:
        for r in range(R):
            want_hist[r, lens[r] - 1] = tok[r]
    assert torch.equal(hd.cpu(), want_hist)
    for r in range(R):
        pen, n, m = rows[r]
        want = expected_row(orig[r, :V], want_hist[r, :lens[r]].to(dev()), pen, n, m, eos)
        assert same_bits(xd[r, :V], want), (r, rows[r], lens[r])
        if rows[r] == (1.0, 0, 0):
            assert torch.equal(xd[r].view(torch.int32), orig[r].view(torch.int32))      # neutral rows: not written
    assert torch.equal(xd[:, V:], orig[:, V:])                                       # the padding columns are never touched


def test_process_matches_transformers_log_softmax_mode():
    from valley_amd import ops
    R, V = 16, 32000
    x, hist, lens, rows = random_case(R, V, V, 80, seed=77, nan=False)
    xd, hd = x.to(dev()), hist.to(dev())
    params = ops.processor_rows([p for p, _, _ in rows], [n for _, n, _ in rows], [m for _, _, m in rows], device=dev())
    length = torch.tensor(lens, dtype=torch.int32, device=dev())
    orig = xd.clone()
    ops.logits_process(xd, params, hd, length, 0, eos=torch.tensor([2], dtype=torch.int32, device=dev()), log_softmax=True)
    for r in range(R):
        pen, n, m = rows[r]
        want = expected_row(orig[r], hist[r, :lens[r]].to(dev()), pen, n, m, [2], log_softmax=True)
        got = xd[r]
        assert torch.equal(torch.isinf(got), torch.isinf(want))
        fin = torch.isfinite(want)
        assert float((got[fin] - want[fin]).abs().max()) <= 1e-6 * max(1.0, float(want[fin].abs().max())), r


def test_process_shared_length_and_no_eos():
    """len from one device counter (+ len_add) for every row; without EOS ids the minimum length does nothing."""
    from valley_amd import ops
    R, V = 4, 500
    x, hist, _, _ = random_case(R, V, V, 64, seed=5)
    xd, hd = x.to(dev()), hist.to(dev())
    params = ops.processor_rows(1.3, 2, 1000, device=dev()).expand(R, 4).contiguous()
    L = torch.tensor([30], dtype=torch.int32, device=dev())
    orig = xd.clone()
    ops.logits_process(xd, params, hd, L, 3)
    for r in range(R):
        want = expected_row(orig[r], hist[r, :33].to(dev()), 1.3, 2, 0, None)
        assert same_bits(xd[r], want)


def test_history_gather_any_parent_map():
    from valley_amd import ops
    g = torch.Generator().manual_seed(9)
    for R, parent in [(12, torch.randint(0, 12, (12,), generator=g)), (8, torch.tensor([1, 0, 3, 4, 2, 5, 5, 7])),
                      (128, torch.randperm(128, generator=g)), (300, torch.randint(0, 300, (300,), generator=g)),
                      (8192, torch.randperm(8192, generator=g))]:
        hist = torch.randint(0, 1 << 20, (R, 150), generator=g, dtype=torch.int32)
        hd = hist.to(dev())
        ops.logits_history_gather(hd, parent.to(torch.int32).to(dev()), 5, 0, len_dev=torch.tensor([137], dtype=torch.int32,
                                                                                                  device=dev()))
        want = hist.clone()
        want[:, 5:137] = hist[parent.long(), 5:137]
        assert torch.equal(hd.cpu(), want), R
    hd = hist.to(dev())                                                   # hi <= lo: nothing moves
    ops.logits_history_gather(hd, torch.randperm(R, generator=g).to(torch.int32).to(dev()), 20, 20)
    assert torch.equal(hd.cpu(), hist)


@pytest.mark.parametrize("V,n_eos", [(32000, 1), (306, 0), (40000, 2)])
def test_scored_candidates_equal_beam_candidates_on_untouched_rows(V, n_eos):
    """Log-softmax mode with neutral parameters, then candidates over the scores: bit for bit vly_beam_candidates."""
    from valley_amd import ops
    B, nb = 2, 4
    R, K = B * nb, ops.beam_k(nb, n_eos)
    g = torch.Generator().manual_seed(V)
    x = (torch.randn((R, V), generator=g) * 4).to(dev())
    x[3, :100] = float("-inf")
    x[5, 7] = float("nan")
    running = (torch.randn(R, generator=g) * 3).to(dev())
    eos = torch.tensor([3, 9][:n_eos], dtype=torch.int32, device=dev()) if n_eos else None
    want = ops.beam_candidates(x, running, B, nb, K, eos, ops.beam_scratch(B, nb, K, dev()))
    y = x.clone()
    ops.logits_process(y, ops.processor_rows([None] * R, device=dev()), torch.zeros((R, 8), dtype=torch.int32, device=dev()),
                       None, 4, log_softmax=True)
    got = ops.logits_beam_candidates(y, running, B, nb, K, eos, ops.beam_scratch(B, nb, K, dev()))
    for a, b in zip(got, want):
        assert torch.equal(a, b)


def test_captured_process_replays_new_inputs():
    from valley_amd import ops
    R, V = 6, 32000
    g = torch.Generator().manual_seed(1)
    logits = torch.empty((R, V), device=dev())
    params = torch.empty((R, 4), dtype=torch.int32, device=dev())
    hist = torch.empty((R, 64), dtype=torch.int32, device=dev())
    length = torch.empty((R,), dtype=torch.int32, device=dev())
    tok = torch.empty((R,), dtype=torch.int32, device=dev())
    eos = torch.tensor([2], dtype=torch.int32, device=dev())

    def fill(k):
        logits.copy_(torch.randn((R, V), generator=g) * 3)
        params.copy_(ops.processor_rows([1.3, 0.7, None, 2.0, 1.1, None][k:] + [1.2] * k, [2, 0, 3, 1, 0, 2][k:] + [3] * k,
                                        [0, 40, 0, 70, 0, 0][k:] + [50] * k))
        hist.copy_(torch.randint(0, 5 + 50 * k, (R, 64), generator=g, dtype=torch.int32))
        length.copy_(torch.randint(1, 60, (R,), generator=g, dtype=torch.int32))
        tok.copy_(torch.randint(0, V, (R,), generator=g, dtype=torch.int32))

    def launch():
        ops.logits_process(logits, params, hist, length, 1, tok=tok, eos=eos)

    fill(0)
    launch()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        launch()
    for k in range(1, 4):
        fill(k)
        state = [t.clone() for t in (logits, params, hist, length, tok)]
        graph.replay()
        got = (logits.clone(), hist.clone())
        for t, s in zip((logits, params, hist, length, tok), state):
            t.copy_(s)
        launch()
        assert torch.equal(got[0].view(torch.int32), logits.view(torch.int32)) and torch.equal(got[1], hist), k


# ---- generate() end to end -----------------------------------------------------------------------------------------------------

def golden_model():
    from tests.test_model_gpu import build_golden_model
    return build_golden_model()


def inputs(case):
    T = G.GCFG["T"]
    if case == "one":
        ids, mask = G.golden_ids("decode")
        img = torch.from_numpy(G.golden_pixels(T, "mixed")).view(1, T, 3, 224, 224).cuda()
    else:
        ids, mask = G.golden_ids("main")
        img = torch.from_numpy(G.golden_pixels(2 * T, "main")).view(2, T, 3, 224, 224).cuda()
    return torch.from_numpy(ids).cuda(), torch.from_numpy(mask).cuda(), img


def greedy_stepper(model, ids, mask, img):
    """The generic forward as generate() drives it: prefill, then one token per row with the mask extended."""
    state = {}

    def step(tok):
        if tok is None:
            state["cache"] = model.model.llama.new_cache(ids.shape[0], 2048)
            state["mask"] = mask
            out = model(input_ids=ids, images=img, attention_mask=mask, past_key_values=state["cache"], use_cache=True)
        else:
            m = state["mask"]
            state["mask"] = m = torch.cat([m, torch.ones((m.shape[0], 1), dtype=m.dtype, device=m.device)], 1)
            out = model(input_ids=tok[:, None], attention_mask=m, past_key_values=state["cache"], use_cache=True)
        return out.logits[:, -1, :].float()
    return step


def beam_stepper(model, ids, mask, img, nb):
    """tests/test_beam_gpu.py's plain-torch beam forward: prompts repeated nb times, the cache reordered by index_select."""
    rep = lambda t: t.repeat_interleave(nb, 0)                # noqa: E731
    state = {}

    def step(tok):
        if tok is None:
            out = model(input_ids=rep(ids), images=rep(img), attention_mask=rep(mask), use_cache=True)
            state["cache"] = out.past_key_values
        else:
            out = model(input_ids=tok.long()[:, None], past_key_values=state["cache"], use_cache=True)
        return out.logits[:, -1, :].float()

    def reorder(p):
        for t in state["cache"].k + state["cache"].v:
            t.copy_(t.index_select(0, p))
    return step, reorder


def ref_greedy(model, ids, mask, img, max_new, eos=None, **kw):
    procs = logits_ref.hf_processors(kw.get("repetition_penalty"), kw.get("no_repeat_ngram_size"), kw.get("min_length"),
                                     kw.get("min_new_tokens"), prompt_len=ids.shape[1], eos=eos)
    return logits_ref.greedy_loop(greedy_stepper(model, ids, mask, img), ids, max_new, procs, eos=eos, pad=0)


def repeated_bigram(row, start):
    """True if a bigram ending at or after ``start`` occurred earlier in the row."""
    t = row.tolist()
    seen = set()
    for i in range(len(t) - 1):
        bg = (t[i], t[i + 1])
        if i + 1 >= start and bg in seen:
            return True
        seen.add(bg)
    return False


PROCS = [dict(repetition_penalty=1.3), dict(repetition_penalty=0.7, no_repeat_ngram_size=3), dict(no_repeat_ngram_size=2),
         dict(repetition_penalty=1.2, no_repeat_ngram_size=2, min_new_tokens=6)]


@pytest.mark.parametrize("kw", PROCS)
def test_generate_greedy_processors_match_reference(kw):
    model = golden_model()
    ids, mask, img = inputs("main")
    ref = ref_greedy(model, ids, mask, img, 10, eos=None, **kw)
    outs = [model.generate(ids, images=img, attention_mask=mask, max_new_tokens=10, use_graph=ug, **kw) for ug in (True, False, None)]
    for o in outs:
        assert torch.equal(o, ref), kw


def test_no_repeat_ngram_breaks_a_greedy_loop():
    """Greedy decoding of the golden model repeats a bigram today; with no_repeat_ngram_size=2 no generated bigram repeats
    one of the sequence (prompt included), and the output changes."""
    model = golden_model()
    ids, mask, img = inputs("main")
    S = ids.shape[1]
    plain = model.generate(ids, images=img, attention_mask=mask, max_new_tokens=24)
    loops = [r for r in range(ids.shape[0]) if repeated_bigram(plain[r], S)]
    assert loops, "the golden prompts no longer loop under greedy decoding"
    for ug in (True, False, None):
        got = model.generate(ids, images=img, attention_mask=mask, max_new_tokens=24, no_repeat_ngram_size=2, use_graph=ug)
        assert not any(repeated_bigram(got[r], S) for r in range(got.shape[0])), ug
        assert not torch.equal(got, plain)


def test_min_new_tokens_keeps_an_early_eos_out():
    model = golden_model()
    ids, mask, img = inputs("main")
    S = ids.shape[1]
    plain = model.generate(ids, images=img, attention_mask=mask, max_new_tokens=8)
    eos = int(plain[0, S + 1])                                     # row 0 would stop after two tokens
    early = model.generate(ids, images=img, attention_mask=mask, max_new_tokens=8, eos_token_id=eos, pad_token_id=0)
    assert int(early[0, S + 1]) == eos
    ref = ref_greedy(model, ids, mask, img, 8, eos=eos, min_new_tokens=6)
    for ug in (True, False, None):
        got = model.generate(ids, images=img, attention_mask=mask, max_new_tokens=8, eos_token_id=eos, pad_token_id=0,
                             min_new_tokens=6, use_graph=ug)
        assert torch.equal(got, ref), ug
        assert not bool((got[:, S:S + 6] == eos).any())
    got = model.generate(ids, images=img, attention_mask=mask, max_new_tokens=8, eos_token_id=eos, pad_token_id=0,
                         min_length=S + 6)
    assert torch.equal(got, ref)


def test_generate_more_than_eight_rows():
    model = golden_model()
    ids, mask, img = inputs("main")
    ids9, mask9 = ids.repeat(5, 1)[:9], mask.repeat(5, 1)[:9]
    img9 = img.repeat(5, 1, 1, 1, 1)[:9]
    kw = dict(repetition_penalty=1.3, no_repeat_ngram_size=2)
    ref = ref_greedy(model, ids9, mask9, img9, 6, **kw)
    got = model.generate(ids9, images=img9, attention_mask=mask9, max_new_tokens=6, **kw)
    assert torch.equal(got, ref)


def test_seeded_sampling_with_processors_in_every_route():
    model = golden_model()
    ids, mask, img = inputs("main")
    kw = dict(images=img, attention_mask=mask, max_new_tokens=10, do_sample=True, temperature=0.9, top_k=50, seed=11,
              repetition_penalty=1.4, no_repeat_ngram_size=2)
    outs = [model.generate(ids, use_graph=ug, **kw) for ug in (True, False, None)]
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2])
    assert not any(repeated_bigram(outs[0][r], ids.shape[1]) for r in range(ids.shape[0]))


def test_host_multinomial_sampling_with_processors():
    model = golden_model()
    ids, mask, img = inputs("main")
    kw = dict(images=img, attention_mask=mask, max_new_tokens=10, do_sample=True, temperature=0.8, no_repeat_ngram_size=2)
    outs = []
    for ug in (True, False, None):
        torch.manual_seed(3)
        outs.append(model.generate(ids, use_graph=ug, **kw))
        assert not any(repeated_bigram(outs[-1][r], ids.shape[1]) for r in range(ids.shape[0])), ug
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2])


@pytest.mark.parametrize("kw", [dict(repetition_penalty=1.3), dict(no_repeat_ngram_size=2, repetition_penalty=0.8)])
def test_generate_beams_with_processors_match_reference(kw):
    model = golden_model()
    ids, mask, img = inputs("main")
    step, reorder = beam_stepper(model, ids, mask, img, 4)
    procs = logits_ref.hf_processors(kw.get("repetition_penalty"), kw.get("no_repeat_ngram_size"), prompt_len=ids.shape[1])
    ref, _ = logits_ref.beam_loop(step, reorder, ids, 4, 6, procs)
    for ug in (True, False, None):
        got = model.generate(ids, images=img, attention_mask=mask, max_new_tokens=6, num_beams=4, use_graph=ug, **kw)
        assert torch.equal(got, ref.cuda()), ug


def test_generate_beams_min_new_tokens_keeps_an_eos_out():
    """Beams with an EOS that a hypothesis reaches early: min_new_tokens masks it on log-probabilities, as HF's beam search
    does, in every route."""
    model = golden_model()
    ids, mask, img = inputs("main")
    S = ids.shape[1]
    step, reorder = beam_stepper(model, ids, mask, img, 4)
    all4, _ = logits_ref.beam_loop(step, reorder, ids, 4, 6, logits_ref.hf_processors())
    eos = int(all4[0, S + 1])
    step, reorder = beam_stepper(model, ids, mask, img, 4)
    early, _ = logits_ref.beam_loop(step, reorder, ids, 4, 6, logits_ref.hf_processors(), eos=eos)
    step, reorder = beam_stepper(model, ids, mask, img, 4)
    procs = logits_ref.hf_processors(repetition_penalty=1.2, min_new_tokens=4, prompt_len=S, eos=eos)
    ref, _ = logits_ref.beam_loop(step, reorder, ids, 4, 6, procs, eos=eos)
    assert not torch.equal(ref, early)
    assert not bool((ref[:, S:S + 4] == eos).any())
    for ug in (True, False, None):
        got = model.generate(ids, images=img, attention_mask=mask, max_new_tokens=6, num_beams=4, eos_token_id=eos, pad_token_id=0,
                             repetition_penalty=1.2, min_new_tokens=4, use_graph=ug)
        assert torch.equal(got, ref.cuda()), ug


def test_generate_beams_with_processors_generic_route_twelve_rows():
    """Three prompts x four beams: above 8 rows the generic forward runs the history gather and the processors on the host
    side of the step."""
    model = golden_model()
    ids, mask, img = inputs("main")
    ids3, mask3, img3 = torch.cat([ids, ids[:1]]), torch.cat([mask, mask[:1]]), torch.cat([img, img[:1]])
    step, reorder = beam_stepper(model, ids3, mask3, img3, 4)
    procs = logits_ref.hf_processors(repetition_penalty=1.3, no_repeat_ngram_size=2, prompt_len=ids3.shape[1])
    ref, _ = logits_ref.beam_loop(step, reorder, ids3, 4, 6, procs)
    got = model.generate(ids3, images=img3, attention_mask=mask3, max_new_tokens=6, num_beams=4, repetition_penalty=1.3,
                         no_repeat_ngram_size=2)
    assert got.shape[0] == 3 and torch.equal(got, ref.cuda())
    assert torch.equal(got[2], got[0])
    plain = model.generate(ids3, images=img3, attention_mask=mask3, max_new_tokens=6, num_beams=4)
    assert not torch.equal(got, plain)


def test_generate_beams_with_an_ngram_that_never_matches_are_todays():
    model = golden_model()
    ids, mask, img = inputs("main")
    kw = dict(images=img, attention_mask=mask, max_new_tokens=6, num_beams=4, return_dict_in_generate=True)
    for ug in (True, None):
        today = model.generate(ids, use_graph=ug, **kw)
        got = model.generate(ids, use_graph=ug, no_repeat_ngram_size=500, **kw)
        assert torch.equal(got.sequences, today.sequences)
        assert torch.equal(got.sequences_scores.view(torch.int32), today.sequences_scores.view(torch.int32))


def test_batcher_mixed_requests_equal_generate_alone():
    from valley_amd.serving import ContinuousBatcher
    model = golden_model()
    T = G.GCFG["T"]
    img = torch.from_numpy(G.golden_pixels(T, "mixed")).view(1, T, 3, 224, 224).cuda()
    reqs = [torch.from_numpy(G.golden_ids(c)[0]).cuda() for c in ("decode2", "decode", "decode2")]
    plain = model.generate(reqs[1], images=img, max_new_tokens=4)
    eos = int(plain[0, reqs[1].shape[1] + 1])
    plan = [(reqs[0], dict(repetition_penalty=1.3, no_repeat_ngram_size=2)), (reqs[1], dict(min_new_tokens=5)), (reqs[2], {})]
    n = 8
    for order in (plan, plan[::-1]):
        cb = ContinuousBatcher(model, slots=4, ctx_max=512, processors=True, eos_token_id=eos)
        slots, got = [], []
        for ids, kw in order:
            s = cb.add(ids, images=img, **kw)
            slots.append(s)
            got.append([int(cb.sess.tok[s])])
        for _ in range(n - 1):
            toks = cb.step()
            for j, s in enumerate(slots):
                got[j].append(toks[s])
        for (ids, kw), toks in zip(order, got):
            alone = model.generate(ids, images=img, max_new_tokens=n, eos_token_id=eos if "min_new_tokens" in kw else None, **kw)
            want = alone[0, ids.shape[1]:].tolist()
            assert toks[:len(want)] == want, kw
    cb = ContinuousBatcher(model, slots=2, ctx_max=512)
    with pytest.raises(ValueError):
        cb.add(reqs[0], images=img, repetition_penalty=1.2)


@pytest.mark.parametrize("precision", ["fp16", "fp32"])
def test_processors_on_other_precisions(precision):
    """The fp16-storage library (its own decode session) and the fp32 engine (the generic route), each in a process of its
    own: greedy in every route and beams, with and without an EOS, against the reference loops."""
    env = dict(os.environ, VALLEY_PRECISION=precision)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "logits_worker.py")], env=env, capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    res = json.loads(r.stdout.strip().splitlines()[-1])
    assert res["precision"] == precision
    if precision == "fp16":
        assert res["library"] == "libvalley_hip_f16.so"
    else:
        assert res["engine"] == "fp32"
    assert all(res["greedy_equal_reference"].values()), res
    assert all(res["beams_equal_reference"].values()), res
    assert all(res["beams_eos_equal_reference"].values()) and res["eos_kept_out"], res
