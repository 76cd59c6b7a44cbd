"""Token log-probabilities on the MI355X: vly_score_rows bit for bit against vly_logits_process(log_softmax) and against the
float64 reference (tests/score_ref.py), top-n with ties, the raw copy, vly_score_record, vly_score_loss, and on the golden
model forward(labels=), score(), generate(output_logprobs=True) in every route and ContinuousBatcher(logprobs=).

The float64 bound is the project's own for this log-sum-exp routine, 1e-6 * max(1, max |want|)
(tests/test_logits_process_gpu.py), or twice the error of logits_process(log_softmax=True) measured against score_ref on the
cases of this file, whichever is larger.  Measured on an MI355X over every width of score_ref.WIDTHS: MEASURED below (DESIGN.md
§4.9), so the project's bound is the one that holds.

"Teacher-forced forward" in the generate tests is forward() fed the generated sequence the way generate()'s generic route
feeds it: the prompt in one call, then one token per call on the KV cache.  One call over the whole sequence runs the
prefill GEMMs instead of the one-token kernels and differs from them at the 16-bit storage's rounding, not at fp32's; it is
compared as well, as an independent reference, at WHOLE below: the project holds one-token logits to 2e-2 of the logits of
other kernels on the same computation (tests/test_model_gpu.py: the session against the generic path, chunked against whole
prefill), and |d lp| <= |d x_t| + |d lse| <= 2 max |d x|.  Not on the int8 engine, whose prefill reads the 16-bit weights."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import golden_cfg as G
from tests import score_ref as SR

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

MEASURED = 8.254e-8      # max |logits_process(log_softmax) - float64| / max(1, max |want|) over SR.WIDTHS on an MI355X
REL = max(1e-6, 2 * MEASURED)
WHOLE = 2 * 2e-2         # generate's log-probabilities against ONE forward over the whole sequence (the module docstring)


def dev():
    return torch.device("cuda:0")


def bits(t):
    return t.contiguous().view(torch.int32)


def within(got, want, what=""):
    """got (fp32 tensor / array) against float64 want: the same infinities and NaNs, finite values within the bound."""
    got = np.asarray(got.detach().cpu().numpy() if isinstance(got, torch.Tensor) else got, dtype=np.float64)
    want = np.asarray(want, dtype=np.float64)
    fin = np.isfinite(want)
    assert np.array_equal(np.isnan(got), np.isnan(want)), what
    assert np.array_equal(got[np.isinf(want)], want[np.isinf(want)]), what
    if fin.any():
        err = np.abs(got[fin] - want[fin]).max()
        scale = max(1.0, np.abs(want[fin]).max())
        print(f"{what}: max err {err:.3e}, scale {scale:.3g}, err / scale {err / scale:.3e} (bound {REL:.1e})")
        assert err <= REL * scale, (what, err, scale)


def log_softmax_rows(xd, V):
    """The existing kernel: x - lse in place on a clone, neutral processor rows, no history."""
    from valley_amd import ops
    y = xd.clone()
    R = y.shape[0]
    ops.logits_process(y[:, :V], ops.processor_rows([None] * R, device=dev()), torch.zeros((R, 1), dtype=torch.int32, device=dev()),
                       log_softmax=True)
    return y


@pytest.mark.parametrize("V", SR.WIDTHS)
def test_rows_equal_logits_process_bit_for_bit(V):
    from valley_amd import lib_score, ops
    x, t0 = SR.rows_case(V)
    xd = torch.from_numpy(x).to(dev())
    orig = xd.clone()
    y = log_softmax_rows(xd, V)
    assert torch.equal(bits(y[:, V:]), bits(orig[:, V:]))
    lse64 = SR.lse(x[:, :V])
    for k, t in enumerate([t0] + SR.rows_case_targets(V)):
        td = torch.from_numpy(t).to(dev())
        copy = torch.full((SR.ROWS, V + 2), 7.0, device=dev())
        tlp, lse, tid, tl = ops.token_logprobs(xd[:, :V], td, copy=copy[:, :V] if k == 0 else None)
        assert tid is None and tl is None
        want = torch.zeros((SR.ROWS,), device=dev())
        for r in range(SR.ROWS):
            if 0 <= int(t[r]) < V:
                want[r] = y[r, int(t[r])]
        assert torch.equal(bits(tlp), bits(want)), (V, k, tlp, want)
        within(tlp, SR.target_logprobs(x[:, :V], t), f"target_lp V={V} targets {k}")
        within(lse, lse64, f"lse V={V}")
        assert float(lse[1]) == 0.0 and float(lse[2]) == 0.0                      # all -inf; a +inf maximum
        if k == 0:
            assert torch.equal(bits(copy[:, :V]), bits(orig[:, :V]))                # the raw row, NaN payloads included
            assert bool((copy[:, V:] == 7.0).all())
        assert torch.equal(bits(xd), bits(orig))                                    # read only; the poisoned padding as it was
    # outputs the call was not asked for are not written: n_top = 0 with buffers given, no target, no lse, no copy
    h = lib_score.load()
    sid = torch.full((SR.ROWS, 4), 12345, dtype=torch.int32, device=dev())
    slp = torch.full((SR.ROWS, 4), 5.5, device=dev())
    lse2 = torch.full((SR.ROWS,), 9.0, device=dev())
    s = torch.cuda.current_stream().cuda_stream
    assert h.vly_score_rows(xd.data_ptr(), V + SR.PAD, V, SR.ROWS, None, None, None, 0, sid.data_ptr(), slp.data_ptr(), None, 0, s) == 0
    assert bool((sid == 12345).all()) and bool((slp == 5.5).all()) and bool((lse2 == 9.0).all())
    assert h.vly_score_rows(xd.data_ptr(), V + SR.PAD, V, SR.ROWS, None, None, lse2.data_ptr(), 0, sid.data_ptr(), slp.data_ptr(), None, 0, s) == 0
    assert torch.equal(bits(lse2), bits(lse)) and bool((sid == 12345).all()) and bool((slp == 5.5).all())


@pytest.mark.parametrize("V", [64, 1025, 32769])
@pytest.mark.parametrize("n", [1, 5, 20])
def test_top_n_ids_exact_with_ties(n, V):
    from valley_amd import ops
    x = SR.ties_case(V)
    xd = torch.from_numpy(x).to(dev())
    _, lse, tid, tl = ops.token_logprobs(xd, top=n)
    ids, lps = SR.topn(x, n)
    assert np.array_equal(tid.cpu().numpy().astype(np.int64), ids), (n, V)
    got = tid.cpu()
    for r in range(x.shape[0]):
        k = int((got[r] >= 0).sum())
        assert k == min(n, int((~np.isnan(x[r])).sum()))
        want = xd[r, got[r, :k].long().to(dev())] - lse[r]                          # fp32 x[id] - lse: the same subtraction
        assert torch.equal(bits(tl[r, :k]), bits(want))
        assert bool((got[r, k:] == -1).all()) and bool(torch.isneginf(tl[r, k:]).all())
    within(tl, lps, f"top_lp n={n} V={V}")
    # rows of distinct values, with targets and the top-n in one call
    g = torch.Generator().manual_seed(n + V)
    z = (torch.randperm(4 * V, generator=g).float().view(4, V) * (8.0 / (4 * V))).to(dev())   # distinct, in [0, 8): |x| stays at |lp|'s scale
    t = torch.tensor([0, V - 1, -100, V // 2], dtype=torch.int32, device=dev())
    tlp, lse, tid, tl = ops.token_logprobs(z, t, top=min(n, V))
    tv, ti = torch.topk(z.double(), min(n, V), dim=-1)
    assert torch.equal(tid.long(), ti)
    within(tl, torch.log_softmax(z.double(), -1).gather(1, ti).cpu().numpy(), f"distinct top_lp n={n} V={V}")


def test_record_columns_guards_and_foreign_tokens():
    from valley_amd import ops
    R, V, ld, L, n = 4, 50, 53, 6, 3
    g = torch.Generator().manual_seed(3)
    raw = (torch.randn((R, ld), generator=g) * 3).to(dev())
    _, lse, tid, tl = ops.token_logprobs(raw[:, :V], top=n)
    tok = torch.tensor([3, -1, V, 49], dtype=torch.int32, device=dev())
    want_lp = torch.stack([raw[r, int(tok[r])] - lse[r] if 0 <= int(tok[r]) < V else torch.zeros((), device=dev()) for r in range(R)])

    def tables():
        flat = [torch.full(((R + 2) * L * k,), v, dtype=dt, device=dev()) for k, v, dt in
                ((1, 77.0, torch.float32), (n, 77, torch.int32), (n, 77.0, torch.float32))]
        views = [flat[0][L:(R + 1) * L].view(R, L), flat[1][L * n:(R + 1) * L * n].view(R, L, n), flat[2][L * n:(R + 1) * L * n].view(R, L, n)]
        return flat, views

    cases = [(torch.tensor([2], dtype=torch.int32), 0, [2] * R), (torch.tensor([2], dtype=torch.int32), 1, [3] * R),
             (torch.tensor([L], dtype=torch.int32), 0, [None] * R), (torch.tensor([0], dtype=torch.int32), -1, [None] * R),
             (torch.tensor([0, 5, L, -1], dtype=torch.int32), 0, [0, 5, None, None]),
             (torch.tensor([-1, 4, 5, -2], dtype=torch.int32), 1, [0, 5, None, None]), (None, 4, [4] * R)]
    for length, add, cols in cases:
        flat, (lp, ids, lps) = tables()
        ops.score_record(raw[:, :V], lse, tok, lp, None if length is None else length.to(dev()), add, top=(tid, tl), top_tables=(ids, lps))
        want = [torch.full_like(f, 77) for f in flat]
        wv = [want[0][L:(R + 1) * L].view(R, L), want[1][L * n:(R + 1) * L * n].view(R, L, n), want[2][L * n:(R + 1) * L * n].view(R, L, n)]
        for r, c in enumerate(cols):
            if c is not None:
                wv[0][r, c], wv[1][r, c], wv[2][r, c] = want_lp[r], tid[r], tl[r]
        for f, w in zip(flat, want):                                                # guard rows and every other cell included
            assert torch.equal(bits(f), bits(w)), (length, add)
    assert float(want_lp[1]) == 0.0 and float(want_lp[2]) == 0.0
    # without the top-n tables
    flat, (lp, _, _) = tables()
    ops.score_record(raw[:, :V], lse, tok, lp, None, 1)
    assert torch.equal(bits(lp[:, 1]), bits(want_lp)) and int((flat[0] != 77.0).sum()) == int((want_lp != 77.0).sum())


@pytest.mark.parametrize("M", [1, 7, 1024, 5000])
def test_loss_count_exact_one_ulp_and_repeatable(M):
    from valley_amd import ops
    V = 32000
    lp, t = SR.loss_case(M, V)
    lpd, td = torch.from_numpy(lp).to(dev()), torch.from_numpy(t).to(dev())
    loss, count = ops.nll_mean(lpd, td, V)
    want, n = SR.nll_mean(lp, t, V)
    assert int(count) == n and n > 0
    w32 = np.float32(want)
    print(f"loss M={M}: got {float(loss)!r}, float32(-mean64) {float(w32)!r}")
    assert abs(np.float64(loss.item()) - np.float64(w32)) <= np.spacing(np.abs(w32))
    again, _ = ops.nll_mean(lpd, td, V)
    assert torch.equal(bits(loss), bits(again))
    none = torch.where(td % 2 == 0, torch.full_like(td, -100), torch.full_like(td, V))
    loss, count = ops.nll_mean(lpd, none, V)
    assert int(count) == 0 and bool(torch.isnan(loss))


def test_cross_entropy_against_torch_float64():
    from valley_amd import ops
    g = torch.Generator().manual_seed(8)
    x = (torch.randn((300, 1003), generator=g) * 4).to(dev())
    t = torch.randint(0, 1000, (300,), generator=g)
    t[::4] = -100
    loss, count = ops.cross_entropy(x[:, :1000], t.to(torch.int32).to(dev()))
    want = torch.nn.functional.cross_entropy(x[:, :1000].double().cpu(), t, ignore_index=-100)
    assert int(count) == int((t != -100).sum())
    within(loss, float(want), "cross_entropy")


# ---- the golden model ------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def golden():
    from tests.test_model_gpu import build_golden_model
    return build_golden_model()


@pytest.fixture(scope="module")
def golden_int8():
    from tests.test_model_gpu import build_golden_model
    model = build_golden_model()
    model.quantize_decode_weights("int8")
    return model


def inputs(case):
    from tests.test_logits_process_gpu import inputs as f
    return f(case)


@pytest.mark.parametrize("case", ["one", "main"])
def test_forward_labels_is_cross_entropy_of_its_own_logits(golden, case):
    """With images; "main" is a padded batch of two.  Raised NotImplementedError before this feature."""
    model = golden
    ids, mask, img = inputs(case)
    labels = ids.clone()
    labels[mask == 0] = -100
    labels[:, 1:4] = -100
    out = model(input_ids=ids, images=img, attention_mask=mask, labels=labels)
    V = out.logits.shape[-1]
    want = torch.nn.functional.cross_entropy(out.logits[:, :-1].double().reshape(-1, V).cpu(), labels[:, 1:].reshape(-1).cpu(),
                                             ignore_index=-100)
    assert out.loss.dim() == 0 and out.loss.dtype == torch.float32
    within(out.loss, float(want), f"forward(labels) {case}")
    tup = model(input_ids=ids, images=img, attention_mask=mask, labels=labels, return_dict=False)
    assert torch.equal(bits(tup[0]), bits(out.loss)) and tup[1].shape == out.logits.shape
    assert model(input_ids=ids, images=img, attention_mask=mask).loss is None
    with pytest.raises(ValueError, match="labels"):
        model(input_ids=ids, images=img, attention_mask=mask, labels=labels[:, :-1])
    none = model(input_ids=ids, images=img, attention_mask=mask, labels=torch.full_like(ids, -100))
    assert bool(torch.isnan(none.loss))
    single = model(input_ids=ids[:1, :1], labels=ids[:1, :1])                        # nothing left after the shift
    assert bool(torch.isnan(single.loss)) and single.loss.dim() == 0


def test_score_sums_and_counts(golden):
    model = golden
    ids, mask, img = inputs("main")
    labels = ids.clone()
    labels[mask == 0] = -100
    res = model.score(ids, labels=labels, images=img, attention_mask=mask)
    B, S = ids.shape
    assert res.token_logprobs.shape == (B, S - 1) and res.token_logprobs.dtype == torch.float32
    assert torch.equal(res.count.cpu(), (labels[:, 1:] != -100).sum(1).cpu())
    assert torch.equal(bits(res.sum), bits(res.token_logprobs.double().sum(1).float()))
    assert bool((res.token_logprobs[labels[:, 1:] == -100] == 0).all())
    out = model(input_ids=ids, images=img, attention_mask=mask, labels=labels)
    want = torch.log_softmax(out.logits[:, :-1].double(), -1).gather(2, labels[:, 1:].clamp(min=0)[:, :, None])[:, :, 0]
    want = torch.where(labels[:, 1:] == -100, torch.zeros_like(want), want)
    within(res.token_logprobs, want.cpu().numpy(), "score token_logprobs")
    within(out.loss, float(-res.sum.double().sum() / res.count.sum()), "loss from score sums")
    every = model.score(ids, images=img, attention_mask=mask)                        # labels=None: every position
    assert torch.equal(every.count.cpu(), torch.full((B,), S - 1))


MODES = {"greedy": dict(), "sampled": dict(do_sample=True, temperature=0.9, top_k=5, top_p=0.9, seed=11),
         "processors": dict(repetition_penalty=1.3, no_repeat_ngram_size=2), "int8": dict()}


@pytest.mark.parametrize("mode", list(MODES))
def test_generate_logprobs_in_every_route(golden, golden_int8, mode):
    from tests import logits_ref
    from tests.test_logits_process_gpu import greedy_stepper
    model = golden_int8 if mode == "int8" else golden
    kw = MODES[mode]
    ids, mask, img = inputs("main")
    B, S = ids.shape
    new, n = 10, 3
    base = dict(images=img, attention_mask=mask, max_new_tokens=new, pad_token_id=0, **kw)
    plain = model.generate(ids, **base)
    eos = int(plain[0, S + 1])                                                       # row 0 ends after two tokens
    base["eos_token_id"] = eos
    outs = []
    for ug in (True, False, None):
        seq = model.generate(ids, use_graph=ug, **base)
        out = model.generate(ids, use_graph=ug, return_dict_in_generate=True, output_logprobs=True, top_logprobs=n, **base)
        assert torch.equal(out.sequences, seq), (mode, ug)
        assert hasattr(model.generate(ids, use_graph=ug, return_dict_in_generate=True, **base), "token_logprobs") is False
        outs.append(out)
    seq = outs[0].sequences
    m = seq.shape[1] - S
    assert int(seq[0, S + 1]) == eos and m > 2
    for o in outs:
        assert o.token_logprobs.shape == (B, m) and o.top_tokens.shape == (B, m, n) and o.top_logprobs.shape == (B, m, n)
        assert torch.equal(o.sequences, seq)
        assert torch.equal(bits(o.token_logprobs), bits(outs[0].token_logprobs)), mode
        assert torch.equal(o.top_tokens, outs[0].top_tokens) and torch.equal(bits(o.top_logprobs), bits(outs[0].top_logprobs)), mode
    o = outs[0]
    # the teacher-forced forward: the prompt, then the sequence token by token
    step = greedy_stepper(model, ids, mask, img)
    procs = logits_ref.hf_processors(kw.get("repetition_penalty"), kw.get("no_repeat_ngram_size"), None, None, prompt_len=S, eos=[eos])
    done = torch.zeros((B,), dtype=torch.bool, device=dev())
    differs, lives = 0, []
    for j in range(m):
        lives.append(~done)
        logits = step(None if j == 0 else seq[:, S + j - 1])
        tok = seq[:, S + j]
        ls = torch.log_softmax(logits.double(), -1)
        want = torch.where(done, torch.zeros((B,), dtype=torch.float64, device=dev()), ls.gather(1, tok[:, None])[:, 0])
        within(o.token_logprobs[:, j], want.cpu().numpy(), f"{mode} token {j}")
        tv, ti = torch.topk(logits.double(), n, dim=-1)
        live = ~done
        assert torch.equal(o.top_tokens[live, j].long(), ti[live]), (mode, j)
        within(o.top_logprobs[live, j], ls.gather(1, ti)[live].cpu().numpy(), f"{mode} top {j}")
        assert bool((o.top_tokens[done, j] == -1).all()) and bool((o.top_logprobs[done, j] == 0).all())
        assert bool((o.token_logprobs[done, j] == 0).all())
        if len(procs):                                                               # the processed distribution is another one
            proc = procs(seq[:, :S + j].cpu(), logits.cpu().clone())
            lp = torch.log_softmax(proc.double(), -1).gather(1, tok.cpu()[:, None])[:, 0]
            differs += int(((lp - want.cpu()).abs()[live.cpu()] > 1e-3).sum())
        if mode in ("greedy", "int8"):                                               # the argmax is the most probable token
            assert torch.equal(o.top_tokens[live, j, 0].long(), tok[live])
            assert torch.equal(bits(o.top_logprobs[live, j, 0]), bits(o.token_logprobs[live, j]))
        done = done | (tok == eos)
    assert bool(done[0]) and bool((o.token_logprobs[0, 2:] == 0).all())
    if mode != "int8":                                                               # one forward over the whole sequence
        full = model(input_ids=seq[:, :-1], images=img,
                     attention_mask=torch.cat([mask, torch.ones((B, m - 1), dtype=mask.dtype, device=mask.device)], 1))
        ls = torch.log_softmax(full.logits[:, S - 1:S - 1 + m].double(), -1)
        want = ls.gather(2, seq[:, S:][:, :, None])[:, :, 0]
        live = torch.stack(lives, dim=1)
        err = float((o.token_logprobs.double() - want).abs()[live].max())
        print(f"{mode}: against one whole-sequence forward max |d lp| {err:.3e} (bound {WHOLE:.1e})")
        assert err <= WHOLE, (mode, err)
    if mode == "processors":
        assert differs > 0, "the processors never changed a chosen token's probability: the raw copy is not exercised"
    if mode == "greedy":
        with pytest.raises(ValueError, match="num_beams"):
            model.generate(ids, num_beams=2, return_dict_in_generate=True, output_logprobs=True, **base)
        with pytest.raises(ValueError, match="return_dict_in_generate"):
            model.generate(ids, output_logprobs=True, **base)
        zero = model.generate(ids, return_dict_in_generate=True, output_logprobs=True, **base)   # top_logprobs = 0
        assert torch.equal(bits(zero.token_logprobs), bits(o.token_logprobs)) and not hasattr(zero, "top_tokens")


@pytest.mark.parametrize("procs", [dict(no_repeat_ngram_size=2), dict()])
@pytest.mark.parametrize("ug", [True, False, None])
def test_generate_host_multinomial_records_the_drawn_token(golden, ug, procs):
    """Sampling without top-k / top-p / seed draws on the host: the recorded value is the drawn token's, in every route, with
    processors (the session records from its raw copy) and without (it reads the step's logits directly)."""
    from tests.test_logits_process_gpu import greedy_stepper
    model = golden
    ids, mask, img = inputs("main")
    S = ids.shape[1]
    kw = dict(images=img, attention_mask=mask, max_new_tokens=5, do_sample=True, temperature=1.5, use_graph=ug, **procs)
    torch.manual_seed(5)
    out = model.generate(ids, return_dict_in_generate=True, output_logprobs=True, top_logprobs=2, **kw)
    torch.manual_seed(5)
    seq = model.generate(ids, **kw)
    assert torch.equal(out.sequences, seq) and out.token_logprobs.shape == (ids.shape[0], 5)
    step = greedy_stepper(model, ids, mask, img)
    for j in range(seq.shape[1] - S):
        logits = step(None if j == 0 else seq[:, S + j - 1])
        ls = torch.log_softmax(logits.double(), -1)
        within(out.token_logprobs[:, j], ls.gather(1, seq[:, S + j][:, None])[:, 0].cpu().numpy(), f"multinomial {ug} {procs} token {j}")
        ti = torch.topk(logits.double(), 2, dim=-1).indices
        assert torch.equal(out.top_tokens[:, j].long(), ti)
        within(out.top_logprobs[:, j], ls.gather(1, ti).cpu().numpy(), f"multinomial {ug} {procs} top {j}")


def teacher_forced(model, ids, mask, img, seq):
    """log_softmax float64 [B, new, V] of forward() fed ``seq``: the prompt, then one token per call on the KV cache"""
    from tests.test_logits_process_gpu import greedy_stepper
    S = ids.shape[1]
    step = greedy_stepper(model, ids, mask, img)
    return torch.stack([torch.log_softmax(step(None if j == 0 else seq[:, S + j - 1]).double(), -1) for j in range(seq.shape[1] - S)], 1)


def test_generate_up_to_the_cache_limit_in_every_route(golden, monkeypatch):
    """S + max_new_tokens beyond the model's positions: the last step runs at the cache's last position and its token has
    index ctx_max — the last column of the session's tables."""
    model = golden
    ids, mask, img = inputs("main")
    B, S = ids.shape
    monkeypatch.setattr(model.config, "max_position_embeddings", S + 4)
    kw = dict(images=img, attention_mask=mask, max_new_tokens=8)
    outs = []
    for ug in (True, False, None):
        seq = model.generate(ids, use_graph=ug, **kw)
        out = model.generate(ids, use_graph=ug, return_dict_in_generate=True, output_logprobs=True, top_logprobs=2, **kw)
        assert torch.equal(out.sequences, seq) and seq.shape[1] == S + 5, (ug, seq.shape)
        assert out.token_logprobs.shape == (B, 5) and out.top_tokens.shape == (B, 5, 2)
        outs.append(out)
    for o in outs[1:]:
        assert torch.equal(o.sequences, outs[0].sequences) and torch.equal(bits(o.token_logprobs), bits(outs[0].token_logprobs))
        assert torch.equal(o.top_tokens, outs[0].top_tokens) and torch.equal(bits(o.top_logprobs), bits(outs[0].top_logprobs))
    seq = outs[0].sequences
    ls = teacher_forced(model, ids, mask, img, seq)
    within(outs[0].token_logprobs, ls.gather(2, seq[:, S:][:, :, None])[:, :, 0].cpu().numpy(), "cache limit")
    assert torch.equal(outs[0].top_tokens[:, :, 0].long(), seq[:, S:])                # greedy: the last token's row included
    assert torch.equal(bits(outs[0].top_logprobs[:, :, 0]), bits(outs[0].token_logprobs))


@pytest.mark.parametrize("ug", [True, False])
def test_session_tables_grow_with_the_cache(golden, ug):
    """A growable cache with logprobs: the tables follow it (copy, capture again) and the columns recorded before survive.
    Every step's record is checked against float64 log_softmax of that step's own logits (greedy, no processors: the step
    leaves them as the lm_head wrote them).  A one-row session is not compared with the generic forward: the project holds
    those two to 2e-2 of each other, not to fp32 rounding (tests/test_model_gpu.py)."""
    from valley_amd.decode import DecodeSession
    model = golden
    ll = model.get_model().llama
    ids, mask, img = inputs("one")
    S, n = ids.shape[1], 9
    cache = ll.new_cache(1, S + 3)
    cache.growable, cache.limit = True, S + 40
    out = model(input_ids=ids, images=img, attention_mask=mask, past_key_values=cache, use_cache=True)
    sess = DecodeSession(ll, cache, use_graph=ug, logprobs=2)
    assert sess.lp_table.shape == (1, S + 4)
    tok = out.logits[:, -1].argmax(-1)
    sess.begin(tok)
    toks, snaps, widths, want, want_top = [tok.clone()], [], set(), [], []
    for i in range(n):
        toks.append(sess.step().long().clone())
        ls = torch.log_softmax(sess.logits[:, :ll.V].double(), -1)
        assert torch.equal(toks[-1], ls.argmax(-1))
        want.append(ls.gather(1, toks[-1][:, None])[:, 0])
        want_top.append(torch.topk(ls, 2, dim=-1))
        widths.add(sess.lp_table.shape[1])
        assert sess.lp_table.shape[1] == cache.ctx_max + 1 and sess.lp_top_tables[0].shape[1] == cache.ctx_max + 1
        snaps.append([t[:, S + 1:S + 2 + i].clone() for t in (sess.lp_table,) + sess.lp_top_tables])
    sess.check()
    assert len(widths) > 1 and cache.ctx_max > S + 3, "the cache never grew: the test covers nothing"
    for i, snap in enumerate(snaps):                                                  # what a step recorded is there at the end
        for t, t0 in zip((sess.lp_table,) + sess.lp_top_tables, snap):
            assert torch.equal(bits(t[:, S + 1:S + 2 + i]), bits(t0)), i
    within(sess.lp_table[:, S + 1:S + 1 + n], torch.stack(want, 1).cpu().numpy(), f"grown tables {ug}")
    assert torch.equal(sess.lp_top_tables[0][:, S + 1:S + 1 + n].long(), torch.stack([t.indices for t in want_top], 1))
    within(sess.lp_top_tables[1][:, S + 1:S + 1 + n], torch.stack([t.values for t in want_top], 1).cpu().numpy(), f"grown top {ug}")
    assert bool((sess.lp_table[:, S + 1 + n:] == 0).all()) and bool((sess.lp_top_tables[0][:, S + 1 + n:] == -1).all())


def test_batcher_slot_filled_to_ctx_max(golden):
    """A slot that runs until its cache rows are full: its last token has index ctx_max, and its own log-probability."""
    from valley_amd.serving import ContinuousBatcher
    model = golden
    ids, mask, img = inputs("one")
    assert bool(mask.all())
    S = ids.shape[1]
    cb = ContinuousBatcher(model, slots=2, ctx_max=S + 3, logprobs=2)
    slot = cb.add(ids, images=img)
    toks, lps = [int(cb.sess.tok[slot])], [cb.first_logprobs[slot]]
    for _ in range(6):
        got = cb.step()
        if slot not in got:
            break
        toks.append(got[slot])
        lps.append(cb.last_logprobs[slot])
    assert cb.full == [slot] and len(toks) == 4                                       # indices S .. S + 3 = ctx_max
    seq = torch.cat([ids, torch.tensor([toks], device=dev())], 1)
    ls = teacher_forced(model, ids, mask, img, seq)
    want = ls.gather(2, seq[:, S:][:, :, None])[0, :, 0].cpu().numpy()
    within(torch.tensor([v[0] for v in lps]), want, "batcher to ctx_max")
    assert [v[1][0] for v in lps] == toks                                             # greedy: the top id is the token
    assert all(np.float32(v[0]).tobytes() == np.float32(v[2][0]).tobytes() for v in lps)
    row = cb.sess.lp_table[slot, S:S + 4].cpu()
    assert torch.equal(bits(row), bits(torch.tensor([v[0] for v in lps], dtype=torch.float32)))


def test_session_refuses_beams_and_the_persistent_step(golden, monkeypatch):
    from valley_amd import decode
    ll = golden.get_model().llama
    with pytest.raises(ValueError, match="beam"):
        decode.DecodeSession(ll, ll.new_cache(4, 64), beams=(2, 2, 8, [2]), logprobs=1)
    with pytest.raises(ValueError, match="logprobs must be in"):
        decode.DecodeSession(ll, ll.new_cache(1, 64), logprobs=21)
    monkeypatch.setattr(decode, "PERSISTENT", True)
    with pytest.raises(ValueError, match="persistent"):
        decode.DecodeSession(ll, ll.new_cache(1, 64), logprobs=1)


def test_batcher_logprobs_equal_the_request_served_alone(golden):
    from valley_amd.serving import ContinuousBatcher
    model = golden
    T = G.GCFG["T"]
    img = torch.from_numpy(G.golden_pixels(T, "mixed")).view(1, T, 3, 224, 224).cuda()
    reqs = [torch.from_numpy(G.golden_ids(c)[0]).cuda() for c in ("decode2", "decode", "decode2")]
    join, steps = [0, 2, 3], 8                                                       # request k joins before step join[k]

    def serve(plan, logprobs, slots=4):
        """plan: [(request index, joining step)] -> per request (tokens, [(lp, ids, lps)])"""
        cb = ContinuousBatcher(model, slots=slots, ctx_max=512, **({} if logprobs is None else {"logprobs": logprobs}))
        got = {}
        for s in range(steps):
            for k, at in plan:
                if at == s:
                    slot = cb.add(reqs[k], images=img)
                    got[k] = (slot, [int(cb.sess.tok[slot])], [cb.first_logprobs[slot]] if logprobs is not None else [])
            toks = cb.step()
            for k, (slot, tk, lp) in got.items():
                tk.append(toks[slot])
                if logprobs is not None:
                    lp.append(cb.last_logprobs[slot])
        if logprobs is not None:                                                    # the slot's table row keeps them all
            for k, (slot, tk, lp) in got.items():
                S = reqs[k].shape[1]
                row = cb.sess.lp_table[slot, S:S + len(lp)].cpu()
                assert torch.equal(bits(row), bits(torch.tensor([v[0] for v in lp], dtype=torch.float32)))
        return {k: (tk, lp) for k, (slot, tk, lp) in got.items()}

    together = serve(list(zip(range(3), join)), 2)
    plain = serve(list(zip(range(3), join)), None)
    for k in range(3):
        assert together[k][0] == plain[k][0], k                                      # tokens unchanged by the switch
        alone = serve([(k, 0)], 2)[k]                                                    # slot 0, idle neighbours
        m = len(together[k][0])
        assert alone[0][:m] == together[k][0]
        for a, b in zip(alone[1][:m], together[k][1]):
            assert np.float32(a[0]).tobytes() == np.float32(b[0]).tobytes(), (k, a, b)
            assert a[1] == b[1] and np.asarray(a[2], dtype=np.float32).tobytes() == np.asarray(b[2], dtype=np.float32).tobytes(), (k, a, b)
        assert all(len(v[1]) == 2 and v[1][0] == t for v, t in zip(together[k][1], together[k][0]))   # greedy: the top id is the token


def test_plain_generate_never_maps_the_library():
    env = {k: v for k, v in os.environ.items() if k not in ("VALLEY_PRECISION", "VALLEY_WEIGHT_QUANT", "VALLEY_HIP_SCORE_LIB")}
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "score_worker.py")], capture_output=True, text=True, env=env,
                       timeout=600)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    res = json.loads(p.stdout.strip().splitlines()[-1])
    assert res["ok"] and res["new_tokens"] == 4 and res["same"] and not res["has_logprobs"]
    assert res["score_lib_loaded"] is False and res["score_lib_mapped"] is False
