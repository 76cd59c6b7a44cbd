"""Beam search on the MI355X: vly_beam_candidates / vly_beam_select against torch (fp64 scores), vly_kv_beam_reorder
bit-exact against index_select (in place, in a captured graph), the beam decode session captured against eager, and
generate(num_beams=...) end to end on the golden model against a plain-torch beam search."""
import json
import os
import subprocess
import sys

import pytest
import torch

from tests import golden_cfg as G

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def dev():
    return torch.device("cuda:0")


# ---- candidates / select ------------------------------------------------------------------------------------------------

def ref_candidates(logits, running, B, nb, K, eos):
    """fp64 log_softmax over the non-NaN logits + running; per prompt the K best, ties to the lower flat index."""
    x = logits.double().cpu()
    R, V = x.shape
    nan = torch.isnan(x)
    lse = torch.logsumexp(torch.where(nan, torch.full_like(x, -float("inf")), x), dim=-1, keepdim=True)
    acc = x - lse + running.double().cpu()[:, None]
    acc = torch.where(nan, torch.full_like(acc, -float("inf")), acc)
    flat = acc.view(B, nb * V)
    order = torch.sort(flat, dim=1, descending=True, stable=True)[1][:, :K]
    score = torch.take_along_dim(flat, order, 1)
    token = order % V
    beam = order // V + torch.arange(B)[:, None] * nb
    hit = torch.isin(token, torch.tensor(eos, dtype=torch.long)) if eos else torch.zeros_like(token, dtype=torch.bool)
    return score.reshape(-1), token.reshape(-1), beam.reshape(-1), hit.reshape(-1)


def ref_select(score, token, beam, hit, B, nb):
    K = score.numel() // B
    v = (score.float() + hit.float() * -1.0e9).view(B, K)
    order = torch.sort(v, dim=1, descending=True, stable=True)[1][:, :nb]
    return (torch.take_along_dim(token.view(B, K), order, 1).reshape(-1), torch.take_along_dim(beam.view(B, K), order, 1).reshape(-1),
            torch.take_along_dim(v, order, 1).reshape(-1))


def run_candidates(logits, running, B, nb, eos):
    from valley_amd import ops
    K = ops.beam_k(nb, len(eos))
    eos_t = torch.tensor(eos, dtype=torch.int32, device=dev()) if eos else None
    scratch = ops.beam_scratch(B, nb, K, dev())
    out = ops.beam_candidates(logits, running, B, nb, K, eos_t, scratch)
    out2 = ops.beam_candidates(logits, running, B, nb, K, eos_t, scratch)      # the tickets are back at zero: same answer
    for a, b in zip(out, out2):
        assert torch.equal(a, b)
    return K, out


@pytest.mark.parametrize("V,ld", [(32000, 32000), (32006, 32008), (97, 97)])
@pytest.mark.parametrize("B", [1, 2])
@pytest.mark.parametrize("nb", [1, 2, 4, 8])
@pytest.mark.parametrize("n_eos", [0, 1, 2])
def test_candidates_and_select_against_torch(V, ld, B, nb, n_eos):
    from valley_amd import ops
    g = torch.Generator().manual_seed(V + 10 * B + 100 * nb + n_eos)
    R = B * nb
    buf = torch.randn((R, ld), generator=g) * 3.0
    buf[0, : V // 7] = -float("inf")                       # -inf logits are allowed
    if V > 1000:
        buf[R - 1, 11:40] = float("nan")                   # NaN is never selected
    logits = buf.to(dev())[:, :V]
    eos = [int(t) for t in torch.randint(0, V, (n_eos,), generator=g)]
    for first in (True, False):
        running = torch.zeros(R) if first else torch.randn(R, generator=g) * 2 - 5
        if first:
            running.view(B, nb)[:, 1:] = -1e9              # the first step's pattern
        if eos and not first:                              # make the EOS ids competitive
            buf2 = buf.clone()
            buf2[:, eos] = buf2[:, :V].nan_to_num(nan=-1e30).max(-1, keepdim=True)[0] - 0.1
            logits = buf2.to(dev())[:, :V]
        K, (score, token, beam, hit) = run_candidates(logits, running.to(dev()), B, nb, eos)
        rs, rt, rb, rh = ref_candidates(logits, running, B, nb, K, eos)
        assert token.cpu().long().tolist() == rt.tolist()
        assert beam.cpu().long().tolist() == rb.tolist()
        assert hit.cpu().bool().tolist() == rh.tolist()
        assert float((score.cpu().double() - rs).abs().max()) < 2e-5
        tok, parent, run = ops.beam_select(score, token, beam, hit, B, nb)
        et, eb, ev = ref_select(score.cpu(), token.cpu(), beam.cpu(), hit.cpu(), B, nb)
        assert torch.equal(tok.cpu(), et) and torch.equal(parent.cpu(), eb) and torch.equal(run.cpu(), ev)


def test_candidates_exact_ties_go_to_the_lower_flat_index():
    B, nb, V = 1, 4, 5000
    g = torch.Generator().manual_seed(3)
    row = torch.randn(V, generator=g)
    row[9] = row[4] = row.max() + 1.0                        # a tie inside a row
    logits = row.repeat(nb, 1).to(dev())                     # and every row equal: ties across beams
    running = torch.zeros(nb, device=dev())
    K, (score, token, beam, hit) = run_candidates(logits, running, B, nb, [])
    _, rt, rb, _ = ref_candidates(logits, running, B, nb, K, [])
    assert token.cpu().long().tolist() == rt.tolist() and beam.cpu().long().tolist() == rb.tolist()
    # flat index j * V + t: beam 0's two tied tokens first, then beam 1's, ...
    assert token.cpu().tolist()[:8] == [4, 9] * 4 and beam.cpu().tolist()[:8] == [0, 0, 1, 1, 2, 2, 3, 3]


def test_select_with_a_host_hit_mask_finishing_most_candidates():
    from valley_amd import ops
    B, nb, K = 2, 4, 8
    g = torch.Generator().manual_seed(4)
    score = torch.sort(torch.randn(B, K, generator=g) - 3, dim=1, descending=True)[0].reshape(-1)
    token = torch.randint(0, 1000, (B * K,), generator=g, dtype=torch.int32)
    beam = (torch.randint(0, nb, (B, K), generator=g) + torch.arange(B)[:, None] * nb).reshape(-1).to(torch.int32)
    hit = torch.ones(B * K, dtype=torch.uint8)
    hit[5] = 0                                               # prompt 0: one survivor, seven hits (more than K - nb)
    hit[K + 7] = 0                                           # prompt 1: the last candidate survives
    d = [t.to(dev()) for t in (score, token, beam, hit)]
    tok, parent, run = ops.beam_select(*d, B, nb)
    et, eb, ev = ref_select(score, token, beam, hit, B, nb)
    assert torch.equal(tok.cpu(), et) and torch.equal(parent.cpu(), eb) and torch.equal(run.cpu(), ev)
    assert int(tok[0]) == int(token[5]) and int(tok[nb]) == int(token[K + 7])


# ---- KV reorder ---------------------------------------------------------------------------------------------------------

def parent_maps(R, g):
    m = {"identity": list(range(R)), "swap": [1, 0] + list(range(2, R)), "cycle3": [1, 2, 0] + list(range(3, R)),
         "all_from_one": [R // 2] * R, "random": torch.randint(0, R, (R,), generator=g).tolist()}
    return m


def make_caches(L, R, heads, ctx, dtype, g):
    def one():
        t = torch.randn((R, heads, ctx, 128), generator=g) * 4
        return t.to(dtype).to(dev()) if dtype != torch.int32 else t.to(dev())
    return [one() for _ in range(L)], [one() for _ in range(L)]


def expected(orig, parent, lo, hi):
    out = orig.clone()
    for r, p in enumerate(parent):
        if p != r:
            out[r, :, lo:hi] = orig[p, :, lo:hi]
    return out


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("R", [4, 8, 12])
def test_kv_reorder_bit_exact(dtype, R):
    from valley_amd import ops
    g = torch.Generator().manual_seed(R)
    L, heads, ctx = 3, 5, 77
    ks, vs = make_caches(L, R, heads, ctx, dtype, g)
    table = ops.kv_beam_table(ks, vs, dev())
    for name, parent in parent_maps(R, g).items():
        for lo, hi in ((0, 77), (13, 50), (40, 41)):
            k0, v0 = [t.clone() for t in ks], [t.clone() for t in vs]
            p = torch.tensor(parent, dtype=torch.int32, device=dev())
            pos = torch.tensor([hi - 2], dtype=torch.int32, device=dev())
            ops.kv_beam_reorder(table, ks[0], p, lo, 2, pos_dev=pos)
            torch.cuda.synchronize()
            for a, a0 in zip(ks + vs, k0 + v0):
                want = expected(a0, parent, lo, hi)
                assert torch.equal(a.view(torch.int16 if dtype == torch.bfloat16 else torch.int32),
                                   want.view(torch.int16 if dtype == torch.bfloat16 else torch.int32)), (name, lo, hi)
            # the torch form of the same thing: index_select on [lo, hi); rows with parent == r and other positions untouched
            idx = torch.tensor(parent, device=dev())
            for a, a0 in zip(ks, k0):
                assert torch.equal(a[:, :, lo:hi], a0[:, :, lo:hi].index_select(0, idx))
                assert torch.equal(a[:, :, :lo], a0[:, :, :lo]) and torch.equal(a[:, :, hi:], a0[:, :, hi:])
            ks, vs = [t.copy_(t0) for t, t0 in zip(ks, k0)], [t.copy_(t0) for t, t0 in zip(vs, v0)]


def test_kv_reorder_in_a_captured_graph():
    from valley_amd import ops
    g = torch.Generator().manual_seed(9)
    L, R, heads, ctx, lo = 2, 8, 4, 64, 10
    ks, vs = make_caches(L, R, heads, ctx, torch.bfloat16, g)
    table = ops.kv_beam_table(ks, vs, dev())
    parent = torch.tensor([3, 3, 0, 1, 7, 6, 5, 4], dtype=torch.int32, device=dev())
    pos = torch.tensor([lo], dtype=torch.int32, device=dev())
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        ops.kv_beam_reorder(table, ks[0], parent, lo, 1, pos_dev=pos)         # warm-up outside capture
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ops.kv_beam_reorder(table, ks[0], parent, lo, 1, pos_dev=pos)
    for p in (12, 40, 5, 63, 70):
        k0 = [t.clone() for t in ks + vs]
        pos.fill_(p)
        graph.replay()
        torch.cuda.synchronize()
        hi = min(p + 1, ctx)
        for a, a0 in zip(ks + vs, k0):
            assert torch.equal(a.view(torch.int16), expected(a0, parent.tolist(), lo, max(hi, lo)).view(torch.int16)), p


# ---- the beam decode session -----------------------------------------------------------------------------------------------

def beam_session_run(use_graph, B=2, nb=4, steps=8, eos=(17,)):
    from valley_amd import ops
    from valley_amd.decode import DecodeSession
    from valley_amd.llama import HipKVCache, HipLlama
    ll = HipLlama(1024, 8, 2752, 2, 32006, 1e-5).init_random(seed=5)       # the small Llama of tests/test_sampling_gpu.py
    g = torch.Generator(device="cuda").manual_seed(21)
    S, R = 40, B * nb
    cache = ll.new_cache(R, S + steps + 2)
    h = torch.randn((B * S, ll.H), generator=g, device="cuda") * 0.02
    x = ll.forward(h, B, S, HipKVCache.rows_of(cache, 0, B))
    table = ops.kv_beam_table(cache.k, cache.v, dev())
    ops.kv_beam_reorder(table, cache.k[0], torch.arange(R, dtype=torch.int32, device=dev()) // nb, 0, S)
    cache.seq_len = S
    logits = ll.logits(x.view(B, S, -1)[:, -1].contiguous()).repeat_interleave(nb, 0).contiguous()
    running = torch.zeros((B, nb), device=dev())
    running[:, 1:] = -1e9
    K = ops.beam_k(nb, len(eos))
    eos_t = torch.tensor(eos, dtype=torch.int32, device=dev())
    cand = ops.beam_candidates(logits, running.view(-1), B, nb, K, eos_t, ops.beam_scratch(B, nb, K, dev()))
    sess = DecodeSession(ll, cache, use_graph=use_graph, beams=(B, nb, S, list(eos)))
    ops.beam_select(*cand, B, nb, tok=sess.tok, parent=sess.parent, running=sess.running)
    sess.begin(sess.tok.clone())
    rec = []
    for _ in range(steps):
        sess.step()
        rec.append(torch.cat([sess.tok.clone(), sess.parent.clone(), sess.running.clone().view(torch.int32)]))
    torch.cuda.synchronize()
    sess.check()
    return torch.stack(rec).cpu(), sess


def test_beam_session_graph_equals_eager():
    a, sg = beam_session_run(True)
    b, _ = beam_session_run(False)
    assert sg.graph is not None
    assert torch.equal(a, b)
    R = 8
    parents = a[:, R:2 * R]
    assert bool((parents != torch.arange(R)).any())        # the beams did move between rows


# ---- generate() end to end ---------------------------------------------------------------------------------------------------

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


def torch_beam(model, ids, mask, img, nb, max_new, eos=None, criteria=(), lp=1.0, es=False, nrs=1):
    """Plain-torch beam search: every prompt repeated nb times through model.forward, torch log_softmax / topk for the
    candidates, the KV cache reordered with index_select; valley_amd.beam (checked against transformers on the CPU) keeps the
    hypotheses."""
    from valley_amd.beam import BeamSearch
    B, S = ids.shape
    R = B * nb
    st = BeamSearch(ids, nb, S + max_new, eos_ids=None if eos is None else [eos], pad_token_id=0, length_penalty=lp,
                    early_stopping=es, num_return_sequences=nrs)
    rep = lambda t: t.repeat_interleave(nb, 0)                # noqa: E731
    out = model(input_ids=rep(ids), images=rep(img), attention_mask=rep(mask), use_cache=True)
    cache = out.past_key_values
    running = st.initial_running().cuda()
    while True:
        logits = out.logits[:, -1, :].float()
        V = logits.shape[-1]
        acc = (torch.log_softmax(logits, -1) + running[:, None]).view(B, nb * V)
        score, idx = torch.topk(acc, st.K)
        parent = idx // V + torch.arange(B, device=idx.device)[:, None] * nb
        seqs = st.candidates(score.reshape(-1), (idx % V).reshape(-1), parent.reshape(-1))
        hits = st.eos_hits()
        for c in criteria:
            r = c(seqs.cuda(), None)
            hits = hits | (r.cpu() if isinstance(r, torch.Tensor) else torch.full_like(hits, bool(r)))
        st.advance(hits)
        if st.done:
            break
        p = st.run_ptr[:, :, st.cur_len - 1 - S].reshape(-1).long().cuda()
        for t in cache.k + cache.v:
            t.copy_(t.index_select(0, p))
        running = st.run_score.reshape(-1).cuda()
        out = model(input_ids=st.run_seq[:, :, st.cur_len - 1].reshape(R, 1).cuda(), past_key_values=cache, use_cache=True)
    seq, sc = st.result()
    return seq.cuda(), sc


@pytest.mark.parametrize("case", ["one", "main"])
def test_generate_beams_matches_torch_reference(case):
    model = golden_model()
    ids, mask, img = inputs(case)
    kw = dict(images=img, attention_mask=mask, max_new_tokens=6)
    ref, ref_sc = torch_beam(model, ids, mask, img, 4, 6)
    outs = [model.generate(ids, num_beams=4, use_graph=ug, return_dict_in_generate=True, **kw) for ug in (True, False, None)]
    for o in outs:
        assert torch.equal(o.sequences, outs[0].sequences)
        assert o.sequences_scores.shape == (ids.shape[0],)
    assert torch.equal(outs[0].sequences, ref)
    assert float((outs[2].sequences_scores - ref_sc).abs().max()) < 1e-3
    # beam search is not greedy decoding: the four hypotheses are distinct, and num_beams=1 is today's greedy output
    all4, _ = torch_beam(model, ids, mask, img, 4, 6, nrs=4)
    greedy = model.generate(ids, **kw)
    assert len({tuple(r.tolist()) for r in all4}) == all4.shape[0]
    assert any(not torch.equal(r[:greedy.shape[1]], greedy[i // 4]) for i, r in enumerate(all4))
    assert torch.equal(model.generate(ids, num_beams=1, **kw), greedy)
    two = model.generate(ids, num_beams=4, num_return_sequences=2, **kw)
    assert two.shape[0] == 2 * ids.shape[0] and torch.equal(two[::2], outs[0].sequences)


def test_generate_beams_with_eos_and_keyword_criterion():
    from tests.fake_tokenizer import FakeTokenizer
    from valley_amd.video import KeywordsStoppingCriteria
    model = golden_model()
    ids, mask, img = inputs("main")
    n_in = ids.shape[1]
    all4, _ = torch_beam(model, ids, mask, img, 4, 6, nrs=4)
    eos = int(all4[1, n_in + 2])                             # a token some hypothesis emits: EOS is reached
    kw = dict(images=img, attention_mask=mask, max_new_tokens=6)
    ref, _ = torch_beam(model, ids, mask, img, 4, 6, eos=eos)
    for ug in (True, None):
        got = model.generate(ids, num_beams=4, eos_token_id=eos, pad_token_id=0, use_graph=ug, **kw)
        assert torch.equal(got, ref), ug
    tok = FakeTokenizer(vocab_text=10 ** 6)
    word = f"w{int(all4[0, n_in + 1])}"
    ref, _ = torch_beam(model, ids, mask, img, 4, 6, criteria=[KeywordsStoppingCriteria([word], tok, ids)])
    for ug in (True, False):
        got = model.generate(ids, num_beams=4, stopping_criteria=[KeywordsStoppingCriteria([word], tok, ids)], use_graph=ug, **kw)
        assert torch.equal(got, ref), ug


def test_generate_beams_generic_path_for_twelve_rows():
    model = golden_model()
    ids, mask, img = inputs("main")
    ids3 = torch.cat([ids, ids[:1]])
    mask3 = torch.cat([mask, mask[:1]])
    img3 = torch.cat([img, img[:1]])
    got = model.generate(ids3, images=img3, attention_mask=mask3, max_new_tokens=4, num_beams=4)
    ref, _ = torch_beam(model, ids3, mask3, img3, 4, 4)
    assert got.shape[0] == 3 and torch.equal(got, ref)
    assert torch.equal(got[2], got[0])                       # the repeated prompt: the same answer in another row


def test_generate_beams_argument_errors():
    model = golden_model()
    ids, mask, img = inputs("one")
    with pytest.raises(ValueError):
        model.generate(ids, images=img, num_beams=2, do_sample=True, max_new_tokens=2)
    with pytest.raises(ValueError):
        model.generate(ids, images=img, num_beams=2, num_return_sequences=3, max_new_tokens=2)


def test_generate_beams_fp16_library():
    env = dict(os.environ, VALLEY_PRECISION="fp16")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "beam_fp16_worker.py")], env=env, capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    res = json.loads(r.stdout.strip().splitlines()[-1])
    assert res["library"] == "libvalley_hip_f16.so"
    assert res["graph_equals_reference"] and res["generic_equals_reference"]
