"""Classifier-free guidance on the MI355X: vly_guide_apply / vly_guide_follow against the reference of tests/guide_ref.py (pinned to
transformers by tests/test_guide_cpu.py) — bit for bit over the device's own log-softmax, and within the project's log-sum-exp
bound of float64 — a captured launch replayed with a rewritten table, and generate() / ContinuousBatcher end to end on the golden
model against the reference loop over the HIP forward's logits."""
import os
import subprocess
import sys

import pytest
import torch

from tests import constrain_ref as CR
from tests import golden_cfg as G
from tests import guide_ref as GR
from tests import logits_ref
from tests.test_logits_process_gpu import greedy_stepper, inputs

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEG_INF = float("-inf")
REL = 1e-6                                                    # tests/test_score_gpu.py's bound for this row_lse, per unit of scale
SCALES = [1.5, 3.0, 0.5, -1.0, 1.0]
BETAS = [0.0, 0.1, 1.0]


def dev():
    return torch.device("cuda:0")


def scores(R, V, ld, seed, special=True):
    """Random logits; where they fit, a NaN, a -inf and a -0.0 per row at columns that differ from row to row (so a pair sees each
    of them in either row alone and, at column 5, in both); NaN in the padding columns."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn((R, ld), generator=g) * 3
    x[:, V:] = float("nan")
    if special and V > 40:
        for r in range(R):
            x[r, 7 + r], x[r, 20 + r], x[r, 30 + r], x[r, 5] = NEG_INF, -0.0, float("nan"), (NEG_INF if r % 2 else float("nan"))
    return x


def device_log_softmax(x):
    """vly_logits_process(log_softmax = 1) over copies of the rows: the bits the guided row is built from."""
    from valley_amd import ops
    y = x.detach().clone().contiguous().to(dev())
    R = y.shape[0]
    ops.logits_process(y, ops.processor_rows([None] * R, device=dev()), torch.zeros((R, 1), dtype=torch.int32, device=dev()), None, 0,
                       None, None, log_softmax=True)
    return y.cpu()


def within_float64(x, got, table):
    """The independent check: scale * (lc - lu) + lu in float64 over float64 log-softmaxes of the finite values, to
    (|g| + |g - 1| + 1) * 1e-6 * max(1, max |lc|, max |lu|) wherever the expected value is finite."""
    f = table.view(torch.float32)
    for c in range(x.shape[0]):
        u = GR.valid_partner(table, c, GR.COND, GR.UNCOND)
        if u is None:
            continue
        g, lb = float(f[c, 2]), float(f[c, 3])
        xc, xu = x[c].double(), x[u].double()
        okc, oku = torch.isfinite(xc), torch.isfinite(xu)
        if not okc.any():
            continue
        lc = xc - torch.logsumexp(xc[okc], 0)
        lu = xu - (torch.logsumexp(xu[oku], 0) if oku.any() else 0.0)
        want = torch.where(oku, g * (lc - lu) + lu, lc)
        scale = max(1.0, float(lc[okc].abs().max()), float(lu[oku].abs().max()) if oku.any() else 0.0)
        bound = (abs(g) + abs(g - 1) + 1) * REL * scale
        live = okc & torch.isfinite(got[c].double())
        if lb > NEG_INF:                                          # a column one rounding from the cut-off may fall either way
            live &= (lc - (lc[okc].max() + lb)).abs() > bound
            assert bool((got[c][okc & (lc < lc[okc].max() + lb - bound)] == NEG_INF).all())
            assert bool(torch.isfinite(got[c][okc & (lc > lc[okc].max() + lb + bound)]).all())
        else:
            assert torch.equal(live, okc), c
        err = float((got[c].double() - want)[live].abs().max()) if live.any() else 0.0
        assert err <= bound, (c, g, err, bound)


def check(x, V, table):
    """Launch on x [R, ld] with the [R, 4] table; exact against the reference over the device's log-softmax; float64 within bound."""
    from valley_amd import ops
    xd = x.to(dev())
    ops.guide(xd[:, :V], table.to(dev()))
    got = xd.cpu()
    assert GR.same_bits(got[:, V:], x[:, V:])                    # the padding columns are never touched
    want = GR.apply(x[:, :V], table, lsm=device_log_softmax)
    assert GR.same_bits(got[:, :V], want)
    for r in range(x.shape[0]):
        if GR.valid_partner(table, r, GR.COND, GR.UNCOND) is None:
            assert GR.same_bits(got[r], x[r]), r                 # neutral, unconditional and malformed rows keep every bit
        else:
            assert not got[r, :V].isnan().any()
    within_float64(x[:, :V], got[:, :V], table)
    return got


def pairs_for(R, k):
    """Adjacent pairs, pairs far apart, the unconditional row below the conditional one, neutral rows between and beside them."""
    s = lambda i: SCALES[(k + i) % len(SCALES)]                 # noqa: E731
    b = lambda i: BETAS[(k + i) % len(BETAS)]                   # noqa: E731
    if R == 2:
        return [(1, 0, s(0), b(0))] if k % 2 else [(0, 1, s(0), b(0))]
    if R == 3:
        return [(2, 0, s(0), b(0))] if k % 2 else [(0, 2, s(0), b(0))]        # row 1 is neutral, between them
    return [(0, 1, s(0), b(0)), (7, 2, s(1), b(1)), (3, 5, s(2), b(2))]       # rows 4 and 6 are neutral


# ---- the kernel ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("V", [1, 63, 1025, 32000, 32003, 40000])
@pytest.mark.parametrize("R", [2, 3, 8])
def test_shapes_rows_and_pairs(V, R):
    ld = V + 5 if V == 32003 else V
    for k in (0, 1):
        x = scores(R, V, ld, seed=V * 10 + R + k)
        check(x, V, GR.table_of(R, pairs_for(R, k + V % 3)))


@pytest.mark.parametrize("scale", SCALES)
def test_scales_and_cut_offs(scale):
    V = 1025
    x = scores(2, V, V, seed=int(scale * 4) + 9)
    x[0, 100], x[0, 200] = x[0, :V].nan_to_num(-100.0, neginf=-100.0).max(), x[0, :V].nan_to_num(-100.0, neginf=-100.0).max()   # a tie at the maximum
    ls = device_log_softmax(x)
    for beta in BETAS:
        got = check(x, V, GR.table_of(2, [(0, 1, scale, beta)]))
        alive = torch.isfinite(got[0])
        if scale == 1.0 and beta == 0.0:
            assert GR.same_bits(got[0], torch.where(ls[0].isnan(), torch.full_like(ls[0], NEG_INF), ls[0]))   # the log-softmax bits
        if beta == 1.0:                                           # only the columns tied at the maximum survive
            assert alive.nonzero().view(-1).tolist() == (ls[0] == ls[0][~ls[0].isnan()].max()).nonzero().view(-1).tolist()
            assert int(alive.sum()) >= 2
        if beta == 0.0:
            assert torch.equal(alive, torch.isfinite(x[0]))


def test_non_finite_columns_and_a_dead_row():
    V = 700
    x = scores(4, V, V, seed=3, special=False)
    x[0, 10], x[0, 11], x[1, 12], x[1, 13] = float("nan"), NEG_INF, float("nan"), NEG_INF      # in either row alone
    x[0, 14], x[1, 14], x[0, 15], x[1, 15] = float("nan"), NEG_INF, NEG_INF, float("nan")      # and in both
    x[2] = NEG_INF                                                # a conditional row that is all -inf
    for beta in (0.0, 0.1):
        got = check(x, V, GR.table_of(4, [(0, 1, 3.0, beta), (2, 3, 1.5, beta)]))
        ls = device_log_softmax(x)
        assert got[0, 10] == NEG_INF and got[0, 11] == NEG_INF and got[0, 14] == NEG_INF and got[0, 15] == NEG_INF
        if beta == 0.0:
            assert GR.same_bits(got[0, 12:14], ls[0, 12:14])      # no guidance where the unconditional row has nothing to say
        assert bool((got[2] == NEG_INF).all())
    x[3] = NEG_INF                                                # ... and an unconditional one: the row is its own log-softmax
    got = check(x, V, GR.table_of(4, [(0, 3, 3.0, 0.0)]))
    assert GR.same_bits(got[0], torch.where(torch.isfinite(x[0]), device_log_softmax(x)[0], torch.full_like(x[0], NEG_INF)))


def test_malformed_partners_leave_the_row_untouched():
    V, R = 300, 4
    x = scores(R, V, V + 3, seed=5)
    bits = lambda v: torch.tensor(v, dtype=torch.float32).view(torch.int32).item()    # noqa: E731
    s, o = bits(2.0), bits(NEG_INF)
    for bad in ([1, 4, s, o], [1, -1, s, o], [1, 1 << 30, s, o],       # outside [0, R)
                [1, 0, s, o],                                          # the row itself
                [1, 1, s, o], [1, 3, s, o]):                           # a neutral row, a conditional row
        table = torch.tensor([bad, [0, 0, s, o], [2, 3, s, o], [1, 2, s, o]], dtype=torch.int32)
        got = check(x, V, table)
        assert GR.same_bits(got[0], x[0]) and not GR.same_bits(got[3], x[3])      # row 3's own pair is guided all the same


def test_a_pair_gives_the_same_bits_wherever_it_stands():
    V = 32000
    a = scores(8, V, V, seed=6)
    b = scores(8, V, V, seed=7)                                   # other neighbours
    b[6], b[3] = a[0], a[1]
    one = check(a, V, GR.table_of(8, [(0, 1, 1.5, 0.1), (4, 5, 3.0, 0.0)]))
    two = check(b, V, GR.table_of(8, [(6, 3, 1.5, 0.1), (0, 1, 0.5, 0.0)]))
    assert GR.same_bits(one[0], two[6])
    again = check(a, V, GR.table_of(8, [(0, 1, 1.5, 0.1)]))
    assert GR.same_bits(one[0], again[0])


def test_captured_launch_follows_a_rewritten_table():
    from valley_amd import ops
    R, V, ld = 6, 32000, 32008
    x = scores(R, V, ld, seed=8)
    logits = x.to(dev())
    rows = ops.guidance_rows(R, [(0, 1, 1.5, 0.0), (2, 3, 3.0, 0.1)], device=dev())
    tok = torch.arange(10, 10 + R, dtype=torch.int32, device=dev())
    ops.guide(logits[:, :V], rows)
    ops.guide_follow(tok, rows)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ops.guide(logits[:, :V], rows)
        ops.guide_follow(tok, rows)
    ls = device_log_softmax(x[:, :V])
    for pairs in ([(0, 3, 1.5, 0.0), (2, 1, -1.0, 0.0)],          # other partners, another scale
                  [(0, 1, 0.5, 1.0)],                             # the second pair switched off
                  [], [(5, 4, 3.0, 0.1), (0, 1, 1.5, 0.0), (2, 3, 3.0, 0.1)]):
        table = GR.table_of(R, pairs)
        rows.copy_(ops.guidance_rows(R, pairs))
        logits.copy_(x)
        tok.copy_(torch.arange(10, 10 + R, dtype=torch.int32))
        graph.replay()
        got = logits.cpu()
        assert GR.same_bits(got[:, :V], GR.apply(x[:, :V], table, lsm=lambda _: ls)) and GR.same_bits(got[:, V:], x[:, V:]), pairs
        assert tok.tolist() == GR.follow(torch.arange(10, 10 + R, dtype=torch.int32), table).tolist(), pairs


def test_follow():
    from valley_amd import ops
    R = 8
    tok = torch.arange(100, 100 + R, dtype=torch.int32)
    table = GR.table_of(R, [(0, 1, 1.5, 0), (7, 2, 3.0, 0), (3, 5, 0.5, 0)])
    got = ops.guide_follow(tok.to(dev()), table.to(dev())).cpu()
    assert got.tolist() == [100, 100, 107, 103, 104, 103, 106, 107] == GR.follow(tok, table).tolist()
    z = 0
    bad = torch.tensor([[2, 8, z, z], [2, 1, z, z], [2, 4, z, z], [2, 2, z, z], [0, 3, z, z], [2, -1, z, z], [1, 7, z, z], [2, 6, z, z]],
                       dtype=torch.int32)                         # out of range, itself, a neutral partner, an unconditional partner; 7 <- 6
    got = ops.guide_follow(tok.to(dev()), bad.to(dev())).cpu()
    assert got.tolist() == [100, 101, 102, 103, 104, 105, 106, 106] == GR.follow(tok, bad).tolist()
    assert ops.guide_follow(tok.to(dev()), GR.table_of(R, []).to(dev())).cpu().tolist() == tok.tolist()


# ---- generate() end to end ----------------------------------------------------------------------------------------------------
NEW = 8
MIN_COMPARED = 6                                              # of NEW tokens: what the reference alone must reach before a near-tie


def text(name, n):
    return G._text("guide." + name, n)


# per case: the scale and the seed of its negative text / frames, chosen with the CPU oracle (see ``model_case``)
CHOICE = {"one_default": (1.3, 0), "one_short": (1.25, 0), "one_long_text": (0.75, 2), "one_noised_frames": (0.5, 8),
          "two_short_padded": (0.5, 5), "two_long_noised_frames": (2.0, 11), "two_penalty": (1.5, 4), "two_bad_words": (1.5, 6)}


def model_case(name, choice=None):
    """-> (which inputs, g, negative ids / mask (CPU, or None), name of the negative frames or None, generate's other arguments).
    The scale and the negative prompt's seed were chosen with the CPU oracle (oracle/valley_oracle.py under ``rounding()``, the
    loop of tests/guide_ref.py) so that the oracle's reference reaches all NEW tokens with every gap between its two best scores
    above the comparison's threshold (see ``compared``; 1.04 to 3 times it over the eight cases); the test asks for MIN_COMPARED."""
    g, k = choice or CHOICE[name]
    one, _ = G.golden_ids("decode")
    main, main_mask = G.golden_ids("main")
    one, main, main_mask = torch.from_numpy(one), torch.from_numpy(main), torch.from_numpy(main_mask)
    short2 = torch.tensor([[0, 0] + [G.BOS] + text(f"s1.{k}", 3), [G.BOS] + text(f"s0.{k}", 5)])
    short2_mask = torch.tensor([[0, 0, 1, 1, 1, 1], [1] * 6])
    long2 = torch.cat([torch.zeros((2, 3), dtype=main.dtype), main], 1)
    long2_mask = torch.cat([torch.zeros((2, 3), dtype=main.dtype), main_mask], 1)
    return {
        "one_default": ("one", g, None, None, None, {}),
        "one_short": ("one", g, torch.tensor([[G.BOS] + text(f"a.{k}", 5)]), None, None, {}),
        "one_long_text": ("one", g, torch.tensor([[G.BOS] + text(f"b.{k}", one.shape[1] + 16)]), None, None, {}),
        "one_noised_frames": ("one", g, one, None, f"guide.noise1.{k}", {}),
        "two_short_padded": ("main", g, short2, short2_mask, None, {}),
        "two_long_noised_frames": ("main", g, long2, long2_mask, f"guide.noise2.{k}", {}),
        "two_penalty": ("main", g, short2, short2_mask, None, dict(repetition_penalty=1.3)),
        "two_bad_words": ("main", g, short2, short2_mask, None, dict(bad_words="from the reference")),
    }[name]


CASES = ["one_default", "one_short", "one_long_text", "one_noised_frames", "two_short_padded", "two_long_noised_frames", "two_penalty",
         "two_bad_words"]


def compared(margins, g):
    """Per row: the number of leading tokens to compare — up to the first step at which the reference's two best final scores lie
    closer than 2 * (|g| + |g - 1|) * 2e-2 (the session and the generic forward agree to 2e-2 per logit, tests/test_model_gpu.py;
    guidance multiplies that by up to |g| + |g - 1|)."""
    thr = 2 * (abs(g) + abs(g - 1)) * 2e-2
    out = []
    for row in margins.tolist():
        near = [i for i, m in enumerate(row) if m < thr]
        out.append(near[0] if near else len(row))
    return out


@pytest.fixture(scope="module")
def model():
    from tests.test_model_gpu import build_golden_model
    return build_golden_model()


def case_tensors(name):
    which, g, neg, neg_mask, frames, kw = model_case(name)
    ids, mask, img = inputs(which)
    T, B = G.GCFG["T"], ids.shape[0]
    neg_img = None if frames is None else torch.from_numpy(G.golden_pixels(B * T, frames)).view(B, T, 3, 224, 224).cuda()
    neg = None if neg is None else neg.cuda()
    neg_mask = None if neg_mask is None else neg_mask.cuda()
    return ids, (mask if which == "main" else None), img, g, neg, neg_mask, neg_img, dict(kw)


def reference(model, ids, mask, img, g, neg, neg_mask, neg_img, back=()):
    nids = ids[:, -1:] if neg is None else neg
    nmask = torch.ones_like(nids) if neg_mask is None else neg_mask
    cmask = torch.ones_like(ids) if mask is None else mask
    return GR.guided_loop(greedy_stepper(model, ids, cmask, img), greedy_stepper(model, nids, nmask, neg_img), ids, NEW, g, 0.0, back)


@pytest.mark.parametrize("name", CASES)
def test_generate_matches_the_reference_loop(model, name):
    ids, mask, img, g, neg, neg_mask, neg_img, kw = case_tensors(name)
    S = ids.shape[1]
    back, gen_kw = (), {}
    if "repetition_penalty" in kw:
        back, gen_kw = logits_ref.hf_processors(kw["repetition_penalty"], prompt_len=S), dict(kw)
    if "bad_words" in kw:                                         # ban what guided decoding says: row 0's first token, row 1's second
        free, _ = reference(model, ids, mask, img, g, neg, neg_mask, neg_img)
        words = [[int(free[0, S])], [int(free[1, S + 1])]]
        back, gen_kw = CR.hf_constraint_processors(words, None, 0, None, None, begin=S), dict(bad_words_ids=words)
    ref, margins = reference(model, ids, mask, img, g, neg, neg_mask, neg_img, back)
    n = compared(margins, g)
    print(f"{name}: g={g} margins={[[round(m, 3) for m in row] for row in margins.tolist()]} compared={n}")
    assert min(n) >= MIN_COMPARED, (name, n, margins)             # a case that compares fewer tokens fails
    plain = model.generate(ids, images=img, attention_mask=mask, max_new_tokens=NEW, **gen_kw)
    assert not torch.equal(ref, plain)                            # guidance acts: the guided tokens are not the unguided ones
    outs = []
    for ug in (True, False):
        got = model.generate(ids, images=img, attention_mask=mask, max_new_tokens=NEW, use_graph=ug, guidance_scale=g,
                             negative_prompt_ids=neg, negative_prompt_attention_mask=neg_mask, negative_images=neg_img, **gen_kw)
        assert tuple(got.shape) == (ids.shape[0], S + NEW) and torch.equal(got[:, :S], ids)
        for r in range(ids.shape[0]):
            assert got[r, S:S + n[r]].tolist() == ref[r, S:S + n[r]].tolist(), (name, ug, r, got[r, S:].tolist(), ref[r, S:].tolist())
        outs.append(got)
    assert torch.equal(outs[0], outs[1])                          # the graph and the eager route: the same kernels, the same bits
    if "bad_words" in kw:
        assert int(outs[0][0, S]) != words[0][0] and int(outs[0][1, S + 1]) != words[1][0]


def test_seeded_and_host_sampling_agree_across_routes(model):
    ids, mask, img, g, neg, neg_mask, neg_img, _ = case_tensors("two_short_padded")
    kw = dict(images=img, attention_mask=mask, max_new_tokens=NEW, do_sample=True, temperature=0.9, guidance_scale=g, negative_prompt_ids=neg,
              negative_prompt_attention_mask=neg_mask, guidance_plausibility=0.1, repetition_penalty=1.2)
    outs = [model.generate(ids, use_graph=ug, top_k=50, seed=11, **kw) for ug in (True, False, True)]
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2])
    other = model.generate(ids, use_graph=True, top_k=50, seed=12, **kw)
    assert not torch.equal(other, outs[0])
    host = []
    for ug in (True, False):                                      # torch.multinomial over the guided logits
        torch.manual_seed(3)
        host.append(model.generate(ids, use_graph=ug, **kw))
    assert torch.equal(host[0], host[1])


def test_plausibility_keeps_the_tokens_within_beta_of_the_best(model):
    """beta = 1 leaves the conditional row's own argmax at every step: the sequence is the unguided one, whatever the scale."""
    ids, mask, img, g, neg, neg_mask, neg_img, _ = case_tensors("one_short")
    plain = model.generate(ids, images=img, max_new_tokens=NEW)
    got = model.generate(ids, images=img, max_new_tokens=NEW, guidance_scale=3.0, negative_prompt_ids=neg, guidance_plausibility=1.0)
    assert torch.equal(got, plain)


def test_refusals_reach_no_kernel(model):
    ids, mask, img = inputs("main")
    kw = dict(images=img, attention_mask=mask, max_new_tokens=4, guidance_scale=2.0)
    for bad, what in ((dict(num_beams=2), "num_beams > 1"), (dict(prompt_lookup_num_tokens=3), "prompt_lookup_num_tokens"),
                      (dict(use_graph=None), "use_graph"), (dict(output_logprobs=True, return_dict_in_generate=True), "output_logprobs"),
                      (dict(negative_prompt_ids=ids[:1]), "one negative prompt per prompt row")):
        with pytest.raises(ValueError, match=what):
            model.generate(ids, **kw, **bad)
    with pytest.raises(ValueError, match="at most 4 prompt rows"):
        model.generate(ids.repeat(3, 1)[:5], images=img.repeat(3, 1, 1, 1, 1)[:5], max_new_tokens=4, guidance_scale=2.0)
    from valley_amd.decode import DecodeSession
    ll = model.model.llama
    with pytest.raises(ValueError, match="needs per_row_positions=True"):
        DecodeSession(ll, ll.new_cache(2, 64), guidance=True)
    with pytest.raises(ValueError, match="no beams and no logprobs"):
        DecodeSession(ll, ll.new_cache(2, 64), per_row_positions=True, guidance=True, logprobs=0)


def test_int8_engine_one_row():
    from tests.test_model_gpu import build_golden_model
    model = build_golden_model()
    model.quantize_decode_weights("int8")
    ids, mask, img, g, neg, neg_mask, neg_img, _ = case_tensors("one_noised_frames")
    plain = model.generate(ids, images=img, max_new_tokens=NEW)
    outs = [model.generate(ids, images=img, max_new_tokens=NEW, use_graph=ug, guidance_scale=g, negative_prompt_ids=neg, negative_images=neg_img)
            for ug in (True, False)]
    assert torch.equal(outs[0], outs[1]) and not torch.equal(outs[0], plain)
    assert torch.equal(model.generate(ids, images=img, max_new_tokens=NEW, guidance_scale=1), plain)


# ---- the batcher --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", [(0, 1, 2), (2, 1, 0)])
def test_batcher_pairs_and_a_plain_request_equal_generate_alone(model, order):
    from valley_amd.serving import ContinuousBatcher
    T = G.GCFG["T"]
    img = torch.from_numpy(G.golden_pixels(T, "mixed")).view(1, T, 3, 224, 224).cuda()
    noise = torch.from_numpy(G.golden_pixels(T, "guide.noise1")).view(1, T, 3, 224, 224).cuda()
    ids = [torch.from_numpy(G.golden_ids(c)[0]).cuda() for c in ("decode", "decode2", "decode2")]
    reqs = [dict(guidance_scale=1.5, negative_prompt_ids=torch.tensor([[G.BOS] + text("a", 5)]).cuda()),
            dict(guidance_scale=3.0, negative_prompt_ids=ids[1], negative_images=noise, guidance_plausibility=0.1), {}]
    n = 6
    alone = [model.generate(ids[i], images=img, max_new_tokens=n, **reqs[i])[0, ids[i].shape[1]:].tolist() for i in range(3)]
    cb = ContinuousBatcher(model, slots=5, ctx_max=512, guidance=True)
    slots, got = {}, {}
    for k, i in enumerate(order):
        if k == 2:                                                # the third joins while the others decode
            for j, t in cb.step().items():
                got[j].append(t)
        slots[i] = cb.add(ids[i], images=img, **reqs[i])
        got[slots[i]] = [int(cb.sess.tok[slots[i]])]
    assert sorted(cb.free_slots()) == [] and len(set(slots.values())) == 3
    while min(len(v) for v in got.values()) < n:
        toks = cb.step()
        assert sorted(toks) == sorted(slots.values())             # conditional and plain slots only
        for j, t in toks.items():
            got[j].append(t)
    for i in range(3):
        assert got[slots[i]][:n] == alone[i], (order, i, got[slots[i]], alone[i])
    pair = cb.partner[slots[0]]
    assert pair is not None and cb.uncond[pair] and cb.length[pair] > 6 and cb.sess.guide[slots[0]].tolist()[:2] == [1, pair]
    assert int(cb.sess.tok[pair]) == int(cb.sess.tok[slots[0]])   # the unconditional slot is fed its pair's token
    cb.release(slots[0])
    assert sorted(cb.free_slots()) == sorted([slots[0], pair]) and cb.partner[pair] is None
    neutral = GR.table_of(1, [])[0].tolist()
    assert cb.sess.guide[slots[0]].tolist() == neutral and cb.sess.guide[pair].tolist() == neutral
    s = cb.add(ids[2], images=img)                                # a reused slot carries nothing over
    again = [int(cb.sess.tok[s])] + [cb.step()[s] for _ in range(3)]
    assert again == alone[2][:4]
    with pytest.raises(ValueError, match="needs ContinuousBatcher"):
        ContinuousBatcher(model, slots=2, ctx_max=512).add(ids[0], images=img, guidance_scale=2.0)


def test_a_scale_of_one_or_none_is_the_plain_call_and_never_loads_the_library():
    code = ("import sys, torch\n"
            "from tests import golden_cfg as G\n"
            "from tests.test_model_gpu import build_golden_model\n"
            "from valley_amd.serving import ContinuousBatcher\n"
            "model = build_golden_model()\n"
            "T = G.GCFG['T']\n"
            "ids = torch.from_numpy(G.golden_ids('decode')[0]).cuda()\n"
            "img = torch.from_numpy(G.golden_pixels(T, 'mixed')).view(1, T, 3, 224, 224).cuda()\n"
            "for ug in (True, False):\n"
            "    plain = model.generate(ids, images=img, max_new_tokens=4, use_graph=ug)\n"
            "    for g in (None, 1, 1.0):\n"
            "        assert torch.equal(model.generate(ids, images=img, max_new_tokens=4, use_graph=ug, guidance_scale=g), plain)\n"
            "    assert torch.equal(model.generate(ids, images=img, max_new_tokens=4, use_graph=ug, guidance_scale=1, negative_prompt_ids=ids), plain)\n"
            "cb = ContinuousBatcher(model, slots=2, ctx_max=512)\n"
            "cb.add(ids, images=img); cb.step()\n"
            "assert cb.sess.guide is None\n"
            "assert 'valley_amd.lib_guide' not in sys.modules and 'libvalley_hip_guide' not in open('/proc/self/maps').read()\n"
            "print('ok')\n")
    p = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, cwd=ROOT, timeout=300)
    assert p.returncode == 0 and p.stdout.strip().endswith("ok"), p.stderr[-3000:]
