"""GPU checks of prompt-lookup speculation under seeded sampling (include/valley_hip_spec_sample.h, valley_amd/spec.py,
generate()):

* vly_spec_counters, exactly, in a guarded buffer, with the clamp of the position;
* the property the feature rests on: a draw of vly_argmax is keyed by (seed, counter), not by the row or the launch;
* SpecDecodeSession(sampling=True) with forced drafts against DecodeSession(sampling=True): no, partial and full acceptance;
* generate(prompt_lookup_num_tokens=k, do_sample=True, seed=s) against the same seeded call without speculation, token for
  token: parameter sets, seeds, stopping, the hand-over to the one-token session, the int8 / int4 engines and the fp16 library;
* nothing else moves: a greedy speculative generation never asks for counters, a plain seeded one never loads the libraries.

Every comparison is an equality of token ids: there is no tolerance in this file."""
import json
import os
import subprocess
import sys

import pytest
import torch

from tests import golden_cfg as G

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
NEW = 24
# (temperature, top_k, top_p): the entry points' T = 0.2, a top-k set, a top-p set, both at a high temperature
PARAMS = [(0.2, 0, 1.0), (1.0, 50, 1.0), (0.8, 0, 0.9), (1.5, 40, 0.95)]
SEEDS = [7, (1 << 40) + 12345]
GUARD = 12


def sample_kw(params, seed):
    T, top_k, top_p = params
    kw = dict(do_sample=True, temperature=T, seed=seed)
    if top_k:
        kw["top_k"] = top_k
    if top_p < 1.0:
        kw["top_p"] = top_p
    return kw


# ---- vly_spec_counters ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 3, 7])
def test_spec_counters(k):
    from valley_amd import ops
    ctx_max = 64
    for pos in (0, 5, ctx_max - (k + 1), ctx_max - 1, ctx_max + 3, -4):
        buf = torch.full((k + 1 + 2 * GUARD,), -99, dtype=torch.int32, device=DEV)
        p = torch.full((1 + 2 * GUARD,), -99, dtype=torch.int32, device=DEV)
        p[GUARD] = pos
        out = ops.spec_counters(p[GUARD:GUARD + 1], k, ctx_max, buf[GUARD:GUARD + k + 1])
        base = max(0, min(pos, ctx_max - (k + 1)))
        assert out.tolist() == [base + j for j in range(k + 1)], (k, pos, out.tolist())
        assert bool((buf[:GUARD] == -99).all()) and bool((buf[GUARD + k + 1:] == -99).all()), (k, pos, "a guard word changed")
        want_p = [-99] * GUARD + [pos] + [-99] * GUARD
        assert p.tolist() == want_p, "pos is an input"
    # the smallest cache a step fits
    one = ops.spec_counters(torch.tensor([9], dtype=torch.int32, device=DEV), k, k + 1, torch.full((k + 1,), -1, dtype=torch.int32, device=DEV))
    assert one.tolist() == list(range(k + 1))


# ---- the draw is a function of (logits, seed, counter) ------------------------------------------------------------------------
@pytest.mark.parametrize("V", [G.GCFG["vocab"], 1003])
@pytest.mark.parametrize("params", PARAMS, ids=lambda p: f"T{p[0]}-k{p[1]}-p{p[2]}")
def test_draws_are_keyed_by_position_not_by_row(params, V):
    from valley_amd import ops
    g = torch.Generator().manual_seed(V)
    x = (3.0 * torch.randn((8, V), generator=g)).to(DEV)
    T, top_k, top_p = params
    counters = [5, 6, 7, 100, 0, 1 << 20, 41, 6]                 # (two rows share a counter: different logits, the same noise)
    ctr = torch.tensor(counters, dtype=torch.int32, device=DEV)
    for seed in SEEDS:
        rows = ops.sampling_rows(T, top_k, top_p, [seed] * 8, device=DEV)
        together = ops.argmax(x.clone(), sampling=rows, ctr=ctr, ctr_add=1).tolist()
        alone = [int(ops.argmax(x[j:j + 1].clone(), sampling=rows[j:j + 1].contiguous(), ctr_add=counters[j] + 1)[0]) for j in range(8)]
        assert together == alone, (params, V, seed, together, alone)
        # ... and through a one-element counter, as the one-token session passes it
        dev = [int(ops.argmax(x[j:j + 1].clone(), sampling=rows[j:j + 1].contiguous(),
                              ctr=torch.tensor([counters[j]], dtype=torch.int32, device=DEV), ctr_add=1)[0]) for j in range(8)]
        assert dev == alone
        assert all(0 <= t < V for t in together)


# ---- the session and generate() ---------------------------------------------------------------------------------------------
class Golden:
    """The golden model, its prompts, and the plain seeded calls the speculative ones are compared with — each computed once,
    when first asked for, and never modified."""

    def __init__(self):
        from tests.test_model_gpu import build_golden_model
        self.model = build_golden_model()
        T = G.GCFG["T"]
        self.img = torch.from_numpy(G.golden_pixels(T, "mixed")).view(1, T, 3, 224, 224).cuda()
        self.prompts = {name: torch.from_numpy(G.golden_ids(name)[0]).cuda() for name in ("decode", "decode2")}
        self._plain = {}

    def plain(self, name, params, seed, use_graph=True, **kw):
        key = (name, params, seed, use_graph, tuple(sorted((k, repr(v)) for k, v in kw.items())))
        if key not in self._plain:
            kw.setdefault("max_new_tokens", NEW)
            self._plain[key] = self.model.generate(self.prompts[name], images=self.img, use_graph=use_graph, **sample_kw(params, seed), **kw)
        return self._plain[key]

    def spec(self, name, params, seed, k, use_graph=True, **kw):
        kw.setdefault("max_new_tokens", NEW)
        return self.model.generate(self.prompts[name], images=self.img, use_graph=use_graph, prompt_lookup_num_tokens=k,
                                   return_dict_in_generate=True, **sample_kw(params, seed), **kw)


@pytest.fixture(scope="module")
def golden():
    return Golden()


SESSION_PARAMS = (1.0, 50, 1.0)          # a set whose draws depend on the noise, hence on the counter
SESSION_SEED = 1234
TRUTH = 17                               # t_0 and 2 (k + 1) tokens behind it at k = 7


def prefilled(golden, name, extra):
    from valley_amd import ops
    ids = golden.prompts[name]
    ll = golden.model.get_model().llama
    cache = ll.new_cache(1, ids.shape[1] + extra)
    out = golden.model(input_ids=ids, images=golden.img, past_key_values=cache, use_cache=True)
    T, top_k, top_p = SESSION_PARAMS
    row = ops.sampling_rows(T, top_k, top_p, [SESSION_SEED], device=DEV)
    first = ops.argmax(out.logits[:, -1, :].contiguous(), sampling=row, ctr_add=ids.shape[1])
    return ll, cache, row, first


@pytest.fixture(scope="module")
def session_truth(golden):
    """t_0 .. t_16 of plain seeded decoding through DecodeSession(sampling=True)."""
    from valley_amd.decode import DecodeSession
    truth = {}
    for name in ("decode2",):
        ll, cache, row, first = prefilled(golden, name, TRUTH + 8)
        sess = DecodeSession(ll, cache, use_graph=True, sampling=True)
        sess.sample.copy_(row)
        sess.begin(first)
        toks = [int(first[0])]
        while len(toks) < TRUTH:
            toks.append(int(sess.step()[0]))
        sess.check()
        truth[name] = toks
    return truth


@pytest.mark.parametrize("use_graph", [True, False], ids=["graph", "eager"])
@pytest.mark.parametrize("k", [1, 3, 7])
def test_session_forced_drafts_under_sampling(golden, session_truth, k, use_graph):
    """For every i in 0 .. k: the draft t_1 .. t_i followed by wrong ids is accepted up to i, the step emits t_1 .. t_{i+1}, and a
    second step (a wholly right draft) goes on with the plain session's tokens."""
    from valley_amd.spec import SpecDecodeSession
    V = G.GCFG["vocab"]
    name = "decode2"
    t = session_truth[name]
    assert len(set(t)) > 2                                       # (the continuation is not one repeated token)
    for i in range(k + 1):
        ll, cache, row, first = prefilled(golden, name, TRUTH + 8)
        assert int(first[0]) == t[0]
        sess = SpecDecodeSession(ll, cache, k, use_graph=use_graph, lookup=False, sampling=True)
        sess.sample.copy_(row.expand(k + 1, 6))
        sess.begin(first, prompt_ids=golden.prompts[name][0])
        pos0 = cache.seq_len
        assert sess.pos.item() == pos0 and sess.stats.tolist() == [0, 0, 0]
        sess.draft.copy_(torch.tensor([t[1 + j] if j < i else (t[1 + j] + 1) % V for j in range(k)], dtype=torch.int32))
        sess.draft_len.fill_(k)
        got = sess.step()
        assert got == t[1:i + 2], (k, i, got, t[1:i + 2])
        assert sess.stats.tolist() == [1, k, i]
        assert cache.seq_len == sess.pos.item() == pos0 + i + 1
        assert sess.ctr.tolist() == [pos0 + j for j in range(k + 1)]
        sess.draft.copy_(torch.tensor(t[i + 2:i + 2 + k], dtype=torch.int32))
        got = sess.step()
        assert got == t[i + 2:i + 3 + k], (k, i, "second step", got, t[i + 2:i + 3 + k])
        assert sess.stats.tolist() == [2, 2 * k, i + k]
        assert cache.seq_len == sess.pos.item() == pos0 + i + k + 2
        sess.check()


@pytest.mark.parametrize("use_graph", [True, False], ids=["graph", "eager"])
@pytest.mark.parametrize("k", [1, 3, 7])
def test_generate_prompt_lookup_is_plain_seeded_sampling(golden, k, use_graph):
    for name, ids in golden.prompts.items():
        for params in PARAMS:
            for seed in SEEDS:
                want = golden.plain(name, params, seed, use_graph)
                out = golden.spec(name, params, seed, k, use_graph)
                s = out.speculation
                new = out.sequences.shape[1] - ids.shape[1]
                print(f"{name} k={k} {params} seed={seed}: {s}")
                assert torch.equal(out.sequences, want), (name, k, params, seed, out.sequences[0, ids.shape[1]:].tolist(),
                                                          want[0, ids.shape[1]:].tolist())
                assert new == NEW and s["steps"] + s["accepted"] == new - 1, (name, k, params, seed, s)
                assert out.sequences_scores is None
    # the seeds and the parameter sets do give different sequences: the equality above is not that of a constant
    a, b = (golden.plain("decode2", PARAMS[1], s, use_graph) for s in SEEDS)
    assert not torch.equal(a, b)


def test_generate_prompt_lookup_stops_like_plain_seeded_sampling(golden, monkeypatch):
    from transformers import StoppingCriteria

    from valley_amd import decode, spec

    class AtLength(StoppingCriteria):
        def __init__(self, n):
            self.n = n

        def __call__(self, input_ids, scores, **kw):
            return input_ids.shape[1] >= self.n

    params, seed = PARAMS[0], SEEDS[0]
    for name, ids in golden.prompts.items():
        n_in = ids.shape[1]
        full = golden.plain(name, params, seed)[0, n_in:].tolist()
        eos = full[5]
        for k in (3, 7):
            want = golden.plain(name, params, seed, eos_token_id=eos)
            got = golden.spec(name, params, seed, k, eos_token_id=eos)
            assert torch.equal(got.sequences, want) and want.shape[1] <= n_in + 6 and int(want[0, -1]) == eos, (name, k)
            s = got.speculation
            assert s["steps"] + s["accepted"] >= want.shape[1] - n_in - 1      # (what a step emitted behind the stop is dropped)
            want = golden.model.generate(ids, images=golden.img, max_new_tokens=NEW, stopping_criteria=[AtLength(n_in + 7)],
                                         **sample_kw(params, seed))
            got = golden.spec(name, params, seed, k, stopping_criteria=[AtLength(n_in + 7)])
            assert torch.equal(got.sequences, want) and want.shape[1] == n_in + 7, (name, k)
            for n in sorted({1, 2, k, k + 1}):
                want = golden.plain(name, params, seed, max_new_tokens=n)
                got = golden.spec(name, params, seed, k, max_new_tokens=n)
                assert torch.equal(got.sequences, want) and want.shape[1] == n_in + n, (name, k, n)
                assert want[0, n_in:].tolist() == full[:n]
    # a cache (S + max_new_tokens deep) that runs out of room for a verify step mid-generation: verify steps first, then the
    # one-token session, whose counters go on from the cache's position
    calls = {"spec": 0, "plain": 0}
    spec_step, plain_step = spec.SpecDecodeSession.step, decode.DecodeSession.step
    monkeypatch.setattr(spec.SpecDecodeSession, "step", lambda self: calls.__setitem__("spec", calls["spec"] + 1) or spec_step(self))
    monkeypatch.setattr(decode.DecodeSession, "step", lambda self: calls.__setitem__("plain", calls["plain"] + 1) or plain_step(self))
    ids = golden.prompts["decode2"]
    for params in (PARAMS[0], PARAMS[1]):
        for n in (10, 12, 14):
            want = golden.plain("decode2", params, seed, max_new_tokens=n)
            calls.update(spec=0, plain=0)
            got = golden.spec("decode2", params, seed, 7, max_new_tokens=n)
            assert torch.equal(got.sequences, want), (params, n, got.sequences[0, ids.shape[1]:].tolist(), want[0, ids.shape[1]:].tolist())
            assert calls["spec"] >= 1 and calls["plain"] >= 1, (params, n, calls)
            s = got.speculation
            assert s["steps"] == calls["spec"] + calls["plain"] and s["steps"] + s["accepted"] >= n - 1


def test_greedy_rows_and_greedy_lookup_never_ask_for_counters(golden, monkeypatch):
    from valley_amd import ops
    calls = []
    real = ops.spec_counters
    monkeypatch.setattr(ops, "spec_counters", lambda *a, **kw: calls.append(a) or real(*a, **kw))
    ids = golden.prompts["decode2"]
    want = golden.model.generate(ids, images=golden.img, max_new_tokens=NEW)
    got = golden.model.generate(ids, images=golden.img, max_new_tokens=NEW, prompt_lookup_num_tokens=3)
    assert torch.equal(got, want) and not calls
    # temperature < GREEDY_T with do_sample=True and a seed: a greedy row, as in the plain call
    got = golden.model.generate(ids, images=golden.img, max_new_tokens=NEW, prompt_lookup_num_tokens=3, do_sample=True,
                                temperature=ops.GREEDY_T / 2, seed=5)
    assert torch.equal(got, want) and not calls
    assert torch.equal(golden.model.generate(ids, images=golden.img, max_new_tokens=NEW, do_sample=True, temperature=ops.GREEDY_T / 2,
                                             seed=5), want)
    # ... and the sampled call does (eager: one call per verify step; the one-token steps at the cache's end make none)
    out = golden.spec("decode2", PARAMS[0], SEEDS[0], 3, use_graph=False)
    assert 1 <= len(calls) <= out.speculation["steps"]


@pytest.mark.parametrize("mode", ["int8", "int4"])
def test_generate_prompt_lookup_sampling_on_the_quantized_engines(mode):
    from tests.test_model_gpu import build_golden_model
    model = build_golden_model()
    model.quantize_decode_weights(mode)
    T = G.GCFG["T"]
    img = torch.from_numpy(G.golden_pixels(T, "mixed")).view(1, T, 3, 224, 224).cuda()
    ids = torch.from_numpy(G.golden_ids("decode2")[0]).cuda()
    kw = dict(images=img, max_new_tokens=NEW, **sample_kw(PARAMS[0], SEEDS[0]))
    want = model.generate(ids, **kw)
    out = model.generate(ids, prompt_lookup_num_tokens=3, return_dict_in_generate=True, **kw)
    assert torch.equal(out.sequences, want), (mode, out.sequences[0, ids.shape[1]:].tolist(), want[0, ids.shape[1]:].tolist())
    s = out.speculation
    assert s["steps"] >= 1 and s["steps"] + s["accepted"] == NEW - 1


# ---- the fp16 storage type, and runs that never sample a verify step ----------------------------------------------------------
def _worker(mode, env_extra):
    env = {k: v for k, v in os.environ.items() if k not in ("VALLEY_PRECISION", "VALLEY_SPEC_ATTN")}
    env.update(env_extra)
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "spec_sampling_worker.py"), mode], capture_output=True, text=True,
                       env=env, timeout=600)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    return json.loads(p.stdout.strip().splitlines()[-1])


def test_spec_sampling_on_the_fp16_library():
    res = _worker("fp16", {"VALLEY_PRECISION": "fp16"})
    assert res["ok"] and res["storage"] == 1 and res["tokens_equal"] and res["steps_plus_accepted"] == res["new_tokens"] - 1


def test_plain_seeded_generate_never_loads_the_spec_libraries():
    res = _worker("off", {})
    assert res["ok"] and res["new_tokens"] == 4
    assert res["spec_lib_loaded"] is False and res["spec_sample_lib_loaded"] is False
    assert res["greedy_lookup_loads_spec"] is True and res["greedy_lookup_loads_spec_sample"] is False
