"""INT4 weight-only decode on the GPU: the quantizer and the GEMVs of libvalley_hip_w4.so checked exactly (tests/w4_checks.py, on
the bf16 library here and on the fp16 library in a child process), then the engine, the decode session and the generation
routes with 4-bit weights."""
import copy
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import golden_cfg as G
from tests import w4_checks, w4_ref

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_quantizer_exact_inputs():
    w4_checks.quantizer_exact()


def test_quantizer_random_rows():
    w4_checks.quantizer_random()


@pytest.mark.parametrize("N,K", w4_ref.SHAPES)
def test_gemv_exact(N, K):
    w4_checks.gemv_exact(N, K)


@pytest.mark.parametrize("N,K", w4_ref.SHAPES)
def test_gemv_random(N, K):
    w4_checks.gemv_random(N, K)


@pytest.mark.parametrize("N,K", w4_ref.SHAPES)
def test_row_independence(N, K):
    w4_checks.row_independence(N, K)


def test_fused_norm_is_the_pair():
    w4_checks.fused_norm()


def test_rejected_shapes():
    w4_checks.rejected_shapes()


def test_ops_reject_wrong_dtypes():
    from valley_amd import lib, ops
    q = torch.full((4, 64), 0x88, dtype=torch.uint8, device="cuda")
    s = torch.ones((4, 1), device="cuda")
    a = torch.ones((1, 128), dtype=torch.bfloat16, device="cuda")
    with pytest.raises(lib.ValleyHipError):
        ops.w4_quantize(torch.zeros((4, 128), dtype=torch.float32, device="cuda"))
    with pytest.raises(lib.ValleyHipError):
        ops.w4_gemv(a.float(), q, s)
    with pytest.raises(lib.ValleyHipError):
        ops.w4_gemv(a, q.to(torch.int8), s)
    with pytest.raises(lib.ValleyHipError):
        ops.w4_gemv(a, q, s.double())
    with pytest.raises(lib.ValleyHipError):
        ops.w4_gemv_rmsnorm(a, torch.ones((128,), device="cuda"), 1e-5, q, s)


def _worker(mode, env_extra):
    env = {k: v for k, v in os.environ.items() if k not in ("VALLEY_PRECISION", "VALLEY_WEIGHT_QUANT")}
    env.update(env_extra)
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "w4_worker.py"), mode], capture_output=True, text=True, env=env,
                       timeout=600)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    return json.loads(p.stdout.strip().splitlines()[-1])


def test_kernels_on_the_fp16_library():
    res = _worker("fp16", {"VALLEY_PRECISION": "fp16"})
    assert res["ok"] and res["storage"] == 1 and res["wq_lib_loaded"] is False


def test_switch_off_never_loads_a_quantization_library():
    res = _worker("off", {})
    assert res["ok"] and res["new_tokens"] == 4
    assert res["weight_quant"] is None and res["wq_keys"] == []
    assert res["w4_lib_loaded"] is False and res["wq_lib_loaded"] is False


# ---- engine: weights for which quantization is lossless ---------------------------------------------------------------
@pytest.fixture(scope="module")
def lossless_engines():
    """(unquantized, quantized) HipLlama(2048, 16, 5504, 2, 1000) sharing ONE set of weights whose projections are q * 2^e groups
    (5504 = 43 * 128)."""
    from valley_amd import runtime
    from valley_amd.llama import HipLlama
    H, I = 2048, 5504
    ref = HipLlama(H, 16, I, 2, 1000, 1e-5).init_random(seed=3)
    exact = []
    for li, L in enumerate(ref.layers):
        ex = {}
        for k, (N, K) in (("w_qkv", (3 * H, H)), ("w_o", (H, H)), ("w_gu", (2 * I, H)), ("w_down", (H, I))):
            w, q, s = w4_ref.exact_weights(N, K, seed=1000 * li + N + K, dtype=runtime.HALF)
            L[k] = w.cuda()
            ex[k] = (q, s)
        exact.append(ex)
    ref._pack()
    qe = HipLlama(H, 16, I, 2, 1000, 1e-5, weight_quant="int4")
    qe.embed, qe.norm, qe.lm_head = ref.embed, ref.norm, ref.lm_head
    qe.layers = [dict(L) for L in ref.layers]
    qe._pack()
    qe.loaded = True
    for L, ex in zip(qe.layers, exact):                                  # lossless: the device quantizer returns exactly (q, 2^e)
        for k, (q, s) in ex.items():
            gq, gs = L["wq_" + k[2:]]
            assert gq.dtype == torch.uint8
            assert torch.equal(w4_ref.unpack(gq), q) and torch.equal(gs.cpu(), s), k
    assert not [k for L in ref.layers for k in L if k.startswith("wq_")]
    return ref, qe


@pytest.mark.parametrize("use_graph", [True, False])
@pytest.mark.parametrize("B", [1, 2, 5])
def test_session_lossless_weights(lossless_engines, B, use_graph):
    from valley_amd import ops
    from valley_amd.decode import DecodeSession
    ref, qe = lossless_engines
    S = 8
    g = torch.Generator().manual_seed(B)
    h0 = torch.randn((B * S, ref.H), generator=g).cuda()
    first = torch.randint(0, 1000, (B,), generator=g).cuda()
    sessions = []
    for ll in (ref, qe):
        cache = ll.new_cache(B, 64)
        ll.forward(h0.clone(), B, S, cache)                              # prefill reads the 16-bit weights in both: the same prompt KV
        sess = DecodeSession(ll, cache, use_graph=use_graph)
        sess.begin(first)
        sessions.append((sess, cache))
    (s_ref, c_ref), (s_q, c_q) = sessions
    for a, b in zip(c_ref.k + c_ref.v, c_q.k + c_q.v):                   # the prompt positions (capturing writes a warm-up step's K / V at S)
        assert torch.equal(a[:, :, :S], b[:, :, :S])
    assert s_q.wq and not s_ref.wq and s_q.q_gemv is ops.w4_gemv
    for step in range(6):
        s_q.tok.copy_(s_ref.tok)                                         # teacher-forced with the unquantized engine's tokens
        t_ref = s_ref.step().clone()
        t_q = s_q.step().clone()
        torch.cuda.synchronize()
        lr = s_ref.logits[:, :ref.V].float().cpu().numpy()
        lq = s_q.logits[:, :ref.V].float().cpu().numpy()
        d = float(np.abs(lr - lq).max())
        print(f"B={B} graph={use_graph} step {step}: max |dlogit| {d:.3e}")
        assert d < 2e-2, (step, d)
        srt = np.sort(lr, axis=1)
        for b in range(B):
            if srt[b, -1] - srt[b, -2] > 0.12:                           # unambiguous argmax only
                assert int(t_ref[b]) == int(t_q[b]), (step, b)


def test_output_attentions_step_reads_int4(lossless_engines):
    """The one-token forward with ``attn`` (HF's output_attentions) decodes the int4 model like every other route: an engine whose
    16-bit q|k|v weights are zeroed behind its int4 copies gives the same bits, and not the uniform probabilities of a zero q|k|v."""
    _ref, qe = lossless_engines
    blind = copy.copy(qe)
    blind._ws = {}
    blind.layers = [dict(L, w_qkv=torch.zeros_like(L["w_qkv"])) for L in qe.layers]
    B, S = 2, 8
    g = torch.Generator().manual_seed(11)
    h0 = torch.randn((B * S, qe.H), generator=g).cuda()
    h1 = torch.randn((B, qe.H), generator=g).cuda()
    got = []
    for eng in (qe, blind):
        cache = qe.new_cache(B, 32)
        qe.forward(h0.clone(), B, S, cache)                              # the same prompt KV, from the intact engine
        probs = []
        x = eng.forward(h1.clone(), B, 1, cache, attn=probs)
        got.append((x.clone(), probs))
    (x_q, p_q), (x_b, p_b) = got
    assert len(p_q) == qe.L and p_q[0].shape == (B, qe.heads, 1, S + 1)
    assert torch.equal(x_q, x_b) and all(torch.equal(a, b) for a, b in zip(p_q, p_b))
    assert float((p_q[0] - 1.0 / (S + 1)).abs().max()) > 1e-3 and bool(torch.isfinite(x_q.float()).all())


def test_a_second_mode_is_refused(lossless_engines):
    _ref, qe = lossless_engines
    with pytest.raises(ValueError, match="int4"):
        qe.quantize_weights("int8")
    assert qe.weight_quant == "int4" and qe.layers[0]["wq_qkv"][0].dtype == torch.uint8


@pytest.fixture(scope="module")
def quantized_golden():
    from tests.test_model_gpu import build_golden_model
    model = build_golden_model()
    model.quantize_decode_weights("int4")
    ll = model.get_model().llama
    assert ll.weight_quant == "int4" and all(("wq_" + k) in L for L in ll.layers for k in ("qkv", "o", "gu", "down"))
    assert all(L["wq_qkv"][0].dtype == torch.uint8 and L["wq_qkv"][1].dim() == 2 for L in ll.layers)
    with pytest.raises(ValueError, match="int4"):
        model.quantize_decode_weights("int8")
    return model


def _decode_inputs():
    T = G.GCFG["T"]
    ids, _ = G.golden_ids("decode")
    img = torch.from_numpy(G.golden_pixels(T, "mixed")).view(1, T, 3, 224, 224).cuda()
    return torch.from_numpy(ids).cuda(), img


def test_generate_routes_agree(quantized_golden):
    model = quantized_golden
    T = G.GCFG["T"]
    ids, mask = G.golden_ids("main")
    images = torch.from_numpy(G.golden_pixels(2 * T, "main")).view(2, T, 3, 224, 224).cuda()
    kw = dict(images=images, attention_mask=torch.from_numpy(mask).cuda(), max_new_tokens=6)
    a = model.generate(torch.from_numpy(ids).cuda(), use_graph=True, **kw)
    b = model.generate(torch.from_numpy(ids).cuda(), use_graph=False, **kw)
    c = model.generate(torch.from_numpy(ids).cuda(), use_graph=None, **kw)
    assert a.shape == (2, ids.shape[1] + 6)
    assert torch.equal(a, b) and torch.equal(a, c)


def test_beams_sampling_and_batcher_run_quantized(quantized_golden):
    from valley_amd import ops
    from valley_amd.serving import ContinuousBatcher
    model = quantized_golden
    ids_t, img = _decode_inputs()
    n_in = ids_t.shape[1]
    greedy = model.generate(ids_t, images=img, max_new_tokens=5)
    beams = model.generate(ids_t, images=img, max_new_tokens=5, num_beams=2)
    assert beams.shape[0] == 1 and beams.shape[1] <= n_in + 5 and torch.equal(beams[:, :n_in], ids_t)
    kw = dict(images=img, max_new_tokens=6, do_sample=True, temperature=0.8, top_k=50)
    s1 = model.generate(ids_t, seed=123, use_graph=True, **kw)
    s2 = model.generate(ids_t, seed=123, use_graph=False, **kw)
    assert torch.equal(s1, s2)
    cb = ContinuousBatcher(model, slots=2, ctx_max=512)
    slots = [cb.add(ids_t, images=img), cb.add(ids_t, images=img)]
    got = {s: [] for s in slots}
    for _ in range(4):
        for s, t in cb.step().items():
            got[s].append(int(t))
    assert cb.sess.wq and cb.sess.q_gemv is ops.w4_gemv
    assert got[slots[0]] == got[slots[1]] and len(got[slots[0]]) == 4      # two identical requests decode alike
    assert greedy.shape == (1, n_in + 5)


def test_prompt_lookup_returns_the_int4_greedy_sequence(quantized_golden):
    model = quantized_golden
    ids_t, img = _decode_inputs()
    plain = model.generate(ids_t, images=img, max_new_tokens=12)
    for use_graph in (True, False):
        spec = model.generate(ids_t, images=img, max_new_tokens=12, prompt_lookup_num_tokens=3, use_graph=use_graph)
        assert torch.equal(spec, plain), use_graph


def test_logprobs_agree_in_the_three_routes(quantized_golden):
    model = quantized_golden
    ids_t, img = _decode_inputs()
    outs = [model.generate(ids_t, images=img, max_new_tokens=6, use_graph=ug, return_dict_in_generate=True, output_logprobs=True,
                           top_logprobs=2) for ug in (True, False, None)]
    bits = lambda t: t.contiguous().view(torch.int32)
    for o in outs[1:]:
        assert torch.equal(o.sequences, outs[0].sequences)
        assert torch.equal(bits(o.token_logprobs), bits(outs[0].token_logprobs))
        assert torch.equal(o.top_tokens, outs[0].top_tokens) and torch.equal(bits(o.top_logprobs), bits(outs[0].top_logprobs))
    assert bool(torch.isfinite(outs[0].token_logprobs).all()) and bool((outs[0].token_logprobs <= 0).all())


def test_persistent_and_oproj_forms_refuse_an_int4_engine(lossless_engines, monkeypatch):
    from valley_amd import decode
    _ref, qe = lossless_engines
    cache = qe.new_cache(1, 32)
    monkeypatch.setattr(decode, "PERSISTENT", True)
    with pytest.raises(ValueError, match="int4"):
        decode.DecodeSession(qe, cache)
    monkeypatch.setattr(decode, "PERSISTENT", False)
    monkeypatch.setattr(decode, "MERGE_IN", "oproj")
    with pytest.raises(ValueError, match="int4"):
        decode.DecodeSession(qe, cache)
