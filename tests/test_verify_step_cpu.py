"""The launches of one step of DecodeSession, SpecDecodeSession and SpecRowsSession — which ops.* functions, in which order, on
which of the session's buffers — recorded on stand-in model and cache objects with every launch function replaced: no GPU, no
library.  decode._norm_gemv (the norm -> projection dispatch of all three) and spec._VerifyStep (the launch order of the two
verify steps) are held to the lists below, which were recorded from the sessions as they stood before either existed."""
from types import SimpleNamespace

import pytest
import torch

from valley_amd import decode, ops, runtime, spec

LAUNCHES = ("embed_splice rmsnorm gemv gemv_rmsnorm wq_gemv wq_gemv_rmsnorm w4_gemv w4_gemv_rmsnorm rope_kv llama_attention decode_attention "
            "decode_attention_rows decode_attention_split gemv_attnmerge argmax incr_i32 spec_draft spec_attention spec_accept spec_counters "
            "spec_rows_draft spec_rows_rope_kv spec_rows_attention spec_rows_accept spec_rows_counters").split()
L = 2


@pytest.fixture
def calls(monkeypatch):
    """Every launch function records (name, ids of positional tensors, {keyword: id}) and launches nothing."""
    rec = []

    def recorder(name):
        def fn(*a, **kw):
            rec.append((name, [id(t) for t in a if isinstance(t, torch.Tensor)], {k: id(t) for k, t in kw.items() if isinstance(t, torch.Tensor)}))
            return kw.get("out")
        return fn

    for name in LAUNCHES:
        monkeypatch.setattr(ops, name, recorder(name))
    for name, v in (("FUSE_NORM", True), ("SPLIT_ATTN", True), ("PERSISTENT", False), ("MERGE_IN", "attn"), ("SPLIT_ROWS", True)):
        monkeypatch.setattr(decode, name, v)
    monkeypatch.setattr(runtime, "PRECISION", "bf16")
    monkeypatch.setattr(runtime, "HALF", torch.bfloat16)
    return rec


def stand_ins(B, H, quant=None, ctx=32):
    """A two-layer model of hidden size H (heads of 128) and a cache of B sequences: CPU tensors, one element per weight."""
    w = lambda: torch.zeros((1,))
    layers = []
    for _ in range(L):
        d = {"ln1": w(), "ln2": w()}
        for n in ("qkv", "o", "gu", "down"):
            d.update({"wq_" + n: (w(), w())} if quant else {"w_" + n: w()})
        layers.append(d)
    heads = H // 128
    ll = SimpleNamespace(L=L, layers=layers, H=H, I=2 * H, V=30, Vpad=32, heads=heads, eps=1e-5, embed=w(), cos=w(), sin=w(), norm=w(),
                         lm_head=w(), device="cpu", weight_quant=quant)
    kv = lambda: [torch.zeros((B, heads, ctx, 1)) for _ in range(L)]
    cache = SimpleNamespace(batch=B, ctx_max=ctx, generation=0, seq_len=4, k=kv(), v=kv(), key_valid=None)
    return ll, cache


def layer_names(fused, q):
    """One decoder layer behind its attention launch: the four dispatch arms of the two norm -> projection seams."""
    g = f"{q}_gemv" if q else "gemv"
    norm_proj = [f"{g}_rmsnorm"] if fused else ["rmsnorm", g]
    return norm_proj, [g] + norm_proj + [g]


def expect(fused, q, head, attn, tail):
    first, rest = layer_names(fused, q)
    return head + (first + attn + rest) * L + (["gemv_rmsnorm"] if fused else ["rmsnorm", "gemv"]) + tail


def check_buffers(sess, rec, ll):
    """Residual and output buffers are the session's own; the norm reads h (into x for the pair), the lm_head writes logits."""
    own = {id(getattr(sess, n)): n for n in ("h", "x", "qkv", "att", "mlp", "logits")}
    outs = []
    for name, pos, kw in rec:
        if name in ("rmsnorm", "gemv", "gemv_rmsnorm", "wq_gemv", "wq_gemv_rmsnorm", "w4_gemv", "w4_gemv_rmsnorm"):
            src, out = own[pos[0]], own[kw["out"]]
            assert (src, out) in (("h", "x"), ("h", "qkv"), ("h", "mlp"), ("h", "logits"), ("x", "qkv"), ("x", "mlp"), ("x", "logits"),
                                  ("att", "h"), ("mlp", "h")), (name, src, out)
            assert (out == "h") == ("residual" in kw) and kw.get("residual", id(sess.h)) == id(sess.h)
            assert (name == "rmsnorm") == (out == "x")
            outs.append(out)
        elif name in ("embed_splice",):
            assert kw["out"] == id(sess.h) and pos[0] == id(sess.tok)
        elif name.endswith("attention") or name.startswith("decode_attention"):
            assert pos[0] == id(sess.qkv) and kw["out"] == id(sess.att)
    per_layer = ["qkv", "h", "mlp", "h"]
    assert [o for o in outs if o != "x"] == per_layer * L + ["logits"]
    # the lm_head streams the 16-bit weight on every engine
    last = [r for r in rec if r[0] in ("gemv", "gemv_rmsnorm")][-1]
    assert id(ll.lm_head) in last[1] and last[2]["out"] == id(sess.logits)


@pytest.mark.parametrize("quant", [None, "int8", "int4"])
@pytest.mark.parametrize("H", [256, 2048])
@pytest.mark.parametrize("B", [1, 2, 4])
def test_decode_session_launches(calls, B, H, quant):
    ll, cache = stand_ins(B, H, quant)
    sess = decode.DecodeSession(ll, cache, use_graph=False)
    sess._enqueue_step()
    fused = H == 2048 and B <= 2                                 # ops.gemv_rmsnorm_ok: at most two rows, 2048 <= K <= 6144
    q = {"int8": "wq", "int4": "w4", None: None}[quant]
    assert [c[0] for c in calls] == expect(fused, q, ["embed_splice"], ["decode_attention_split"], ["argmax", "incr_i32"])
    check_buffers(sess, calls, ll)
    if H == 256 and B == 1 and quant is None:                    # the list itself, once, as it was recorded
        assert [c[0] for c in calls] == ["embed_splice",
                                         "rmsnorm", "gemv", "decode_attention_split", "gemv", "rmsnorm", "gemv", "gemv",
                                         "rmsnorm", "gemv", "decode_attention_split", "gemv", "rmsnorm", "gemv", "gemv",
                                         "rmsnorm", "gemv", "argmax", "incr_i32"]
    if H == 2048 and B == 2 and quant == "int8":
        assert [c[0] for c in calls] == ["embed_splice",
                                         "wq_gemv_rmsnorm", "decode_attention_split", "wq_gemv", "wq_gemv_rmsnorm", "wq_gemv",
                                         "wq_gemv_rmsnorm", "decode_attention_split", "wq_gemv", "wq_gemv_rmsnorm", "wq_gemv",
                                         "gemv_rmsnorm", "argmax", "incr_i32"]


def test_decode_session_without_the_split_attention(calls, monkeypatch):
    monkeypatch.setattr(decode, "SPLIT_ATTN", False)
    for per_row, attn in ((False, "decode_attention"), (True, "decode_attention_rows")):
        del calls[:]
        ll, cache = stand_ins(2, 2048)
        sess = decode.DecodeSession(ll, cache, use_graph=False, per_row_positions=per_row)
        sess._enqueue_step()
        assert [c[0] for c in calls] == expect(True, None, ["embed_splice"], [attn], ["argmax", "incr_i32"])
        check_buffers(sess, calls, ll)


@pytest.mark.parametrize("quant", [None, "int8"])
@pytest.mark.parametrize("k,H", [(1, 2048), (3, 256), (3, 2048)])
@pytest.mark.parametrize("attn", ["split", "prefill"])
@pytest.mark.parametrize("sampling", [False, True])
def test_spec_decode_session_launches(calls, monkeypatch, sampling, attn, k, H, quant):
    monkeypatch.setenv("VALLEY_SPEC_ATTN", attn)
    ll, cache = stand_ins(1, H, quant)
    sess = spec.SpecDecodeSession(ll, cache, k, use_graph=False, sampling=sampling)
    sess._enqueue_step()
    fused = H == 2048 and k == 1
    tail = (["spec_counters"] if sampling else []) + ["argmax", "spec_accept"]
    want = expect(fused, "wq" if quant else None, ["spec_draft", "embed_splice"],
                  ["rope_kv", "llama_attention" if attn == "prefill" else "spec_attention"], tail)
    assert [c[0] for c in calls] == want
    check_buffers(sess, calls, ll)
    if (k, H, quant, attn, sampling) == (3, 256, None, "split", True):
        assert want == ["spec_draft", "embed_splice",
                        "rmsnorm", "gemv", "rope_kv", "spec_attention", "gemv", "rmsnorm", "gemv", "gemv",
                        "rmsnorm", "gemv", "rope_kv", "spec_attention", "gemv", "rmsnorm", "gemv", "gemv",
                        "rmsnorm", "gemv", "spec_counters", "argmax", "spec_accept"]
    # the flat tables of one sequence, and what the draft and the acceptance are handed
    assert [tuple(t.shape) for t in (sess.hist, sess.draft, sess.draft_len, sess.emit, sess.stats, sess.pos, sess.tok, sess.am)] == \
        [(32,), (k,), (1,), (k + 2,), (3,), (1,), (k + 1,), (k + 1,)]
    assert calls[0][1] == [id(t) for t in (sess.hist, sess.pos, sess.draft, sess.draft_len, sess.tok)]
    assert calls[-1][1] == [id(t) for t in (sess.am, sess.draft, sess.draft_len, sess.hist, sess.pos, sess.emit, sess.tok, sess.stats)]
    assert calls[-2][2]["out"] == id(sess.am) and (not sampling or calls[-2][2]["ctr"] == id(sess.ctr) == calls[-3][1][1])
    rope = [c for c in calls if c[0] == "rope_kv"]
    assert [c[1][:3] for c in rope] == [[id(sess.qkv), id(cache.k[li]), id(cache.v[li])] for li in range(L)]
    assert all(c[2]["past_dev"] == id(sess.pos) for c in calls if c[0] in ("rope_kv", "llama_attention", "spec_attention"))


@pytest.mark.parametrize("quant", [None, "int4"])
@pytest.mark.parametrize("B,k,H", [(1, 1, 2048), (2, 3, 256), (2, 1, 2048), (4, 1, 256)])
@pytest.mark.parametrize("sampling", [False, True])
def test_spec_rows_session_launches(calls, sampling, B, k, H, quant):
    ll, cache = stand_ins(B, H, quant)
    sess = spec.SpecRowsSession(ll, cache, k, use_graph=False, sampling=sampling)
    sess._enqueue_step()
    fused = H == 2048 and B * (k + 1) <= 2
    tail = (["spec_rows_counters"] if sampling else []) + ["argmax", "spec_rows_accept"]
    want = expect(fused, "w4" if quant else None, ["spec_rows_draft", "embed_splice"], ["spec_rows_rope_kv", "spec_rows_attention"], tail)
    assert [c[0] for c in calls] == want
    check_buffers(sess, calls, ll)
    if (B, k, H, quant, sampling) == (1, 1, 2048, None, False):
        assert want == ["spec_rows_draft", "embed_splice",
                        "gemv_rmsnorm", "spec_rows_rope_kv", "spec_rows_attention", "gemv", "gemv_rmsnorm", "gemv",
                        "gemv_rmsnorm", "spec_rows_rope_kv", "spec_rows_attention", "gemv", "gemv_rmsnorm", "gemv",
                        "gemv_rmsnorm", "argmax", "spec_rows_accept"]
    assert [tuple(t.shape) for t in (sess.hist, sess.draft, sess.draft_len, sess.emit, sess.stats, sess.pos, sess.live, sess.tok, sess.am)] == \
        [(B, 32), (B, k), (B,), (B, k + 2), (B, 3), (B,), (B,), (B * (k + 1),), (B * (k + 1),)]
    assert calls[0][1] == [id(t) for t in (sess.hist, sess.pos, sess.draft, sess.draft_len, sess.tok)] and calls[0][2]["live"] == id(sess.live)
    assert calls[-1][1] == [id(t) for t in (sess.am, sess.draft, sess.draft_len, sess.hist, sess.pos, sess.emit, sess.tok, sess.stats)]
    assert calls[-1][2]["live"] == id(sess.live) and calls[-2][2]["out"] == id(sess.am)
    assert not sampling or calls[-2][2]["ctr"] == id(sess.ctr) == calls[-3][1][1]
    for name in ("spec_rows_rope_kv", "spec_rows_attention"):
        got = [c[1] for c in calls if c[0] == name]
        assert [g[:3] for g in got] == [[id(sess.qkv), id(cache.k[li]), id(cache.v[li])] for li in range(L)] and all(id(sess.pos) in g for g in got)


def test_the_two_verify_steps_share_one_body():
    """What the subclasses keep is what differs: the launch order, the capture and the check are the base class's."""
    for cls in (spec.SpecDecodeSession, spec.SpecRowsSession):
        assert issubclass(cls, spec._VerifyStep)
        for name in ("_enqueue_step", "_capture", "check"):
            assert name not in vars(cls) and name in vars(spec._VerifyStep)
    assert spec._norm_gemv is decode._norm_gemv
