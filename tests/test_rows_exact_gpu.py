"""Every norm, pool, splice, cast and glue kernel against the row oracle (tests/row_oracle.py): one test per dispatch branch of
launch_norm (the id names the branch; the oracle's mirror of the dispatch asserts it), every form on every branch, planted rows,
partial tails, guard rows after every output, and bit-exact results wherever the operation is exactly representable.

Through valley_amd.ops / ops_f32 where the wrapper takes the caller's output; through the C ABI where it allocates its own
(both-output LayerNorm, pool_tokens, temporal_scores, cast, delta_prep / delta_finish, the fp32 twins): the output has to stand
inside a guard buffer.

No kernel needed a fix.  Two things in the plan did: (4097, 2048) is norm_kernel<8> (512 float4 = 8 per lane), so (4097, 2052) was
added for norm_kernel<16>; and one 16-bit ulp alone cannot hold at outputs below 1e-3 in magnitude, where the ulp is smaller than any
fp32 evaluation's error, so the fp32 rule's bound is added to the ulp (tests/row_oracle.py, proof in tests/test_rows_exact_cpu.py).
Figures of the largest case, norm_kernel<32> at (4097, 8192), bf16: fp32 output 5.1e-6 from float64 (E = 2.5e-6), 2.8e-5 of the
16-bit elements differ from ref64.to(HALF) (cap 1e-3).

Measured on one MI355X: the module's 263 tests take 5 s of wall time on the bf16 library and 6 s on the fp16 library (no test above
one second); the fp16 kernel-suite child of tests/test_fp16_gpu.py takes 78 s with this module included (its limit is 600 s)."""
import pytest
import torch

from tests import row_oracle as R
from valley_amd.runtime import HALF

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def L():
    from valley_amd import lib
    return lib.load()


def st():
    return torch.cuda.current_stream().cuda_stream


def call(name, *args):
    rc = getattr(L(), name)(*args, st())
    assert rc == 0, (name, rc, L().vly_last_error())
    torch.cuda.synchronize()


def ptr(t):
    return None if t is None else t.data_ptr()


# ---- 1. norms ---------------------------------------------------------------------------------------------------------------------
NORM_IDS = [f"{b}-{M}x{D}" for b, M, D in R.NORM_SHAPES]


def run_norm(case, form):
    """-> (h, y16, y32) views inside their guard buffers, and the buffers."""
    from valley_amd import ops
    M, D = case.M, case.D
    hbuf, h = R.guarded_rows(M, D, torch.float32, DEV)
    h.copy_(R.expand(case, case.xu, DEV))
    x0 = h.clone()
    g, b = case.gamma.to(DEV), case.beta.to(DEV)
    bufs = {"h": hbuf}
    y16 = y32 = None
    if not form.endswith("only"):
        bufs["y16"], y16 = R.guarded_rows(M, D, HALF, DEV)
    if form == "ln16":
        ops.layernorm(h, g, b, R.LN_EPS, out=y16)
    elif form == "ln16+32":
        bufs["y32"], y32 = R.guarded_rows(M, D, torch.float32, DEV)
        call("vly_layernorm", h.data_ptr(), g.data_ptr(), b.data_ptr(), y16.data_ptr(), y32.data_ptr(), M, D, R.LN_EPS)
    elif form == "rms":
        ops.rmsnorm(h, g, R.RMS_EPS, out=y16)
    else:
        d0 = R.expand(case, case.d0u, DEV)
        d1 = R.expand(case, case.d1u, DEV) if form.startswith("add2") else None
        rms = form.endswith("rms") or form == "add2_only"               # (add-only: once through each entry point's template)
        only = form.endswith("only")
        ops.add_norm(h, d0, None if only else g, None if (only or rms) else b, R.RMS_EPS if rms else R.LN_EPS, out=y16, rms=rms, delta2=d1)
    torch.cuda.synchronize()
    if not form.startswith("add"):
        R.assert_bits(h, x0, f"{form}: the input of a plain norm changed")
    return (h if form.startswith("add") else None), y16, y32, bufs


@pytest.mark.parametrize("form", R.NORM_FORMS)
@pytest.mark.parametrize("branch,M,D", R.NORM_SHAPES, ids=NORM_IDS)
def test_norm(branch, M, D, form):
    case = R.norm_case(M, D, HALF, branch)
    h, y16, y32, bufs = run_norm(case, form)
    res = R.check_norm(case, form, h, y16, y32, f"{form} on {branch} ({M}, {D})")
    print(branch, M, D, form, res)
    for name, buf in bufs.items():
        R.assert_guards(buf, M, D, f"{form} ({M}, {D}): {name}")


def test_norm_arguments():
    """-22 for D % 4 != 0, D > 8192 and a misaligned pointer, from every entry point's launcher, before anything is launched."""
    lib = L()
    x = torch.zeros((4, 8200), dtype=torch.float32, device=DEV)
    y = torch.full((4, 8200), R.SENTINEL, dtype=HALF, device=DEV)
    g = torch.ones((8200,), dtype=torch.float32, device=DEV)
    d = torch.zeros((4, 8200), dtype=HALF, device=DEV)
    for D in (1026, 8196, 6):
        assert lib.vly_layernorm(x.data_ptr(), g.data_ptr(), g.data_ptr(), y.data_ptr(), None, 2, D, 1e-5, st()) == -22
        assert lib.vly_rmsnorm(x.data_ptr(), g.data_ptr(), y.data_ptr(), 2, D, 1e-6, st()) == -22
        assert lib.vly_add_rmsnorm(x.data_ptr(), d.data_ptr(), g.data_ptr(), y.data_ptr(), 2, D, 1e-6, st()) == -22
        assert lib.vly_add2_layernorm(x.data_ptr(), d.data_ptr(), d.data_ptr(), g.data_ptr(), g.data_ptr(), y.data_ptr(), 2, D, 1e-5, st()) == -22
    xp, gp, yp, dp = x.data_ptr(), g.data_ptr(), y.data_ptr(), d.data_ptr()
    assert lib.vly_rmsnorm(xp + 4, gp, yp, 2, 1024, 1e-6, st()) == -22                       # x: 16 bytes
    assert lib.vly_rmsnorm(xp, gp + 8, yp, 2, 1024, 1e-6, st()) == -22                       # gamma: 16 bytes
    assert lib.vly_rmsnorm(xp, gp, yp + 2, 2, 1024, 1e-6, st()) == -22                       # y16: 8 bytes
    assert lib.vly_layernorm(xp, gp, gp + 4, yp, None, 2, 1024, 1e-5, st()) == -22           # beta
    assert lib.vly_layernorm(xp, gp, gp, yp, xp + 8, 2, 1024, 1e-5, st()) == -22             # y32: 16 bytes
    assert lib.vly_add_layernorm(xp, dp + 2, gp, gp, yp, 2, 1024, 1e-5, st()) == -22         # delta: 8 bytes
    assert lib.vly_add2_rmsnorm(xp, dp, dp + 4, gp, yp, 2, 1024, 1e-6, st()) == -22          # the second delta
    assert lib.vly_rmsnorm(xp, gp, yp, 2, 1024, 1e-6, st()) == 0                             # (and the same call, aligned, runs)
    torch.cuda.synchronize()
    assert bool((y[2:] == R.SENTINEL).all()) and bool((x == 0).all())


@pytest.mark.parametrize("rms", [0, 1], ids=["ln", "rms"])
@pytest.mark.parametrize("M,D", R.NORM_F32_SHAPES)
def test_norm_f32_twins(M, D, rms):
    """vly_norm_f32 and vly_norm_split3_f32, the vector kernels (D % 4 == 0) and the scalar ones, Kp > D: pad columns zero."""
    from valley_amd import ops_f32
    case = R.NormCase(M, D, HALF)
    x, g, b = case.xu[case.idx].to(DEV), case.gamma.to(DEV), case.beta.to(DEV)
    form = "rms" if rms else "ln16"
    ref, e_plain, e_big = case.truth(form)
    full = ref[case.idx]
    bound = R.f32_bounds(case, e_plain, e_big, DEV)
    ybuf, y = R.guarded_rows(M, D, torch.float32, DEV)
    ops_f32.norm(x, g, None if rms else b, R.RMS_EPS if rms else R.LN_EPS, out=y)
    torch.cuda.synchronize()
    print(M, D, form, "E", e_plain, e_big, "err", R.assert_f32(y, full, bound, f"norm_f32 {form} ({M}, {D})"))
    R.assert_guards(ybuf, M, D, "norm_f32")
    if "zero" in case.planted:
        r = case.planted["zero"]
        assert bool((y[r] == 0).all()) if rms else bool((y[r] == b).all())
    k64 = (D + 63) // 64 * 64
    for Kp in ([k64] if k64 > D else []) + [k64 + 64]:
        obuf, o3 = R.guarded_rows(M, 3 * Kp, HALF, DEV)
        call("vly_norm_split3_f32", x.data_ptr(), g.data_ptr(), None if rms else b.data_ptr(), o3.data_ptr(), M, D, Kp,
             R.RMS_EPS if rms else R.LN_EPS, rms)
        R.split3_check(o3, full, D, Kp, max(e_plain, e_big), f"norm_split3_f32 {form} ({M}, {D}) Kp {Kp}")
        R.assert_guards(obuf, M, 3 * Kp, "norm_split3_f32")


# ---- 2. RoPE + KV append ------------------------------------------------------------------------------------------------------------
def _rope_run(shape, dtype, host_past, dev_past):
    from valley_amd import ops, ops_f32
    B, S, heads, _, ctx_max = shape
    cos, sin = R.rope_tables(ctx_max)
    qkv0 = R.rope_inputs(B, S, heads, dtype)
    qbuf, q = R.guarded_rows(B * S, 3 * heads * 128, dtype, DEV)
    q.copy_(qkv0)
    kc = torch.full((B, heads, ctx_max, 128), R.SENTINEL, dtype=dtype, device=DEV)
    vc = torch.full_like(kc, R.SENTINEL)
    if dtype == torch.float32:
        ops_f32.rope_kv(q, kc, vc, cos.to(DEV), sin.to(DEV), B, S, heads, host_past)
    else:
        pd = None if dev_past is None else torch.tensor([dev_past], dtype=torch.int32, device=DEV)
        ops.rope_kv(q, kc, vc, cos.to(DEV), sin.to(DEV), B, S, heads, host_past, past_dev=pd)
    torch.cuda.synchronize()
    R.assert_guards(qbuf, B * S, 3 * heads * 128, "rope_kv: qkv")
    return qkv0, q, kc, vc


@pytest.mark.parametrize("shape", R.ROPE_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_rope_kv(shape):
    qkv0, q, kc, vc = _rope_run(shape, HALF, shape[3], None)
    R.check_rope(shape, qkv0, q, kc, vc, shape[3])


@pytest.mark.parametrize("shape", R.ROPE_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_rope_kv_f32(shape):
    qkv0, q, kc, vc = _rope_run(shape, torch.float32, shape[3], None)
    R.check_rope(shape, qkv0, q, kc, vc, shape[3], "rope_kv_f32")


@pytest.mark.parametrize("shape", R.ROPE_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_rope_kv_device_position_and_clamp(shape):
    """past_len_dev is the position used (the host value is another one on purpose); above ctx_max - S it clamps to ctx_max - S."""
    B, S, heads, past, ctx_max = shape
    host = 0 if past else ctx_max - S
    qkv0, q, kc, vc = _rope_run(shape, HALF, host, past)
    R.check_rope(shape, qkv0, q, kc, vc, past, "rope_kv, device position")
    for over in (ctx_max - S + 1, ctx_max + 1000):
        qkv0, q, kc, vc = _rope_run(shape, HALF, 0, over)
        R.check_rope(shape, qkv0, q, kc, vc, ctx_max - S, f"rope_kv, device position {over} clamped")


# ---- 3. pooling and scores ------------------------------------------------------------------------------------------------------------
def _pool_run(feats, mode, scores, dtype):
    B, T, _, W = feats.shape
    obuf, out = R.guarded_rows(B * (256 + T), W, dtype, DEV)
    fd = feats.to(DEV)
    sd = None if scores is None else scores.to(DEV)
    call("vly_pool_tokens_f32" if dtype == torch.float32 else "vly_pool_tokens", fd.data_ptr(), out.data_ptr(), B, T, W, mode, ptr(sd))
    R.assert_guards(obuf, B * (256 + T), W, "pool_tokens: out")
    return out.view(B, 256 + T, W)


@pytest.mark.parametrize("twin", [False, True], ids=["half", "f32"])
@pytest.mark.parametrize("mode", [R.POOL_MEAN, R.POOL_MAX, R.POOL_IMPORTANCE], ids=["mean", "max", "importance"])
@pytest.mark.parametrize("B,T,W", R.POOL_SHAPES)
def test_pool_tokens(B, T, W, mode, twin):
    feats = R.pool_feats(B, T, W)
    scores = R.pool_scores(B, T) if mode == R.POOL_IMPORTANCE else None
    out = _pool_run(feats, mode, scores, torch.float32 if twin else HALF)
    R.check_pool(feats, mode, scores, out, f"pool_tokens{'_f32' if twin else ''} ({B}, {T}, {W}) mode {mode}")


def test_pool_tokens_importance_single_frame_weight_is_one():
    feats = R.pool_feats(1, 1, 4)
    out = _pool_run(feats, R.POOL_IMPORTANCE, torch.tensor([[-37.5]]), HALF)
    R.assert_bits(out.cpu()[:, :256].contiguous(), feats[:, 0, 1:].to(HALF), "importance at T = 1")


@pytest.mark.parametrize("with_bias", [True, False], ids=["bias", "nobias"])
@pytest.mark.parametrize("F,W", R.SCORE_SHAPES)
def test_temporal_scores_exact(F, W, with_bias):
    feats, w, bias, truth = R.score_case(F, W, with_bias)
    buf = torch.full((F + 3,), R.SENTINEL, dtype=torch.float32, device=DEV)
    fd, wd, bd = feats.to(DEV), w.to(DEV), None if bias is None else bias.to(DEV)
    call("vly_temporal_scores", fd.data_ptr(), wd.data_ptr(), ptr(bd), buf.data_ptr(), F, W)
    R.assert_bits(buf[:F].cpu(), truth.float(), f"temporal_scores F = {F} W = {W}")
    assert bool((buf[F:] == R.SENTINEL).all()), "temporal_scores wrote past score F - 1"


# ---- 4. splice, cast, patchify, ViT embedding, counter -------------------------------------------------------------------------------
@pytest.mark.parametrize("twin", [False, True], ids=["half", "f32"])
@pytest.mark.parametrize("R_", R.SPLICE_R)
@pytest.mark.parametrize("H", R.SPLICE_H)
def test_embed_splice(H, R_, twin):
    from valley_amd import ops, ops_f32
    dtype = torch.float32 if twin else HALF
    emb, vis = R.splice_tables(H, dtype)
    fn = ops_f32.embed_splice if twin else ops.embed_splice
    for tokens_only in (False, True):
        rmap = R.splice_map(R_, tokens_only)
        obuf, out = R.guarded_rows(R_, H, torch.float32, DEV)
        fn(rmap.to(DEV), emb.to(DEV), None if tokens_only else vis.to(DEV), out=out)
        torch.cuda.synchronize()
        R.assert_bits(out.cpu(), R.splice_truth(rmap, emb, vis), f"embed_splice H = {H} R = {R_}")
        R.assert_guards(obuf, R_, H, "embed_splice: out")


@pytest.mark.parametrize("n", [8, 2056])
def test_cast_to_storage_type(n):
    x = R.cast_values(n, HALF)
    buf = torch.full((n + 16,), R.SENTINEL, dtype=HALF, device=DEV)
    xd = x.to(DEV)
    call("vly_cast_f32_bf16", xd.data_ptr(), buf.data_ptr(), n)
    R.assert_bits(buf[:n].cpu(), x.to(HALF), f"cast n = {n}")
    assert bool((buf[n:] == R.SENTINEL).all()), "cast wrote past element n - 1"


@pytest.mark.parametrize("F", [1, 3])
def test_patchify_every_column_decoded(F):
    from valley_amd import ops
    img = R.patch_image(F, HALF)
    obuf, out = R.guarded_rows(F * 256, 640, HALF, DEV)
    ops.patchify(img.to(DEV), out=out)
    torch.cuda.synchronize()
    R.check_patchify(out, F)
    R.assert_guards(obuf, F * 256, 640, "patchify: out")
    for kp in (592, 640):
        obuf, out = R.guarded_rows(F * 256, kp, torch.float32, DEV)
        imf = R.patch_image(F, torch.float32).to(DEV)
        call("vly_patchify_f32", imf.data_ptr(), out.data_ptr(), F, kp)
        R.check_patchify(out, F, f"patchify_f32 kp = {kp}")
        R.assert_guards(obuf, F * 256, kp, "patchify_f32: out")


@pytest.mark.parametrize("F", [1, 3])
def test_vit_embed_ln(F):
    from valley_amd import ops
    po, cls, pos, gm, bt = (t.to(DEV) for t in R.vit_embed_case(F))
    hbuf, h = R.guarded_rows(F * 257, 1024, torch.float32, DEV)
    ops.vit_embed_ln(po, cls, pos, gm, bt, F, R.LN_EPS, out=h)
    torch.cuda.synchronize()
    R.check_vit_embed(F, h)
    R.assert_guards(hbuf, F * 257, 1024, "vit_embed_ln: h")


@pytest.mark.parametrize("n,delta", R.INCR)
def test_incr_i32(n, delta):
    from valley_amd import ops
    buf = torch.arange(100, 100 + n + 8, dtype=torch.int32, device=DEV)
    want = buf.clone()
    want[4:4 + n] += delta
    ops.incr_i32(buf[4:4 + n], delta)
    torch.cuda.synchronize()
    assert torch.equal(buf, want), (buf.tolist(), want.tolist())


# ---- 5. temporal-transformer glue -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("twin", [False, True], ids=["half", "f32"])
@pytest.mark.parametrize("B,T,H", R.DELTA_SHAPES)
def test_delta_prep(B, T, H, twin):
    feats, pos, _, _ = R.delta_case(B, T, H)
    stt = torch.float32 if twin else HALF
    n = B * 256
    abuf, x_all = R.guarded_rows(n * T, H, stt, DEV)
    l16buf, l16 = R.guarded_rows(n, H, stt, DEV)
    l32buf, l32 = R.guarded_rows(n, H, torch.float32, DEV)
    mbuf, mean = R.guarded_rows(n, H, torch.float32, DEV)
    fd, pd = feats.to(DEV), pos.to(DEV)
    if twin:
        call("vly_delta_prep_f32", fd.data_ptr(), pd.data_ptr(), x_all.data_ptr(), l32.data_ptr(), mean.data_ptr(), B, T, H)
    else:
        call("vly_delta_prep", fd.data_ptr(), pd.data_ptr(), x_all.data_ptr(), l16.data_ptr(), l32.data_ptr(), mean.data_ptr(), B, T, H)
    R.check_delta_prep(feats, pos, x_all, None if twin else l16, l32, mean, f"delta_prep{'_f32' if twin else ''} ({B}, {T}, {H})")
    for name, buf, rows in (("x_all", abuf, n * T), ("x_last16", l16buf, 0 if twin else n), ("x_last32", l32buf, n), ("mean", mbuf, n)):
        R.assert_guards(buf, rows, H, f"delta_prep: {name}")


@pytest.mark.parametrize("twin", [False, True], ids=["half", "f32"])
@pytest.mark.parametrize("B,T,H", R.DELTA_SHAPES)
def test_delta_finish(B, T, H, twin):
    feats, _, delta, mean_in = R.delta_case(B, T, H)
    stt = torch.float32 if twin else HALF
    obuf, out = R.guarded_rows(B * (256 + T), H, stt, DEV)
    fd, dd, md = feats.to(DEV), delta.to(DEV), mean_in.to(DEV)
    call("vly_delta_finish_f32" if twin else "vly_delta_finish", dd.data_ptr(), md.data_ptr(), fd.data_ptr(), out.data_ptr(), B, T, H)
    R.check_delta_finish(feats, delta, mean_in, out.view(B, 256 + T, H), f"delta_finish{'_f32' if twin else ''} ({B}, {T}, {H})")
    R.assert_guards(obuf, B * (256 + T), H, "delta_finish: out")
