"""GPU unit parity: every HIP kernel (through the C ABI) vs a plain fp32 PyTorch statement of the
same op on the same seeded inputs.  Tolerances are written per test: a bound on 16-bit outputs is a multiple of EPS (one rounding of the
storage type: 2^-7 on bf16, 8x smaller on fp16), fp32-output paths are held to their own fp32 bounds."""
import math

import numpy as np
import pytest
import torch

from valley_amd.runtime import HALF  # the library's 16-bit storage type: bf16, or fp16 under VALLEY_PRECISION=fp16 (this process is bound by the environment)

pytestmark = pytest.mark.gpu
EPS = torch.finfo(HALF).eps      # one rounding of the 16-bit storage type: 2^-7 (bf16), 2^-10 (fp16)


def dev():
    return torch.device("cuda:0")


def rnd(shape, seed, scale=1.0, dtype=torch.float32):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.randn(shape, generator=g) * scale).to(dtype)


def relerr(got, ref):
    got, ref = got.float().cpu(), ref.float().cpu()
    return float((got - ref).norm() / (ref.norm() + 1e-30))


def maxabs(got, ref):
    return float((got.float().cpu() - ref.float().cpu()).abs().max())


# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tile", [1, 2, 3, 4, 5, 6, 7, 8, 9, 51, 53, 54, 55, 73, 74, 76, 83, 84, 86, 93, 94, 97, 98, 99, 197, 198, 199])
@pytest.mark.parametrize("M,N,K", [(300, 264, 128), (1028, 1024, 1024), (64, 512, 64), (513, 4096, 640)])
def test_gemm_plain(M, N, K, tile):
    from valley_amd import ops
    a = rnd((M, K), 1, dtype=HALF)
    w = rnd((N, K), 2, 0.05, dtype=HALF)
    ref = a.float() @ w.float().t()
    out = ops.gemm_mfma(a.to(dev()), w.to(dev()), out_dtype=torch.float32, tile_hint=tile)
    torch.cuda.synchronize()
    # fp32 accumulation of exact bf16 products: only summation-order noise
    assert maxabs(out, ref) < 2e-4 * math.sqrt(K), (maxabs(out, ref))
    out16 = ops.gemm_mfma(a.to(dev()), w.to(dev()), tile_hint=tile)
    assert relerr(out16, ref) < 0.512 * EPS


@pytest.mark.parametrize("tile", [1, 2, 3, 4, 5, 6, 7, 8, 9, 51, 53, 54, 55, 73, 74, 76, 83, 84, 86, 93, 94, 97, 98, 99, 197, 198, 199])
def test_gemm_epilogues(tile):
    from valley_amd import ops
    M, N, K = 771, 1024, 256
    a = rnd((M, K), 3, dtype=HALF)
    w = rnd((N, K), 4, 0.05, dtype=HALF)
    bias = rnd((N,), 5, 0.5)
    res = rnd((M, N), 6)
    base = a.float() @ w.float().t() + bias
    d = dev()
    # bias + residual, fp32 out (the residual-stream update)
    out = ops.gemm_mfma(a.to(d), w.to(d), bias.to(d), res.to(d), out_dtype=torch.float32, tile_hint=tile)
    assert maxabs(out, base + res) < 5e-3
    # quick_gelu
    out = ops.gemm_mfma(a.to(d), w.to(d), bias.to(d), epilogue=ops.EPI_QUICK_GELU, tile_hint=tile)
    ref = base * torch.sigmoid(1.702 * base)
    assert relerr(out, ref) < 0.512 * EPS
    # swiglu on interleaved rows
    out = ops.gemm_mfma(a.to(d), w.to(d), epilogue=ops.EPI_SWIGLU, tile_hint=tile)
    nb = a.float() @ w.float().t()
    ref = torch.nn.functional.silu(nb[:, 0::2]) * nb[:, 1::2]
    assert out.shape == (M, N // 2)
    assert relerr(out, ref) < 0.512 * EPS


@pytest.mark.parametrize("tile", [1, 2, 5, 7, 8, 9, 51, 86, 94, 97, 98, 99, 197, 198, 199])
def test_gemm_ragged_columns_through_lds_epilogue(tile):
    """N % 8 == 4: the last 16-byte chunk of every output row is half valid (the LDS full-line epilogue writes
    8 bytes there), with and without the SwiGLU halving; an output row stride that is not 16-byte aligned
    (falls back to the fragment stores) gives the same values."""
    from valley_amd import ops
    M, K = 333, 192
    for N, epi in ((260, ops.EPI_NONE), (520, ops.EPI_SWIGLU), (132, ops.EPI_QUICK_GELU)):
        a = rnd((M, K), 61, dtype=HALF).to(dev())
        w = rnd((N, K), 62, 0.05, dtype=HALF).to(dev())
        base = a.float() @ w.float().t()
        if epi == ops.EPI_SWIGLU:
            ref = torch.nn.functional.silu(base[:, 0::2]) * base[:, 1::2]
        elif epi == ops.EPI_QUICK_GELU:
            ref = base * torch.sigmoid(1.702 * base)
        else:
            ref = base
        No = ref.shape[1]
        out = torch.full((M, No + 12), 7.0, dtype=HALF, device=dev())         # guard columns
        assert (No + 12) % 8 == 0 and No % 8 == 4
        ops.gemm_mfma(a, w, epilogue=epi, out=out[:, :No], tile_hint=tile)              # ldc % 8 == 0: 16-byte aligned rows
        assert relerr(out[:, :No], ref) < 0.512 * EPS
        assert float((out[:, No:].float() - 7.0).abs().max()) == 0.0                   # nothing written past N
        out2 = torch.full((M, No + 2), 7.0, dtype=HALF, device=dev())         # ldc % 8 != 0: fragment-store path
        ops.gemm_mfma(a, w, epilogue=epi, out=out2[:, :No], tile_hint=tile)
        assert torch.equal(out2[:, :No], out[:, :No])
        assert float((out2[:, No:].float() - 7.0).abs().max()) == 0.0


def test_gemm_strided_a_and_asymmetric():
    """A with a row stride (a slice of a wider buffer) and a weight with one hot row/col: catches
    transposed fragments that symmetric data would hide."""
    from valley_amd import ops
    d = dev()
    big = rnd((200, 512), 7, dtype=HALF).to(d)
    a = big[:, 128:384]
    w = torch.zeros((128, 256), dtype=HALF)
    w[3, 17] = 1.0
    w[100, 255] = 2.0
    out = ops.gemm_mfma(a, w.to(d), out_dtype=torch.float32)
    ref = a.float().cpu() @ w.float().t()
    assert maxabs(out, ref) == 0.0


@pytest.mark.parametrize("M", [1, 2, 3, 5, 8, 11, 16])
def test_gemv(M):
    """vly_gemv_bf16: the VALU weight-streaming kernels (M <= 2) and, from three rows on, the matrix-core form (round 5:
    gemv_mfma_kernel — N = 1000 leaves the last 16-row block half empty, M = 11 / 16 are beyond the VALU kernels' eight rows)."""
    from valley_amd import ops
    N, K = 1000, 1024
    d = dev()
    a = rnd((M, K), 8, dtype=HALF)
    w = rnd((N, K), 9, 0.05, dtype=HALF)
    bias = rnd((N,), 10, 0.5)
    res = rnd((M, N), 11)
    base = a.float() @ w.float().t()
    out = ops.gemv(a.to(d), w.to(d), bias.to(d), res.to(d), out_dtype=torch.float32)
    assert maxabs(out, base + bias + res) < 2e-3
    out = ops.gemv(a.to(d), w.to(d), epilogue=ops.EPI_SWIGLU)
    ref = torch.nn.functional.silu(base[:, 0::2]) * base[:, 1::2]
    assert relerr(out, ref) < 0.512 * EPS
    if M >= 3:
        # a row's result depends on that row and the weights only: the same rows inside a larger batch give the same bits
        # (serving.ContinuousBatcher: a request's tokens do not depend on what the other slots hold)
        # (inside one form of the kernel: up to eight rows and nine to sixteen rows may take different row-block shapes, hence
        # different summation orders — a decode session's batch is fixed, so a request never crosses that line)
        top = 8 if M <= 8 else 16
        big = torch.cat([a, rnd((top - M, K), 12, dtype=HALF)], 0)[:top].to(d) if M < top else a.to(d)
        full = ops.gemv(big, w.to(d), bias.to(d), out_dtype=torch.float32)
        assert torch.equal(full[:M], ops.gemv(a.to(d), w.to(d), bias.to(d), out_dtype=torch.float32))


@pytest.mark.parametrize("M,N,K", [(3, 64, 64), (8, 20, 128), (16, 1000, 192), (9, 48, 320), (4, 4096, 64 * 21)])
def test_gemv_rows_short_and_ragged_k(M, N, K):
    """The LDS-ring form at the edges of its K split: fewer K pairs than waves (K = 64: one pair, three idle waves), pair counts that
    do not fill the ring (2, 3, 5) or a group (21), a last row block with 4 valid rows (N = 20), both slot layouts (M <= 8, M > 8)."""
    from valley_amd import ops
    d = dev()
    a = rnd((M, K), 31, dtype=HALF).to(d)
    w = rnd((N, K), 32, 0.05, dtype=HALF).to(d)
    bias = rnd((N,), 33, 0.5).to(d)
    base = a.float() @ w.float().t()
    out = ops.gemv(a, w, bias, out_dtype=torch.float32)
    assert maxabs(out.cpu(), (base + bias).cpu()) < 2e-3 * max(1.0, float(base.abs().max()))
    o16 = ops.gemv(a, w)
    assert relerr(o16, base) < 0.512 * EPS


@pytest.mark.parametrize("N,K,epi", [(5120, 5120, 0), (27648, 5120, 2), (5120, 13824, 0), (4096, 11008, 0), (32008, 5120, 0)])
def test_gemv_rows_on_the_matrix_cores_at_decode_shapes(N, K, epi):
    """The decode projections of the 13B / 7B models at eight live requests (K = 11008 = 172 pairs: the ragged tail of the K split;
    N = 32008: a partial last block) against fp32, and the VALU kernel's result on the same operands (VLY_GEMV_MFMA=0 is read
    once per process, so the comparison is with the reference only)."""
    from valley_amd import ops
    d = dev()
    M = 8
    a = rnd((M, K), 21, dtype=HALF).to(d)
    w = rnd((N, K), 22, 0.02, dtype=HALF).to(d)
    base = a.float() @ w.float().t()
    if epi == 2:
        out = ops.gemv(a, w, epilogue=ops.EPI_SWIGLU)
        ref = torch.nn.functional.silu(base[:, 0::2]) * base[:, 1::2]
        assert relerr(out, ref) < 0.64 * EPS
    else:
        res = rnd((M, N), 23).to(d)
        out = ops.gemv(a, w, residual=res, out_dtype=torch.float32)
        assert relerr(out, base + res) < 1e-5 if HALF == torch.float32 else relerr(out, base + res) < 2e-3


@pytest.mark.parametrize("M,N,K", [(1, 15360, 5120), (2, 1000, 4096), (1, 32008, 5120), (1, 4098, 2048), (2, 64, 6144), (1, 6, 4096)])
def test_gemv_rmsnorm_is_bit_identical_to_the_pair(M, N, K):
    """vly_gemv_rmsnorm_bf16 == vly_rmsnorm then vly_gemv_bf16, bit for bit (all three epilogue / out forms the decode step
    uses, plus bias + residual), and both agree with the fp32 formula."""
    from valley_amd import ops
    d = dev()
    h = (rnd((M, K), 31, 1.5) + 0.1).to(d)
    g = (rnd((K,), 32, 0.1) + 1.0).to(d)
    w = rnd((N, K), 33, 0.03, dtype=HALF).to(d)
    bias = rnd((N,), 34, 0.5).to(d)
    res = rnd((M, N), 35).to(d)
    x = ops.rmsnorm(h, g, 1e-6)
    for kw in (dict(), dict(out_dtype=torch.float32), dict(bias=bias, residual=res, out_dtype=torch.float32)) + \
            ((dict(epilogue=ops.EPI_SWIGLU),) if N % 2 == 0 else ()):
        pair = ops.gemv(x, w, **kw)
        fused = ops.gemv_rmsnorm(h, g, 1e-6, w, **kw)
        assert torch.equal(pair, fused), kw
    hf = h.float().cpu()
    xr = (g.cpu() * (hf * torch.rsqrt(hf.pow(2).mean(-1, keepdim=True) + 1e-6))).to(HALF).float()
    ref = xr @ w.float().cpu().t()
    assert relerr(ops.gemv_rmsnorm(h, g, 1e-6, w, out_dtype=torch.float32), ref) < 0.384 * EPS
    assert not ops.gemv_rmsnorm_ok(3, K) and not ops.gemv_rmsnorm_ok(1, 1024)
    with pytest.raises(Exception):
        ops.gemv_rmsnorm(h[:, :1024].contiguous(), g[:1024].contiguous(), 1e-6, w[:, :1024].contiguous())


# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [1024, 4096, 5120, 256])
def test_norms(D):
    from valley_amd import ops
    d = dev()
    x = rnd((37, D), 12, 2.0) + 0.3
    g = rnd((D,), 13, 0.1) + 1.0
    b = rnd((D,), 14, 0.1)
    y16, y32 = ops.layernorm(x.to(d), g.to(d), b.to(d), 1e-5, want_f32=True)
    ref = torch.nn.functional.layer_norm(x, (D,), g, b, 1e-5)
    assert maxabs(y32, ref) < 2e-5
    assert maxabs(y16, ref.to(HALF)) <= 5.12 * EPS   # at most one 16-bit ulp at |x| < 8 (4 EPS)
    y = ops.rmsnorm(x.to(d), g.to(d), 1e-6)
    ref = g * (x * torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + 1e-6))
    assert relerr(y, ref) < 0.384 * EPS


def test_patchify_matches_conv():
    from valley_amd import ops
    d = dev()
    F = 3
    img = rnd((F, 3, 224, 224), 15, dtype=HALF)
    wt = rnd((1024, 3, 14, 14), 16, 0.02, dtype=HALF)
    cols = ops.patchify(img.to(d))
    ref_cols = torch.nn.functional.unfold(img.float(), kernel_size=14, stride=14).transpose(1, 2).reshape(F * 256, 588)
    assert maxabs(cols[:, :588], ref_cols) == 0.0
    assert float(cols[:, 588:].float().abs().max()) == 0.0
    wpad = torch.zeros((1024, 640), dtype=HALF)
    wpad[:, :588] = wt.reshape(1024, 588)
    out = ops.gemm_mfma(cols, wpad.to(d), out_dtype=torch.float32)
    ref = torch.nn.functional.conv2d(img.float(), wt.float(), stride=14).flatten(2).transpose(1, 2).reshape(F * 256, 1024)
    assert maxabs(out, ref) < 2e-3


def test_vit_embed_ln():
    from valley_amd import ops
    d = dev()
    F = 2
    po = rnd((F * 256, 1024), 17)
    cls, pos = rnd((1024,), 18), rnd((257, 1024), 19, 0.1)
    g, b = rnd((1024,), 20, 0.1) + 1.0, rnd((1024,), 21, 0.1)
    out = ops.vit_embed_ln(po.to(d), cls.to(d), pos.to(d), g.to(d), b.to(d), F, 1e-5)
    emb = torch.cat([cls.expand(F, 1, 1024), po.view(F, 256, 1024)], 1) + pos[None]
    ref = torch.nn.functional.layer_norm(emb, (1024,), g, b, 1e-5).view(F * 257, 1024)
    assert maxabs(out, ref) < 2e-5


def test_vit_attention():
    from valley_amd import ops
    d = dev()
    F = 3
    qkv = rnd((F * 257, 3072), 22, 1.0, dtype=HALF)
    qkv[5, :64] *= 6.0            # one spiky query row
    out = ops.vit_attention(qkv.to(d), F)
    x = qkv.float().view(F, 257, 3, 16, 64)
    q, k, v = (x[:, :, i].transpose(1, 2) for i in range(3))
    a = torch.softmax(q @ k.transpose(-1, -2) * 0.125, dim=-1)
    ref = (a @ v).transpose(1, 2).reshape(F * 257, 1024)
    assert maxabs(out, ref) < 3.2 * EPS
    assert relerr(out, ref) < 0.768 * EPS


def test_llama_attention_register_staged_kernel_still_passes():
    """VLY_LLAMA_ATTN=1 selects the round-2 kernel (llama_attn_kernel: tiles through registers, one workgroup per CU) in the
    EXPERIMENTAL library (libvalley_hip_exp.so, VALLEY_EXPERIMENTAL=1) — the default kernel's bit-identity witness; the switch is read
    once per process, so the attention tests re-run under it in a child."""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.join(root, "tests", "test_kernels_gpu.py"), "-q", "-x", "-p", "no:cacheprovider",
                        "-k", "attention and not register_staged and not forced_kernel"],
                       env=dict(os.environ, VLY_LLAMA_ATTN="1", VALLEY_EXPERIMENTAL="1"), capture_output=True, timeout=900, cwd=root)
    assert r.returncode == 0, r.stdout.decode(errors="replace")[-1500:]


@pytest.mark.parametrize("F,kernel", [(3, "1"), (40, "1"), (70, "1"), (40, "4")])
def test_vit_attention_forced_kernel(F, kernel):
    """VLY_VIT_ATTN=1 runs rounds 2-5's workgroup-per-head kernel (vit_attn_kernel, kept as the A/B arm of the persistent default), 4 names
    the default explicitly; both against the fp32 formula.  The switch is read once per process, so the run is a child (tools/vit_attn_time.py)."""
    import json
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, VLY_VIT_ATTN=kernel)
    r = subprocess.run([sys.executable, os.path.join(root, "tools", "vit_attn_time.py"), str(F)], env=env, capture_output=True, timeout=300)
    assert r.returncode == 0, r.stderr.decode(errors="replace")[-500:]
    line = json.loads([ln for ln in r.stdout.decode().splitlines() if ln.startswith("{")][-1])
    assert line["kernel"] == kernel and line["rel_l2_vs_fp32"] < 0.512 * EPS and line["max_abs"] < 5.12 * EPS, line


@pytest.mark.parametrize("F", [1, 17, 64, 129])
def test_vit_attention_persistent_default(F):
    """vly_vit_attention = the persistent kernel (one 16-wave workgroup per CU walking its heads): against the fp32 formula (spiky rows
    included), every frame and head, with fewer heads than CUs (16), with a ragged walk (272 and 2064 heads on 256 CUs) and an even one
    (1024); the 257th query — split over the keys across eight waves and merged one head later — checked on its own."""
    from valley_amd import ops
    d = dev()
    qkv = rnd((F * 257, 3072), 220 + F, 1.0, dtype=HALF)
    qkv[5, :64] *= 6.0
    qkv[256, 64:128] *= 5.0       # the last query of frame 0, head 1
    qkv[F * 257 - 1, :64] *= 4.0
    out = ops.vit_attention(qkv.to(d), F).cpu()
    worst = worst_last = 0.0
    for f0 in range(0, F, 16):
        n = min(16, F - f0)
        x = qkv[f0 * 257:(f0 + n) * 257].float().view(n, 257, 3, 16, 64)
        q, k, v = (x[:, :, i].transpose(1, 2) for i in range(3))
        a = torch.softmax(q @ k.transpose(-1, -2) * 0.125, dim=-1)
        ref = (a @ v).transpose(1, 2).reshape(n, 257, 1024)
        got = out[f0 * 257:(f0 + n) * 257].float().view(n, 257, 1024)
        worst = max(worst, float((got - ref).abs().max()))
        worst_last = max(worst_last, float((got[:, 256] - ref[:, 256]).abs().max()))
        assert relerr(got, ref) < 0.768 * EPS
    assert worst < 3.2 * EPS and worst_last < 3.2 * EPS, (worst, worst_last)


@pytest.mark.parametrize("F", [5, 40, 130])
def test_vit_attention_three_kernels_agree(F, monkeypatch):
    """The persistent default, the two-workgroups-per-CU form (VLY_VIT_ATTN=5, attention_vit_pp.inc) and rounds 2-5's workgroup-per-head
    kernel (VLY_VIT_ATTN=1) on the same inputs (the switch is read per call): the 256 full-tile queries of every head are bit-identical between
    the two persistent kernels (same arithmetic, same order); the 257th query (its partials associate differently) and the workgroup-per-head
    kernel (scale outside the exponent's FMA) agree to the storage type's rounding."""
    from valley_amd import ops
    d = dev()
    qkv = rnd((F * 257, 3072), 300 + F, 1.0, dtype=HALF).to(d)
    monkeypatch.delenv("VLY_VIT_ATTN", raising=False)
    a = ops.vit_attention(qkv, F).view(F, 257, 1024)
    monkeypatch.setenv("VLY_VIT_ATTN", "5")
    b = ops.vit_attention(qkv, F).view(F, 257, 1024)
    monkeypatch.setenv("VLY_VIT_ATTN", "1")
    c = ops.vit_attention(qkv, F).view(F, 257, 1024)
    monkeypatch.delenv("VLY_VIT_ATTN", raising=False)
    assert torch.equal(a[:, :256], b[:, :256])
    assert relerr(b[:, 256].float(), a[:, 256].float()) < 0.384 * EPS and relerr(c.float(), a.float()) < 0.384 * EPS
    assert torch.equal(a, ops.vit_attention(qkv, F).view(F, 257, 1024))          # (and run to run)


@pytest.mark.parametrize("mode", [0, 1])
def test_pool_tokens(mode):
    from valley_amd import ops
    d = dev()
    B, T, W = 2, 5, 1024
    f = rnd((B, T, 257, W), 23)
    out = ops.pool_tokens(f.to(d).view(-1, W), B, T, mode)
    pooled = f[:, :, 1:].mean(1) if mode == 0 else f[:, :, 1:].max(1)[0]
    ref = torch.cat([pooled, f[:, :, 0]], dim=1)
    assert maxabs(out, ref.to(HALF)) <= 2.56 * EPS
    assert relerr(out, ref) < 0.384 * EPS


def test_embed_splice():
    from valley_amd import ops
    d = dev()
    V, H, NV = 50, 256, 7
    emb = rnd((V, H), 24, dtype=HALF)
    vis = rnd((NV, H), 25, dtype=HALF)
    rmap = torch.tensor([0, 49, -1, -7, 3, -2, 10], dtype=torch.int32)
    out = ops.embed_splice(rmap.to(d), emb.to(d), vis.to(d))
    ref = torch.stack([emb[v].float() if v >= 0 else vis[-v - 1].float() for v in rmap.tolist()])
    assert maxabs(out, ref) == 0.0


def _rope_tables(n, theta=10000.0):
    inv = 1.0 / (theta ** (torch.arange(0, 128, 2, dtype=torch.float32) / 128))
    ang = torch.arange(n, dtype=torch.float32)[:, None] * inv[None]
    return ang.cos().contiguous(), ang.sin().contiguous()


def _ref_attention(q, k, v, past, key_valid):
    """q [B,h,S,128], k/v [B,h,kv,128] fp32; causal + validity; fp32 softmax."""
    B, h, S, _ = q.shape
    kv = k.shape[2]
    s = q @ k.transpose(-1, -2) * (128 ** -0.5)
    i = torch.arange(S)[:, None] + past
    j = torch.arange(kv)[None]
    allowed = (j <= i)[None, None].expand(B, 1, S, kv)
    if key_valid is not None:
        allowed = allowed & key_valid[:, None, None, :].bool()
    s = torch.where(allowed, s, torch.tensor(-1e30))
    return torch.softmax(s, -1) @ v


@pytest.mark.parametrize("B,S,past,heads,pad", [(2, 75, 0, 2, 9), (1, 336, 0, 3, 0), (2, 1, 130, 2, 5), (1, 40, 100, 2, 0)])
def test_rope_kv_and_llama_attention(B, S, past, heads, pad):
    from valley_amd import ops
    d = dev()
    Hq = heads * 128
    ctx_max = 512
    cos, sin = _rope_tables(ctx_max)
    kc = torch.zeros((B, heads, ctx_max, 128), dtype=HALF)
    vc = torch.zeros_like(kc)
    if past:
        kc[:, :, :past] = rnd((B, heads, past, 128), 30, dtype=HALF)
        vc[:, :, :past] = rnd((B, heads, past, 128), 31, dtype=HALF)
    qkv = rnd((B * S, 3 * Hq), 32, dtype=HALF)
    kcd, vcd, qd = kc.to(d), vc.to(d), qkv.to(d).clone()
    ops.rope_kv(qd, kcd, vcd, cos.to(d), sin.to(d), B, S, heads, past)
    # reference rope
    x = qkv.float().view(B, S, 3, heads, 128)
    pos = torch.arange(S) + past
    c = torch.cat([cos[pos], cos[pos]], -1)[None, :, None]
    sn = torch.cat([sin[pos], sin[pos]], -1)[None, :, None]

    def rot(t):
        return torch.cat([-t[..., 64:], t[..., :64]], -1)
    qr = x[:, :, 0] * c + rot(x[:, :, 0]) * sn
    kr = x[:, :, 1] * c + rot(x[:, :, 1]) * sn
    assert maxabs(qd.view(B, S, 3, heads, 128)[:, :, 0], qr.to(HALF)) <= 5.12 * EPS
    assert maxabs(kcd[:, :, past:past + S], kr.transpose(1, 2).to(HALF)) <= 5.12 * EPS
    assert maxabs(vcd[:, :, past:past + S], x[:, :, 2].transpose(1, 2)) == 0.0
    assert float(kcd[:, :, past + S:].float().abs().max()) == 0.0

    kv = past + S
    valid = torch.ones((B, kv), dtype=torch.uint8)
    if pad:
        valid[0, :pad] = 0                      # left padding on sample 0
    out = ops.llama_attention(qd, kcd, vcd, valid.to(d) if pad else None, B, S, heads, past)
    qf = qd.float().cpu().view(B, S, 3, heads, 128)[:, :, 0].transpose(1, 2)
    ref = _ref_attention(qf, kcd[:, :, :kv].float().cpu(), vcd[:, :, :kv].float().cpu(), past, valid if pad else None)
    ref = ref.transpose(1, 2).reshape(B * S, Hq)
    got = out.float().cpu()
    rows = torch.ones(B * S, dtype=torch.bool)
    if pad and past == 0:
        rows[:pad] = False                      # fully-masked (padded) query rows are don't-care
    assert maxabs(got[rows], ref[rows]) < 3.2 * EPS
    assert relerr(got[rows], ref[rows]) < 0.768 * EPS


@pytest.mark.parametrize("B,past,heads,pad,ctx_max", [(1, 0, 2, 0, 256), (2, 130, 2, 5, 512), (1, 511, 3, 0, 2048),
                                                       (3, 700, 2, 600, 2048), (1, 1300, 1, 0, 2048)])
def test_decode_attention_fused_equals_rope_then_attention(B, past, heads, pad, ctx_max):
    """vly_decode_attention (RoPE + KV append + attention, one launch) vs vly_rope_kv + vly_llama_attention:
    the appended cache rows are bit-identical, the attention output agrees to bf16 rounding (the fused kernel
    uses a chunked online softmax: several chunks at past >= 512, incl. a fully masked first chunk)."""
    from valley_amd import ops
    d = dev()
    Hq = heads * 128
    cos, sin = _rope_tables(ctx_max)
    cos, sin = cos.to(d), sin.to(d)
    kc = torch.zeros((B, heads, ctx_max, 128), dtype=HALF)
    vc = torch.zeros_like(kc)
    if past:
        kc[:, :, :past] = rnd((B, heads, past, 128), 30, dtype=HALF)
        vc[:, :, :past] = rnd((B, heads, past, 128), 31, dtype=HALF)
    qkv = rnd((B, 3 * Hq), 32, dtype=HALF).to(d)
    valid = None
    if pad:
        valid = torch.ones((B, past + 1), dtype=torch.uint8)
        valid[0, :pad] = 0
        valid = valid.to(d)
    k1, v1, q1 = kc.to(d), vc.to(d), qkv.clone()
    ops.rope_kv(q1, k1, v1, cos, sin, B, 1, heads, past)
    want = ops.llama_attention(q1, k1, v1, valid, B, 1, heads, past)
    k2, v2 = kc.to(d), vc.to(d)
    got = ops.decode_attention(qkv, k2, v2, cos, sin, valid, B, heads, past)
    assert torch.equal(k1, k2) and torch.equal(v1, v2)
    assert maxabs(got, want) <= 2.56 * EPS and relerr(got, want) < 0.512 * EPS, (maxabs(got, want), relerr(got, want))
    # device-side position (hipGraph replay path)
    k3, v3 = kc.to(d), vc.to(d)
    pos = torch.tensor([past], dtype=torch.int32, device=d)
    got3 = ops.decode_attention(qkv, k3, v3, cos, sin, valid, B, heads, 0, past_dev=pos)
    assert torch.equal(got3, got) and torch.equal(k3, k2)


@pytest.mark.parametrize("B,past,pad,ctx_max,per_row", [(1, 0, 0, 64, False), (1, 5, 0, 600, False), (1, 336, 0, 600, False),
                                                        (2, 463, 7, 600, False), (1, 1100, 0, 1200, False), (2, 255, 0, 300, True),
                                                        (2, 700, 300, 1024, True), (1, 64, 0, 128, False)])
def test_decode_attention_split_and_merge(B, past, pad, ctx_max, per_row):
    """vly_decode_attention_split + vly_gemv_attnmerge_bf16 vs vly_decode_attention(_rows) + vly_gemv_bf16: the appended cache rows
    are bit-identical; the projected output agrees to the rounding of the attention output (one bf16 ulp of a few elements,
    through a K = 2048 dot product).  Covers empty splits (short contexts), two passes per split (kv_len > 1024), masks,
    per-row positions, the position on a split boundary (past = 64)."""
    from valley_amd import lib
    if not lib.experimental():
        pytest.skip("round-3 split + merge entry points: libvalley_hip_exp.so (tests/test_experimental_gpu.py runs this test)")
    from valley_amd import ops
    d = dev()
    heads, N = 16, 264                       # K = 2048: the narrowest width the fused GEMVs take
    Hq = heads * 128
    cos, sin = _rope_tables(ctx_max)
    cos, sin = cos.to(d), sin.to(d)
    pasts = [past, max(past - 130, 0)][:B] if per_row else [past] * B
    kc = torch.zeros((B, heads, ctx_max, 128), dtype=HALF)
    vc = torch.zeros_like(kc)
    for b in range(B):
        if pasts[b]:
            kc[b, :, :pasts[b]] = rnd((heads, pasts[b], 128), 30 + b, dtype=HALF)
            vc[b, :, :pasts[b]] = rnd((heads, pasts[b], 128), 40 + b, dtype=HALF)
    qkv = rnd((B, 3 * Hq), 32, dtype=HALF).to(d)
    w = rnd((N, Hq), 33, 0.05, dtype=HALF).to(d)
    res = rnd((B, N), 34).to(d)
    valid = None
    if pad or per_row:
        valid = torch.ones((B, ctx_max), dtype=torch.uint8)
        valid[0, :pad] = 0
        valid = valid.to(d)
    pos = torch.tensor(pasts if per_row else [past], dtype=torch.int32, device=d)
    k1, v1 = kc.to(d), vc.to(d)
    if per_row:
        att = ops.decode_attention_rows(qkv, k1, v1, cos, sin, valid, B, heads, pos)
    else:
        att = ops.decode_attention(qkv, k1, v1, cos, sin, valid, B, heads, 0, past_dev=pos)
    want = ops.gemv(att, w, residual=res, out_dtype=torch.float32)
    k2, v2 = kc.to(d), vc.to(d)
    parts = ops.decode_partials(B, heads, d)
    ops.decode_attention_split(qkv, k2, v2, cos, sin, valid, B, heads, 0, parts, past_dev=pos, per_row=per_row)
    got = ops.gemv_attnmerge(parts, w, residual=res, out_dtype=torch.float32)
    assert torch.equal(k1, k2) and torch.equal(v1, v2)
    assert relerr(got - res, want - res) < 0.512 * EPS and maxabs(got, want) < 2.56 * EPS, (relerr(got - res, want - res), maxabs(got, want))
    # the merged attention output itself, through an identity-like projection: rows of W = unit vectors
    eye = torch.zeros((256, Hq), dtype=HALF)
    eye[torch.arange(256), torch.arange(256) * 8] = 1.0
    m_att = ops.gemv_attnmerge(parts, eye.to(d), out_dtype=torch.float32)
    assert maxabs(m_att, att[:, ::8][:, :256].float()) <= 2.56 * EPS
    if not per_row:                          # host-side position, bf16 output
        k3, v3 = kc.to(d), vc.to(d)
        parts3 = ops.decode_partials(B, heads, d)
        ops.decode_attention_split(qkv, k3, v3, cos, sin, valid[:, :past + 1].contiguous() if valid is not None else None, B, heads, past, parts3)
        assert torch.equal(parts3, parts) and torch.equal(k3, k2)
        assert relerr(ops.gemv_attnmerge(parts, w), want - res) < 1.024 * EPS


@pytest.mark.parametrize("B,heads,pasts,pad,ctx_max", [(8, 40, [463, 336, 0, 64, 399, 255, 128, 1], 5, 600), (3, 16, [700, 63, 1100], 300, 1200),
                                                       (5, 32, [10, 20, 30, 40, 50], 0, 64), (1, 16, [336], 0, 600)])
def test_decode_attention_merged_rows(B, heads, pasts, pad, ctx_max):
    """vly_decode_attention_merged with per-row positions — the attention of serving.ContinuousBatcher's captured step for any number
    of rows (round 5; one to eight live requests) — against vly_decode_attention_rows: identical cache appends, outputs equal to the
    rounding of the split summation order; the ticket counters are back at zero; a second launch on the same inputs is bit-identical
    (the merge order is fixed, whichever workgroup of a head finishes last); a row's output does not depend on the other rows.
    Eight rows x 40 heads run three splits per head, five x 32 three, the others four (decode_split_launch)."""
    from valley_amd import ops
    d = dev()
    cos, sin = _rope_tables(ctx_max)
    cos, sin = cos.to(d), sin.to(d)
    kc = torch.zeros((B, heads, ctx_max, 128), dtype=HALF)
    vc = torch.zeros_like(kc)
    for b in range(B):
        if pasts[b]:
            kc[b, :, :pasts[b]] = rnd((heads, pasts[b], 128), 130 + b, dtype=HALF)
            vc[b, :, :pasts[b]] = rnd((heads, pasts[b], 128), 140 + b, dtype=HALF)
    qkv = rnd((B, 3 * heads * 128), 132, dtype=HALF).to(d)
    valid = torch.ones((B, ctx_max), dtype=torch.uint8)
    valid[0, :min(pad, pasts[0])] = 0
    valid = valid.to(d)
    pos = torch.tensor(pasts, dtype=torch.int32, device=d)
    k1, v1 = kc.to(d), vc.to(d)
    want = ops.decode_attention_rows(qkv, k1, v1, cos, sin, valid, B, heads, pos)
    outs = []
    for _ in range(2):
        k2, v2 = kc.to(d), vc.to(d)
        parts = ops.decode_partials(B, heads, d)
        arrivals = torch.zeros((B * heads,), dtype=torch.int32, device=d)
        got = torch.empty((B, heads * 128), dtype=HALF, device=d)
        ops.decode_attention_split(qkv, k2, v2, cos, sin, valid, B, heads, 0, parts, past_dev=pos, per_row=True, out=got, arrivals=arrivals)
        torch.cuda.synchronize()
        assert int(arrivals.abs().sum().item()) == 0
        assert torch.equal(k1, k2) and torch.equal(v1, v2)
        outs.append(got)
    assert torch.equal(outs[0], outs[1])
    assert maxabs(outs[0], want) <= 2.56 * EPS and relerr(outs[0], want) < 0.512 * EPS, (maxabs(outs[0], want), relerr(outs[0], want))
    # a row's output does not depend on what the OTHER rows of the same launch hold (the launch's shape — rows, heads, hence the
    # number of splits per head — is the session's, not the request's): other rows' queries, caches and positions replaced
    if B > 1:
        qkv4 = qkv.clone()
        qkv4[1:] = rnd((B - 1, 3 * heads * 128), 133, dtype=HALF).to(d)
        kc4, vc4 = kc.clone(), vc.clone()
        kc4[1:] = kc4[1:].flip(0) * 0.5
        vc4[1:] = vc4[1:].flip(0) * 0.5
        pos4 = pos.clone()
        pos4[1:] = torch.clamp(pos[1:].flip(0) + 3, max=ctx_max - 2)
        other = torch.empty((B, heads * 128), dtype=HALF, device=d)
        ops.decode_attention_split(qkv4, kc4.to(d), vc4.to(d), cos, sin, valid, B, heads, 0, ops.decode_partials(B, heads, d), past_dev=pos4,
                                   per_row=True, out=other, arrivals=torch.zeros((B * heads,), dtype=torch.int32, device=d))
        assert torch.equal(other[0], outs[0][0])


@pytest.mark.parametrize("tile", [0, 2, 7, 8, 84, 86, 9])
@pytest.mark.parametrize("M,N,K", [(1312, 1024, 1024), (300, 264, 192), (77, 512, 128)])
def test_gemm_splitk2_and_add2_rmsnorm(M, N, K, tile):
    """vly_gemm_bf16_splitk2: the two bf16 partials are the two K halves (each checked on its own), and
    vly_add2_rmsnorm consumes them like vly_add_rmsnorm consumes their sum."""
    from valley_amd import ops
    a = rnd((M, K), 71, dtype=HALF).to(dev())
    w = rnd((N, K), 72, 0.05, dtype=HALF).to(dev())
    bias = rnd((N,), 73, 0.3).to(dev())
    o0 = torch.empty((M, N), dtype=HALF, device=dev())
    o1 = torch.empty_like(o0)
    ops.gemm_mfma_splitk2(a, w, bias, o0, o1, tile)
    h0 = (K // 64) // 2 * 64
    r0 = a[:, :h0].float() @ w[:, :h0].float().t() + bias
    r1 = a[:, h0:].float() @ w[:, h0:].float().t()
    assert relerr(o0, r0) < 0.512 * EPS and relerr(o1, r1) < 0.512 * EPS
    if N % 4 == 0 and N >= 256:
        D = N
        h = rnd((M, D), 74).to(dev())
        g = (1.0 + 0.1 * rnd((D,), 75)).to(dev())
        h2 = h.clone()
        y2 = ops.add_norm(h2, o0, g, None, 1e-5, rms=True, delta2=o1)
        hs = h + o0.float() + o1.float()
        ref = g * (hs * torch.rsqrt((hs * hs).mean(-1, keepdim=True) + 1e-5))
        assert maxabs(h2, hs) < 1e-5
        assert relerr(y2, ref) < 0.64 * EPS
        be = rnd((D,), 76, 0.1).to(dev())                  # the CLIP form: two deltas + LayerNorm, and add-only
        h3 = h.clone()
        y3 = ops.add_norm(h3, o0, g, be, 1e-5, delta2=o1)
        assert maxabs(h3, hs) < 1e-5
        assert relerr(y3, torch.nn.functional.layer_norm(hs, (D,), g, be, 1e-5)) < 0.64 * EPS
        h4 = h.clone()
        assert ops.add_norm(h4, o0, None, None, 1e-5, delta2=o1) is None and maxabs(h4, hs) < 1e-5


def test_c_abi_smoke_binary():
    """The C ABI from a host that is neither Python nor torch: tests/c_abi/abi_smoke.cpp dlopens libvalley_hip.so,
    runs vly_gemm_bf16 (+bias, quick_gelu), an argument-error path and vly_rmsnorm on hipMalloc'ed buffers and
    checks them against its own host arithmetic."""
    import subprocess
    from valley_amd import build as b
    exe = b.build_abi_smoke(verbose=False)
    r = subprocess.run([exe, b.LIB], capture_output=True, text=True, timeout=120)
    print(r.stdout, r.stderr)
    assert r.returncode == 0, (r.stdout, r.stderr)
    assert "C ABI smoke: OK" in r.stdout


def test_argmax():
    from valley_amd import ops
    x = rnd((5, 32006), 40)
    x[2, 31999] = 50.0
    x[3, 7] = 60.0
    x[3, 9] = 60.0
    got = ops.argmax(x.to(dev())).cpu()
    assert got.tolist() == x.argmax(-1).tolist()


def test_temporal_importance_pooling():
    """v2: scores = Linear(256*W -> 1)(flatten(patches)); softmax over frames; weighted sum (valley_model.py:113-121)."""
    from valley_amd import ops
    d = dev()
    B, T, W = 2, 6, 256
    f = rnd((B, T, 257, W), 50)
    w = rnd((256 * W,), 51, 0.02)
    b = rnd((1,), 52)
    sc = ops.temporal_scores(f.to(d).view(-1, W), w.to(d), b.to(d), B * T)
    ref_sc = (f[:, :, 1:].reshape(B * T, -1) @ w) + b
    assert maxabs(sc, ref_sc) < 2e-3
    out = ops.pool_tokens(f.to(d).view(-1, W), B, T, ops.POOL_IMPORTANCE, sc)
    wt = torch.softmax(ref_sc.view(B, T), dim=1)
    pooled = (wt[:, :, None, None] * f[:, :, 1:]).sum(1)
    ref = torch.cat([pooled, f[:, :, 0]], dim=1)
    assert relerr(out, ref) < 0.384 * EPS


@pytest.mark.parametrize("D,rms", [(1024, False), (4096, True), (5120, True)])
def test_add_norm(D, rms):
    """h += delta (bf16) fused with the following LayerNorm / RMSNorm; gamma=None -> add only."""
    from valley_amd import ops
    d = dev()
    M = 333
    h = rnd((M, D), 60, 2.0)
    delta = rnd((M, D), 61, 0.5, dtype=HALF)
    g = rnd((D,), 62, 0.1) + 1.0
    b = rnd((D,), 63, 0.1)
    hd = h.to(d).clone()
    y = ops.add_norm(hd, delta.to(d), g.to(d), None if rms else b.to(d), 1e-5, rms=rms)
    hs = h + delta.float()
    assert maxabs(hd, hs) == 0.0
    if rms:
        ref = g * (hs * torch.rsqrt(hs.pow(2).mean(-1, keepdim=True) + 1e-5))
    else:
        ref = torch.nn.functional.layer_norm(hs, (D,), g, b, 1e-5)
    assert relerr(y, ref) < 0.384 * EPS
    hd2 = h.to(d).clone()
    assert ops.add_norm(hd2, delta.to(d), None, None, 1e-5, rms=rms) is None
    assert maxabs(hd2, hs) == 0.0


@pytest.mark.parametrize("shape", [(2, 360, 480), (2, 480, 270), (1, 200, 310), (3, 256, 256), (1, 720, 1280)])
def test_preprocess_frames_gpu_vs_oracle(shape):
    """N2: GPU Pillow-equivalent resize + crop + normalise vs the CPU oracle (itself bit-exact vs PIL and
    pinned to the reference fixture).  fp32 output: bit-level (same integer resample, same fp32 formula
    up to one ulp of the division); bf16 output: one rounding."""
    from oracle import preprocess_oracle as P
    from valley_amd.preprocess import preprocess_frames_gpu
    T, H, Wd = shape
    frames = np.random.default_rng(H + Wd).integers(0, 256, (T, H, Wd, 3), dtype=np.uint8)
    ref = torch.from_numpy(P.preprocess_frames(frames)).permute(1, 0, 2, 3)          # [T,3,224,224]
    got = preprocess_frames_gpu(torch.from_numpy(frames).to(dev()), out_dtype=torch.float32)
    assert maxabs(got, ref) < 2e-6
    got16 = preprocess_frames_gpu(torch.from_numpy(frames).to(dev()))
    assert maxabs(got16, ref.to(HALF)) <= 2.048 * EPS


def test_gemm_online_tuner_decides_and_stays_correct(monkeypatch, tmp_path):
    """ops.gemm in "tuned" mode: every call while the shape is undecided runs a different candidate kernel
    on the real operands; all of them are valid results, a decision is reached after TUNE_TRIALS timed
    calls per candidate plus the re-timing of the finalists, it is written to the cache file and later calls use it."""
    from valley_amd import ops
    monkeypatch.setattr(ops, "GEMM_MODE", "tuned")
    monkeypatch.setattr(ops, "_TUNE_CACHE", str(tmp_path / "tune.json"))
    monkeypatch.setattr(ops, "_TUNED", {})
    monkeypatch.setattr(ops, "_ONLINE", {})
    M, N, K = 1312, 1024, 512
    a = rnd((M, K), 11, dtype=HALF).to(dev())
    w = rnd((N, K), 12, 0.05, dtype=HALF).to(dev())
    bias = rnd((N,), 13, 0.5).to(dev())
    ref = a.float() @ w.float().t() + bias
    calls = 0
    while calls < 400:
        out = ops.gemm(a, w, bias, out_dtype=torch.float32)
        calls += 1
        assert maxabs(out, ref) < 2e-4 * math.sqrt(K) + 1e-3
        torch.cuda.synchronize()
        if ops.tuning_pending() == 0:
            break
    assert ops.tuning_pending() == 0, "no decision after %d calls" % calls
    assert calls <= len(ops.CANDIDATES) * ops.TUNE_TRIALS + ops.TUNE_FINALISTS * 2 * ops.TUNE_TRIALS + 4
    key = (M, N, K, ops.EPI_NONE, torch.float32, True, False)
    assert key in ops._TUNED
    saved = dict(ops._TUNED)
    ops._TUNED.clear()
    assert ops.load_tune_cache(str(tmp_path / "tune.json")) == 1 and ops._TUNED == saved
    assert maxabs(ops.gemm(a, w, bias, out_dtype=torch.float32), ref) < 2e-4 * math.sqrt(K) + 1e-3
    assert ops.sk_error_flag(dev()) == 0


def test_gemm_without_online_trials_is_one_kernel_from_the_first_call(monkeypatch):
    """VALLEY_TUNE_ONLINE=0 (round 4): a shape the table does not know takes the static whole-tile choice — no candidate
    trials, nothing pending, and every call returns the SAME bits (in-place trials return valid results that differ by fp32
    summation order between candidates)."""
    from valley_amd import ops
    monkeypatch.setattr(ops, "GEMM_MODE", "tuned")
    monkeypatch.setattr(ops, "TUNE_ONLINE", False)
    monkeypatch.setattr(ops, "_TUNED", {})
    monkeypatch.setattr(ops, "_ONLINE", {})
    M, N, K = 1312, 1024, 512
    a = rnd((M, K), 11, dtype=HALF).to(dev())
    w = rnd((N, K), 12, 0.05, dtype=HALF).to(dev())
    bias = rnd((N,), 13, 0.5).to(dev())
    ref = a.float() @ w.float().t() + bias
    first = ops.gemm(a, w, bias, out_dtype=torch.float32).clone()
    assert maxabs(first, ref) < 2e-4 * math.sqrt(K) + 1e-3
    for _ in range(5):
        assert torch.equal(ops.gemm(a, w, bias, out_dtype=torch.float32), first)
    assert ops.tuning_pending() == 0 and not ops._TUNED
    tiles = ops.gemm_mfma(a, w, bias, None, ops.EPI_NONE, torch.float32, None, 0)
    assert torch.equal(tiles, first)                       # = the static heuristic's kernel


@pytest.mark.parametrize("N,K", [(264, 128), (4096, 1024), (1000, 640)])
def test_pack_weight_layout(N, K):
    """vly_pack_weight_bf16: [N,K] -> [K/64][ceil(N/64)][64][64], rows past N zero."""
    from valley_amd import ops
    w = rnd((N, K), 81, dtype=HALF).to(dev())
    pw = ops.PackedWeight(w)
    nb = (N + 63) // 64
    ref = torch.zeros((nb * 64, K), dtype=HALF, device=dev())
    ref[:N] = w
    ref = ref.view(nb, 64, K // 64, 64).permute(2, 0, 1, 3).contiguous()
    assert tuple(pw.blocks.shape) == (K // 64, nb, 64, 64) and torch.equal(pw.blocks, ref)
    assert pw.plain is w and tuple(pw.shape) == (N, K)


@pytest.mark.parametrize("tile", [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 51, 53, 54, 55, 73, 74, 76, 83, 84, 86, 93, 94, 97, 98, 99, 197, 198, 199])
def test_gemm_packed_weights_bit_identical(tile):
    """The block-ordered weight copy changes addresses, not arithmetic: every tile / loop variant returns the same
    bits as with the row-major weights (ragged N included), through every epilogue; so does the split-K pair."""
    from valley_amd import ops
    M, N, K = 771, 1000, 256
    a = rnd((M, K), 82, dtype=HALF).to(dev())
    w = rnd((N, K), 83, 0.05, dtype=HALF).to(dev())
    bias = rnd((N,), 84, 0.5).to(dev())
    res = rnd((M, N), 85).to(dev())
    pw = ops.PackedWeight(w)
    for kw in (dict(), dict(bias=bias, residual=res, out_dtype=torch.float32), dict(bias=bias, epilogue=ops.EPI_QUICK_GELU),
               dict(epilogue=ops.EPI_SWIGLU)):
        assert torch.equal(ops.gemm_mfma(a, pw, tile_hint=tile, **kw), ops.gemm_mfma(a, w, tile_hint=tile, **kw)), kw
    if tile in (0, 2, 6, 7, 8, 76, 84, 86):
        o = [torch.empty((M, N), dtype=HALF, device=dev()) for _ in range(4)]
        ops.gemm_mfma_splitk2(a, pw, bias, o[0], o[1], tile)
        ops.gemm_mfma_splitk2(a, w, bias, o[2], o[3], tile)
        assert torch.equal(o[0], o[2]) and torch.equal(o[1], o[3])
    # the kernels that read row-major weights take the plain copy
    assert torch.equal(ops.gemm_streamk(a, pw), ops.gemm_streamk(a, w))
    assert torch.equal(ops.gemv(a[:4], pw), ops.gemv(a[:4], w))


@pytest.mark.parametrize("M,N,K,epi,tile", [
    (2688, 27648, 5120, 2, 297),      # 13B gate|up on 256-row tiles (round 4): 4 whole rounds + 164 tiles in three slices, summed on the matrix cores
    (2816, 27648, 5120, 2, 297),      # configs[3]'s per-GPU shape of the same GEMM
    (2688, 15360, 5120, 0, 297), (2688, 5120, 13824, 0, 297), (1312, 22016, 4096, 2, 297),
    (771, 1000, 256, 1, 297), (1000, 3000, 640, 0, 297),
    (2688, 27648, 5120, 2, 298),      # 13B gate|up on 224-row tiles: 5 whole rounds + 16 tiles, eight slices each
    (2688, 15360, 5120, 0, 298),      # 13B q|k|v: 2 rounds + 208 tiles (no split pays: S = 1)
    (2688, 5120, 13824, 0, 298),      # 13B down: 240 tiles on 256 CUs, 216 K tiles per tile
    (1312, 22016, 4096, 2, 299),      # 7B gate|up: 2 rounds + 90 tiles in two slices — the shape it is shipped for
    (1312, 4096, 11008, 0, 299),      # 7B down: 112 tiles, two slices each: every tile is shared
    (2048, 8192, 512, 0, 298),        # ragged 224-row tiling of an exact problem
    (771, 1000, 256, 1, 299),         # 20 tiles of 4 K tiles: ragged M and N, quick_gelu + bias
    (513, 520, 128, 0, 299),          # 2 K tiles per tile: one slice at most
    (1000, 3000, 640, 0, 299), (900, 2040, 1024, 0, 298)])
def test_gemm_p4_streamk(M, N, K, epi, tile):
    """The persistent 4-wave kernel with its remainder round split along K (vly_gemm_bf16_streamk, tile hints 298 / 299) against
    the same kernel without the split (198 / 199): identical where no tile is shared, fp32 summation order apart where one
    is; fp32 outputs with bias + residual, the packed weight copy (bit-identical), and no hand-off failure."""
    from valley_amd import lib, ops
    if tile == 297 and not lib.experimental():
        pytest.skip("tile hint 297 lives in libvalley_hip_exp.so (VALLEY_EXPERIMENTAL=1): tests/test_experimental_gpu.py runs it")
    d = dev()
    a = rnd((M, K), 91, dtype=HALF).to(d)
    w = rnd((N, K), 92, 0.03, dtype=HALF).to(d)
    bias = rnd((N,), 93, 0.5).to(d) if epi != ops.EPI_SWIGLU else None
    want = ops.gemm_mfma(a, w, bias, epilogue=epi, tile_hint=tile - 100)
    got = ops.gemm_streamk(a, w, bias, epilogue=epi, tile_hint=tile)
    assert relerr(got, want) < 0.256 * EPS, relerr(got, want)
    assert (got != want).float().mean() < 0.02                    # a bf16 ulp here and there, in pool tiles only
    assert torch.equal(ops.gemm_streamk(a, ops.PackedWeight(w), bias, epilogue=epi, tile_hint=tile), got)
    if epi == ops.EPI_NONE:
        res = rnd((M, N), 94).to(d)
        want32 = ops.gemm_mfma(a, w, bias, res, out_dtype=torch.float32, tile_hint=tile - 100)
        got32 = ops.gemm_streamk(a, w, bias, res, out_dtype=torch.float32, tile_hint=tile)
        assert maxabs(got32, want32) < 1e-4 * math.sqrt(K) + 1e-4, maxabs(got32, want32)
        if M * N * K < 1 << 31:
            ref = a.float().cpu() @ w.float().cpu().t() + bias.cpu() + res.cpu()
            assert maxabs(got32, ref) < 2e-4 * math.sqrt(K) + 1e-3
    torch.cuda.synchronize()
    assert ops.sk_error_flag(d) == 0


def test_gemm_packed_rejects_half_tile_loops():
    from valley_amd import ops
    from valley_amd.lib import ValleyHipError
    a = rnd((256, 128), 86, dtype=HALF).to(dev())
    pw = ops.PackedWeight(rnd((256, 128), 87, dtype=HALF).to(dev()))
    for t in (11, 33):
        with pytest.raises(ValleyHipError):
            ops.gemm_mfma(a, pw, tile_hint=t)


# ---- the HIP kernels against op-level outputs of the HF sub-modules (tests/golden/g6_ops.npz) ---------
def _g6():
    import os
    return np.load(os.path.join(os.path.dirname(__file__), "golden", "g6_ops.npz"))


def test_g6_rmsnorm_eps_and_layernorm_vs_hf():
    """LlamaRMSNorm at eps 1e-5 (Llama-2) and 1e-6 (LLaMA-1 / Vicuna-13B), nn.LayerNorm(1024): bf16 output = the HF fp32
    output rounded once (<= 1 bf16 ulp), fp32 LayerNorm output to 2e-5."""
    from tests.golden_r2_cfg import OPS, op_input, op_weights
    from valley_amd import ops
    g, d = _g6(), dev()
    x = torch.from_numpy(op_input("rms.x", (5, OPS["H"]))).to(d)
    wn = torch.from_numpy(op_weights("rms.w", (OPS["H"],), 0.1, 1.0)).to(d)
    for eps in (1e-5, 1e-6):
        ref = torch.from_numpy(g[f"rmsnorm_eps{eps:g}"])
        y = ops.rmsnorm(x, wn, eps)
        assert maxabs(y, ref.to(HALF)) <= float(ref.abs().max()) * EPS + 1e-6               # one 16-bit ulp at the largest value
        assert relerr(y, ref) < 0.384 * EPS
    # the two eps settings differ by less than a bf16 ulp here, so also check the statistic itself on a tiny-norm row
    tiny = (x[:1] * 1e-3).contiguous()
    r5 = wn.cpu() * (tiny.cpu() * torch.rsqrt(tiny.cpu().pow(2).mean(-1, keepdim=True) + 1e-5))
    r6 = wn.cpu() * (tiny.cpu() * torch.rsqrt(tiny.cpu().pow(2).mean(-1, keepdim=True) + 1e-6))
    assert relerr(ops.rmsnorm(tiny, wn, 1e-5), r5) < 0.384 * EPS and relerr(ops.rmsnorm(tiny, wn, 1e-6), r6) < 0.384 * EPS
    assert relerr(r5, r6) > 0.1                                               # eps matters at this scale: 1e-6 != 1e-5
    y16, y32 = ops.layernorm(torch.from_numpy(op_input("ln.x", (5, 1024))).to(d), torch.from_numpy(op_weights("ln.w", (1024,), 0.1, 1.0)).to(d),
                             torch.from_numpy(op_weights("ln.b", (1024,), 0.1)).to(d), 1e-5, want_f32=True)
    assert maxabs(y32, torch.from_numpy(g["layernorm"])) < 2e-5


def test_g6_rope_positions_vs_hf():
    """vly_rope_kv at positions {0, 1, 327, 2047} (rotate-half, fp32 tables) vs HF apply_rotary_pos_emb: the bf16 result
    is the fp32 HF value rounded once."""
    from tests.golden_r2_cfg import OPS, op_input
    from valley_amd import ops
    g, d = _g6(), dev()
    heads = OPS["heads"]
    cos, sin = _rope_tables(2048)
    assert maxabs(cos[OPS["rope_positions"]], torch.from_numpy(g["rope_cos"])[0, :, :64]) < 1e-6
    q = torch.from_numpy(op_input("rope.q", (1, heads, 4, 128)))
    k = torch.from_numpy(op_input("rope.k", (1, heads, 4, 128)))
    for i, pos in enumerate(OPS["rope_positions"]):
        qkv = torch.zeros((1, 3 * heads * 128), dtype=HALF)
        qkv[0, :heads * 128] = q[0, :, i].reshape(-1).to(HALF)
        qkv[0, heads * 128:2 * heads * 128] = k[0, :, i].reshape(-1).to(HALF)
        qd = qkv.to(d)
        kc = torch.zeros((1, heads, 2048, 128), dtype=HALF, device=d)
        vc = torch.zeros_like(kc)
        ops.rope_kv(qd, kc, vc, cos.to(d), sin.to(d), 1, 1, heads, pos)
        # HF rotated the fp32 q; the kernel rotates the bf16-rounded q: compare against the rotation of the rounded input
        qb, kb = q[0, :, i].to(HALF).float(), k[0, :, i].to(HALF).float()
        c = torch.from_numpy(g["rope_cos"])[0, i]
        s = torch.from_numpy(g["rope_sin"])[0, i]
        rot = lambda t: torch.cat([-t[..., 64:], t[..., :64]], -1)  # noqa: E731
        want_q, want_k = qb * c + rot(qb) * s, kb * c + rot(kb) * s
        assert maxabs(qd.view(3, heads, 128)[0], want_q.to(HALF)) <= 4.096 * EPS, pos
        assert maxabs(kc[0, :, pos], want_k.to(HALF)) <= 4.096 * EPS, pos
        # and the HF fixture itself (fp32 input) within the input rounding
        assert maxabs(qd.view(3, heads, 128)[0], torch.from_numpy(g["rope_q"])[0, :, i]) < 5.12 * EPS, pos


def test_g6_llama_attention_block_and_mlp_vs_hf():
    """LlamaAttention (eager, causal, left-padded batch of 2, head_dim 128) and LlamaMLP (SwiGLU) through the kernels the
    prefill uses: fused q|k|v GEMM -> vly_rope_kv -> vly_llama_attention -> o GEMM; interleaved gate/up GEMM with the
    SwiGLU epilogue -> down GEMM.  bf16 operand tolerance: rel-L2 < 8e-3."""
    from tests.golden_r2_cfg import OPS, op_input, op_weights
    from valley_amd import ops
    from valley_amd.llama import HipLlama
    g, d, o = _g6(), dev(), OPS
    H, heads, B, S = o["H"], o["heads"], 2, o["S"]
    bf = HALF
    W = {n: torch.from_numpy(op_weights(f"att.{n}", (H, H), 0.05)).to(d, bf) for n in ("q_proj", "k_proj", "v_proj", "o_proj")}
    x = torch.from_numpy(op_input("att.h", (B, S, H))).view(B * S, H).to(d, bf)
    qkv = ops.gemm_mfma(x, torch.cat([W["q_proj"], W["k_proj"], W["v_proj"]], 0).contiguous())
    cos, sin = _rope_tables(256)
    kc = torch.zeros((B, heads, 256, 128), dtype=bf, device=d)
    vc = torch.zeros_like(kc)
    ops.rope_kv(qkv, kc, vc, cos.to(d), sin.to(d), B, S, heads, 0)
    valid = torch.ones((B, 256), dtype=torch.uint8)
    valid[1, :o["pad"]] = 0
    att = ops.llama_attention(qkv, kc, vc, valid.to(d), B, S, heads, 0)
    y = ops.gemm_mfma(att, W["o_proj"], out_dtype=torch.float32).view(B, S, H).cpu()
    ref = torch.from_numpy(g["llama_attention"])
    keep = valid[:, :S].bool()
    e = relerr(y[keep], ref[keep])
    print("G6 attention block rel-L2", e)
    assert e < 1.024 * EPS
    gate = torch.from_numpy(op_weights("mlp.gate", (o["I"], H), 0.05)).to(d, bf)
    up = torch.from_numpy(op_weights("mlp.up", (o["I"], H), 0.05)).to(d, bf)
    down = torch.from_numpy(op_weights("mlp.down", (H, o["I"]), 0.05)).to(d, bf)
    xm = torch.from_numpy(op_input("mlp.x", (7, H))).to(d, bf)
    xm = torch.cat([xm, torch.zeros((9, H), dtype=bf, device=d)], 0)                        # 16 rows: the MFMA path, not the GEMV
    mid = ops.gemm_mfma(xm, HipLlama._interleave(gate, up), epilogue=ops.EPI_SWIGLU)
    out = ops.gemm_mfma(mid, down, out_dtype=torch.float32)[:7].cpu()
    e = relerr(out, torch.from_numpy(g["llama_mlp"]))
    print("G6 SwiGLU MLP rel-L2", e)
    assert e < 1.024 * EPS


def test_g6_clip_mlp_and_attention_vs_hf():
    """CLIPMLP (quick_gelu) and CLIPAttention (N = 257, 16 heads x 64) through fc1(+bias, quick_gelu) / fc2 GEMMs and the
    fused q|k|v GEMM -> vly_vit_attention -> out_proj GEMM."""
    from tests.golden_r2_cfg import OPS, op_input, op_weights
    from valley_amd import ops
    g, d, o = _g6(), dev(), OPS
    bf = HALF
    tw = lambda n, shp, std=0.03: torch.from_numpy(op_weights(n, shp, std)).to(d)  # noqa: E731
    x = torch.cat([torch.from_numpy(op_input("cmlp.x", (9, 1024))), torch.zeros(7, 1024)], 0).to(d, bf)
    mid = ops.gemm_mfma(x, tw("cmlp.fc1.w", (o["VI"], 1024)).to(bf), tw("cmlp.fc1.b", (o["VI"],), 0.1), epilogue=ops.EPI_QUICK_GELU)
    out = ops.gemm_mfma(mid, tw("cmlp.fc2.w", (1024, o["VI"])).to(bf), tw("cmlp.fc2.b", (1024,), 0.1), out_dtype=torch.float32)[:9]
    e = relerr(out, torch.from_numpy(g["clip_mlp"]))
    print("G6 CLIP MLP rel-L2", e)
    assert e < 1.024 * EPS
    wq = torch.cat([tw(f"catt.{n}.w", (1024, 1024)) for n in ("q_proj", "k_proj", "v_proj")], 0).to(bf).contiguous()
    bq = torch.cat([tw(f"catt.{n}.b", (1024,), 0.1) for n in ("q_proj", "k_proj", "v_proj")], 0).contiguous()
    xa = torch.from_numpy(op_input("catt.x", (2, 257, 1024))).view(-1, 1024).to(d, bf)
    att = ops.vit_attention(ops.gemm_mfma(xa, wq, bq), 2)
    y = ops.gemm_mfma(att, tw("catt.out_proj.w", (1024, 1024)).to(bf), tw("catt.out_proj.b", (1024,), 0.1), out_dtype=torch.float32)
    e = relerr(y.view(2, 257, 1024)[:, ::4], torch.from_numpy(g["clip_attention"]))
    print("G6 CLIP attention rel-L2", e)
    assert e < 1.024 * EPS


@pytest.mark.parametrize("M,N,K,epi", [(128, 4096, 1024, 1), (128, 1024, 4096, 0), (32, 3072, 1024, 0), (200, 64, 128, 3), (9, 32, 640, 0),
                                         (256, 1024, 1024, 0)])
def test_gemm_skinny(M, N, K, epi):
    """vly_gemm_skinny_bf16 (the latency-optimised kernel for the F-row remainders of the tall ViT GEMMs) vs an fp32
    product: one bf16 rounding of the result; ragged M (rows past the edge never stored); a strided A (a row slice of a
    wider buffer, as the remainder rows are); the transpose detector."""
    from valley_amd import ops
    d = dev()
    big = rnd((M + 3, K + 64), 91, dtype=HALF).to(d)
    a = big[3:, 64:]                                                     # row stride K + 64, 16-byte aligned start
    w = rnd((N, K), 92, 0.05, dtype=HALF).to(d)
    bias = rnd((N,), 93, 0.5).to(d)
    base = a.float() @ w.float().t() + bias
    ref = base * torch.sigmoid(1.702 * base) if epi == 1 else base.clamp_min(0) if epi == 3 else base
    out = torch.full((M + 2, N), 7.0, dtype=HALF, device=d)
    ops.gemm_skinny(a, w, bias, epilogue=epi, out=out[:M])
    assert relerr(out[:M], ref) < 0.512 * EPS
    assert float((out[M:].float() - 7.0).abs().max()) == 0.0              # nothing written past M
    assert relerr(out[:M], ops.gemm_mfma(a, w, bias, epilogue=epi)) < 0.384 * EPS   # same math as the tile kernel (summation order only)
    w1 = torch.zeros((N, K), dtype=HALF, device=d)
    w1[5, K - 3] = 1.0
    o1 = ops.gemm_skinny(a, w1)
    assert maxabs(o1[:, 5], a[:, K - 3]) == 0.0 and float(o1[:, :5].float().abs().max()) == 0.0
    from valley_amd.lib import ValleyHipError
    with pytest.raises(ValleyHipError):
        ops.gemm_skinny(rnd((300, K), 1, dtype=HALF).to(d), w)     # M > 256 is not this kernel's job


@pytest.mark.parametrize("tile", [0, 1, 2, 3, 4, 5, 8, 9, 51, 53, 54, 55, 73, 74, 83, 84, 93, 94, 97, 98, 99, 197, 198, 199])
@pytest.mark.parametrize("B,S,heads,past", [(2, 75, 2, 0), (1, 336, 3, 0), (3, 40, 2, 100)])
def test_gemm_qkv_rope_fused_bit_identical(tile, B, S, heads, past):
    """vly_gemm_bf16_qkv_rope (RoPE + KV append in the q|k|v GEMM epilogue) vs vly_gemm_bf16 followed by vly_rope_kv:
    rotated q, the appended cache rows of k and v — every bit equal, on row-major and block-ordered weights; cache rows
    outside [past, past + S) untouched."""
    from valley_amd import ops
    d = dev()
    H, K, ctx = heads * 128, 256, 512
    a = rnd((B * S, K), 101, dtype=HALF).to(d)
    w = rnd((3 * H, K), 102, 0.05, dtype=HALF).to(d)
    cos, sin = _rope_tables(ctx)
    cos, sin = cos.to(d), sin.to(d)
    seedk = rnd((B, heads, ctx, 128), 103, dtype=HALF).to(d)
    k0, v0 = seedk.clone(), (seedk * 0.5).clone()
    ref = ops.gemm_mfma(a, w, tile_hint=tile)
    ops.rope_kv(ref, k0, v0, cos, sin, B, S, heads, past)
    for wt in (w, ops.PackedWeight(w)):
        qkv = torch.full((B * S, 3 * H), 7.0, dtype=HALF, device=d)
        k1, v1 = seedk.clone(), (seedk * 0.5).clone()
        ops.gemm_mfma_qkv_rope(a, wt, qkv, ops.RopeKV(k1, v1, cos, sin, B, S, heads, past), tile)
        assert torch.equal(qkv[:, :H], ref[:, :H])
        assert torch.equal(k1, k0) and torch.equal(v1, v0)
        assert float((qkv[:, H:].float() - 7.0).abs().max()) == 0.0        # the k / v columns of the buffer are not written


def test_gemm_qkv_rope_rejects_narrow_tiles_and_falls_back():
    from valley_amd import ops
    from valley_amd.lib import ValleyHipError
    d = dev()
    B, S, heads, K = 1, 64, 2, 128
    a = rnd((B * S, K), 104, dtype=HALF).to(d)
    w = rnd((3 * heads * 128, K), 105, 0.05, dtype=HALF).to(d)
    cos, sin = (t.to(d) for t in _rope_tables(128))
    kc = torch.zeros((B, heads, 128, 128), dtype=HALF, device=d)
    rope = ops.RopeKV(kc, torch.zeros_like(kc), cos, sin, B, S, heads, 0)
    qkv = torch.empty((B * S, 3 * heads * 128), dtype=HALF, device=d)
    for t in (6, 7, 76, 86):                               # 192-column tiles cannot hold a head's two halves
        with pytest.raises(ValleyHipError):
            ops.gemm_mfma_qkv_rope(a, w, qkv, rope, t)
    ops.gemm_qkv_rope(a, w, qkv, rope)                     # the dispatcher picks a tile that can
    ref = ops.gemm_mfma(a, w)
    k2 = torch.zeros_like(kc)
    ops.rope_kv(ref, k2, torch.zeros_like(kc), cos, sin, B, S, heads, 0)
    assert torch.equal(qkv[:, :heads * 128], ref[:, :heads * 128]) and torch.equal(kc, k2)


@pytest.mark.parametrize("shape", [(4100, 4360, 320), (8200, 4360, 128), (6000, 6104, 192)])
@pytest.mark.parametrize("tile", [197, 198, 199])
def test_gemm_persistent_many_tiles_bit_identical_to_tile9(tile, shape):
    """The persistent 4-wave kernel on a problem with MORE tiles than workgroups (several tiles per workgroup, a partial
    last round, ragged last tile row and column, dead waves): same MFMA, same K order as the 16-wave tile -> identical bits,
    for every epilogue, bf16 and fp32 outputs, fp32 residual, row-major and block-ordered weights.  Round 5: the bf16-output
    instantiations hold their accumulators by name and roll a finished tile's epilogue into the next tile's first K tile —
    (8200, 4360, 128) is 594 tiles of TWO K tiles (every K tile is a boundary or follows one, three tiles per workgroup),
    (6000, 6104, 192) three K tiles; a wave that sat a tile out and is live in the next one re-reads its fragments."""
    from valley_amd import ops
    d = dev()
    M, N, K = shape                                             # (4100, 4360): 17 x 18 tiles of 256 x 256 = 306 > 256 workgroups
    a = rnd((M, K), 201, dtype=HALF).to(d)
    w = rnd((N, K), 202, 0.05, dtype=HALF).to(d)
    bias = rnd((N,), 203, 0.5).to(d)
    res = rnd((M, N), 204).to(d)
    for wt in (w, ops.PackedWeight(w)):
        for kw in (dict(), dict(bias=bias), dict(bias=bias, epilogue=ops.EPI_QUICK_GELU), dict(epilogue=ops.EPI_SWIGLU),
                   dict(bias=bias, epilogue=ops.EPI_RELU), dict(out_dtype=torch.float32), dict(bias=bias, residual=res, out_dtype=torch.float32)):
            got = ops.gemm_mfma(a, wt, tile_hint=tile, **kw)
            ref = ops.gemm_mfma(a, wt, tile_hint=9, **kw)
            assert torch.equal(got, ref), (tile, sorted(kw))
    # an output view whose rows are not 16-byte aligned falls back to the one-tile-per-workgroup kernel: same values
    out = torch.full((M, N + 2), 7.0, dtype=HALF, device=d)
    ops.gemm_mfma(a, w, bias, out=out[:, :N], tile_hint=tile)
    assert torch.equal(out[:, :N], ops.gemm_mfma(a, w, bias, tile_hint=9)) and float((out[:, N:].float() - 7.0).abs().max()) == 0.0
