"""Exact mask, address and count checks of every attention kernel (tests/attention_oracle.py): constructed inputs whose correct output is
known to the bit, through valley_amd.ops / ops_f32.

  (a) pointer       the output row is V[target], bit for bit (gap >= 160 log2 units: every other probability is exactly 0 in fp32);
  (b) invisibility  replacing every key / V row a query may not see leaves its output row bit-identical;
  (c) count         q = 0, 0/1 V: the output is count_c / n within one ulp of the storage type (4 ulps on fp32 outputs).

Why each holds exactly for a kernel (read from the kernels, valley_amd/csrc):
  * llama_attn2_kernel / llama_attn_kernel: p = exp2(s - m) with s = NEG_BIG on masked keys; once a real key has set m, masked p = 0 and
    earlier garbage is scaled by alpha = exp2(NEG_BIG - m) = 0 (finite x 0); p is packed to 16 bits for the PV MFMA, and 1 and 0 pack
    exactly; one 1.f / l, one multiply, one rounding.  Rows with no visible key accumulate p = 1 on masked keys: don't-care, excluded.
  * decode_attn_kernel, decode_fused_kernel, decode_split_kernel (+ in-launch merge, + the o-projection prologue's merge): fp32 fmaf sums
    of p x V; chunks and splits combine with weights exp2(m_part - m), which are exactly 1 or 0 under (a) and exactly 1 (or 0 for an
    empty / all-masked part) under (c); one division t / l.
  * the ViT kernels: keys 257 .. 271 get NEG_BIG, the PV chunks' rows up to 287 are zeros with p = 0; the 257th query's partials merge
    with weights exactly 1 or 0 as above.
  * attention_f32 (scalar and MFMA), attn_probs_kernel: -inf / NEG_BIG masks, expf / exp2 of 0 is 1 and of less than -110 is 0.
  * delta_attn_kernel: __expf(0) = 1, __expf(-gap) = 0; no mask, so (b) does not apply (every key of a unit is visible; the unit's
    addressing is probed by (a), whose V rows differ per (sequence, head, step)).
No kernel needs a bound wider than the issue's: nothing is substituted.

Measured on one MI355X: the module's 251 tests take 20 s of wall time on the bf16 library, 8 s of it the experimental library's child;
the fp16 kernel-suite child of tests/test_fp16_gpu.py takes 84 s with this module included (about 70 s without; its limit is 600 s)."""
import os
import subprocess
import sys

import pytest
import torch

from tests import attention_oracle as AO
from valley_amd.runtime import HALF

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PREFILL = AO.prefill_cases()
DEC_UNIFORM = AO.decode_uniform_cases()
DEC_ROWS = AO.decode_rows_cases()


def dev():
    return torch.device("cuda:0")


def _ids(cases):
    return [c.name for c in cases]


def _qkv(inp, dtype):
    """Rotated q in the q slot of a q | k | v buffer (the attention entry points read nothing else of it)."""
    c = inp.case
    qkv = torch.full((c.B * c.S, 3, c.heads * 128), 3.0, dtype=dtype, device=inp.q.device)
    qkv[:, 0] = inp.q.reshape(c.B * c.S, c.heads * 128)
    return qkv.view(c.B * c.S, 3 * c.heads * 128)


# ---- prefill: vly_llama_attention (llama_attn2_kernel; S = 1: decode_attn_kernel), host and device position ------------------------
def run_prefill(past_dev=False):
    def run(inp):
        from valley_amd import ops
        c = inp.case
        pd = torch.tensor([c.past], dtype=torch.int32, device=dev()) if past_dev else None
        out = ops.llama_attention(_qkv(inp, HALF), inp.k, inp.v, inp.valid, c.B, c.S, c.heads, 0 if past_dev else c.past, past_dev=pd)
        return out.view(c.B, c.S, c.heads, 128)
    return run


@pytest.mark.parametrize("case", PREFILL, ids=_ids(PREFILL))
def test_prefill_pointer(case):
    AO.check_pointer(case, run_prefill(), HALF, dev())


@pytest.mark.parametrize("case", PREFILL, ids=_ids(PREFILL))
def test_prefill_count(case):
    AO.check_count(case, run_prefill(), HALF, dev())


@pytest.mark.parametrize("case", PREFILL, ids=_ids(PREFILL))
def test_prefill_invisible(case):
    AO.check_invisible(case, run_prefill(), HALF, dev())


@pytest.mark.parametrize("case", PREFILL[::4], ids=_ids(PREFILL[::4]))
def test_prefill_device_position(case):
    """The past_dev form (the captured graph's): the host argument is 0, the position comes from device memory."""
    AO.check_pointer(case, run_prefill(True), HALF, dev(), rounds=1)
    AO.check_count(case, run_prefill(True), HALF, dev())
    AO.check_invisible(case, run_prefill(True), HALF, dev(), cuts=AO.thin_cuts(case.S))


# ---- attention_probs (attn_probs_kernel, 16-bit and fp32 operands) ---------------------------------------------------------------
PROBS = [c for c in PREFILL if c.S * c.heads <= 129 * 3][::2]


@pytest.mark.parametrize("f32", [False, True], ids=["half", "f32"])
@pytest.mark.parametrize("case", PROBS, ids=_ids(PROBS))
def test_attention_probs(case, f32):
    """(a): the row of probabilities is exactly one-hot at the target; (c): 1 / n on the visible keys within 4 fp32 ulps and exactly 0
    elsewhere; (b): the rows do not change with the invisible keys.  A row with no visible key is a row of zeros (the kernel's contract)."""
    from valley_amd import ops
    dt = torch.float32 if f32 else HALF
    kv = case.kv_lens()[0]
    live = case.live_rows()

    def probs(inp):
        return ops.attention_probs(_qkv(inp, dt), inp.k.to(dt).contiguous(), inp.valid, case.B, case.S, case.heads, case.past)    # [B, heads, S, kv]
    inp = AO.build_pointer(case, HALF, dev())
    p = probs(inp).cpu()
    onehot = torch.zeros_like(p).scatter_(-1, inp.targets.cpu().permute(0, 2, 1)[..., None], 1.0) * live[:, None, :, None]
    assert torch.equal(AO.bits(p), AO.bits(onehot)), f"{case.name}: {int((p != onehot).sum())} probabilities are not the one-hot row"
    p = probs(AO.build_count(case, HALF, dev())).cpu().double()
    vis = case.vis()[:, None, :, :kv].double()
    want = vis / vis.sum(-1, keepdim=True).clamp_min(1.0)
    assert bool(((p - want).abs() <= 4 * AO.ulp(want, torch.float32) * (want != 0)).all()), float((p - want).abs().max())
    base = AO.build_dense(case, HALF, dev())
    a = probs(base)
    for cut in AO.thin_cuts(case.S):
        b = probs(AO.replace_invisible(base, cut))
        assert torch.equal(AO.bits(a[:, :, :cut + 1]), AO.bits(b[:, :, :cut + 1])), (case.name, cut)


# ---- the fused decode entry points -------------------------------------------------------------------------------------------------
def _decode_runner(entry):
    """entry: host | dev | rows | merged | split_pair.  The caches go in with the new token's rows poisoned; after the launch they must
    equal vly_rope_kv's append bit for bit (as the existing decode tests compare them) and be untouched everywhere else."""
    def run(inp):
        from valley_amd import ops
        c = inp.case
        d = dev()
        B, heads = c.B, c.heads
        cos, sin = (t.to(d) for t in AO.rope_tables(c.ctx_max))
        pos = torch.tensor(c.pasts, dtype=torch.int32, device=d)
        bi = torch.arange(B, device=d)
        kc, vc = inp.k.clone(), inp.v.clone()
        kc[bi, :, pos.long()] = 7.0
        vc[bi, :, pos.long()] = 7.0
        k0, v0 = kc.clone(), vc.clone()
        for b in range(B):                                            # the reference append: vly_rope_kv, one row of the batch at a time
            ops.rope_kv(inp.qkv_raw[b:b + 1].clone(), k0[b:b + 1], v0[b:b + 1], cos, sin, 1, 1, heads, c.pasts[b])
        qkv = inp.qkv_raw
        if entry == "host":
            out = ops.decode_attention(qkv, kc, vc, cos, sin, inp.valid, B, heads, c.past)
        elif entry == "dev":
            out = ops.decode_attention(qkv, kc, vc, cos, sin, inp.valid, B, heads, 0, past_dev=pos[:1].clone())
        elif entry == "rows":
            out = ops.decode_attention_rows(qkv, kc, vc, cos, sin, inp.valid, B, heads, pos)
        elif entry == "merged":
            arrivals = torch.zeros((B * heads,), dtype=torch.int32, device=d)
            out = torch.empty((B, heads * 128), dtype=HALF, device=d)
            ops.decode_attention_split(qkv, kc, vc, cos, sin, inp.valid, B, heads, 0, ops.decode_partials(B, heads, d), past_dev=pos, per_row=True,
                                       out=out, arrivals=arrivals)
            assert int(arrivals.abs().sum().item()) == 0
        else:                                                         # round 3's pair: partials merged in the o projection's prologue
            parts = ops.decode_partials(B, heads, d)
            ops.decode_attention_split(qkv, kc, vc, cos, sin, inp.valid, B, heads, 0, parts, past_dev=pos, per_row=True)
            eye = torch.eye(heads * 128, dtype=HALF, device=d)
            out = ops.gemv_attnmerge(parts, eye, out_dtype=torch.float32).to(HALF)     # (x 1 and + 0 in fp32: the merged value itself)
        assert torch.equal(kc, k0) and torch.equal(vc, v0), f"{c.name} {entry}: the appended cache rows differ from vly_rope_kv's, or another row changed"
        return out.view(B, 1, heads, 128)
    return run


def _decode_checks(case, entry):
    run = _decode_runner(entry)
    AO.check_pointer(case, run, HALF, dev())
    AO.check_count(case, run, HALF, dev())
    AO.check_invisible(case, run, HALF, dev())


@pytest.mark.parametrize("entry", ["host", "dev", "rows", "merged"])
@pytest.mark.parametrize("case", DEC_UNIFORM, ids=_ids(DEC_UNIFORM))
def test_decode_one_position(case, entry):
    """vly_decode_attention (host and device position), vly_decode_attention_rows and vly_decode_attention_merged at every past of the
    issue's list, against the oracle (not against another kernel): two rows, the second left-padded (a wholly masked first chunk and
    wholly masked splits at the long ones), interior holes on every third."""
    _decode_checks(case, entry)


@pytest.mark.parametrize("entry", ["rows", "merged"])
@pytest.mark.parametrize("case", DEC_ROWS, ids=_ids(DEC_ROWS))
def test_decode_rows(case, entry):
    """Per-row positions, short rows (0, 1, 63, 64) beside long ones (1300, 4000), pads up to 600, at the launch shapes of the merged
    kernel: 8 rows x 40 heads, 5 x 32, 1 x 16 (kv_len == ctx_max = 4001)."""
    _decode_checks(case, entry)


SPLIT_PAIR = [c for c in DEC_UNIFORM if c.pasts[0] in (0, 64, 512, 1025, 4000)]


@pytest.mark.parametrize("case", SPLIT_PAIR, ids=_ids(SPLIT_PAIR))
def test_decode_split_pair(case):
    """vly_decode_attention_split + vly_gemv_attnmerge_bf16 (the experimental library's pair; M = 2 rows, 16 heads: K = 2048, the narrowest
    the merging GEMV takes), through an identity projection."""
    from valley_amd import lib
    if not lib.experimental():
        pytest.skip("libvalley_hip_exp.so only: runs in the child of test_experimental_library_kernels_meet_the_oracle")
    _decode_checks(AO.Case(**{**case.__dict__, "heads": 16, "name": case.name + "-h16"}), "split_pair")


def test_experimental_library_kernels_meet_the_oracle():
    """The register-staged prefill kernel (llama_attn_kernel: VLY_LLAMA_ATTN=1, read once per process, in libvalley_hip_exp.so) on the
    prefill cases of this module, and the split + merge pair, in a child (the pattern of
    test_llama_attention_register_staged_kernel_still_passes)."""
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.join(ROOT, "tests", "test_attention_exact_gpu.py"), "-m", "gpu", "-q", "-x",
                        "-p", "no:cacheprovider", "-k", "test_prefill_ or test_decode_split_pair"],
                       env=dict(os.environ, VLY_LLAMA_ATTN="1", VALLEY_EXPERIMENTAL="1"), capture_output=True, timeout=900, cwd=ROOT)
    tail = r.stdout.decode(errors="replace")[-2500:]
    assert r.returncode == 0, tail
    assert " passed" in tail and "skipped" not in tail.splitlines()[-1], tail


# ---- ViT ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kernel", [None, "5", "1"], ids=["persistent", "two-group", "per-head"])
@pytest.mark.parametrize("F", AO.VIT_FRAMES)
def test_vit(F, kernel, monkeypatch):
    """The persistent default, VLY_VIT_ATTN=5 and =1 (read per call).  (c) proves that the padded keys 257 .. 271 of the score tiles
    and .. 287 of the PV chunks are never counted: n = 257, not 272 or 288.  (b), ViT form: other frames' and heads' q | k | v replaced."""
    from valley_amd import ops
    if kernel is None:
        monkeypatch.delenv("VLY_VIT_ATTN", raising=False)
    else:
        monkeypatch.setenv("VLY_VIT_ATTN", kernel)

    def run(qkv):
        return ops.vit_attention(qkv, F)
    AO.vit_check_pointer(F, run, HALF, dev())
    AO.vit_check_count(F, run, HALF, dev())
    AO.vit_check_invisible(F, run, HALF, dev())


# ---- the fp32 set ------------------------------------------------------------------------------------------------------------------
F32 = AO.f32_cases()


@pytest.mark.parametrize("case", F32, ids=_ids(F32))
def test_f32_llama_attention(case):
    """ops_f32.llama_attention (vly_attention_f32: attention_f32_kernel below 16 queries, attention_f32_mfma_kernel from 16): its cache
    argument ends at kv_len = past + S (n_kv), so the rows from kv_len to ctx_max are replaced in (b) like any other unseen row."""
    from valley_amd import ops_f32

    def run(inp):
        return ops_f32.llama_attention(_qkv(inp, torch.float32), inp.k.float(), inp.v.float(), inp.valid, case.B, case.S, case.heads,
                                       case.past).view(case.B, case.S, case.heads, 128)
    f32 = torch.float32
    AO.check_pointer(case, lambda i: run(i), f32, dev(), rounds=1)
    AO.check_count(case, run, f32, dev(), ulps=4.0)
    AO.check_invisible(case, run, f32, dev())


@pytest.mark.parametrize("F", [1, 3])
def test_f32_vit_attention(F):
    from valley_amd import ops_f32

    def run(qkv):
        return ops_f32.vit_attention(qkv.float().contiguous(), F)
    AO.vit_check_pointer(F, run, torch.float32, dev())
    AO.vit_check_count(F, run, torch.float32, dev(), ulps=4.0)
    AO.vit_check_invisible(F, run, torch.float32, dev())


@pytest.mark.parametrize("f32", [False, True], ids=["half", "f32"])
@pytest.mark.parametrize("nseq,T,H,nhead", AO.DELTA_SHAPES)
def test_delta_attention(nseq, T, H, nhead, f32):
    """ops.delta_attention and ops_f32.delta_attention: (a) and (c).  No (b): the operation has no mask — all T keys of a unit are
    visible, there is nothing a query may not see inside its unit; (a)'s V rows differ per (sequence, step, head), so a unit that read
    another unit's keys or values fails it."""
    from valley_amd import ops, ops_f32
    dt = torch.float32 if f32 else HALF
    fn = ops_f32.delta_attention if f32 else ops.delta_attention
    q, kv, want = AO.delta_build_pointer(nseq, T, H, nhead, dt, dev())
    got = fn(q, kv, T, nhead).cpu()
    assert got.dtype == want.dtype and torch.equal(AO.bits(got), AO.bits(want)), f"{int((got != want).any(-1).sum())} rows are not their target's V"
    q, kv, want = AO.delta_build_count(nseq, T, H, nhead, dt, dev())
    got = fn(q, kv, T, nhead).cpu().double()
    assert bool(((got - want).abs() <= (4 if f32 else 1) * AO.ulp(want, dt) * (want != 0)).all()), float((got - want).abs().max())
