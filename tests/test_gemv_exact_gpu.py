"""Exact decode GEMV oracle: every weight-streaming branch of valley_amd/csrc/gemv_bf16.hip against the truth, bit for bit.

Cases, the dispatch mirror and the checks live in tests/gemv_oracle.py (its docstring holds the exactness argument); every check
asserts through the mirror that its call reaches the kernel it names.  The two shapes the suite had before stay where they were
(test_gemv_is_exact in tests/test_gemm_exact_gpu.py).  Branches behind environment switches run in tests/gemv_worker.py, once each;
vly_gemv_attnmerge_bf16 (experimental library) is held to the truth in tests/test_decode_merge_gpu.py."""
import json
import os
import subprocess
import sys

import pytest
import torch

from tests import gemv_oracle as G
from tests.row_oracle import SENTINEL
from valley_amd.runtime import HALF

pytestmark = pytest.mark.gpu
D = G.D
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------ 1. VALU kernels, M <= 2
@pytest.mark.parametrize("M", [1, 2])
@pytest.mark.parametrize("N,K", [(1001, 1032), (3, 8)])
def test_short_rows_are_exact(M, N, K):
    """gemv_kernel<MR, *, *, 1, 2> (K < 2048: a wave owns a row pair) — test_gemv_is_exact's branch, here with odd N, a K that is no
    multiple of 64 and a single chunk, and with the mirror's word that it is this kernel."""
    G.check_linear(M, N, K, f"gemv_kernel<MR={M},KS=1,NR=2>")


@pytest.mark.parametrize("M", [1, 2])
@pytest.mark.parametrize("N,K", [(s.N, s.K) for s in G.split_shapes()])
def test_k_split_is_exact(M, N, K):
    """gemv_kernel<MR, *, *, 4, 2>: the fixed-order sum over four waves through LDS, has1 / bias / ldr / lda edges."""
    G.check_linear(M, N, K, f"gemv_kernel<MR={M},KS=4,NR=2>")


@pytest.mark.parametrize("M", [1, 2])
@pytest.mark.parametrize("which", [0, 1, 2, 3])
def test_four_rows_per_workgroup_is_exact(M, which):
    """gemv_kernel<MR, *, *, 4, 4> by the natural rule at K = 8192: N = 16 CUs + 1, + 2, + 3 (the ragged remainders of a four-row
    block) and 20 CUs.  A device on which the rule does not select four rows for these N fails here (check_linear asserts the mirror)."""
    s = G.four_row_shapes(G.cu_count())[which]
    assert G.four_rows(s.N, s.K, G.cu_count()), (s, G.cu_count())
    G.check_linear(M, s.N, s.K, f"gemv_kernel<MR={M},KS=4,NR=4>", full=which in (1, 2))


@pytest.mark.parametrize("M", [1, 2])
def test_valu_epilogues_within_one_ulp(M):
    """SwiGLU and QUICK_GELU of the K-split kernel and of the four-row kernel (whose last block holds one (gate, up) pair)."""
    small, big = G.epilogue_shapes(G.cu_count())
    G.check_epilogues(M, small.N, small.K, f"gemv_kernel<MR={M},KS=4,NR=2>")
    G.check_epilogues(M, big.N, big.K, f"gemv_kernel<MR={M},KS=4,NR=4>")


# ------------------------------------------------------------------------------------------------ 2. VALU fallback, 3 <= M <= 8
@pytest.mark.parametrize("M", G.FALLBACK_MS)
@pytest.mark.parametrize("N,K,layout,reason", G.FALLBACK)
def test_valu_fallback_is_exact(M, N, K, layout, reason):
    """gemv_kernel<4 / 8>: what 3 <= M <= 8 runs when the matrix-core form's vector accesses do not line up, with the min(m, M - 1)
    row clamp at M = 3, 5, 7."""
    G.check_linear(M, N, K, f"gemv_kernel<MR={4 if M <= 4 else 8},KS={4 if K >= 2048 else 1},NR=2>", layout=layout, reason=reason)


@pytest.mark.parametrize("M", G.FALLBACK_MS)
def test_valu_fallback_epilogues_within_one_ulp(M):
    N, K = G.FALLBACK_EPILOGUE
    G.check_epilogues(M, N, K, f"gemv_kernel<MR={4 if M <= 4 else 8},KS=1,NR=2>")


@pytest.mark.parametrize("N,K", [(1001, 1024), (1002, 2056)])
def test_valu_fallback_is_batch_invariant(N, K):
    """Rows 0 .. M - 1 of an 8-row call equal the M-row call, bit for bit, for M = 5, 7 (both run the MR = 8 kernel: one summation
    order) — the property test_gemv states for the matrix-core form."""
    from valley_amd import ops
    g = torch.Generator(device="cpu").manual_seed(5)
    a = torch.randn((8, K), generator=g).to(HALF).to(D)
    w = (0.05 * torch.randn((N, K), generator=g)).to(HALF).to(D)
    b = torch.randn((N,), generator=g).to(D)
    for od in (torch.float32, HALF):
        whole = torch.empty((8, N), dtype=od, device=D)
        assert G._call_branch(8, N, K, G.EPI_NONE, whole, b, None)[0] == f"gemv_kernel<MR=8,KS={4 if K >= 2048 else 1},NR=2>"
        ops.gemv(a, w, b, None, ops.EPI_NONE, od, whole)
        for M in (5, 7):
            part = torch.empty((M, N), dtype=od, device=D)
            assert G._call_branch(M, N, K, G.EPI_NONE, part, b, None)[0] == f"gemv_kernel<MR=8,KS={4 if K >= 2048 else 1},NR=2>"
            ops.gemv(a[:M], w, b, None, ops.EPI_NONE, od, part)
            assert torch.equal(part, whole[:M]), (M, N, K, od)


# ------------------------------------------------------------------------------------------------ 3. matrix-core forms
@pytest.mark.parametrize("N,K,M", [(s.N, s.K, M) for s in G.MFMA for M in s.Ms])
def test_matrix_core_forms_are_exact(N, K, M):
    """The sixteen-row form for M <= 8 (reached by N >= 12273 or by K % 128 != 0) and BIGM, beside test_gemv_is_exact's HALF8 shapes."""
    want = "gemv_mfma2<BIGM>" if M > 8 else "gemv_mfma2<16>"
    G.check_linear(M, N, K, want, full=N < 2000 or M == 3)


@pytest.mark.parametrize("N,K,M,branch", G.MFMA_EPILOGUE)
def test_matrix_core_epilogues_within_one_ulp(N, K, M, branch):
    G.check_epilogues(M, N, K, branch)


# ------------------------------------------------------------------------------------------------ 4. behind environment switches
def _worker(which, env_add):
    env = {k: v for k, v in os.environ.items() if k != "VALLEY_HIP_LIB" and not k.startswith("VLY_GEMV_")}
    env.update(env_add)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "gemv_worker.py"), which], cwd=ROOT, env=env, stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, timeout=300)
    out = r.stdout.decode(errors="replace")
    assert r.returncode == 0, out[-3000:]
    res = json.loads([ln for ln in out.splitlines() if ln.startswith("{")][-1])
    assert res["ok"] and res["which"] == which and res["storage"] == (1 if HALF == torch.float16 else 0), res
    return res


def test_pinned_four_rows_and_valu_rows_are_exact():
    """VLY_GEMV_ROWS=4 VLY_GEMV_MFMA=0: the four-row kernel at (9, 2048), (10, 2056), (1001, 4096) on any device; the VALU MR = 4 / 8
    kernels at aligned shapes, K split included."""
    res = _worker("A", G.WORKER_A_ENV)
    assert set(res["reached"]) == {"gemv_kernel<MR=1,KS=4,NR=4>", "gemv_kernel<MR=2,KS=4,NR=4>", "gemv_kernel<MR=4,KS=1,NR=2>",
                                   "gemv_kernel<MR=8,KS=1,NR=2>", "gemv_kernel<MR=4,KS=4,NR=2>", "gemv_kernel<MR=8,KS=4,NR=2>"}, res
    assert res["linear_checks"] == 15


def test_global_fragment_matrix_core_form_is_exact():
    """VLY_GEMV_MFMA=1: gemv_mfma_kernel, shipped in both libraries as the A/B form."""
    res = _worker("B", G.WORKER_B_ENV)
    assert res["reached"] == ["gemv_mfma"] and res["linear_checks"] == 16, res


# ------------------------------------------------------------------------------------------------ 5. vly_gemv_rmsnorm_bf16
def _norm_shapes():
    # (N as a multiple of the CU count and a remainder, K): the device is asked when the test runs, not at collection
    return [(0, s.N, s.K) for s in G.norm_shapes(1)[:6]] + [(8, -2, 2048), (8, 2, 2048), (16, 6, 2048), (24, 3, 2048), (0, 1001, 5120)]


def _plan_is_what_the_case_is_for(per_cu, rem, plan):
    if per_cu == 8:
        assert plan.grid == G.cu_count() and (set(plan.reduces) == {1} if rem < 0 else plan.reduces[0] == 2 and set(plan.reduces[1:]) == {1}), plan
    elif per_cu == 16:
        assert max(plan.reduces) == 3 and "break" in plan.exits, plan
    elif per_cu == 24:
        assert max(plan.reduces) == 4 and plan.exits == {"end", "break"}, plan


@pytest.mark.parametrize("M", [1, 2])
@pytest.mark.parametrize("per_cu,rem,K", _norm_shapes())
def test_gemv_rmsnorm_is_exact(M, per_cu, rem, K):
    """The exact prologue (x = gamma h / 2): every output of the fused norm + GEMV is the float64 truth rounded once, across the
    CH = 2 / 3 boundary with the ragged chunk of each, and at the grid edges (one, two, three and four trips, odd N)."""
    N = per_cu * G.cu_count() + rem
    plan = G.norm_plan(M, N, K, G.cu_count())
    assert plan.kernel == f"gemv_norm_kernel<MR={M},CH={2 if K <= 4096 else 3},PRO=0>"
    _plan_is_what_the_case_is_for(per_cu, rem, plan)
    G.check_norm_linear(M, N, K)
    if N % 2 == 0:
        G.check_norm_swiglu(M, N, K)


@pytest.mark.parametrize("M", [1, 2])
@pytest.mark.parametrize("per_cu,rem,K", _norm_shapes())
def test_gemv_rmsnorm_is_bit_identical_to_the_pair_at_the_edges(M, per_cu, rem, K):
    """ops.rmsnorm then ops.gemv on Gaussian H, as test_gemv_rmsnorm_is_bit_identical_to_the_pair, at the ragged K and grid-edge N."""
    from valley_amd import ops
    N = per_cu * G.cu_count() + rem
    g = torch.Generator(device="cpu").manual_seed(31 + K + M)
    h = (1.5 * torch.randn((M, K), generator=g) + 0.1).to(D)
    gm = (0.1 * torch.randn((K,), generator=g) + 1.0).to(D)
    w = (0.03 * torch.randn((N, K), generator=g)).to(HALF).to(D)
    bias, res = (0.5 * torch.randn((N,), generator=g)).to(D), torch.randn((M, N), generator=g).to(D)
    x = ops.rmsnorm(h, gm, 1e-6)
    for kw in (dict(), dict(out_dtype=torch.float32), dict(bias=bias, residual=res, out_dtype=torch.float32)) + \
            ((dict(epilogue=ops.EPI_SWIGLU),) if N % 2 == 0 else ()):
        assert torch.equal(ops.gemv(x, w, **kw), ops.gemv_rmsnorm(h, gm, 1e-6, w, **kw)), (M, N, K, kw)


# ------------------------------------------------------------------------------------------------ refusals
def _refused(fn, name, args, outs):
    from valley_amd import lib
    L = lib.load()
    before = [o.clone() for o in outs]
    rc = getattr(L, fn)(*args)
    torch.cuda.synchronize()
    msg = L.vly_last_error().decode(errors="replace")
    assert rc == -22, (name, rc)
    assert fn in msg, (name, msg)
    for o, b in zip(outs, before):
        assert torch.equal(o, b), f"{name}: the output was written"


def test_gemv_refusals():
    """-22, an error text that names the entry point, and an untouched output (buffers are sized for the refused shape)."""
    from valley_amd import ops
    a = torch.ones((17, 1032), dtype=HALF, device=D)
    w = torch.ones((1002, 1032), dtype=HALF, device=D)
    r = torch.zeros((17, 1002), dtype=torch.float32, device=D)
    c = torch.full((17, 1002), SENTINEL, dtype=torch.float32, device=D)
    p = lambda t: t.data_ptr()                                                      # noqa: E731
    # (A, W, bias, residual, C, M, N, K, lda, ldw, ldc, ldr, epilogue, out_dtype, stream)
    for name, args in (
            ("M = 17", (p(a), p(w), None, None, p(c), 17, 1000, 1024, 1032, 1032, 1002, 0, ops.EPI_NONE, ops.OUT_F32, None)),
            ("K % 8", (p(a), p(w), None, None, p(c), 1, 1000, 1028, 1032, 1032, 1002, 0, ops.EPI_NONE, ops.OUT_F32, None)),
            ("SwiGLU + residual", (p(a), p(w), None, p(r), p(c), 1, 1000, 1024, 1032, 1032, 1002, 1002, ops.EPI_SWIGLU, ops.OUT_BF16, None)),
            ("SwiGLU, odd N", (p(a), p(w), None, None, p(c), 1, 1001, 1024, 1032, 1032, 1002, 0, ops.EPI_SWIGLU, ops.OUT_BF16, None)),
            ("QUICK_GELU to fp32, M = 2", (p(a), p(w), None, None, p(c), 2, 1000, 1024, 1032, 1032, 1002, 0, ops.EPI_QUICK_GELU, ops.OUT_F32, None)),
            ("ReLU, M = 8", (p(a), p(w), None, None, p(c), 8, 1000, 1024, 1032, 1032, 1000, 0, ops.EPI_RELU, ops.OUT_BF16, None)),
            ("SwiGLU to fp32, M = 11", (p(a), p(w), None, None, p(c), 11, 1000, 1024, 1032, 1032, 1000, 0, ops.EPI_SWIGLU, ops.OUT_F32, None)),
            ("M = 9, N % 4", (p(a), p(w), None, None, p(c), 9, 1001, 1024, 1032, 1032, 1002, 0, ops.EPI_NONE, ops.OUT_F32, None)),
            ("M = 16, K % 64", (p(a), p(w), None, None, p(c), 16, 1000, 1032, 1032, 1032, 1000, 0, ops.EPI_NONE, ops.OUT_F32, None))):
        _refused("vly_gemv_bf16", name, args, [c])


def test_gemv_rmsnorm_refusals():
    from valley_amd import lib, ops
    K = 6160
    h = torch.ones((3, K), dtype=torch.float32, device=D)
    gm = torch.ones((K,), dtype=torch.float32, device=D)
    w = torch.ones((12, K), dtype=HALF, device=D)
    r = torch.zeros((3, 12), dtype=torch.float32, device=D)
    c = torch.full((3, 12), SENTINEL, dtype=torch.float32, device=D)
    p = lambda t: t.data_ptr()                                                      # noqa: E731
    # (H, gamma, eps, W, bias, residual, C, M, N, K, ldh, ldw, ldc, ldr, epilogue, out_dtype, stream)
    cases = [("M = 3", (p(h), p(gm), 1e-6, p(w), None, None, p(c), 3, 12, 2048, K, K, 12, 0, ops.EPI_NONE, ops.OUT_F32, None))]
    for Kbad in (2040, 6152, 2052):
        cases.append((f"K = {Kbad}", (p(h), p(gm), 1e-6, p(w), None, None, p(c), 1, 12, Kbad, K, K, 12, 0, ops.EPI_NONE, ops.OUT_F32, None)))
    cases += [("SwiGLU, odd N", (p(h), p(gm), 1e-6, p(w), None, None, p(c), 1, 11, 2048, K, K, 12, 0, ops.EPI_SWIGLU, ops.OUT_BF16, None)),
              ("SwiGLU + residual", (p(h), p(gm), 1e-6, p(w), None, p(r), p(c), 1, 12, 2048, K, K, 12, 12, ops.EPI_SWIGLU, ops.OUT_BF16, None)),
              ("QUICK_GELU", (p(h), p(gm), 1e-6, p(w), None, None, p(c), 1, 12, 2048, K, K, 12, 0, ops.EPI_QUICK_GELU, ops.OUT_BF16, None)),
              ("SwiGLU to fp32", (p(h), p(gm), 1e-6, p(w), None, None, p(c), 2, 12, 2048, K, K, 12, 0, ops.EPI_SWIGLU, ops.OUT_F32, None))]
    for name, args in cases:
        _refused("vly_gemv_rmsnorm_bf16", name, args, [c])
    # C overlapping H: the first words, the last word of row M - 1, and (16-bit) the tail of a row
    for name, cptr, M, od in (("C = H", p(h), 1, ops.OUT_F32), ("C on the last word of H's row 1", p(h) + (K + 2048 - 1) * 4, 2, ops.OUT_F32),
                              ("16-bit C inside H", p(h) + 2044 * 4, 1, ops.OUT_BF16)):
        _refused("vly_gemv_rmsnorm_bf16", name, (p(h), p(gm), 1e-6, p(w), None, None, cptr, M, 12, 2048, K, K, 12, 0, ops.EPI_NONE, od, None), [h])
    assert "overlaps H" in lib.load().vly_last_error().decode()
