"""Exact GEMM oracle: every GEMM path against the true product, bit for bit.

Operands are integers |a| <= 16 and multiples of 2^-3 with |w| <= 4 (exact in bf16 and in fp16); bias and residual are fp32 values
on the 2^-3 grid.  Every partial sum is then a multiple of 2^-3 below 2^24 * 2^-3 in magnitude (asserted per case), so it is exact
in fp32 whatever the tile shape, the K order, the split or the stream-K fix-up.  Hence:
  * an fp32 output equals the float64 truth exactly;
  * a 16-bit output equals ``truth.to(HALF)`` exactly (round to nearest even, overflow to +-inf) — a partial sum that passes
    through 16-bit storage, an epilogue that truncates, or one wrong element on a ragged edge shows up as a mismatch.
Planted rows and columns put chosen exact results at the storage type's rounding ties and overflow edges.  QUICK_GELU and SwiGLU
are not exact: their 16-bit outputs are held to one ulp of the fp32 torch activation of the exact pre-activation instead."""
import functools
import json
import math
import os

import pytest
import torch

from tests.row_oracle import SENTINEL, assert_guards, guarded as _guarded      # (the guards live with the row oracle now)
from valley_amd import ops as _ops
from valley_amd.runtime import HALF  # the library's 16-bit storage type: bf16, or fp16 under VALLEY_PRECISION=fp16

pytestmark = pytest.mark.gpu
D = "cuda:0"
FP16 = HALF == torch.float16
EXACT_LIMIT = 2.0 ** 21          # 2^24 * 2^-3: below it every multiple of 2^-3 is an fp32 number

# exact results at the 16-bit type's rounding ties and overflow edge (as final outputs: bias and residual are taken out of the product)
if FP16:
    EDGES = [2049.0, 2051.0, -2049.0, -2051.0, 1025.5, 32784.0, 65504.0, 65519.0, 65520.0, -65520.0]
else:
    EDGES = [257.0, 259.0, -257.0, -259.0, 256.125, 4112.0, 4144.0, -65792.0, 66304.0, 1052672.0, -1060864.0]

HINTS_TILE = [1, 2, 3, 4, 5, 6, 7, 8, 9, 51, 53, 54, 55, 73, 74, 76, 83, 84, 86, 93, 94, 97, 98, 99, 197, 198, 199]
HINTS_NAMED = [194, 397, 398, 497]


def _terms(v):
    """v (a multiple of 2^-3) as a sum of terms with at most 8 significant bits and |t| <= 2^15: each exact in bf16 and fp16."""
    out = []
    while v != 0.0:
        m = min(abs(v), 32768.0)
        q = 2.0 ** (math.floor(math.log2(m)) - 7)
        t = math.copysign(math.floor(m / q) * q, v)
        out.append(t)
        v -= t
    return out


class Case:
    """a [M, K] and w [N, K] in HALF (host), optional fp32 bias [N] / residual [M, N], and the float64 truth of a @ w^T + bias
    (+ residual).  ``plant`` puts EDGES at chosen (row, column) pairs through dedicated K slots that only planted rows use."""

    def __init__(self, M, N, K, seed, bias=False, residual=False, plant=True, amax=16, wmax=4, device="cpu"):
        g = torch.Generator(device=device).manual_seed(seed)
        a = torch.randint(-amax, amax + 1, (M, K), generator=g, device=device, dtype=torch.int32).double()
        w = torch.randint(-8 * wmax, 8 * wmax + 1, (N, K), generator=g, device=device, dtype=torch.int32).double() / 8
        b = torch.randint(-256, 257, (N,), generator=g, device=device, dtype=torch.int32).double() / 8 if bias else None
        r = torch.randint(-256, 257, (M, N), generator=g, device=device, dtype=torch.int32).double() / 8 if residual else None
        self.pairs = []
        if plant:
            rows = [x for x in (0, M - 1, 1, M - 2, M // 2, M // 2 + 1, M // 3, 2, M - 3, M // 4, M // 5, 3) if 0 <= x < M]
            cols = [y for y in (N - 1, 0, N - 2, 1, N // 2, N - 3, N // 3, 2, N - 4, N // 4, N // 5, 3) if 0 <= y < N]
            slot = 0
            for p, T in enumerate(EDGES):
                rr, cc = rows[p % len(rows)], cols[p % len(cols)]
                want = T - (float(b[cc]) if b is not None else 0.0) - (float(r[rr, cc]) if r is not None else 0.0)
                ts = _terms(want)
                if slot + len(ts) > K or rr in [x for x, _ in self.pairs] or cc in [y for _, y in self.pairs]:
                    continue
                self.pairs.append((rr, cc))
                w[cc] = 0.0                                      # the planted column sees nothing but its own slots
                a[:, slot:slot + len(ts)] = 0.0                  # ... which belong to the planted row alone
                w[[y for _, y in self.pairs[:-1]], slot:slot + len(ts)] = 0.0
                a[rr, slot:slot + len(ts)] = 1.0
                w[cc, slot:slot + len(ts)] = torch.tensor(ts, dtype=torch.float64, device=device)
                slot += len(ts)
        self.a64, self.w64, self.b64, self.r64 = a, w, b, r
        prod = a @ w.t()
        bound = a.abs() @ w.abs().t()
        if b is not None:
            prod = prod + b
            bound = bound + b.abs()
        if r is not None:
            prod = prod + r
            bound = bound + r.abs()
        # exactness: no partial sum (any order, any split) reaches 2^24 grid steps
        assert float(bound.max()) < EXACT_LIMIT, float(bound.max())
        self.truth = prod
        self.a = a.to(HALF)
        self.w = w.to(HALF)
        assert torch.equal(self.a.double(), a) and torch.equal(self.w.double(), w)
        self.bias = b.float() if b is not None else None
        self.res = r.float() if r is not None else None

    def dev(self):
        return (self.a.to(D), self.w.to(D), None if self.bias is None else self.bias.to(D),
                None if self.res is None else self.res.to(D))


def expect(truth, dtype):
    return truth.float() if dtype == torch.float32 else truth.to(HALF)


def assert_exact(got, truth, what):
    """got (device or host) == truth rounded once to got's dtype, infinities included; names the first mismatches."""
    want = expect(truth, got.dtype).to(got.device)
    eq = got == want
    if bool(eq.all()):
        return
    bad = (~eq).nonzero()[:6].tolist()
    detail = ", ".join(f"[{i},{j}] got {float(got[i, j])!r} want {float(want[i, j])!r} (exact {float(truth[i, j])!r})" for i, j in bad)
    raise AssertionError(f"{what}: {int((~eq).sum())} of {eq.numel()} elements differ from the exact result: {detail}")


def guarded(M, No, dtype, rows=3, cols=None):
    return _guarded(M, No, dtype, rows, cols, device=D)


@functools.lru_cache(maxsize=16)
def case(M, N, K, seed, bias=False, residual=False, plant=True, amax=16, wmax=4):
    return Case(M, N, K, seed, bias, residual, plant, amax, wmax)


def strided(a):
    """a [M, K] as a column window of a wider buffer (row stride K + 128)."""
    M, K = a.shape
    big = torch.full((M, K + 128), 3.0, dtype=a.dtype, device=a.device)
    big[:, 64:64 + K] = a
    return big[:, 64:64 + K]


# ------------------------------------------------------------------------------------------------ (a) whole-tile hints
SHAPES_A = [(333, 260, 64), (517, 1028, 1536), (700, 1032, 640)]     # odd M; N = 4 (mod 8); one K step; long K; N % 8 = 0 for 397/398


@pytest.mark.parametrize("M,N,K", SHAPES_A)
@pytest.mark.parametrize("hint", HINTS_TILE + HINTS_NAMED)
def test_tile_hints_are_exact(hint, M, N, K):
    from valley_amd import ops
    for has_b, has_r in ((False, False), (True, False), (False, True), (True, True)):
        c = case(M, N, K, 11, has_b, has_r)
        a, w, b, r = c.dev()
        pw = ops.PackedWeight(w)
        for variant, av, wv in (("plain", a, w), ("strided A", strided(a), w), ("p64", a, pw)):
            runs = [(ops.EPI_NONE, torch.float32)]
            if not has_r:
                runs += [(ops.EPI_NONE, HALF), (ops.EPI_RELU, HALF)]
            for epi, od in runs:
                what = f"hint {hint} {variant} {M}x{N}x{K} epi {epi} bias {has_b} residual {has_r} out {od}"
                buf, out = guarded(M, N, od)
                ops.gemm_mfma(av, wv, b, r, epi, od, out, hint)
                truth = c.truth
                if epi == ops.EPI_RELU:
                    truth = torch.relu(truth)
                assert_exact(out, truth, what)
                assert_guards(buf, M, N, what)


# ------------------------------------------------------------------------------------------------ (b) stream-K
SK_HINTS = [t for kind, t in _ops.CANDIDATES if kind == "sk"]


@pytest.mark.parametrize("M,N,K", [(1312, 2048, 1024), (2600, 1032, 640)])
@pytest.mark.parametrize("hint", SK_HINTS)
def test_streamk_hints_are_exact(hint, M, N, K):
    """M large enough that the remainder round is split between workgroups (the slab fix-up carries fp32 partials)."""
    from valley_amd import ops
    for has_b, has_r in ((False, False), (True, True)):
        c = case(M, N, K, 21, has_b, has_r)
        a, w, b, r = c.dev()
        wv = ops.PackedWeight(w) if hint in (297, 298, 299) else w
        runs = [(torch.float32, None)] + ([] if has_r else [(HALF, None)])
        for od, _ in runs:
            what = f"stream-K hint {hint} {M}x{N}x{K} bias {has_b} residual {has_r} out {od}"
            buf, out = guarded(M, N, od)
            ops.gemm_streamk(a, wv, b, r, ops.EPI_NONE, od, out, hint)
            assert_exact(out, c.truth, what)
            assert_guards(buf, M, N, what)
        if not has_r:
            buf, out = guarded(M, N, HALF)
            ops.gemm_streamk(a, wv, b, None, ops.EPI_RELU, HALF, out, hint)
            assert_exact(out, torch.relu(c.truth), f"stream-K hint {hint} ReLU")
    assert ops.sk_error_flag(torch.device(D)) == 0


# ------------------------------------------------------------------------------------------------ (c) split-K pairs
def _halves(c, bias):
    K = c.a64.shape[1]
    k0 = (K // 64 >> 1) * 64
    p0 = c.a64[:, :k0] @ c.w64[:, :k0].t()
    p1 = c.a64[:, k0:] @ c.w64[:, k0:].t()
    if bias is not None:
        p0 = p0 + c.b64
    return p0, p1


@pytest.mark.parametrize("M,N,K", [(333, 260, 128), (1312, 1024, 1088), (77, 512, 192)])
@pytest.mark.parametrize("hint", [0, 2, 6, 7, 8, 76, 84, 86])
def test_splitk2_partials_are_each_rounded_once(hint, M, N, K):
    from valley_amd import ops
    for has_b in (False, True):
        c = case(M, N, K, 31, has_b, False)
        a, w, b, _ = c.dev()
        p0, p1 = _halves(c, b)
        for variant, wv in (("plain", w), ("p64", ops.PackedWeight(w))):
            buf0, o0 = guarded(M, N, HALF)
            buf1, o1 = guarded(M, N, HALF)
            ops.gemm_mfma_splitk2(a, wv, b, o0, o1, hint)
            what = f"split-K pair hint {hint} {variant} {M}x{N}x{K} bias {has_b}"
            assert_exact(o0, p0, what + " (first half + bias)")
            assert_exact(o1, p1, what + " (second half)")
            assert_guards(buf0, M, N, what)
            assert_guards(buf1, M, N, what)


@pytest.mark.parametrize("kind,hint", [("tile2k", t) for t in (2, 6, 7, 8, 76, 84, 86)] + [("tile", 8), ("tile", 197)])
def test_gemm2_pair_dispatch_is_exact(kind, hint, monkeypatch):
    """ops.gemm2 (EPI_PAIR): a table choice of the tile2k kind returns two partials, each the RNE rounding of its own exact half-K
    sum, the bias in the first; an ordinary kind returns one exact product and leaves out2 untouched."""
    from valley_amd import ops
    monkeypatch.setattr(ops, "GEMM_MODE", "tuned")
    M, N, K = 1312, 1028, 1024
    for has_b in (False, True):
        c = case(M, N, K, 41, has_b, False)
        a, w, b, _ = c.dev()
        key = ops._tune_key(M, N, K, ops.EPI_PAIR, HALF, has_b, False, w)
        monkeypatch.setitem(ops._TUNED, key, (kind, hint))
        buf0, o0 = guarded(M, N, HALF)
        buf1, o1 = guarded(M, N, HALF)
        n = ops.gemm2(a, w, o0, o1, b)
        what = f"gemm2 {kind} {hint} bias {has_b}"
        if kind == "tile2k":
            assert n == 2, what
            p0, p1 = _halves(c, b)
            assert_exact(o0, p0, what + " (first partial)")
            assert_exact(o1, p1, what + " (second partial)")
            assert_guards(buf1, M, N, what)
        else:
            assert n == 1, what
            assert_exact(o0, c.truth, what)
            assert bool((buf1 == SENTINEL).all()), what + ": out2 was written"
        assert_guards(buf0, M, N, what)


# ------------------------------------------------------------------------------------------------ (d) small-M kernels
@pytest.mark.parametrize("M,N,K", [(9, 256, 128), (77, 1024, 640), (200, 4096, 2048), (256, 96, 512)])
def test_skinny_is_exact(M, N, K):
    from valley_amd import ops
    for has_b in (False, True):
        c = case(M, N, K, 51, has_b, False)
        a, w, b, _ = c.dev()
        for variant, wv in (("plain", w), ("p64", ops.PackedWeight(w))):
            for epi in (ops.EPI_NONE, ops.EPI_RELU):
                what = f"skinny {variant} {M}x{N}x{K} epi {epi} bias {has_b}"
                assert ops.skinny_ok(M, N, K, epi, HALF, None), what
                buf, out = guarded(M, N, HALF)
                ops.gemm_skinny(a, wv, b, epi, out)
                assert_exact(out, torch.relu(c.truth) if epi == ops.EPI_RELU else c.truth, what)
                assert_guards(buf, M, N, what)


@pytest.mark.parametrize("M", [1, 2, 3, 5, 8, 11, 16])
@pytest.mark.parametrize("N,K", [(1000, 1024), (4100, 320)])
def test_gemv_is_exact(M, N, K):
    """M <= 2: the VALU weight-streaming kernels; 3 <= M <= 16: the matrix-core form (no ReLU epilogue in either)."""
    from valley_amd import ops
    for has_b, has_r in ((False, False), (True, False), (True, True)):
        c = case(M, N, K, 61 + M, has_b, has_r)
        a, w, b, r = c.dev()
        for variant, wv in (("plain", w), ("p64", ops.PackedWeight(w))):
            runs = [(ops.EPI_NONE, torch.float32)] + ([] if has_r else [(ops.EPI_NONE, HALF)])
            for epi, od in runs:
                what = f"gemv {variant} M={M} {N}x{K} epi {epi} bias {has_b} residual {has_r} out {od}"
                buf, out = guarded(M, N, od)
                ops.gemv(a, wv, b, r, epi, od, out)
                assert_exact(out, c.truth, what)
                assert_guards(buf, M, N, what)


# ------------------------------------------------------------------------------------------------ (e) by-name hints: bias values
BIAS_VALUES = [0.0, 3 * 2.0 ** -20, 11 * 2.0 ** -20, round(1e-3 * 2 ** 19) * 2.0 ** -19, 7e4, -7e4, 1e6, -1e6]


@pytest.mark.parametrize("bias_value", BIAS_VALUES)
@pytest.mark.parametrize("hint", [397, 398, 497])
def test_named_hints_bias_values_are_exact(hint, bias_value):
    """The bias enters exactly, whatever its magnitude.  Small biases ride on a product |P| <= 1 (exact in 21 bits); large ones are
    cancelled in half of the rows by dedicated K slots (1 x the exact 16-bit pieces of -bias), so those rows come out small and
    finite in 16 bits while the others overflow (to +-inf in fp16) — a bias that passes through the storage type in pieces
    (gemm_p32.hip on fp16 storage before it added the bias in fp32) turns into inf / NaN or loses its low bits."""
    from valley_amd import ops
    M, N, K = 700, 1032, 640
    g = torch.Generator(device="cpu").manual_seed(71)
    a = torch.zeros((M, K), dtype=torch.float64)
    w = torch.zeros((N, K), dtype=torch.float64)
    a[:, 64:72] = torch.randint(-1, 2, (M, 8), generator=g).double()
    w[:, 64:72] = torch.randint(-1, 2, (N, 8), generator=g).double() / 8
    if abs(bias_value) >= 1:
        ts = _terms(-bias_value)
        a[0::2, :len(ts)] = 1.0
        w[:, :len(ts)] = torch.tensor(ts, dtype=torch.float64)
    bias = torch.full((N,), bias_value, dtype=torch.float64)
    bias[N - 1] = 0.0
    truth = a @ w.t() + bias
    bound = a.abs() @ w.abs().t() + bias.abs()
    assert float(bound.max()) < 2.0 ** 24 * 2.0 ** -20 if abs(bias_value) < 1 else float(bound.max()) < EXACT_LIMIT
    assert torch.equal(truth.float().double(), truth)            # the fp32 result is exact
    ad, wd, bd = a.to(HALF).to(D), w.to(HALF).to(D), bias.float().to(D)
    assert torch.equal(ad.double().cpu(), a) and torch.equal(wd.double().cpu(), w)
    for od in (torch.float32, HALF):
        for variant, wv in (("plain", wd), ("p64", ops.PackedWeight(wd))):
            what = f"hint {hint} {variant} bias {bias_value!r} out {od}"
            buf, out = guarded(M, N, od)
            ops.gemm_mfma(ad, wv, bd, None, ops.EPI_NONE, od, out, hint)
            assert_exact(out, truth, what)
            assert_guards(buf, M, N, what)


# ------------------------------------------------------------------------------------------------ (f) nonlinear epilogues
def ulp16(x):
    """One unit in the last place of the 16-bit type at |x| (subnormal spacing below the normal range)."""
    fi = torch.finfo(HALF)
    mag = x.abs().clamp_min(fi.tiny)
    return torch.exp2(torch.floor(torch.log2(mag))) * fi.eps


def act_ref(pre, epi):
    from valley_amd import ops
    p = pre.float()
    if epi == ops.EPI_QUICK_GELU:
        return p * torch.sigmoid(1.702 * p)
    return torch.nn.functional.silu(p[:, 0::2]) * p[:, 1::2]


def assert_activation(got, pre, epi, what):
    """16-bit output within one ulp of the fp32 torch activation of the exact pre-activation (2^-100 at the least), and +-inf
    exactly where that activation rounded to 16 bits overflows."""
    ref = act_ref(pre.cpu(), epi)
    got = got.float().cpu()
    ref16 = ref.to(HALF).float()
    inf = torch.isinf(ref16)
    assert torch.equal(torch.isinf(got), inf) and torch.equal(got[inf], ref16[inf]), f"{what}: overflow pattern differs"
    fin = ~inf
    err = (got[fin] - ref[fin]).abs()
    # below 2^-100 the activation's fp32 exp / reciprocal may flush to zero (pre-activations under -50): not a 16-bit rounding
    tol = ulp16(ref[fin]).clamp_min(2.0 ** -100)
    bad = err > tol
    assert not bool(bad.any()), (f"{what}: {int(bad.sum())} outputs beyond one ulp, worst {float((err / tol).max()):.2f} ulp; "
                                 f"first got {got[fin][bad][:4].tolist()} ref {ref[fin][bad][:4].tolist()}")


# pre-activations up to |x| ~ 60 in the random part; the planted edges add overflow (fp16) and large values
@pytest.mark.parametrize("hint", HINTS_TILE + HINTS_NAMED)
def test_nonlinear_epilogues_within_one_ulp(hint):
    from valley_amd import ops
    for epi, (M, N, K), has_b in ((ops.EPI_QUICK_GELU, (333, 1032, 640), True), (ops.EPI_SWIGLU, (517, 1040, 640), False)):
        c = case(M, N, K, 81, has_b, False, True, 4, 1)
        a, w, b, _ = c.dev()
        No = N // 2 if epi == ops.EPI_SWIGLU else N
        for variant, wv in (("plain", w), ("p64", ops.PackedWeight(w))):
            what = f"hint {hint} {variant} epi {epi} {M}x{N}x{K}"
            buf, out = guarded(M, No, HALF)
            ops.gemm_mfma(a, wv, b, None, epi, HALF, out, hint)
            assert_activation(out, c.truth, epi, what)
            assert_guards(buf, M, No, what)


@pytest.mark.parametrize("M,N,K,packed", [(333, 2304, 640, False), (517, 1152, 1024, True), (1000, 27648 // 8, 256, True)])
def test_hint_194_swiglu_within_one_ulp(M, N, K, packed):
    """Hint 194 (192 x 384 persistent tile, SwiGLU into aligned 16-bit rows) at ragged shapes it takes."""
    from valley_amd import ops
    c = case(M, N, K, 91, False, False, True, 4, 1)
    a, w, _, _ = c.dev()
    wv = ops.PackedWeight(w) if packed else w
    buf, out = guarded(M, N // 2, HALF)
    ops.gemm_mfma(a, wv, None, None, ops.EPI_SWIGLU, HALF, out, 194)
    assert_activation(out, c.truth, ops.EPI_SWIGLU, f"hint 194 {M}x{N}x{K}")
    assert_guards(buf, M, N // 2, "hint 194")


@pytest.mark.parametrize("hint", [0, 51, 55, 73, 76, 84, 86, 155, 186, 298, 299])
def test_streamk_nonlinear_epilogues_within_one_ulp(hint):
    from valley_amd import ops
    M, N, K = 1312, 2048, 1024
    for epi, has_b in ((ops.EPI_QUICK_GELU, True), (ops.EPI_SWIGLU, False)):
        c = case(M, N, K, 95, has_b, False, True, 4, 1)
        a, w, b, _ = c.dev()
        wv = ops.PackedWeight(w) if hint in (297, 298, 299) else w
        No = N // 2 if epi == ops.EPI_SWIGLU else N
        buf, out = guarded(M, No, HALF)
        ops.gemm_streamk(a, wv, b, None, epi, HALF, out, hint)
        assert_activation(out, c.truth, epi, f"stream-K {hint} epi {epi}")
        assert_guards(buf, M, No, f"stream-K {hint} epi {epi}")
    assert ops.sk_error_flag(torch.device(D)) == 0


# ------------------------------------------------------------------------------------------------ (g) shipped-table replay
_TABLE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "valley_amd", "tuned", "gfx950.json")
with open(_TABLE) as _f:
    TABLE = json.load(_f)


def _spy(monkeypatch, ops):
    """Record (kind, tile hint) of every launch the dispatcher makes."""
    log = []
    for name, kind in (("gemm_mfma", "tile"), ("gemm_streamk", "sk"), ("gemm_mfma_splitk2", "tile2k"), ("gemm_skinny", "skinny"),
                       ("gemm_mfma_qkv_rope", "tile")):
        fn = getattr(ops, name)

        def wrap(*args, _fn=fn, _kind=kind, _name=name, **kw):
            hint = kw.get("tile_hint", args[-1] if _name in ("gemm_mfma_splitk2", "gemm_mfma_qkv_rope") else (args[7] if len(args) > 7 else 0))
            if _kind == "skinny":
                hint = 0
            log.append((_kind, hint))
            return _fn(*args, **kw)
        monkeypatch.setattr(ops, name, wrap)
    return log


@pytest.mark.parametrize("entry", TABLE, ids=lambda e: "-".join(str(x) for x in e["key"]).replace("torch.", ""))
def test_shipped_table_entry_runs_its_kernel_exactly(entry, monkeypatch):
    from valley_amd import ops
    monkeypatch.setattr(ops, "GEMM_MODE", "tuned")
    key = entry["key"]
    M, N, K, epi, dt, has_b, has_r = key[:7]
    extra = key[7:]
    p64, tiles = "p64" in extra, "tiles" in extra
    od = torch.float32 if dt == "torch.float32" else HALF
    want = (entry["kind"], entry["tile"])
    c = Case(M, N, K, 101, has_b, has_r, plant=False, device=D) if epi != ops.EPI_QUICK_GELU and epi != ops.EPI_SWIGLU else \
        Case(M, N, K, 101, has_b, has_r, plant=False, amax=4, wmax=1, device=D)
    a, w = c.a, c.w
    b = c.bias
    r = c.res
    wv = ops.PackedWeight(w) if p64 else w
    tkey = ops._tune_key(M, N, K, epi, od, has_b, has_r, wv) + (("tiles",) if tiles else ())
    assert ops._TUNED.get(tkey) == want, (tkey, ops._TUNED.get(tkey), want)
    log = _spy(monkeypatch, ops)
    try:
        if epi == ops.EPI_PAIR:
            buf0, o0 = guarded(M, N, od)
            buf1, o1 = guarded(M, N, od)
            n = ops.gemm2(a, wv, o0, o1, b)
            assert log == [want], (log, want)
            if n == 2:
                k0 = (K // 64 >> 1) * 64
                p0 = c.a64[:, :k0] @ c.w64[:, :k0].t()
                if b is not None:
                    p0 = p0 + c.b64
                assert_exact(o0, p0, f"table {key} first partial")
                del p0
                assert_exact(o1, c.a64[:, k0:] @ c.w64[:, k0:].t(), f"table {key} second partial")
            else:
                assert_exact(o0, c.truth, f"table {key}")
                assert bool((buf1 == SENTINEL).all())
            assert_guards(buf0, M, N, f"table {key}")
        elif epi == ops.EPI_QKV_ROPE:
            B, S, heads = 1, M, N // 3 // 128
            kc = torch.zeros((B, heads, S, 128), dtype=HALF, device=D)
            vc = torch.zeros_like(kc)
            pos = torch.arange(S, dtype=torch.float32, device=D)[:, None]
            inv = 1.0 / (10000.0 ** (torch.arange(0, 128, 2, dtype=torch.float32, device=D) / 128))
            cos, sin = torch.cos(pos * inv).contiguous(), torch.sin(pos * inv).contiguous()
            qkv = torch.empty((M, N), dtype=HALF, device=D)
            ops.gemm_qkv_rope(a, wv, qkv, ops.RopeKV(kc, vc, cos, sin, B, S, heads, 0))
            assert log == [want], (log, want)
            # the fused epilogue is bit-identical to the exact product followed by rope_kv
            plain = torch.empty((M, N), dtype=HALF, device=D)
            ops.gemm_mfma(a, wv, out=plain, tile_hint=197)
            assert_exact(plain, c.truth, f"table {key} (the product under the fused RoPE)")
            kc2, vc2 = torch.zeros_like(kc), torch.zeros_like(vc)
            ops.rope_kv(plain, kc2, vc2, cos, sin, B, S, heads, 0)
            H = N // 3
            assert torch.equal(qkv[:, :H], plain[:, :H]) and torch.equal(kc, kc2) and torch.equal(vc, vc2), f"table {key}"
        else:
            No = N // 2 if epi == ops.EPI_SWIGLU else N
            buf, out = guarded(M, No, od)
            if tiles:
                ops.gemm_tiles_tuned(a, wv, b, r, out=out)
            else:
                ops.gemm(a, wv, b, r, epi, od, out)
            assert log == [want], (log, want)
            if epi in (ops.EPI_QUICK_GELU, ops.EPI_SWIGLU):
                assert_activation(out, c.truth, epi, f"table {key}")
            else:
                assert_exact(out, c.truth, f"table {key}")
            assert_guards(buf, M, No, f"table {key}")
        if entry["kind"] == "sk":
            assert ops.sk_error_flag(torch.device(D)) == 0
    finally:
        del c, a, w, b, r, wv
        torch.cuda.empty_cache()
