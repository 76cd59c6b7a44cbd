"""The row-kernel oracle: cases, float64 truths and checks for the HBM-bound row kernels (norm_elementwise.hip, temporal_delta.hip and
their fp32 twins in precise_f32.hip).  Host only: nothing here needs a GPU; tests/test_rows_exact_gpu.py feeds the checks with what
the HIP kernels wrote, tests/test_rows_exact_cpu.py with torch emulations of the kernels and with mutated emulations that must fail.

What is held exactly, and why it can be:
  * copies, casts, max, gathers: the output is the input (rounded once to the storage type): bit for bit;
  * the residual update h += delta: one fp32 add per delta, IEEE: equals the same add on the CPU, in the kernel's order;
  * sums of grid-valued inputs (multiples of 2^-6 below 8, or of 2^-2 below 2 for the score's products): every partial sum in any
    order is a multiple of the grid below 2^24 grid steps, hence exact in fp32 (the bound is asserted per case, as the GEMM oracle's
    ``Case`` does).
What is not exact is held by three rules:
  * fp32 outputs: |got - ref64| <= 8 E, E = the largest |torch fp32 - ref64| of the same formula on the same case (the factor covers
    another summation order and the hardware rsqrt / exp), never more than 2e-5, the project's older bound.  The mean-1000 row has
    its own E;
  * 16-bit outputs: every element within one ulp of ``ref64.to(HALF)`` (as |got - want| <= ulp(want), not a bit distance), and at
    most 1e-3 of a case's elements different from it at all — a condition: the fp32 formula itself differs in < 2e-4 of them.
    A norm's 16-bit output is an fp32 result rounded once, so the fp32 rule's bound (a few 1e-6) is added to the ulp: it is the whole
    tolerance only for outputs below 1e-3 in magnitude, whose own ulp is smaller than any fp32 evaluation's absolute error (the
    torch fp32 formula itself lands two ulps from the truth at an output of 1.2e-6: test_rows_exact_cpu.py shows it);
  * importance pooling: one 16-bit ulp plus 8 E.

Large-M norm cases (M = 4097 is what reaches norm_kernel<16 / 20 / 32>) draw their rows from 131 distinct ones (row i = base row
i mod 131, planted rows apart): truths are computed on the distinct rows and expanded by index, the comparison still covers every
element of every row.  131 is odd and larger than any block of rows a workgroup handles: a row read or written at the wrong index
differs, unless it is off by a multiple of 131."""
import functools
import math
import os
import re
from typing import Dict, List, Optional

import torch

from tests.attention_oracle import bits, rope64, rope_tables, ulp  # noqa: F401  (one ulp / bits definition for both oracles)

SENTINEL = 7.0
CAP = 1e-3                      # share of a case's 16-bit elements that may differ from ref64.to(HALF) at all
F32_FACTOR = 8.0
F32_CEIL = 2e-5                 # the project's older bound on fp32 norm outputs (tests/test_kernels_gpu.py)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- guards (moved here from tests/test_gemm_exact_gpu.py, which imports them back) ---------------------------------------------------
def guarded(M, No, dtype, rows=3, cols=None, device="cuda:0"):
    """An output view [M, No] inside a sentinel-filled buffer with guard rows below and guard columns to the right (16-bit rows
    stay 16-byte aligned)."""
    if cols is None:
        cols = (8 - No % 8) % 8 + 8 if dtype != torch.float32 else 4
    buf = torch.full((M + rows, No + cols), SENTINEL, dtype=dtype, device=device)
    return buf, buf[:M, :No]


def assert_guards(buf, M, No, what):
    outside = torch.ones(buf.shape, dtype=torch.bool, device=buf.device)
    outside[:M, :No] = False
    assert bool((buf[outside] == SENTINEL).all()), f"{what}: a guard row or column was written"


def guarded_rows(M, D, dtype, device):
    """Rows are contiguous in the row kernels' ABI: three guard rows after row M - 1, no guard columns."""
    return guarded(M, D, dtype, rows=3, cols=0, device=device)


# ---- the three rules --------------------------------------------------------------------------------------------------------------
def assert_bits(got: torch.Tensor, want: torch.Tensor, what: str) -> None:
    """Bit for bit (NaNs: both NaN)."""
    want = want.to(got.device)
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype, got.shape, want.shape)
    if got.dtype.is_floating_point:
        eq = (bits(got) == bits(want)) | (torch.isnan(got) & torch.isnan(want))
    else:
        eq = got == want
    if bool(eq.all()):
        return
    bad = (~eq).nonzero()[:4].tolist()
    detail = ", ".join(f"{i} got {float(got[tuple(i)])!r} want {float(want[tuple(i)])!r}" for i in bad)
    raise AssertionError(f"{what}: {int((~eq).sum())} of {eq.numel()} elements differ from the exact result: {detail}")


def assert_half(got: torch.Tensor, ref64: torch.Tensor, what: str, extra=0.0, cap: Optional[float] = CAP) -> float:
    """16-bit rule: |got - ref64.to(dtype)| <= ulp(want) (+ extra) everywhere, at most ``cap`` of the elements different at all.
    Returns the share that differs."""
    want = ref64.to(got.device).to(got.dtype)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    w64 = want.double()
    err = (got.double() - w64).abs()
    tol = ulp(w64, got.dtype) + extra
    bad = ~(err <= tol)
    if bool(bad.any()):
        i = tuple(bad.nonzero()[0].tolist())
        raise AssertionError(f"{what}: element {i} is {float(got[i])!r}, want {float(want[i])!r} (float64 {float(ref64[i])!r}): more than "
                             f"one {got.dtype} ulp; {int(bad.sum())} of {bad.numel()} elements")
    share = float((got != want).sum()) / max(1, got.numel())
    if cap is not None:
        assert (got != want).sum() <= cap * got.numel(), f"{what}: {share:.2e} of the elements differ from ref64.to({got.dtype}) (cap {cap:g})"
    return share


def assert_f32(got: torch.Tensor, ref64: torch.Tensor, bound, what: str) -> float:
    ref64 = ref64.to(got.device)
    assert got.dtype == torch.float32 and got.shape == ref64.shape, (what, got.dtype, got.shape, ref64.shape)
    err = (got.double() - ref64).abs()
    bad = ~(err <= bound)
    if bool(bad.any()):
        i = tuple(bad.nonzero()[0].tolist())
        b = bound if isinstance(bound, float) else float(torch.as_tensor(bound).max())
        raise AssertionError(f"{what}: element {i} is {float(got[i])!r}, float64 {float(ref64[i])!r}: off by {float(err[i]):.3e}, bound {b:.3e}; "
                             f"{int(bad.sum())} of {bad.numel()} elements")
    return float(err.max()) if err.numel() else 0.0


def err32(t32: torch.Tensor, ref64: torch.Tensor) -> float:
    """E of the fp32 rule."""
    return float((t32.double() - ref64).abs().max()) if ref64.numel() else 0.0


def grid(shape, gen, steps: int, scale: float) -> torch.Tensor:
    """fp32 multiples of ``scale`` with |x| <= steps * scale."""
    return torch.randint(-steps, steps + 1, shape, generator=gen, dtype=torch.int32).float() * scale


# ---------------------------------------------------------------------------------------------------------------------------------
# 1. norms
# ---------------------------------------------------------------------------------------------------------------------------------
NORM_SHAPES = [("row", 1, 4), ("row", 3, 1028), ("row", 64, 8192), ("row", 2, 8188), ("row", 70, 2048), ("row", 5, 5120),
               ("norm_kernel<4>", 65, 1024), ("norm_kernel<4>", 67, 260),
               ("norm_kernel<8>", 65, 1028), ("norm_kernel<8>", 67, 2044), ("norm_kernel<8>", 4097, 2048),
               ("norm_kernel<16>", 4097, 2052), ("norm_kernel<16>", 4097, 4096),
               ("norm_kernel<20>", 4097, 4100), ("norm_kernel<20>", 4097, 5120),
               ("norm_kernel<32>", 4097, 5124), ("norm_kernel<32>", 4097, 8192)]
# (4097, 2048) is 512 float4 = 8 per lane: norm_kernel<8> past the row kernel's M <= 4096, not <16>; <16> starts at D = 2052
NORM_FORMS = ["ln16", "ln16+32", "rms", "add_ln", "add_rms", "add_only", "add2_ln", "add2_rms", "add2_only"]
NORM_F32_SHAPES = [(5, 1028), (70, 2048), (3, 1027), (67, 260), (6, 30), (9, 4100)]       # D % 4 != 0: the scalar kernels
ROWS_PER_BLOCK = 2
PERIOD = 131
LN_EPS, RMS_EPS = 1e-5, 1e-6


def norm_branch(M: int, D: int) -> str:
    """launch_norm's dispatch (norm_elementwise.hip), mirrored: tests/test_rows_exact_cpu.py pins it to the source text."""
    if M <= 64 or (D >= 2048 and M <= 4096):
        return "row"
    nv = (D // 4 + 63) // 64
    for n in (4, 8, 16, 20):
        if nv <= n:
            return f"norm_kernel<{n}>"
    return "norm_kernel<32>"


def norm_dispatch_in_source() -> Dict[str, object]:
    """The same facts read from the .hip text."""
    src = open(os.path.join(ROOT, "valley_amd", "csrc", "norm_elementwise.hip")).read()
    body = src[src.index("int launch_norm("):src.index("#undef VLY_NORM")]
    m = re.search(r"if \(M <= (\d+) \|\| \(D >= (\d+) && M <= (\d+)\)\) \{", body)
    ladder = re.findall(r"if \(nv <= (\d+)\) VLY_NORM\((\d+)\);", body)
    last = re.search(r"else VLY_NORM\((\d+)\);", body)
    return dict(row=tuple(int(x) for x in m.groups()) if m else None, ladder=[(int(a), int(b)) for a, b in ladder],
                last=int(last.group(1)) if last else None, nv="const int nv = (D / 4 + 63) / 64;" in body,
                rows_per_block=int(re.search(r"constexpr int ROWS_PER_BLOCK = (\d+);", src).group(1)),
                limits="D % 4 || D > 8192" in body)


def ln64(x, g, b, eps):
    x, g, b = x.double(), g.double(), b.double()
    mu = x.mean(-1, keepdim=True)
    c = x - mu
    return c * torch.rsqrt((c * c).mean(-1, keepdim=True) + eps) * g + b


def rms64(x, g, eps):
    x = x.double()
    return g.double() * (x * torch.rsqrt((x * x).mean(-1, keepdim=True) + eps))


def ln32(x, g, b, eps):
    mu = x.mean(-1, keepdim=True)
    c = x - mu
    return c * torch.rsqrt((c * c).mean(-1, keepdim=True) + eps) * g + b


def rms32(x, g, eps):
    return g * (x * torch.rsqrt((x * x).mean(-1, keepdim=True) + eps))


class NormCase:
    """x = 0.3 + 2 N(0, 1), gamma = 1 +- 0.1, beta = +- 0.1; planted rows: all zero, constant 7.25, mean 1000 with unit spread, only the
    last element non-zero (as many of the four as M leaves room for beside one ordinary row).  The mean-1000 row is 1000 +- {0.5, 1,
    1.5} in +- pairs, its deltas +- {0.5, 1} likewise: its sums are exact in fp32 and its mean is exactly 1000 in every form, so the
    8 E rule is as well conditioned on it as on any row (with N(0, 1) spread the mean falls between two fp32 numbers 6.1e-5 apart and E
    is how close torch's happens to land: 1e-5 to 5e-5 here, less than a correct kernel's error in one form of eight) — and a
    one-pass variance, E[x^2] at 1e6 with an fp32 spacing of 0.06 against a variance of 1.2, is off by percents.  ``idx`` [M] maps every row to its
    distinct row in ``xu`` / ``d0u`` / ``d1u``; the deltas are zero on the zero and the constant row (their sums stay what they are).
    One element of an ordinary row holds h = 1, d0 = 2^-24, d1 = 2^-23: (h + d0) + d1 = 1 + 2^-23 but (h + d1) + d0 = 1 + 2^-22."""

    def __init__(self, M: int, D: int, half, branch: Optional[str] = None):
        self.M, self.D, self.half = M, D, half
        if branch is not None:
            assert norm_branch(M, D) == branch, f"({M}, {D}) runs {norm_branch(M, D)}, not {branch}"
        g = torch.Generator(device="cpu").manual_seed(1000 * M + D)
        U = min(M, PERIOD)
        kinds = ["big", "zero", "last", "const"][:max(0, min(4, M - 1))]
        spots = []
        for p in (M - 1, 0, M // 2, 1):
            if p not in spots:
                spots.append(p)
        self.planted = dict(zip(kinds, spots))                     # kind -> row
        xu = 0.3 + 2.0 * torch.randn((U + len(kinds), D), generator=g)
        d0 = (0.5 * torch.randn((U + len(kinds), D), generator=g)).to(half)
        d1 = (0.5 * torch.randn((U + len(kinds), D), generator=g)).to(half)
        idx = torch.arange(M) % PERIOD
        self.urow = {}
        for n, k in enumerate(kinds):
            u = U + n
            idx[self.planted[k]] = u
            self.urow[k] = u
            if k == "zero":
                xu[u] = 0.0
            elif k == "const":
                xu[u] = 7.25
            elif k == "big":
                xu[u] = 1000.0 + self._paired(g, [0.5, 1.0, 1.5])
                d0[u] = self._paired(g, [0.5, 1.0]).to(half)
                d1[u] = self._paired(g, [0.5]).to(half)
            else:
                xu[u] = 0.0
                xu[u, D - 1] = 3.5
            if k in ("zero", "const"):
                d0[u] = 0.0
                d1[u] = 0.0
        plain = [r for r in range(M) if r not in self.planted.values()]
        self.order_row = int(idx[plain[-1]])
        xu[self.order_row, 0], d0[self.order_row, 0], d1[self.order_row, 0] = 1.0, 2.0 ** -24, 2.0 ** -23
        self.xu, self.d0u, self.d1u, self.idx = xu, d0, d1, idx
        self.gamma = 1.0 + 0.1 * torch.randn((D,), generator=g)
        self.beta = 0.1 * torch.randn((D,), generator=g)
        self.beta[self.beta == 0] = 0.05

    def _paired(self, g, mags) -> torch.Tensor:
        """[D] multiples of 0.5 in +- pairs at shuffled places: the sum is exactly 0, and with 1000 added every partial sum in any
        order is a multiple of 0.5 below 2^24 steps (D <= 8192), exact in fp32."""
        D = self.D
        n = D // 2                                                   # (an odd D leaves one element at 0)
        m = torch.tensor(mags)[torch.randint(0, len(mags), (n,), generator=g)]
        v = torch.zeros(D)
        perm = torch.randperm(D, generator=g)
        v[perm[:n]], v[perm[n:2 * n]] = m, -m
        assert (1000.0 + 4.0) * D * 2 < 2.0 ** 24 and float(v.double().sum()) == 0.0
        return v

    def h_after(self, form: str) -> Optional[torch.Tensor]:
        """The residual stream after an add form, on the distinct rows: fp32 adds on the CPU, in the kernel's order."""
        if not form.startswith("add"):
            return None
        h = self.xu + self.d0u.float()
        if form.startswith("add2"):
            h = h + self.d1u.float()
        return h

    def truth(self, form: str):
        """(ref64 on the distinct rows or None, E of the ordinary rows, E of the mean-1000 row)."""
        x = self.h_after(form)
        x = self.xu if x is None else x
        if form.endswith("only"):
            return None, 0.0, 0.0
        if form.endswith("rms"):
            ref, t32 = rms64(x, self.gamma, RMS_EPS), rms32(x, self.gamma, RMS_EPS)
        else:
            ref, t32 = ln64(x, self.gamma, self.beta, LN_EPS), ln32(x, self.gamma, self.beta, LN_EPS)
        big = torch.zeros(x.shape[0], dtype=torch.bool)
        if "big" in self.urow:
            big[self.urow["big"]] = True
        return ref, err32(t32[~big], ref[~big]), err32(t32[big], ref[big])


@functools.lru_cache(maxsize=4)
def norm_case(M, D, half, branch=None) -> NormCase:
    return NormCase(M, D, half, branch)


def f32_bounds(case: NormCase, e_plain: float, e_big: float, device) -> torch.Tensor:
    """Per-row bound [M, 1] of the fp32 rule."""
    b = torch.full((case.M, 1), min(F32_FACTOR * e_plain, F32_CEIL), dtype=torch.float64)
    if "big" in case.planted:
        b[case.planted["big"]] = min(F32_FACTOR * e_big, F32_CEIL)
    return b.to(device)


def check_norm(case: NormCase, form: str, h: Optional[torch.Tensor], y16: Optional[torch.Tensor], y32: Optional[torch.Tensor],
               what: str = "") -> Dict[str, float]:
    """h / y16 / y32: the full [M, D] outputs (None where the form has none).  Comparisons run on the outputs' device."""
    what = what or f"{form} {case.M}x{case.D}"
    res = {}
    hw = case.h_after(form)
    if hw is not None:
        assert h is not None
        idx = case.idx.to(h.device)
        assert_bits(h, hw.to(h.device)[idx], f"{what}: residual stream h")
    ref, e_plain, e_big = case.truth(form)
    if ref is None:
        assert y16 is None and y32 is None
        return res
    res["E"], res["E_big"] = e_plain, e_big
    assert y16 is not None
    dev = y16.device
    idx = case.idx.to(dev)
    full = ref.to(dev)[idx]
    b32 = f32_bounds(case, e_plain, e_big, dev)
    res["share"] = assert_half(y16, full, f"{what}: 16-bit output", extra=b32)
    if y32 is not None:
        res["err32"] = assert_f32(y32, full, b32, f"{what}: fp32 output")
    if "zero" in case.planted:
        r = case.planted["zero"]
        if form.endswith("rms"):
            assert bool((y16[r] == 0).all()), f"{what}: RMSNorm of the zero row is not exactly 0"
        else:
            assert_bits(y16[r], case.beta.to(y16.dtype), f"{what}: LayerNorm of the zero row is not beta rounded once")
            if y32 is not None:
                assert_bits(y32[r], case.beta, f"{what}: LayerNorm (fp32) of the zero row is not beta")
    return res


def expand(case: NormCase, t: torch.Tensor, device) -> torch.Tensor:
    return t.to(device)[case.idx.to(device)].contiguous()


# ---- the kernels' own fp32 order, in torch (the CPU module's stand-in for a kernel) -------------------------------------------------
def butterfly(v: torch.Tensor) -> torch.Tensor:
    """wave_sum: v += v[lane ^ 32], ^ 16, ... ^ 1 over the last axis (64 lanes)."""
    lane = torch.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        v = v + v[..., lane ^ o]
    return v


def emu_norm_stats(x: torch.Tensor, threads: int, rms: bool, eps: float, one_pass: bool = False):
    """x fp32 [M, D], D % 4 == 0 -> (mean [M, 1], rstd [M, 1]) summed as norm_kernel (threads = 64) / norm_row_kernel (256) sum."""
    M, D = x.shape
    nvec = D // 4
    trips = (nvec + threads - 1) // threads
    xp = torch.zeros((M, trips * threads * 4), dtype=torch.float32)
    xp[:, :D] = x
    v = xp.view(M, trips, threads, 4)
    live = (torch.arange(trips * threads).view(trips, threads) < nvec)[None, :, :, None]

    def total(parts):                                            # parts [M, trips, threads] -> [M, 1]
        s = torch.zeros((M, threads), dtype=torch.float32)
        for i in range(trips):
            s = s + parts[:, i]
        w = butterfly(s.view(M, threads // 64, 64))[..., 0]
        t = w[:, 0]
        for k in range(1, threads // 64):
            t = t + w[:, k]
        return t[:, None]

    if rms:
        sq = v * v
        s = total(((sq[..., 0] + sq[..., 1]) + sq[..., 2]) + sq[..., 3])
        return torch.zeros((M, 1)), torch.rsqrt(s / float(D) + eps)
    s = total(((v[..., 0] + v[..., 1]) + v[..., 2]) + v[..., 3])
    mean = s / float(D)
    if one_pass:                                                 # the mutation: E[x^2] - mean^2
        sq = v * v
        q = total(((sq[..., 0] + sq[..., 1]) + sq[..., 2]) + sq[..., 3]) / float(D) - mean * mean
        return mean, torch.rsqrt(q.clamp_min(0.0) + eps)
    c = torch.where(live, v - mean[:, :, None, None], torch.zeros(()))
    c = c * c
    q = total(((c[..., 0] + c[..., 1]) + c[..., 2]) + c[..., 3])
    return mean, torch.rsqrt(q / float(D) + eps)


def truncate(x: torch.Tensor, half) -> torch.Tensor:
    """fp32 -> 16-bit storage by truncation (the mutation of every rounding store)."""
    if half == torch.bfloat16:
        return (x.contiguous().view(torch.int32) & -65536).view(torch.float32).to(half)
    r = x.to(half)
    over = r.float().abs() > x.abs()
    step = torch.nextafter(r, torch.zeros((), dtype=half))
    return torch.where(over, step, r)


def emu_norm(case: NormCase, form: str, threads: int, one_pass=False, trunc=False, swap=False):
    """The kernel on the CPU -> (h, y16, y32) full [M, D] (None where the form has none); mutations: one-pass variance, truncating
    store, the two deltas added in the other order."""
    x = case.xu[case.idx].clone()
    h = None
    if form.startswith("add"):
        d0, d1 = case.d0u[case.idx].float(), case.d1u[case.idx].float()
        if form.startswith("add2"):
            x = (x + d1) + d0 if swap else (x + d0) + d1
        else:
            x = x + d0
        h = x
    if form.endswith("only"):
        return h, None, None
    rms = form.endswith("rms")
    mean, rstd = emu_norm_stats(x, threads, rms, RMS_EPS if rms else LN_EPS, one_pass)
    y = case.gamma * (x * rstd) if rms else (x - mean) * rstd * case.gamma + case.beta
    y16 = truncate(y, case.half) if trunc else y.to(case.half)
    return h, y16, (y if form == "ln16+32" else None)


# fp32 twins: vly_norm_f32 / vly_norm_split3_f32
def split3_check(out3: torch.Tensor, ref64: torch.Tensor, D: int, Kp: int, e: float, what: str) -> None:
    """[hi | hi | lo], hi = rn16(y), lo = rn16(y - hi): hi by the 16-bit rule; hi + lo within 8 E of the truth plus what the split
    itself drops (u^2 |y| with u = eps / 2, and half a subnormal step of the storage type); both hi images equal; pad columns zero."""
    half = out3.dtype
    fi = torch.finfo(half)
    hi, hi2, lo = out3[:, :D], out3[:, Kp:Kp + D], out3[:, 2 * Kp:2 * Kp + D]
    assert_bits(hi2.contiguous(), hi.contiguous(), f"{what}: the two hi images")
    assert_half(hi.contiguous(), ref64, f"{what}: hi", extra=min(F32_FACTOR * e, F32_CEIL))
    ref64 = ref64.to(out3.device)
    bound = min(F32_FACTOR * e, F32_CEIL) + (fi.eps / 2) ** 2 * ref64.abs() + fi.tiny * fi.eps / 2
    err = ((hi.double() + lo.double()) - ref64).abs()
    assert bool((err <= bound).all()), f"{what}: hi + lo is off by {float((err - bound).max()):.3e} more than the bound"
    for seg in range(3):
        assert bool((out3[:, seg * Kp + D:(seg + 1) * Kp] == 0).all()), f"{what}: pad columns of segment {seg} are not zero"


# ---------------------------------------------------------------------------------------------------------------------------------
# 2. RoPE + KV append
# ---------------------------------------------------------------------------------------------------------------------------------
ROPE_SHAPES = [(1, 1, 1, 0, 8), (2, 3, 3, 5, 8), (1, 33, 2, 0, 64), (2, 1, 2, 130, 256)]         # (B, S, heads, past, ctx_max)


def rope_inputs(B, S, heads, dtype):
    g = torch.Generator(device="cpu").manual_seed(77 + 13 * B + S + 7 * heads)
    q = torch.randn((B * S, 3 * heads * 128), generator=g)
    q[q.abs() < 2.0 ** -6] = 0.75
    return q.to(dtype)


def check_rope(shape, qkv0: torch.Tensor, qkv: torch.Tensor, kc: torch.Tensor, vc: torch.Tensor, at: int, what: str = "rope_kv") -> None:
    """qkv0: the input; qkv / kc / vc: after the call, the caches having been full of SENTINEL before; ``at``: the position the rows
    must have gone to (past, the device value, or its clamp)."""
    B, S, heads, _, ctx_max = shape
    dtype = qkv0.dtype
    cos, sin = rope_tables(ctx_max)
    x = qkv0.cpu().view(B, S, 3, heads, 128)
    pos = at + torch.arange(S)
    c, s = cos[pos][None, :, None, :], sin[pos][None, :, None, :]                 # [1, S, 1, 64]
    q64, k64 = rope64(x[:, :, 0].double(), c, s), rope64(x[:, :, 1].double(), c, s)
    got = qkv.cpu().view(B, S, 3, heads, 128)
    kc, vc = kc.cpu(), vc.cpu()
    krows = kc[:, :, at:at + S].transpose(1, 2)                                    # [B, S, heads, 128]
    vrows = vc[:, :, at:at + S].transpose(1, 2)
    if dtype == torch.float32:
        # fmaf(x, c, +-(p * s)): one rounding of p s, one of the result: <= 2^-23 (|x c| + |p s|)
        def mag(t):                                                           # [B, S, heads, 128] -> |x c| + |p s|
            lo, hi, ca, sa = t[..., :64].double().abs(), t[..., 64:].double().abs(), c.double().abs(), s.double().abs()
            return torch.cat([lo * ca + hi * sa, hi * ca + lo * sa], -1)
        assert_f32(got[:, :, 0].contiguous(), q64, 2.0 ** -23 * mag(x[:, :, 0]), f"{what}: q'")
        assert_f32(krows.contiguous(), k64, 2.0 ** -23 * mag(x[:, :, 1]), f"{what}: k' in the cache")
    else:
        assert_half(got[:, :, 0].contiguous(), q64, f"{what}: q'", cap=None)
        assert_half(krows.contiguous(), k64, f"{what}: k' in the cache", cap=None)
    if at == 0:                                                                   # position 0: cos = 1, sin = 0: the identity
        assert_bits(got[:, 0, 0].contiguous(), x[:, 0, 0].contiguous(), f"{what}: q at position 0")
        assert_bits(krows[:, 0].contiguous(), x[:, 0, 1].contiguous(), f"{what}: k at position 0")
    assert_bits(vrows.contiguous(), x[:, :, 2].contiguous(), f"{what}: v in the cache")
    assert_bits(got[:, :, 1:].contiguous(), x[:, :, 1:].contiguous(), f"{what}: the k | v slots of qkv")
    other = torch.ones(ctx_max, dtype=torch.bool)
    other[at:at + S] = False
    for name, cache in (("K", kc), ("V", vc)):
        rows = (cache[:, :, other] != SENTINEL).flatten(0, 1).any(-1).any(0).nonzero().flatten().tolist()
        assert not rows, f"{what}: {name} cache rows {[int(other.nonzero().flatten()[r]) for r in rows]} outside [{at}, {at + S}) were written"


def emu_rope(shape, qkv0: torch.Tensor, at: int, off_rows: int = 0):
    """rope_kv_kernel in torch: fp32 fmaf(x, c, -+(p s)) (fp64 product and sum rounded once stand in for the fma)."""
    B, S, heads, _, ctx_max = shape
    dtype = qkv0.dtype
    cos, sin = rope_tables(ctx_max)
    x = qkv0.view(B, S, 3, heads, 128)
    pos = at + torch.arange(S)
    c, s = cos[pos][None, :, None, :].double(), sin[pos][None, :, None, :].double()

    def rot(t):
        lo, hi = t[..., :64].double(), t[..., 64:].double()
        plo, phi = (hi * s).float().double(), (lo * s).float().double()
        return torch.cat([(lo * c - plo).float(), (hi * c + phi).float()], -1).to(dtype)

    out = x.clone()
    out[:, :, 0] = rot(x[:, :, 0])
    kc = torch.full((B, heads, ctx_max, 128), SENTINEL, dtype=dtype)
    vc = torch.full_like(kc, SENTINEL)
    kc[:, :, at + off_rows:at + off_rows + S] = rot(x[:, :, 1]).transpose(1, 2)
    vc[:, :, at + off_rows:at + off_rows + S] = x[:, :, 2].transpose(1, 2)
    return out.view(B * S, -1), kc, vc


# ---------------------------------------------------------------------------------------------------------------------------------
# 3. pooling and scores
# ---------------------------------------------------------------------------------------------------------------------------------
POOL_SHAPES = [(1, 1, 4), (1, 3, 12), (2, 8, 1024), (3, 2, 260)]                 # (B, T, W)
POOL_MEAN, POOL_MAX, POOL_IMPORTANCE = 0, 1, 2
GRID_STEPS, GRID = 512, 2.0 ** -6                                                # |x| <= 8 in steps of 2^-6
EXACT_STEPS = 2.0 ** 24


@functools.lru_cache(maxsize=8)
def pool_feats(B, T, W) -> torch.Tensor:
    """fp32 [B, T, 257, W] on the grid; the exactness condition of the mean (any order) is asserted."""
    g = torch.Generator(device="cpu").manual_seed(300 + 5 * B + 3 * T + W)
    f = grid((B, T, 257, W), g, GRID_STEPS, GRID)
    assert float(f.abs().sum(1).max()) / GRID < EXACT_STEPS
    return f


def pool_scores(B, T) -> torch.Tensor:
    """Spread +-40: row b holds +40 and (T > 1) -40 — a weight of e^-80, nothing beside 1 in fp32 — at rotating frames."""
    s = torch.linspace(-13.0, 17.0, B * T).view(B, T).clone()
    for b in range(B):
        s[b, b % T] = 40.0
        if T > 1:
            s[b, (b + 1) % T] = -40.0
    return s


def pool_truth(feats: torch.Tensor, mode: int, scores: Optional[torch.Tensor] = None, cls_shift: int = 0, mean_div: int = 0):
    """float64 [B, 256 + T, W].  cls_shift / mean_div: the mutations (CLS of frame t + shift; mean over T - 1)."""
    B, T = feats.shape[:2]
    p = feats[:, :, 1:].double()
    if mode == POOL_MAX:
        pooled = p.amax(1)
    elif mode == POOL_MEAN:
        pooled = p.sum(1) / (mean_div or T)
    else:
        pooled = (torch.softmax(scores.double(), 1)[:, :, None, None] * p).sum(1)
    cls = feats[:, (torch.arange(T) + cls_shift) % T, 0].double()
    return torch.cat([pooled, cls], 1)


def pool_e(feats: torch.Tensor, mode: int, scores: Optional[torch.Tensor]) -> float:
    p = feats[:, :, 1:]
    if mode == POOL_IMPORTANCE:
        t32 = (torch.softmax(scores, 1)[:, :, None, None] * p).sum(1)
    else:
        t32 = p.sum(1) / float(feats.shape[1])
    return err32(t32, pool_truth(feats, mode, scores)[:, :256])


def check_pool(feats: torch.Tensor, mode: int, scores: Optional[torch.Tensor], out: torch.Tensor, what: str = "pool_tokens") -> None:
    """out [B, 256 + T, W], 16-bit or fp32 (the twin)."""
    B, T = feats.shape[:2]
    truth = pool_truth(feats, mode, scores)
    out = out.cpu()
    f32 = out.dtype == torch.float32
    want = truth.float() if f32 else truth.to(out.dtype)
    assert_bits(out[:, 256:].contiguous(), want[:, 256:].contiguous(), f"{what}: CLS rows")
    got, tr = out[:, :256].contiguous(), truth[:, :256].contiguous()
    if mode == POOL_MAX or (mode == POOL_MEAN and T & (T - 1) == 0):
        assert_bits(got, want[:, :256].contiguous(), f"{what}: mode {mode} at T = {T} is exact")
    elif mode == POOL_MEAN:
        # an exact sum, then one division or a multiplication by fl(1 / T): at most two roundings
        if f32:
            assert_f32(got, tr, ulp(tr, torch.float32), f"{what}: mean at T = {T}")
        else:
            assert_half(got, tr, f"{what}: mean at T = {T}")
    else:
        e = pool_e(feats, mode, scores)
        if f32:
            assert_f32(got, tr, F32_FACTOR * e + ulp(tr, torch.float32), f"{what}: importance")
        else:
            assert_half(got, tr, f"{what}: importance", extra=F32_FACTOR * e, cap=None)


def emu_pool(feats: torch.Tensor, mode: int, scores: Optional[torch.Tensor], half, cls_shift=0, mean_div=0, trunc=False) -> torch.Tensor:
    """pool_kernel in torch: frames added in order, one multiplication by fl(1 / T), one rounding."""
    B, T = feats.shape[:2]
    p = feats[:, :, 1:]
    if mode == POOL_IMPORTANCE:
        wt = torch.exp(scores - scores.amax(1, keepdim=True))
        wt = wt / wt.sum(1, keepdim=True)
        o = torch.zeros_like(p[:, 0])
        for t in range(T):
            o = o + wt[:, t, None, None] * p[:, t]
    else:
        o = p[:, 0].clone()
        for t in range(1, T):
            o = torch.maximum(o, p[:, t]) if mode == POOL_MAX else o + p[:, t]
        if mode == POOL_MEAN:
            o = o * (torch.ones(()) / float(mean_div or T))
    o = torch.cat([o, feats[:, (torch.arange(T) + cls_shift) % T, 0]], 1)
    if half == torch.float32:
        return o
    return truncate(o, half) if trunc else o.to(half)


SCORE_SHAPES = [(F, W) for F in (1, 3) for W in (4, 68, 1024)]
SCORE_STEP = 2.0 ** -2


@functools.lru_cache(maxsize=8)
def score_case(F, W, with_bias: bool):
    """feats multiples of 2^-2 with |x| <= 2, weights with |w| <= 1, bias on the products' 2^-4 grid: every partial sum of products is
    a multiple of 2^-4 below 2^24 steps (asserted), so the score is exact in fp32 in any order, fused or not."""
    g = torch.Generator(device="cpu").manual_seed(500 + 3 * F + W)
    feats = grid((F, 257, W), g, 8, SCORE_STEP)
    w = grid((256 * W,), g, 4, SCORE_STEP)
    bias = grid((1,), g, 64, SCORE_STEP ** 2) if with_bias else None
    bound = (feats[:, 1:].reshape(F, -1).double().abs() @ w.double().abs()).max() + (float(bias.abs()) if with_bias else 0.0)
    assert float(bound) / SCORE_STEP ** 2 < EXACT_STEPS, float(bound)
    truth = feats[:, 1:].reshape(F, -1).double() @ w.double() + (bias.double() if with_bias else 0.0)
    return feats, w, bias, truth


# ---------------------------------------------------------------------------------------------------------------------------------
# 4. splice, cast, patchify, ViT embedding, counter
# ---------------------------------------------------------------------------------------------------------------------------------
SPLICE_H = [8, 520, 5120]
SPLICE_R = [1, 4, 5, 9]
SPLICE_V, SPLICE_NV = 11, 6


def splice_map(R: int, tokens_only: bool = False) -> torch.Tensor:
    """First and last row of both tables, one row of each twice (as far as R rows reach)."""
    V, NV = SPLICE_V, SPLICE_NV
    full = [-NV, V - 1, 0, -1, V - 1, -NV, 3, -2, 0]
    if tokens_only:
        full = [V - 1, 0, V - 1, 3, 0, 5, 1, V - 2, 2]
    return torch.tensor(full[:R], dtype=torch.int32)


def splice_tables(H: int, dtype):
    g = torch.Generator(device="cpu").manual_seed(600 + H)
    return torch.randn((SPLICE_V, H), generator=g).to(dtype), torch.randn((SPLICE_NV, H), generator=g).to(dtype)


def splice_truth(rmap: torch.Tensor, embed: torch.Tensor, visual: Optional[torch.Tensor]) -> torch.Tensor:
    return torch.stack([embed[v].float() if v >= 0 else visual[-v - 1].float() for v in rmap.tolist()])


def emu_splice(rmap, embed, visual, drop_last_chunk=False, stray=False) -> torch.Tensor:
    """embed_splice_kernel in torch, inside its guard buffer [R + 3, H]; mutations: the last 8-column chunk not written, the first
    guard row written."""
    R, H = rmap.numel(), embed.shape[1]
    buf = torch.full((R + 3, H), SENTINEL, dtype=torch.float32)
    n = H - 8 if drop_last_chunk else H
    buf[:R, :n] = splice_truth(rmap, embed, visual)[:, :n]
    if stray:
        buf[R, :8] = 0.0
    return buf


def cast_values(n: int, half) -> torch.Tensor:
    """fp32 [n]: the storage type's rounding ties both ways, its largest finite value, the first value that rounds to infinity and the
    last that does not, +-0, +-inf, NaN, fp16's subnormal range and its tie at 2^-25; the rest random over many binades.  The specials
    stand at the front and again in the last chunk of eight."""
    if half == torch.bfloat16:
        u = 2.0 ** -8                                                            # half an ulp at 1
        big = float(torch.finfo(half).max)
        tie, below = (float(torch.tensor([b], dtype=torch.int32).view(torch.float32)) for b in (0x7F7F8000, 0x7F7F7FFF))
        sp = [1 + u, 1 + 3 * u, -(1 + u), -(1 + 3 * u), 1 + u + 2.0 ** -20, 1 + u - 2.0 ** -20, big, -big,
              tie, below, 0.0, -0.0, math.inf, -math.inf, math.nan, 2.0 ** -126]
    else:
        u = 2.0 ** -11
        sp = [1 + u, 1 + 3 * u, -(1 + u), -(1 + 3 * u), 1 + u + 2.0 ** -20, 1 + u - 2.0 ** -20, 65504.0, -65504.0, 65520.0,
              65520.0 * (1 - 2.0 ** -24), 0.0, -0.0, math.inf, -math.inf, math.nan, 2.0 ** -14,
              2.0 ** -24, 2.0 ** -25, -(2.0 ** -25), 2.0 ** -25 * (1 + 2.0 ** -10), 3 * 2.0 ** -25, 2.0 ** -26, 1023 * 2.0 ** -24,
              2.0 ** -14 - 2.0 ** -25, 5.5 * 2.0 ** -24, 1e-6]
    sp = torch.tensor(sp, dtype=torch.float32)
    if n <= 8:
        return sp[[0, 1, 2, 8, 9, 11, 13, 14]].clone()
    g = torch.Generator(device="cpu").manual_seed(700 + n)
    x = torch.randn((n,), generator=g) * torch.exp2(torch.randint(-20, 16, (n,), generator=g).float())
    x[:sp.numel()] = sp
    x[n - 8:] = sp[[1, 3, 8, 9, 11, 14, 6, 0]]
    return x


def patch_image(F: int, dtype) -> torch.Tensor:
    """[F, 3, 224, 224]: pixel (f, c, y, x) holds its own flat index — as the integer itself in fp32, as the 16-bit pattern of the
    index mod 65536 in a 16-bit type (compared as bits; 65536 pixels are 292 image rows and 128 pixels apart)."""
    idx = torch.arange(F * 3 * 224 * 224, dtype=torch.int64).view(F, 3, 224, 224)
    if dtype == torch.float32:
        return idx.float()
    v = idx & 0xFFFF
    return (v - ((v & 0x8000) << 1)).to(torch.int16).view(dtype)


def patch_truth_index(F: int, kp: int) -> torch.Tensor:
    """int64 [F * 256, kp]: the flat pixel index column k of row (f, py, px) must hold; -1 on the pad columns."""
    row = torch.arange(F * 256)[:, None]
    k = torch.arange(kp)[None, :]
    f, p = row // 256, row % 256
    py, px = p // 16, p % 16
    c, r = k // 196, k % 196
    ky, kx = r // 14, r % 14
    idx = ((f * 3 + c) * 224 + py * 14 + ky) * 224 + px * 14 + kx
    return torch.where(k < 588, idx, torch.full_like(idx, -1))


def check_patchify(out: torch.Tensor, F: int, what: str = "patchify") -> None:
    out = out.cpu().contiguous()
    kp = out.shape[1]
    want = patch_truth_index(F, kp)
    if out.dtype == torch.float32:
        got = out.long()
        assert bool((out == got.float()).all())
    else:
        got = out.view(torch.int16).long() & 0xFFFF
        want = torch.where(want >= 0, want & 0xFFFF, want)
    pad = want < 0
    assert bool((out[pad] == 0).all()) and bool((bits(out)[pad] == 0).all()), f"{what}: pad columns 588..{kp - 1} are not zero"
    bad = (got != want) & ~pad
    if bool(bad.any()):
        r, k = bad.nonzero()[0].tolist()
        raise AssertionError(f"{what}: row {r} (frame {r // 256}, patch {r % 256}) column {k} holds pixel {int(got[r, k])}, want {int(want[r, k])} "
                             f"(mod 65536 for a 16-bit image); {int(bad.sum())} elements")


def vit_embed_case(F: int):
    g = torch.Generator(device="cpu").manual_seed(800 + F)
    po = torch.randn((F * 256, 1024), generator=g)
    cls, pos = torch.randn((1024,), generator=g), 0.1 * torch.randn((257, 1024), generator=g)
    gm, bt = 1.0 + 0.1 * torch.randn((1024,), generator=g), 0.1 * torch.randn((1024,), generator=g)
    return po, cls, pos, gm, bt


def check_vit_embed(F: int, h: torch.Tensor, shift_cls: int = 0, what: str = "vit_embed_ln") -> None:
    po, cls, pos, gm, bt = vit_embed_case(F)
    emb = torch.cat([cls.expand(F, 1, 1024), po.view(F, 256, 1024)], 1)
    ref = ln64(emb.double() + pos.double()[None], gm, bt, LN_EPS).view(F * 257, 1024)
    e = err32(ln32(emb + pos[None], gm, bt, LN_EPS).view(F * 257, 1024), ref)
    bound = min(F32_FACTOR * e, F32_CEIL)
    h = h.cpu()
    for f in range(F):
        assert_f32(h[f * 257], ref[f * 257], bound, f"{what}: the CLS row of frame {f}")
    assert_f32(h[F * 257 - 1], ref[F * 257 - 1], bound, f"{what}: the last patch row")
    assert_f32(h, ref, bound, what)


INCR = [(n, d) for n in (1, 64, 65) for d in (1, -3)]

# ---------------------------------------------------------------------------------------------------------------------------------
# 5. temporal-transformer glue
# ---------------------------------------------------------------------------------------------------------------------------------
DELTA_SHAPES = [(1, 1, 4), (2, 3, 12), (1, 8, 1024)]                             # (B, T, H)


@functools.lru_cache(maxsize=4)
def delta_case(B, T, H):
    """feats [B, T, 257, H] on the grid, every value a code of (b, t, token, column): a transposed or shifted index shows."""
    b = torch.arange(B)[:, None, None, None]
    t = torch.arange(T)[None, :, None, None]
    p = torch.arange(257)[None, None, :, None]
    c = torch.arange(H)[None, None, None, :]
    feats = (((37 * p + 101 * t + 211 * b + 7 * c + (p * c) % 13) % 1024) - 512).float() * GRID
    assert float(feats.abs().sum(1).max()) / GRID < EXACT_STEPS
    g = torch.Generator(device="cpu").manual_seed(900 + B + T + H)
    pos = torch.randn((T, H), generator=g)
    delta = torch.randn((B * 256, H), generator=g)
    mean_in = torch.randn((B * 256, H), generator=g)
    return feats, pos, delta, mean_in


def delta_prep_truth(feats, pos, wrong_t: bool = False, mean_div: int = 0):
    """(x fp32 [B*256*T, H] = one fp32 add, x_last [B*256, H], mean float64 [B*256, H]).  wrong_t: x_all indexed (b, t, p) — the mutation."""
    B, T, _, H = feats.shape
    x = feats[:, :, 1:] + pos[None, :, None, :]                                   # [B, T, 256, H]
    xt = x if wrong_t else x.transpose(1, 2)                                      # -> [B, 256, T, H]
    mean = feats[:, :, 1:].double().sum(1) / (mean_div or T)
    return xt.reshape(B * 256 * T, H).contiguous(), x[:, T - 1].reshape(B * 256, H).contiguous(), mean.reshape(B * 256, H)


def check_delta_prep(feats, pos, x_all, x_last16, x_last32, mean, what: str = "delta_prep") -> None:
    """x_all / x_last16 in the storage type (or fp32: the _f32 form, x_last16 None)."""
    B, T, _, H = feats.shape
    xw, lw, mw = delta_prep_truth(feats, pos)
    st = x_all.dtype
    assert_bits(x_all.cpu(), xw.to(st), f"{what}: x_all[(b 256 + p) T + t]")
    if x_last16 is not None:
        assert_bits(x_last16.cpu(), lw.to(st), f"{what}: x_last (16-bit)")
    assert_bits(x_last32.cpu(), lw, f"{what}: x_last (fp32)")
    mean = mean.cpu()
    if T & (T - 1) == 0:
        assert_bits(mean, mw.float(), f"{what}: mean at T = {T} is exact")
    else:
        e = err32(feats[:, :, 1:].sum(1).reshape(B * 256, H) / float(T), mw)
        assert_f32(mean, mw, F32_FACTOR * e, f"{what}: mean at T = {T}")


def delta_finish_truth(feats, delta, mean_in, cls_shift: int = 0, clip_shift: int = 0) -> torch.Tensor:
    """fp32 [B, 256 + T, H]: rows < 256 one fp32 add; rows >= 256 the CLS row of frame r - 256 of clip b."""
    B, T, _, H = feats.shape
    top = (delta + mean_in).view(B, 256, H)
    cls = feats[(torch.arange(B) + clip_shift) % B][:, (torch.arange(T) + cls_shift) % T, 0]
    return torch.cat([top, cls], 1)


def check_delta_finish(feats, delta, mean_in, out, what: str = "delta_finish") -> None:
    want = delta_finish_truth(feats, delta, mean_in).to(out.dtype)
    out = out.cpu()
    assert_bits(out[:, :256].contiguous(), want[:, :256].contiguous(), f"{what}: rows below 256 = (delta + mean) rounded once")
    assert_bits(out[:, 256:].contiguous(), want[:, 256:].contiguous(), f"{what}: rows from 256 = the CLS row of frame r - 256 of the clip")
