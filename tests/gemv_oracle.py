"""The decode GEMV oracle: cases, a mirror of the dispatch of valley_amd/csrc/gemv_bf16.hip, the exact norm / merge inputs and the
checks that tests/test_gemv_exact_gpu.py, tests/gemv_worker.py and tests/test_decode_merge_gpu.py run.  Importing it needs no GPU;
tests/test_gemv_exact_cpu.py checks the oracle itself.

Exactness (the GEMM oracle's argument, tests/test_gemm_exact_gpu.py): activations are integers |a| <= 16, weights multiples of
2^-3 with |w| <= 4, bias and residual fp32 values on the 2^-3 grid.  Every partial sum, in any order and any split — lanes, waves,
the LDS sum over four waves, MFMA chains — is a multiple of 2^-3 below 2^21 (16 * 4 * K + 64 < 2^21 up to K = 13824; ``Case``
asserts it), so an fp32 output IS the float64 truth and a 16-bit output is ``truth.to(HALF)``.

vly_gemv_rmsnorm_bf16 is held to the truth through an exact prologue (``NormCase``): a row of H holds the magnitudes {1, 2, 4}
with counts (4m, K - 5m, m), m = K // 16, so its sum of squares is the integer 4 K in any order, the mean square is 4 and
rstd = 0.5 (1 - d), d ~ eps / 8; with integer gamma the normalised value rounds to gamma h / 2 in bf16 and in fp16 (multiples of
0.5, |x| <= 16), and the GEMV over it is exact on the 2^-4 grid (16 * 4 * 6144 * 16 < 2^24).

Every case names the kernel it is meant for; the checks assert through ``gemv_branch`` / ``norm_plan`` — from the pointers and
strides actually passed — that the call reaches it, so a case cannot drift onto another kernel unnoticed."""
import functools
import os
import re
from typing import List, NamedTuple, Optional

import numpy as np
import torch

from tests.row_oracle import ROOT, SENTINEL, assert_guards, guarded as _guarded
from tests.test_gemm_exact_gpu import EDGES, EXACT_LIMIT, Case, _terms, assert_activation, assert_exact, strided  # noqa: F401
from valley_amd.runtime import HALF

D = "cuda:0"
EPI_NONE, EPI_QUICK_GELU, EPI_SWIGLU, EPI_RELU = 0, 1, 2, 3
CU_COUNTS = (256, 64, 32)                  # the device partitions the dispatch rule is checked at on the CPU
NORM_LIMIT = 2.0 ** 20                     # 2^24 * 2^-4: the norm cases' products are multiples of 2^-4


# ---------------------------------------------------------------------------------------------------------------------------------
# 1. the dispatch of vly_gemv_bf16, mirrored
# ---------------------------------------------------------------------------------------------------------------------------------
def _balance(wgs: int, slots: int) -> np.float32:
    return np.float32(wgs) / np.float32(((wgs + slots - 1) // slots) * slots)


def four_rows(N: int, K: int, cus: int, pin: int = 0) -> bool:
    """launch_mr's rule for MR <= 2 (VLY_GEMV_ROWS pins it)."""
    if K < 2048 or N < 8:
        return False
    if pin:
        return pin == 4
    return K >= 8192 and bool(_balance((N + 3) // 4, cus * 5) > np.float32(_balance((N + 1) // 2, cus * 8) + np.float32(0.02)))


def mfma_blockers(M, N, K, epi=EPI_NONE, out32=True, ldc=None, c_ptr=0, bias_ptr=None, res_ptr=None, ldr=0) -> List[str]:
    """Why vly_gemv_bf16's ``mfma_ok`` is false (empty: it is true), in the order of the source's conjunction."""
    No = N // 2 if epi == EPI_SWIGLU else N
    ldc = No if ldc is None else ldc
    why = []
    if K % 64:
        why.append("K % 64")
    if N % 4:
        why.append("N % 4")
    if ldc % 4:
        why.append("ldc % 4")
    if c_ptr & (15 if out32 else (3 if epi == EPI_SWIGLU else 7)):
        why.append("C alignment")
    if epi == EPI_SWIGLU and not out32 and ldc % 2:
        why.append("ldc % 2")
    if bias_ptr is not None and bias_ptr & 15:
        why.append("bias alignment")
    if res_ptr is not None and (ldr % 4 or res_ptr & 15):
        why.append("residual alignment")
    return why


def gemv_branch(M, N, K, cus, epi=EPI_NONE, out32=True, residual=False, blockers=(), rows_pin=0, mfma_env: Optional[int] = None) -> str:
    """The kernel vly_gemv_bf16 launches ("refused": -22).  ``blockers``: mfma_blockers() of the call; rows_pin / mfma_env: the
    VLY_GEMV_ROWS / VLY_GEMV_MFMA switches of the process (None: unset)."""
    if M <= 0 or M > 16 or N <= 0 or K <= 0 or K % 8 or (epi == EPI_SWIGLU and (N % 2 or residual)):
        return "refused"
    if not ((epi == EPI_NONE) or (epi in (EPI_QUICK_GELU, EPI_SWIGLU) and not out32)):
        return "refused"
    no_mfma = mfma_env == 0
    if M >= 3 and not blockers and not (no_mfma and M <= 8):
        if mfma_env == 1:
            return "gemv_mfma"
        if M <= 8 and K % 128 == 0 and (N + 15) // 16 < 3 * 256:
            return "gemv_mfma2<HALF8>"
        return "gemv_mfma2<BIGM>" if M > 8 else "gemv_mfma2<16>"
    if M > 8:
        return "refused"
    MR = 1 if M == 1 else 2 if M == 2 else 4 if M <= 4 else 8
    KS = 4 if K >= 2048 else 1
    NR = 4 if MR <= 2 and four_rows(N, K, cus, rows_pin) else 2
    return f"gemv_kernel<MR={MR},KS={KS},NR={NR}>"


def dispatch_in_source() -> dict:
    """The facts the mirror rests on, read from the .hip text (tests/test_gemv_exact_cpu.py pins them)."""
    src = open(os.path.join(ROOT, "valley_amd", "csrc", "gemv_bf16.hip")).read()
    return dict(
        split="const bool split = K >= 2048;" in src,
        four="four = pin ? pin == 4 : K >= 8192 && balance((N + 3) / 4, cus * 5) > balance((N + 1) / 2, cus * 8) + 0.02f;" in src,
        four_guard="if (split && MR <= 2 && N >= 8) {" in src,
        half8="const bool half8 = M <= 8 && K % 128 == 0 && (half_pin >= 0 ? half_pin != 0 : (N + 15) / 16 < 3 * 256);" in src,
        mfma_ok=bool(re.search(r"const bool mfma_ok = K % 64 == 0 && N % 4 == 0 && ldc % 4 == 0 &&", src)),
        c_align="((uintptr_t)C & (out_dtype == VLY_OUT_F32 ? 15 : (epilogue == VLY_EPI_SWIGLU ? 3 : 7))) == 0" in src,
        rows="if (M >= min_rows && M >= 3 && mfma_ok && !(no_mfma && M <= 8))" in src,
        ladder=all(s in src for s in ("if (M == 1) return launch_mr<1>", "if (M == 2) return launch_mr<2>",
                                      "if (M <= 4) return launch_mr<4>", "return launch_mr<8>")),
        norm_ch="if (K <= 4096) VLY_GEMVN_CH(E, O, 2);" in src and "else VLY_GEMVN_CH(E, O, 3);" in src,
        norm_grid="dim3 grid(groups < cu_count() ? groups : cu_count()), block(1024);" in src,
        norm_limits="M > 2 || N <= 0 || K < 2048 || K > 6144 || K % 8 || ldh % 4" in src,
        norm_loop="for (int n0 = first, nb = (int)blockIdx.x * 2; nb < N; n0 += 2 * stride, nb += 2 * stride) {" in src
                  and "if (nb + stride >= N) break;" in src,
    )


class NormPlan(NamedTuple):
    kernel: str        # gemv_norm_kernel<MR, CH, PRO>
    grid: int
    reduces: tuple     # per workgroup: how many reduce_pair calls it makes (they alternate red[0], red[1], red[0] ...)
    exits: frozenset   # how the workgroups leave the loop: "break" (after a red[0] trip) / "end" (the loop condition, after red[1])


def norm_plan(M: int, N: int, K: int, cus: int, pro: int = 0) -> NormPlan:
    """launch_norm_mr and the trip loop of gemv_norm_kernel, mirrored ("refused" as the kernel for shapes the entry points turn down)."""
    if M <= 0 or M > 2 or N <= 0 or K < 2048 or K > 6144 or K % 8:
        return NormPlan("refused", 0, (), frozenset())
    pairs = (N + 1) // 2
    groups = (pairs + 3) // 4
    grid = min(groups, cus)
    stride = grid * 4 * 2
    reduces, exits = [], set()
    for blk in range(grid):
        nb, n = blk * 2, 0
        how = "end"
        while nb < N:
            n += 1
            if nb + stride >= N:
                how = "break"
                break
            n += 1
            nb += 2 * stride
        reduces.append(n)
        exits.add(how)
    return NormPlan(f"gemv_norm_kernel<MR={M},CH={2 if K <= 4096 else 3},PRO={pro}>", grid, tuple(reduces), frozenset(exits))


# ---------------------------------------------------------------------------------------------------------------------------------
# 2. the case lists: (M values, N, K, the kernel each M must reach)
# ---------------------------------------------------------------------------------------------------------------------------------
class Shape(NamedTuple):
    N: int
    K: int
    Ms: tuple
    why: str


def split_shapes() -> List[Shape]:
    """gemv_kernel<MR, *, *, 4, 2>: four waves split K, summed through LDS."""
    return [Shape(6, 2048, (1, 2), "three workgroups, K exactly one chunk round"),
            Shape(1001, 2056, (1, 2), "odd N; ragged last chunk: wave 3 gets one lane of work"),
            Shape(64, 4096, (1, 2), "two chunk rounds"),
            Shape(258, 11008, (1, 2), "the 13B down projection's K"),
            Shape(10, 13824, (1, 2), "the largest K; N >= 8 but the balance rule keeps two rows")]


def four_row_shapes(cus: int) -> List[Shape]:
    """gemv_kernel<MR, *, *, 4, 4> by the natural rule: the three ragged remainders of a four-row block and the full one."""
    return [Shape(16 * cus + 1, 8192, (1, 2), "one live row in the last block"), Shape(16 * cus + 2, 8192, (1, 2), "one live pair"),
            Shape(16 * cus + 3, 8192, (1, 2), "a pair and a half"), Shape(20 * cus, 8192, (1, 2), "full blocks, the rule's upper edge")]


def epilogue_shapes(cus: int) -> List[Shape]:
    return [Shape(1032, 2048, (1, 2), "K split"), Shape(16 * cus + 2, 8192, (1, 2), "four rows, ragged last block")]


FALLBACK_MS = (3, 4, 5, 7, 8)
# (N, K, how the output is laid out, the reason mfma_ok must be false for)
FALLBACK = [(1001, 1024, "plain", "N % 4"), (1002, 2056, "plain", "K % 64"), (1000, 1024, "ldc", "ldc % 4"), (1000, 1024, "offset", "C alignment")]
FALLBACK_EPILOGUE = (1002, 1032)

MFMA = [Shape(12292, 128, (3, 8), "the sixteen-row form for M <= 8: (N + 15) / 16 >= 768"),
        Shape(20, 128, (9, 12, 16), "BIGM, two blocks, the second with four live rows"),
        Shape(1000, 192, (9, 11, 16), "BIGM, K % 128 != 0"),
        Shape(1000, 192, (3, 8), "the sixteen-row form by K % 128 != 0")]
MFMA_EPILOGUE = [(1000, 1024, 3, "gemv_mfma2<HALF8>"), (1004, 1024, 8, "gemv_mfma2<HALF8>"), (1000, 192, 3, "gemv_mfma2<16>"),
                 (1004, 192, 8, "gemv_mfma2<16>"), (1000, 1024, 11, "gemv_mfma2<BIGM>"), (1004, 192, 11, "gemv_mfma2<BIGM>")]

WORKER_A_ENV = {"VLY_GEMV_ROWS": "4", "VLY_GEMV_MFMA": "0"}
WORKER_A_FOUR = [Shape(9, 2048, (1, 2), "three blocks, one live row in the last"), Shape(10, 2056, (1, 2), "ragged chunk"),
                 Shape(1001, 4096, (1, 2), "odd N")]
WORKER_A_VALU = [Shape(1000, 1024, (3, 5, 8), "aligned: only the switch keeps the VALU kernel"), Shape(4100, 320, (3, 5, 8), ""),
                 Shape(1000, 2048, (3, 5, 8), "the K split at MR = 4 / 8")]
WORKER_B_ENV = {"VLY_GEMV_MFMA": "1"}
WORKER_B = [Shape(1000, 1024, (3, 8, 11, 16), ""), Shape(4100, 320, (3, 8, 11, 16), "five K pairs: one group and three singles"),
            Shape(20, 64, (3, 8, 11, 16), "one K pair: wave 0 alone"), Shape(1004, 2048, (3, 8, 11, 16), "two groups per wave")]
WORKER_B_EPILOGUE = [(1000, 1024), (1004, 2048)]

NORM_K = (2048, 2056, 4096, 4104, 6136, 6144)


def norm_shapes(cus: int) -> List[Shape]:
    out = [Shape(6, K, (1, 2), "CH boundary / ragged chunk") for K in NORM_K]
    out += [Shape(8 * cus - 2, 2048, (1, 2), "one trip, ragged last group"), Shape(8 * cus + 2, 2048, (1, 2), "a second trip for block 0 only"),
            Shape(16 * cus + 6, 2048, (1, 2), "three trips"), Shape(24 * cus + 3, 2048, (1, 2), "four trips, odd N"),
            Shape(1001, 5120, (1, 2), "the 13B hidden size, odd N")]
    return out


MERGE_HEADS = (16, 40, 48)

# every row of the issue's table -> the kernels that stand for it
TABLE_ROWS = {
    "K < 2048, MR = 1, 2": ["gemv_kernel<MR=1,KS=1,NR=2>", "gemv_kernel<MR=2,KS=1,NR=2>"],
    "K split": ["gemv_kernel<MR=1,KS=4,NR=2>", "gemv_kernel<MR=2,KS=4,NR=2>"],
    "four rows per workgroup": ["gemv_kernel<MR=1,KS=4,NR=4>", "gemv_kernel<MR=2,KS=4,NR=4>"],
    "VALU fallback": ["gemv_kernel<MR=4,KS=1,NR=2>", "gemv_kernel<MR=8,KS=1,NR=2>", "gemv_kernel<MR=4,KS=4,NR=2>", "gemv_kernel<MR=8,KS=4,NR=2>"],
    "matrix cores, LDS ring": ["gemv_mfma2<HALF8>", "gemv_mfma2<BIGM>", "gemv_mfma2<16>"],
    "matrix cores, A/B form": ["gemv_mfma"],
    "norm prologue": ["gemv_norm_kernel<MR=1,CH=2,PRO=0>", "gemv_norm_kernel<MR=2,CH=2,PRO=0>", "gemv_norm_kernel<MR=1,CH=3,PRO=0>",
                      "gemv_norm_kernel<MR=2,CH=3,PRO=0>"],
    "merge prologue": ["gemv_norm_kernel<MR=1,CH=2,PRO=1>", "gemv_norm_kernel<MR=2,CH=2,PRO=1>", "gemv_norm_kernel<MR=1,CH=3,PRO=1>",
                       "gemv_norm_kernel<MR=2,CH=3,PRO=1>"],
    "refusals": ["refused"],
}


def listed_branches(cus: int) -> set:
    """Every kernel the listed cases select at a device of ``cus`` compute units (layouts as the checks build them)."""
    got = set()
    for s in [Shape(1000, 1024, (1, 2, 3, 5, 8, 11, 16), ""), Shape(4100, 320, (1, 2, 3, 5, 8, 11, 16), "")] + split_shapes() + \
            four_row_shapes(cus) + epilogue_shapes(cus) + MFMA:
        got |= {gemv_branch(M, s.N, s.K, cus) for M in s.Ms}
    for N, K, layout, why in FALLBACK:
        for M in FALLBACK_MS:
            blk = mfma_blockers(M, N, K, ldc=N + 5 if layout == "ldc" else None, c_ptr=2 if layout == "offset" else 0,
                                out32=layout != "offset")
            got.add(gemv_branch(M, N, K, cus, out32=layout != "offset", blockers=blk))
    for s in WORKER_A_FOUR + WORKER_A_VALU:
        got |= {gemv_branch(M, s.N, s.K, cus, rows_pin=4, mfma_env=0) for M in s.Ms}
    for s in WORKER_B:
        got |= {gemv_branch(M, s.N, s.K, cus, mfma_env=1) for M in s.Ms}
    for s in norm_shapes(cus):
        got |= {norm_plan(M, s.N, s.K, cus).kernel for M in s.Ms}
    for heads in MERGE_HEADS:
        got |= {norm_plan(M, 6, heads * 128, cus, pro=1).kernel for M in (1, 2)}
    got.add(gemv_branch(17, 1000, 1024, cus))
    return got


# ---------------------------------------------------------------------------------------------------------------------------------
# 3. the exact norm input and the exact merge input
# ---------------------------------------------------------------------------------------------------------------------------------
class NormCase:
    """h fp32 [M, K] (a window of a wider buffer when M = 2), integer gamma, w [N, K] in HALF, optional bias / residual, and the
    float64 truth of (gamma h / 2) @ w^T + bias + residual.  EDGES are planted through K positions where x = +-1 is forced
    (gamma = 2, |h| = 1), spread over the whole of K so that every wave carries some; one row may carry several edges."""

    def __init__(self, M, N, K, seed, bias=False, residual=False, plant=True, gmax=8, wmax=4, device="cpu"):
        g = torch.Generator(device="cpu").manual_seed(seed)
        m = K // 16
        self.M, self.N, self.K = M, N, K
        self.eps = 1e-5 if seed % 2 else 1e-6
        b = torch.randint(-256, 257, (N,), generator=g, dtype=torch.int32).double() / 8 if bias else None
        r = torch.randint(-256, 257, (M, N), generator=g, dtype=torch.int32).double() / 8 if residual else None
        w = torch.randint(-8 * wmax, 8 * wmax + 1, (N, K), generator=g, dtype=torch.int32).double() / 8
        gamma = torch.randint(1, gmax + 1, (K,), generator=g, dtype=torch.int32).double() * (torch.randint(0, 2, (K,), generator=g) * 2 - 1)
        plan = []                                                            # (row, column, terms)
        if plant:
            cols = [y for y in (N - 1, 0, N - 2, 1, N // 2, N - 3, N // 3, 2, N - 4, N // 4, N // 5, 3) if 0 <= y < N]
            cols = list(dict.fromkeys(cols))[:max(1, N // 2)]                    # (half of the columns at the least stay ordinary)
            for p, T in enumerate(EDGES[:len(cols)]):
                rr, cc = p % M, cols[p]
                want = T - (float(b[cc]) if b is not None else 0.0) - (float(r[rr, cc]) if r is not None else 0.0)
                plan.append((rr, cc, _terms(want)))
        nslots = sum(len(ts) for _, _, ts in plan)
        forced = [(j * (K // nslots)) + (K // nslots) // 2 for j in range(nslots)] if nslots else []
        assert len(set(forced)) == nslots and nslots <= 4 * m
        gamma[forced] = 2.0
        free = torch.ones(K, dtype=torch.bool)
        free[forced] = False
        mags = torch.cat([torch.full((4 * m - nslots,), 1.0), torch.full((K - 5 * m,), 2.0), torch.full((m,), 4.0)]).double()
        h = torch.ones((M, K), dtype=torch.float64)
        for row in range(M):                                                 # every row its own shuffle
            h[row, free] = mags[torch.randperm(K - nslots, generator=g)]
        h = h * (torch.randint(0, 2, (M, K), generator=g) * 2 - 1)
        x = gamma[None, :] * h / 2
        self.planted = []
        slot = 0
        for rr, cc, ts in plan:
            w[cc] = 0.0
        for rr, cc, ts in plan:
            pos = forced[slot:slot + len(ts)]
            assert bool((x[:, pos].abs() == 1).all())
            w[cc, pos] = torch.tensor(ts, dtype=torch.float64) * x[rr, pos]
            slot += len(ts)
            self.planted.append((rr, cc))
        # the counts the prologue's exactness rests on, after forcing
        for row in range(M):
            a = h[row].abs()
            assert (int((a == 1).sum()), int((a == 2).sum()), int((a == 4).sum())) == (4 * m, K - 5 * m, m)
            assert float((h[row] * h[row]).sum()) == 4.0 * K
        self.h64, self.gamma64, self.x64, self.w64, self.b64, self.r64 = h, gamma, x, w, b, r
        x, w = x.to(device), w.to(device)
        prod, bound = x @ w.t(), x.abs() @ w.abs().t()
        if b is not None:
            prod, bound = prod + b.to(device), bound + b.abs().to(device)
        if r is not None:
            prod, bound = prod + r.to(device), bound + r.abs().to(device)
        # exactness: ordinary columns hold multiples of 2^-4 below 2^24 steps; a planted column sees x = +-1 only: the 2^-3 grid
        pc = torch.zeros(N, dtype=torch.bool, device=device)
        pc[[c for _, c in self.planted]] = True
        assert bool((~pc).any()) and float(bound[:, ~pc].max()) < NORM_LIMIT, float(bound[:, ~pc].max())
        if self.planted:
            assert float(bound[:, pc].max()) < EXACT_LIMIT, float(bound[:, pc].max())
        self.truth = prod
        self.w = self.w64.to(HALF)
        assert torch.equal(self.w.double(), self.w64) and torch.equal(self.x64.to(HALF).double(), self.x64)
        self.h = h.float()
        self.gamma = gamma.float()
        self.bias = b.float() if b is not None else None
        self.res = r.float() if r is not None else None

    def dev(self, device=D):
        """(h, gamma, w, bias, residual) on the device; with two rows h is a window of a wider buffer (ldh = K + 8)."""
        h = self.h.to(device)
        if self.M == 2:
            big = torch.full((2, self.K + 8), 3.0, dtype=torch.float32, device=device)
            big[:, 4:4 + self.K] = h
            h = big[:, 4:4 + self.K]
        return (h, self.gamma.to(device), self.w.to(device), None if self.bias is None else self.bias.to(device),
                None if self.res is None else self.res.to(device))


def perturbed_norm_x(h32: torch.Tensor, gamma32: torch.Tensor, eps: float, steps: int, dtype) -> torch.Tensor:
    """norm_row_kernel's arithmetic with the rsqrt pushed ``steps`` fp32 ulps: gamma * (h * rstd), rounded once to ``dtype``."""
    K = h32.shape[1]
    s = (h32 * h32).sum(-1, keepdim=True)
    rstd = torch.rsqrt(s / float(K) + eps)
    toward = torch.full_like(rstd, 4.0 if steps > 0 else 0.0)
    for _ in range(abs(steps)):
        rstd = torch.nextafter(rstd, toward)
    return (gamma32 * (h32 * rstd)).to(dtype)


class MergeCase:
    """Partials of vly_decode_attention_split whose merge is exact: every split of a head holds the same maximum and l = 0.5 (the
    merged denominator is 2), integer P·V sums whose total is at most 32 in magnitude: x = total / 2, multiples of 0.5 with
    |x| <= 16, exact in both 16-bit types; the o projection over it is exact on the 2^-4 grid."""

    def __init__(self, M, N, heads, seed, bias=False, residual=False, splits=4, device="cpu"):
        g = torch.Generator(device="cpu").manual_seed(seed)
        K = heads * 128
        self.M, self.N, self.K = M, N, K
        o = torch.randint(-8, 9, (M, heads, splits, 128), generator=g, dtype=torch.int32).double()
        p = torch.zeros((M, heads, splits, 132), dtype=torch.float64)
        p[..., 0] = torch.randint(-6, 7, (M, heads, 1), generator=g).double() / 2          # the same maximum in every split of a head
        p[..., 1] = 0.5
        p[..., 2:4] = SENTINEL                                                             # (unused words)
        p[..., 4:] = o
        x = (o.sum(2) / 2).reshape(M, K)
        w = torch.randint(-32, 33, (N, K), generator=g, dtype=torch.int32).double() / 8
        b = torch.randint(-256, 257, (N,), generator=g, dtype=torch.int32).double() / 8 if bias else None
        r = torch.randint(-256, 257, (M, N), generator=g, dtype=torch.int32).double() / 8 if residual else None
        prod, bound = x @ w.t(), x.abs() @ w.abs().t()
        if b is not None:
            prod, bound = prod + b, bound + b.abs()
        if r is not None:
            prod, bound = prod + r, bound + r.abs()
        assert float(bound.max()) < NORM_LIMIT and float(x.abs().max()) <= 16
        assert torch.equal(x.to(HALF).double(), x) and torch.equal(w.to(HALF).double(), w)
        self.x64, self.truth = x, prod
        self.partials, self.w = p.float(), w.to(HALF)
        self.bias = b.float() if b is not None else None
        self.res = r.float() if r is not None else None


# ---------------------------------------------------------------------------------------------------------------------------------
# 4. the checks (these launch kernels: GPU tests and the worker call them)
# ---------------------------------------------------------------------------------------------------------------------------------
def cu_count() -> int:
    return torch.cuda.get_device_properties(0).multi_processor_count


def env_switches():
    """(rows_pin, mfma_env) of this process, as gemv_bf16.hip reads them."""
    rows = os.environ.get("VLY_GEMV_ROWS")
    mf = os.environ.get("VLY_GEMV_MFMA")
    return (int(rows) if rows else 0), (int(mf) if mf is not None else None)


@functools.lru_cache(maxsize=6)
def gcase(M, N, K, seed, bias=False, residual=False, amax=16, wmax=4):
    """A ``Case`` generated on the device (the CPU builds no 4098 x 8192 double matrix)."""
    return Case(M, N, K, seed, bias, residual, True, amax, wmax, device=D)


def window(M, No, dtype, layout="plain"):
    """(buffer, view [M, No], the view's first column).  "ldc": an fp32 row stride that is no multiple of four; "offset": a 16-bit
    view that starts 2 bytes off 8-byte alignment."""
    if layout == "plain":
        buf, out = _guarded(M, No, dtype, 3, None, device=D)
        return buf, out, 0
    if layout == "ldc":
        assert dtype == torch.float32
        buf, out = _guarded(M, No, dtype, 3, 5 if (No + 5) % 4 else 6, device=D)
        assert out.stride(0) % 4, out.stride(0)
        return buf, out, 0
    assert layout == "offset" and dtype != torch.float32
    buf = torch.full((M + 3, No + 16 - No % 8), SENTINEL, dtype=dtype, device=D)
    out = buf[:M, 1:1 + No]
    assert out.data_ptr() % 8 == 2
    return buf, out, 1


def assert_window_guards(buf, M, No, c0, what):
    if c0 == 0:
        return assert_guards(buf, M, No, what)
    outside = torch.ones(buf.shape, dtype=torch.bool, device=buf.device)
    outside[:M, c0:c0 + No] = False
    assert bool((buf[outside] == SENTINEL).all()), f"{what}: an element outside the output window was written"


def res_window(r):
    """r [M, N] as a column window of a wider buffer (ldr = N + 24, 32 bytes in: the matrix-core forms' alignment holds when N % 4 == 0)."""
    M, N = r.shape
    big = torch.full((M, N + 24), 5.0, dtype=r.dtype, device=r.device)
    big[:, 8:8 + N] = r
    return big[:, 8:8 + N]


def _call_branch(M, N, K, epi, out, b, r):
    rows_pin, mfma_env = env_switches()
    blk = mfma_blockers(M, N, K, epi, out.dtype == torch.float32, out.stride(0), out.data_ptr(), None if b is None else b.data_ptr(),
                        None if r is None else r.data_ptr(), 0 if r is None else r.stride(0))
    return gemv_branch(M, N, K, cu_count(), epi, out.dtype == torch.float32, r is not None, blk, rows_pin, mfma_env), blk


def check_linear(M, N, K, branch, seed=61, layout="plain", reason=None, full=True, reached=None):
    """ops.gemv against the truth, bit for bit: bias / residual in {none, bias, bias + residual} x out {fp32, 16-bit (no residual)}
    x {plain weight, PackedWeight (K % 64 == 0), strided A, a residual window}; guards checked; every call must reach ``branch``
    (and, with ``reason``, be kept off the matrix cores for that reason).  ``full`` False: the variants run on one combination."""
    from valley_amd import ops
    for has_b, has_r in ((False, False), (True, False), (True, True)):
        c = gcase(M, N, K, seed + M, has_b, has_r)
        a, w, b, r = c.dev()
        variants = [("plain", a, w, r)]
        if full or has_r:
            variants.append(("strided A", strided(a), w, r))
            if K % 64 == 0:
                variants.append(("p64", a, ops.PackedWeight(w), r))
            if has_r:
                variants.append(("residual window", a, w, res_window(r)))
        for variant, av, wv, rv in variants:
            dtypes = [torch.float32] + ([] if has_r else [HALF])
            if layout == "ldc":
                dtypes = [torch.float32]
            elif layout == "offset":
                dtypes = [] if has_r else [HALF]
            for od in dtypes:
                what = f"gemv {variant} M={M} {N}x{K} bias {has_b} residual {has_r} out {od} [{branch}]"
                buf, out, c0 = window(M, N, od, layout)
                got, blk = _call_branch(M, N, K, EPI_NONE, out, b, rv)
                assert got == branch, f"{what}: the dispatch mirror says {got} (mfma blockers {blk})"
                if reason is not None:
                    assert reason in blk, f"{what}: expected mfma_ok false by {reason}, blockers {blk}"
                ops.gemv(av, wv, b, rv, EPI_NONE, od, out)
                assert_exact(out, c.truth, what)
                assert_window_guards(buf, M, N, c0, what)
                if reached is not None:
                    reached.add(got)


def check_epilogues(M, N, K, branch, seed=81, reached=None):
    """SwiGLU (16-bit, N even) and QUICK_GELU (16-bit, bias) within one ulp of the fp32 torch activation of the exact pre-activation:
    the ``amax = 4, wmax = 1`` cases of the GEMM oracle's test_nonlinear_epilogues_within_one_ulp."""
    from valley_amd import ops
    assert N % 2 == 0
    for epi, has_b in ((EPI_QUICK_GELU, True), (EPI_SWIGLU, False)):
        c = gcase(M, N, K, seed + M, has_b, False, 4, 1)
        a, w, b, _ = c.dev()
        No = N // 2 if epi == EPI_SWIGLU else N
        for variant, av in (("plain", a), ("strided A", strided(a))):
            what = f"gemv {variant} M={M} {N}x{K} epi {epi} [{branch}]"
            buf, out, _ = window(M, No, HALF)
            got, blk = _call_branch(M, N, K, epi, out, b, None)
            assert got == branch, f"{what}: the dispatch mirror says {got} (mfma blockers {blk})"
            ops.gemv(av, w, b, None, epi, HALF, out)
            assert_activation(out, c.truth, epi, what)
            assert_guards(buf, M, No, what)
            if reached is not None:
                reached.add(got)


@functools.lru_cache(maxsize=4)
def ncase(M, N, K, seed, bias=False, residual=False, plant=True, gmax=8, wmax=4):
    return NormCase(M, N, K, seed, bias, residual, plant, gmax, wmax, device=D)


def check_norm_linear(M, N, K, seed=71):
    """ops.gemv_rmsnorm on the exact prologue against the truth, bit for bit: {none, bias, bias + residual} x {fp32, 16-bit}."""
    from valley_amd import ops
    for has_b, has_r in ((False, False), (True, False), (True, True)):
        c = ncase(M, N, K, seed + M + K, has_b, has_r)
        h, gm, w, b, r = c.dev()
        assert M == 1 or h.stride(0) != K
        rv = res_window(r) if has_r else None
        for od in (torch.float32, HALF):
            what = f"gemv_rmsnorm M={M} {N}x{K} eps {c.eps} bias {has_b} residual {has_r} out {od}"
            buf, out, _ = window(M, N, od)
            ops.gemv_rmsnorm(h, gm, c.eps, w, b, rv, EPI_NONE, od, out)
            assert_exact(out, c.truth, what)
            assert_guards(buf, M, N, what)


def check_norm_swiglu(M, N, K, seed=75):
    from valley_amd import ops
    assert N % 2 == 0
    c = ncase(M, N, K, seed + M + K, False, False, True, 2, 1)
    h, gm, w, _, _ = c.dev()
    what = f"gemv_rmsnorm SwiGLU M={M} {N}x{K}"
    buf, out, _ = window(M, N // 2, HALF)
    ops.gemv_rmsnorm(h, gm, c.eps, w, None, None, EPI_SWIGLU, HALF, out)
    assert_activation(out, c.truth, EPI_SWIGLU, what)
    assert_guards(buf, M, N // 2, what)
