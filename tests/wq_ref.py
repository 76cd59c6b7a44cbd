"""Torch-CPU reference of the INT8 weight-only quantizer (include/valley_hip_wq.h) and the builders of EXACT cases.

The rule, per row: s = amax / 127.0f (IEEE fp32), q = clamp(rint(w / s), -127, 127) (IEEE fp32 division, ties to even); an all-zero
row gives s = 1, q = 0; -128 never occurs.

Exact cases: weight rows w = q * 2^e with integer q in [-127, 127] (at least one +-127 per row) and e in [-9, -3] per row,
activations and residual integers in [-4, 4].  Every value is exact in bf16 and fp16, every partial sum is an integer multiple
of 2^e below 2^24 * 2^e for K <= 13824 (13824 * 127 * 4 < 2^23), so any fp32 summation order is exact and the quantizer must
return exactly (q, 2^e)."""
import torch

SHAPES = [(2, 16), (6, 1040), (34, 4112), (10, 13824)]          # (N, K) of the GEMV tests
QUANT_SHAPES = [(1, 16), (6, 1040), (34, 4112)]


def quantize_ref(w: torch.Tensor):
    """w [N, K] of any float dtype (CPU) -> (q int8 [N, K], scale fp32 [N]) by the rule above, in fp32 arithmetic."""
    w = w.detach().cpu().to(torch.float32)
    amax = w.abs().amax(dim=1)
    s = torch.where(amax > 0, amax / torch.tensor(127.0, dtype=torch.float32), torch.ones_like(amax))
    q = torch.clamp(torch.round(w / s[:, None]), -127, 127).to(torch.int8)
    return q, s


def tie_distance(w: torch.Tensor, s: torch.Tensor) -> torch.Tensor:
    """| frac(w / s) - 0.5 | in float64: how far each element sits from a rounding tie."""
    r = w.detach().cpu().to(torch.float64) / s.to(torch.float64)[:, None]
    return ((r - torch.floor(r)) - 0.5).abs()


def exact_weights(N: int, K: int, seed: int, dtype=torch.bfloat16):
    """-> (w [N, K] in ``dtype`` = q * 2^e exactly, q int8 [N, K], scale fp32 [N] = 2^e)."""
    g = torch.Generator().manual_seed(seed)
    q = torch.randint(-127, 128, (N, K), generator=g, dtype=torch.int32)
    col = torch.randint(0, K, (N,), generator=g)
    sign = torch.randint(0, 2, (N,), generator=g, dtype=torch.int32) * 2 - 1
    q[torch.arange(N), col] = 127 * sign
    e = torch.randint(-9, -2, (N,), generator=g)                  # [-9, -3]
    scale = torch.pow(torch.tensor(2.0, dtype=torch.float32), e.to(torch.float32))
    w = (q.to(torch.float32) * scale[:, None]).to(dtype)
    assert torch.equal(w.to(torch.float32), q.to(torch.float32) * scale[:, None])
    return w, q.to(torch.int8), scale


def exact_activations(M: int, K: int, seed: int, dtype=torch.bfloat16):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(-4, 5, (M, K), generator=g, dtype=torch.int32).to(dtype)


def exact_residual(M: int, N: int, seed: int):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(-4, 5, (M, N), generator=g, dtype=torch.int32).to(torch.float32)


def _primes(lo: int, hi: int):
    return [n for n in range(lo, hi) if all(n % d for d in range(2, int(n ** 0.5) + 1))]


def random_rows(N: int, K: int, seed: int, dtype=torch.bfloat16):
    """Random 16-bit rows for the quantizer.  Row n: Gaussian with sigma = amax_n / 3, cut off at amax_n * 63/64, and one planted
    maximum +-amax_n = p_n * 2^(e_n - t) with its own PRIME p_n in [2^t, 2^(t+1)) (t = 7 mantissa bits in bf16, 10 in fp16) and its own
    binade e_n in [-8, 1]: every row has another amax, so another scale out of amax / 127.0f, and q fills [-127, 127].
    Why a prime: in a 16-bit row w / s = 127 m_w 2^-d / m_a is a ratio of short integers, and for a random amax dozens of elements
    per row sit EXACTLY on a rounding tie (measured on plain Gaussian bf16 rows: 10-22 per 4112), where the fp32 rounding of the
    scale decides the result and pushes |q s - w| up to 2^-17 s past s / 2 — far above the 0.1 % the device may differ on.  With a
    prime mantissa m_a >= 2^t (coprime to 2 and to 127) a tie needs m_a | m_w, i.e. |w| = amax 2^-j, and 127 * 2^-j is a half-integer
    for j = 1 only: an element that equals +-amax / 2 is moved one ulp towards zero.  Every other element is at least
    1 / (2 m_a 2^d) >= 2^(-t-2-d) from a tie, while the two fp32 roundings (of s and of w / s) move w / s by at most 2^(-16-d)."""
    g = torch.Generator().manual_seed(seed)
    t = 7 if dtype == torch.bfloat16 else 10
    primes = _primes(2 ** t, 2 ** (t + 1))
    p = torch.tensor([primes[int(i)] for i in torch.randint(0, len(primes), (N,), generator=g)], dtype=torch.float64)
    e = torch.randint(-8, 2, (N,), generator=g).to(torch.float64)
    amax = (p * torch.pow(torch.tensor(2.0, dtype=torch.float64), e - t)).to(torch.float32)[:, None]      # exact in ``dtype``
    w = torch.randn((N, K), generator=g) * (amax / 3)
    w = torch.minimum(torch.maximum(w, -amax * (63.0 / 64.0)), amax * (63.0 / 64.0)).to(dtype)
    half = (w.to(torch.float32).abs() == amax / 2)
    w = torch.where(half, (w.to(torch.float32) * (1 - 2.0 ** -(t + 1))).to(dtype), w)                       # one ulp below the binade's start
    col = torch.randint(0, K, (N,), generator=g)
    sign = (torch.randint(0, 2, (N,), generator=g) * 2 - 1).to(torch.float32)
    w[torch.arange(N), col] = (sign * amax[:, 0]).to(dtype)
    wf = w.to(torch.float32).abs()
    assert torch.equal(wf.amax(dim=1), amax[:, 0]) and int((wf == amax).sum()) == N and not bool((wf == amax / 2).any())
    return w
