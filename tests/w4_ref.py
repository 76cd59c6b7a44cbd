"""Torch-CPU reference of the INT4 weight-only format and quantizer (include/valley_hip_w4.h) and the builders of EXACT cases.

The rule, per row n and group g of 128 consecutive k: s = amax / 7.0f (IEEE fp32), q = clamp(rint(w / s), -7, 7) (IEEE fp32
division, ties to even); an all-zero group gives s = 1, q = 0; -8 never occurs.

The layout (the header's formula): u = q + 8 in [1, 15]; element (n, k) lies in the little-endian 32-bit word k / 8 of row n, in
nibble p = (k % 8) / 2 + 4 * (k % 2) of that word, i.e. in byte 4 * (k / 8) + p / 2 of the row, low nibble for even p and high
nibble for odd p.  Scales: fp32 [N, K / 128].

Exact cases: weight groups w = q * 2^e with integer q in [-7, 7] (at least one +-7 per group) and e in [-8, -3], another e in
each neighbouring group of a row (e = -8 + (g + n) % 6: a kernel that reads another group's or row's scale cannot pass),
activations and residual integers in [-4, 4].  Every value is exact in bf16 and fp16 and every partial sum of a * w is an integer
multiple of 2^-8 below 2^24 * 2^-8 for K <= 13824 (13824 * 7 * 4 * 2^5 < 2^24), so any fp32 summation order is exact and the
quantizer must return exactly (q, 2^e).

The kernel multiplies by q + c (c = OFFSET[dtype]: 136 on bf16, 1032 on fp16) and subtracts c * sum(a) per chunk of 32 weights;
the same inequality for that form: a chunk's sum of a * (q + c) is an integer of magnitude <= 32 * 4 * (7 + 1032) = 132992 < 2^24,
the chunk's sum of a is an integer <= 128, their combination d - c t is the integer sum of a * q (<= 896), and its product with
2^e joins the accumulation of multiples of 2^-8 bounded as above: every operation of the header's arithmetic is exact on these
cases."""
import torch

from tests import wq_ref

GROUP = 128
SHAPES = [(2, 128), (6, 1152), (34, 4224), (10, 13824)]         # (N, K) of the GEMV tests
QUANT_SHAPES = SHAPES[:3]
OFFSET = {torch.bfloat16: 136.0, torch.float16: 1032.0}         # the c of valley_hip_w4.h
_E_OF_P = [0, 2, 4, 6, 1, 3, 5, 7]                              # element (k % 8) held by nibble p of a word


def pack(q: torch.Tensor) -> torch.Tensor:
    """q integer [N, K] in [-7, 7] -> uint8 [N, K / 2] in the header's layout."""
    N, K = q.shape
    u = (q.to(torch.int32) + 8).reshape(N, K // 8, 8)
    assert int(u.min()) >= 1 and int(u.max()) <= 15
    nib = u[:, :, _E_OF_P]                                       # [N, K / 8, 8]: nibble p of each word
    return (nib[:, :, 0::2] | (nib[:, :, 1::2] << 4)).reshape(N, K // 2).to(torch.uint8)


def unpack(packed: torch.Tensor) -> torch.Tensor:
    """uint8 [N, K / 2] -> q int8 [N, K]."""
    N, K2 = packed.shape
    b = packed.cpu().to(torch.int32).reshape(N, K2 // 4, 4)
    nib = torch.stack([b & 15, b >> 4], dim=-1).reshape(N, K2 // 4, 8)   # nibble p = 2 * byte + (high ? 1 : 0)
    u = torch.empty_like(nib)
    u[:, :, _E_OF_P] = nib
    return (u - 8).reshape(N, 2 * K2).to(torch.int8)


def quantize_ref(w: torch.Tensor):
    """w [N, K] of any float dtype (CPU) -> (q int8 [N, K], scale fp32 [N, K / 128]) by the rule above, in fp32 arithmetic."""
    w = w.detach().cpu().to(torch.float32)
    N, K = w.shape
    wg = w.reshape(N, K // GROUP, GROUP)
    amax = wg.abs().amax(dim=2)
    s = torch.where(amax > 0, amax / torch.tensor(7.0, dtype=torch.float32), torch.ones_like(amax))
    q = torch.clamp(torch.round(wg / s[:, :, None]), -7, 7).to(torch.int8)
    return q.reshape(N, K), s


def expand(s: torch.Tensor) -> torch.Tensor:
    """scale [N, G] -> [N, K]: every element's scale."""
    return s.repeat_interleave(GROUP, dim=1)


def tie_distance(w: torch.Tensor, s: torch.Tensor) -> torch.Tensor:
    """| frac(w / s) - 0.5 | in float64: how far each element sits from a rounding tie."""
    r = w.detach().cpu().to(torch.float64) / expand(s).to(torch.float64)
    return ((r - torch.floor(r)) - 0.5).abs()


def exact_weights(N: int, K: int, seed: int, dtype=torch.bfloat16):
    """-> (w [N, K] in ``dtype`` = q * 2^e exactly, q int8 [N, K], scale fp32 [N, K / 128] = 2^e)."""
    g = torch.Generator().manual_seed(seed)
    G = K // GROUP
    q = torch.randint(-7, 8, (N, G, GROUP), generator=g, dtype=torch.int32)
    col = torch.randint(0, GROUP, (N, G), generator=g)
    sign = torch.randint(0, 2, (N, G), generator=g, dtype=torch.int32) * 2 - 1
    q.scatter_(2, col[:, :, None], (7 * sign)[:, :, None])
    e = -8 + (torch.arange(G)[None, :] + torch.arange(N)[:, None]) % 6
    scale = torch.pow(torch.tensor(2.0, dtype=torch.float32), e.to(torch.float32))
    w = (q.to(torch.float32) * scale[:, :, None]).reshape(N, K).to(dtype)
    q = q.reshape(N, K)
    assert torch.equal(w.to(torch.float32), q.to(torch.float32) * expand(scale))
    return w, q.to(torch.int8), scale


exact_activations = wq_ref.exact_activations
exact_residual = wq_ref.exact_residual


def random_rows(N: int, K: int, seed: int, dtype=torch.bfloat16):
    """Random 16-bit rows for the quantizer: every group of 128 is one row of wq_ref.random_rows (Gaussian body, one planted amax
    with a prime mantissa, +-amax / 2 moved one ulp).  The argument there holds with 7 for 127: w / s = 7 m_w 2^-d / m_a, a tie
    needs m_a | m_w, i.e. |w| = amax 2^-j, and 7 * 2^-j is a half-integer for j = 1 only."""
    return wq_ref.random_rows(N * (K // GROUP), GROUP, seed, dtype).reshape(N, K)


def random_quantized(N: int, K: int, g: torch.Generator):
    """Random q in [-7, 7] and fp32 scales in (0.5 .. 1.5) * 1e-3 -> (q int8 [N, K], packed, scale [N, G])."""
    q = torch.randint(-7, 8, (N, K), generator=g, dtype=torch.int32).to(torch.int8)
    s = (torch.rand((N, K // GROUP), generator=g) + 0.5) * 1e-3
    return q, pack(q), s
