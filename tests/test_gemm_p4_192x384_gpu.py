"""Tile hint 194: the persistent GEMM on 192 x 384 tiles (gemm_p4_kernel<192, 384, SwiGLU>, valley_amd/csrc/gemm_bf16.hip), whose waves
hold 72 accumulator blocks — 64 in a0 .. a255, 8 in v224 .. v255.  Every output adds the same MFMA products in the same K order as the
256 x 256 tile (hint 197), wherever its tile sits, so the two must agree bit for bit: the 13B gate|up shape on block-packed and on
row-major weights, ragged M and N, M below one tile, repeated launches, guard rows and columns; what the tile does not take runs 197."""
import pytest
import torch

from valley_amd.runtime import HALF

pytestmark = pytest.mark.gpu
D = "cuda:0"
EPI_SWIGLU = 2
EPS = torch.finfo(HALF).eps      # one rounding of the 16-bit storage type: 2^-7 (bf16), 2^-10 (fp16)


def rnd(shape, seed, scale=1.0):
    g = torch.Generator(device=D).manual_seed(seed)
    return (torch.randn(shape, generator=g, device=D) * scale).to(HALF)


def both(a, w, **kw):
    from valley_amd import ops
    got = ops.gemm_mfma(a, w, epilogue=EPI_SWIGLU, tile_hint=194, **kw)
    ref = ops.gemm_mfma(a, w, epilogue=EPI_SWIGLU, tile_hint=197, **kw)
    torch.cuda.synchronize()
    return got, ref


@pytest.mark.parametrize("packed", [True, False])
def test_13b_gate_up_matches_hint_197_bit_for_bit(packed):
    from valley_amd import ops
    M, N, K = 2688, 27648, 5120
    a = rnd((M, K), 1)
    w = rnd((N, K), 2, 0.02)
    got, ref = both(a, ops.PackedWeight(w) if packed else w)
    assert torch.isfinite(got.float()).all()
    assert torch.equal(got, ref)
    # and it is the SwiGLU of the product (spot rows against fp32)
    rows = torch.tensor([0, 1, 191, 192, 1337, M - 1], device=D)
    y = a[rows].float() @ w.float().t()
    want = torch.nn.functional.silu(y[:, 0::2]) * y[:, 1::2]
    assert float((got[rows].float() - want).norm() / want.norm()) < 0.512 * EPS


@pytest.mark.parametrize("M,N,K,packed", [
    (2600, 27648, 1024, True),      # ragged M: the last tile row holds 104 of 192 rows (one wave slab outside the problem)
    (200, 27648, 1024, False),      # 2 tile rows, the second 8 rows high; fewer tiles than CUs
    (100, 4096, 640, True),         # M below one tile
    (1, 1536, 512, False),          # one row
    (2688, 3088, 1024, True),       # ragged N: 3088 = 8 x 384 + 16 (the last n-tile 16 columns wide)
    (1000, 1040, 768, False),       # ragged M and N, N a multiple of 16 only
    (777, 7696, 1024, True),        # 7696 = 20 x 384 + 16
    (4000, 11008, 4096, False),     # more tiles than CUs on a non-Llama shape
])
def test_ragged_shapes_match_hint_197(M, N, K, packed):
    from valley_amd import ops
    a = rnd((M, K), 3)
    w = rnd((N, K), 4, 0.05)
    got, ref = both(a, ops.PackedWeight(w) if packed else w)
    assert torch.equal(got, ref)


def test_guard_rows_and_columns_are_never_written():
    """Output into a wider, taller buffer through a strided view: nothing past column N / 2 or row M changes."""
    M, N, K = 500, 1552, 640
    a_big = rnd((M + 7, K + 64), 5)
    a = a_big[:M, 64:]
    w = rnd((N, K), 6, 0.05)
    from valley_amd import ops
    out = torch.full((M + 5, N // 2 + 40), 7.0, dtype=HALF, device=D)
    ops.gemm_mfma(a, w, epilogue=EPI_SWIGLU, out=out[:M, :N // 2], tile_hint=194)
    ref = ops.gemm_mfma(a, w, epilogue=EPI_SWIGLU, tile_hint=197)
    torch.cuda.synchronize()
    assert torch.equal(out[:M, :N // 2], ref)
    assert bool((out[:, N // 2:] == 7.0).all()) and bool((out[M:] == 7.0).all())


def test_repeated_launches_are_bit_identical():
    from valley_amd import ops
    a = rnd((2688, 2048), 7)
    w = ops.PackedWeight(rnd((9216, 2048), 8, 0.05))
    first = ops.gemm_mfma(a, w, epilogue=EPI_SWIGLU, tile_hint=194)
    for _ in range(5):
        again = ops.gemm_mfma(a, w, epilogue=EPI_SWIGLU, tile_hint=194)
        torch.cuda.synchronize()
        assert torch.equal(again, first)


def test_what_the_tile_does_not_take_runs_hint_197():
    """Other epilogues, fp32 output, a bias, K below two K tiles, an output row stride that is not a multiple of 8: hint 194 is hint 197."""
    from valley_amd import ops
    a = rnd((600, 512), 9)
    w = rnd((1536, 512), 10, 0.05)
    bias = torch.randn(1536, device=D)
    for kw in (dict(epilogue=0), dict(epilogue=1), dict(epilogue=3), dict(epilogue=0, out_dtype=torch.float32),
               dict(epilogue=EPI_SWIGLU, bias=bias)):
        assert torch.equal(ops.gemm_mfma(a, w, tile_hint=194, **kw), ops.gemm_mfma(a, w, tile_hint=197, **kw)), kw
    a64 = rnd((600, 64), 11)
    w64 = rnd((1536, 64), 12, 0.05)
    assert torch.equal(ops.gemm_mfma(a64, w64, epilogue=EPI_SWIGLU, tile_hint=194), ops.gemm_mfma(a64, w64, epilogue=EPI_SWIGLU, tile_hint=197))
    o1 = torch.empty((600, 770), dtype=HALF, device=D)
    o2 = torch.empty((600, 770), dtype=HALF, device=D)
    ops.gemm_mfma(a, w, epilogue=EPI_SWIGLU, out=o1[:, :768], tile_hint=194)
    ops.gemm_mfma(a, w, epilogue=EPI_SWIGLU, out=o2[:, :768], tile_hint=197)
    torch.cuda.synchronize()
    assert torch.equal(o1[:, :768], o2[:, :768])
