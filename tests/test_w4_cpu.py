"""CPU-side checks of INT4 weight-only decode: the packed layout obeys the header's formula, the reference quantizer keeps its properties, and the switches parse and
refuse as documented."""
import pytest
import torch

from tests import w4_ref


def test_pack_round_trips_and_obeys_the_formula():
    g = torch.Generator().manual_seed(4)
    q = torch.randint(-7, 8, (5, 384), generator=g, dtype=torch.int32).to(torch.int8)
    q[0, :15] = torch.arange(-7, 8, dtype=torch.int8)                   # the full range, in order
    p = w4_ref.pack(q)
    assert p.dtype == torch.uint8 and tuple(p.shape) == (5, 192)
    assert torch.equal(w4_ref.unpack(p), q)
    # hand-computed positions: k -> (byte of the row, high nibble?)   [word k / 8, nibble (k % 8) / 2 + 4 (k % 2)]
    where = {0: (0, False), 1: (2, False), 2: (0, True), 3: (2, True), 4: (1, False), 5: (3, False), 6: (1, True), 7: (3, True),
             8: (4, False), 13: (7, False), 127: (63, True), 128: (64, False), 383: (191, True)}
    for n in (0, 3):
        for k, (byte, high) in where.items():
            got = int(p[n, byte]) >> 4 if high else int(p[n, byte]) & 15
            assert got == int(q[n, k]) + 8, (n, k)
    # the formula itself, element by element
    for k in range(384):
        pn = (k % 8) // 2 + 4 * (k % 2)
        byte = 4 * (k // 8) + pn // 2
        assert ((int(p[2, byte]) >> (4 * (pn % 2))) & 15) == int(q[2, k]) + 8


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_reference_quantizer_properties(dtype):
    w = w4_ref.random_rows(9, 1152, 12, dtype)
    w[3] = 0
    w[5, 256:384] = 0
    q, s = w4_ref.quantize_ref(w)
    wf = w.to(torch.float32)
    assert q.dtype == torch.int8 and s.dtype == torch.float32 and tuple(s.shape) == (9, 9)
    assert int(q.min()) >= -7 and int(q.max()) <= 7                     # -8 never occurs
    s64 = w4_ref.expand(s).to(torch.float64)                            # the bound is on real numbers: evaluated in float64
    err = (q.to(torch.float64) * s64 - wf.to(torch.float64)).abs()
    assert bool((err <= (s64 / 2) * (1 + 2.0 ** -20)).all()), float((err / s64).max())
    qg, wg = q.reshape(9, 9, 128), wf.reshape(9, 9, 128)
    amax_at = wg.abs().argmax(dim=2)
    for n in range(9):
        for gi in range(9):
            if n == 3 or (n == 5 and gi == 2):
                assert float(s[n, gi]) == 1.0 and int(qg[n, gi].abs().max()) == 0
            else:
                assert abs(int(qg[n, gi, amax_at[n, gi]])) == 7
    live = torch.ones((9, 9), dtype=torch.bool)
    live[3] = False
    live[5, 2] = False
    dist = w4_ref.tie_distance(w, s).reshape(9, 9, 128)[live]
    assert float(dist.min()) >= 2.0 ** -16


def test_exact_builder_round_trips_through_the_reference():
    for (N, K) in w4_ref.QUANT_SHAPES:
        for dtype in (torch.bfloat16, torch.float16):
            w, q, s = w4_ref.exact_weights(N, K, seed=N + K, dtype=dtype)
            q2, s2 = w4_ref.quantize_ref(w)
            assert torch.equal(q2, q) and torch.equal(s2, s)
            assert bool((q.reshape(N, K // 128, 128).abs().amax(dim=2) == 7).all())
            if K > 128:
                assert bool((s[:, 1:] != s[:, :-1]).all())              # neighbouring groups: another exponent


def test_w4_ops_reject_cpu_tensors():
    from valley_amd import lib, ops
    w = torch.zeros((4, 128), dtype=torch.bfloat16)
    q, s = torch.zeros((4, 64), dtype=torch.uint8), torch.ones((4, 1))
    with pytest.raises(lib.ValleyHipError):
        ops.w4_quantize(w)
    with pytest.raises(lib.ValleyHipError):
        ops.w4_gemv(torch.zeros((1, 128), dtype=torch.bfloat16), q, s)
    with pytest.raises(lib.ValleyHipError):
        ops.w4_gemv_rmsnorm(torch.zeros((1, 128)), torch.ones(128), 1e-5, q, s)
    assert ops.w4_gemv_rmsnorm_ok(1, 2048) and ops.w4_gemv_rmsnorm_ok(2, 6144) and ops.w4_gemv_rmsnorm_ok(2, 4224)
    assert not ops.w4_gemv_rmsnorm_ok(3, 4096) and not ops.w4_gemv_rmsnorm_ok(1, 1920) and not ops.w4_gemv_rmsnorm_ok(1, 6272)
    assert not ops.w4_gemv_rmsnorm_ok(1, 4160)


def test_weight_quant_switch_parsing(monkeypatch):
    from valley_amd import llama
    assert llama.WEIGHT_QUANT_MODES == ("int8", "int4")
    assert llama.parse_weight_quant("int4") == "int4" and llama.parse_weight_quant(" INT4 ") == "int4"
    with pytest.raises(ValueError, match="'int8', 'int4'"):
        llama.parse_weight_quant("fp8", "VALLEY_WEIGHT_QUANT")
    monkeypatch.setenv("VALLEY_WEIGHT_QUANT", "int4")
    assert llama.resolve_weight_quant(None, "bf16") == "int4"
    monkeypatch.setenv("VALLEY_WEIGHT_QUANT", "int3")
    with pytest.raises(ValueError, match="VALLEY_WEIGHT_QUANT"):
        llama.HipLlama(2048, 16, 5504, 2, 1000, 1e-5)


def test_fp32_precision_refuses_int4(monkeypatch):
    from valley_amd import llama, runtime
    monkeypatch.setattr(runtime, "PRECISION", "fp32")
    with pytest.raises(ValueError, match="fp32"):
        llama.HipLlama(2048, 16, 5504, 2, 1000, 1e-5, weight_quant="int4")
    monkeypatch.setenv("VALLEY_WEIGHT_QUANT", "int4")
    with pytest.raises(ValueError, match="fp32"):
        llama.HipLlama(2048, 16, 5504, 2, 1000, 1e-5)


def test_quant_ops_table():
    from valley_amd import ops
    assert ops.quant_ops("int8") == (ops.wq_quantize, ops.wq_gemv, ops.wq_gemv_rmsnorm, ops.wq_gemv_rmsnorm_ok)
    assert ops.quant_ops("int4") == (ops.w4_quantize, ops.w4_gemv, ops.w4_gemv_rmsnorm, ops.w4_gemv_rmsnorm_ok)
    with pytest.raises(ValueError, match="fp8"):
        ops.quant_ops("fp8")


def test_cli_takes_weight_quant_int4():
    from valley_amd import cli
    assert cli.parse_args(["--weight-quant", "int4"]).weight_quant == "int4"
    assert cli.parse_args(["--weight-quant", "int8"]).weight_quant == "int8"
    with pytest.raises(SystemExit):
        cli.parse_args(["--weight-quant", "fp8"])
