"""CPU-side checks of INT8 weight-only decode: the reference quantizer keeps its properties, and the switches parse and
refuse as documented."""
import pytest
import torch

from tests import wq_ref


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_reference_quantizer_properties(dtype):
    # wq_ref.random_rows: rows whose amax has a prime mantissa hold no element on a rounding tie (its docstring says why: on plain
    # Gaussian 16-bit rows dozens of elements per row are exact ties, which the rounded scale pushes 2^-17 past s / 2)
    w = wq_ref.random_rows(9, 1040, 12, dtype)
    w[3] = 0
    q, s = wq_ref.quantize_ref(w)
    wf = w.to(torch.float32)
    assert q.dtype == torch.int8 and s.dtype == torch.float32
    assert int(q.min()) >= -127                                         # -128 never occurs
    s64 = s.to(torch.float64)[:, None]                                  # the bound is on real numbers: evaluated in float64
    err = (q.to(torch.float64) * s64 - wf.to(torch.float64)).abs()
    assert bool((err <= (s64 / 2) * (1 + 2.0 ** -20)).all()), float((err / s64).max())
    amax_at = wf.abs().argmax(dim=1)
    for n in range(w.shape[0]):
        if n == 3:
            assert float(s[n]) == 1.0 and int(q[n].abs().max()) == 0
        else:
            assert abs(int(q[n, amax_at[n]])) == 127


def test_exact_builder_round_trips_through_the_reference():
    for (N, K) in wq_ref.QUANT_SHAPES:
        for dtype in (torch.bfloat16, torch.float16):
            w, q, s = wq_ref.exact_weights(N, K, seed=N + K, dtype=dtype)
            q2, s2 = wq_ref.quantize_ref(w)
            assert torch.equal(q2, q) and torch.equal(s2, s)


def test_wq_ops_reject_cpu_tensors():
    from valley_amd import lib, ops
    w = torch.zeros((4, 32), dtype=torch.bfloat16)
    q, s = torch.zeros((4, 32), dtype=torch.int8), torch.ones(4)
    with pytest.raises(lib.ValleyHipError):
        ops.wq_quantize(w)
    with pytest.raises(lib.ValleyHipError):
        ops.wq_gemv(torch.zeros((1, 32), dtype=torch.bfloat16), q, s)
    with pytest.raises(lib.ValleyHipError):
        ops.wq_gemv_rmsnorm(torch.zeros((1, 32)), torch.ones(32), 1e-5, q, s)
    assert ops.wq_gemv_rmsnorm_ok(1, 2048) and ops.wq_gemv_rmsnorm_ok(2, 6144) and ops.wq_gemv_rmsnorm_ok(2, 4112)
    assert not ops.wq_gemv_rmsnorm_ok(3, 4096) and not ops.wq_gemv_rmsnorm_ok(1, 2032) and not ops.wq_gemv_rmsnorm_ok(1, 6160)
    assert not ops.wq_gemv_rmsnorm_ok(1, 4104)


def test_weight_quant_switch_parsing(monkeypatch):
    from valley_amd import llama
    for off in (None, "", "0"):
        assert llama.parse_weight_quant(off) is None
    assert llama.parse_weight_quant("int8") == "int8"
    with pytest.raises(ValueError, match="int8"):
        llama.parse_weight_quant("fp8", "VALLEY_WEIGHT_QUANT")
    # the engine reads the environment where it reads VALLEY_PACK_WEIGHTS: a bad value is refused before anything is allocated
    monkeypatch.setenv("VALLEY_WEIGHT_QUANT", "e4m3")
    with pytest.raises(ValueError, match="VALLEY_WEIGHT_QUANT"):
        llama.HipLlama(2048, 16, 5504, 2, 1000, 1e-5)


def test_fp32_precision_refuses_quantization(monkeypatch):
    from valley_amd import llama, runtime
    monkeypatch.setattr(runtime, "PRECISION", "fp32")
    with pytest.raises(ValueError, match="fp32"):
        llama.HipLlama(2048, 16, 5504, 2, 1000, 1e-5, weight_quant="int8")
    monkeypatch.setenv("VALLEY_WEIGHT_QUANT", "int8")
    with pytest.raises(ValueError, match="fp32"):
        llama.HipLlama(2048, 16, 5504, 2, 1000, 1e-5)


def test_cli_takes_weight_quant():
    from valley_amd import cli
    assert cli.parse_args(["--weight-quant", "int8"]).weight_quant == "int8"
    assert cli.parse_args([]).weight_quant is None
