"""Kernel-level checks of libvalley_hip_wq.so on the bound 16-bit storage type (runtime.HALF): called by tests/test_wq_gpu.py on
the bf16 library and by tests/wq_worker.py in a child process on the fp16 library.  Every function asserts; none returns."""
import itertools
import math

import torch

from tests import wq_ref

SENT = -77.0                                                    # exact in bf16, fp16 and fp32; no result of these cases equals it by construction of the checks


def _half():
    from valley_amd import runtime
    return runtime.HALF


def _bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


def _guarded(M, No, dtype, extra=3):
    buf = torch.full((8, No + extra), SENT, dtype=dtype, device="cuda")
    return buf, buf[:M, :No]


def _guards_intact(buf, M, No):
    return bool((buf[M:] == SENT).all()) and bool((buf[:, No:] == SENT).all())


def quantizer_exact():
    from valley_amd import ops
    for (N, K) in wq_ref.QUANT_SHAPES:
        w, q, s = wq_ref.exact_weights(N, K, seed=100 + N, dtype=_half())
        gq, gs = ops.wq_quantize(w.cuda())
        assert torch.equal(gq.cpu(), q) and torch.equal(_bits(gs.cpu()), _bits(s)), (N, K)
    z = torch.zeros((3, 32), dtype=_half(), device="cuda")      # all-zero rows: s = 1, q = 0
    gq, gs = ops.wq_quantize(z)
    assert int(gq.abs().max()) == 0 and bool((gs == 1.0).all())
    # a strided source (rows of a wider buffer)
    w, q, s = wq_ref.exact_weights(6, 1040, seed=7, dtype=_half())
    big = torch.zeros((6, 1048), dtype=_half(), device="cuda")
    big[:, :1040] = w.cuda()
    gq, gs = ops.wq_quantize(big[:, :1040])
    assert torch.equal(gq.cpu(), q) and torch.equal(gs.cpu(), s)


def quantizer_random(seed=12):
    """Random rows: the scale bit for bit, q equal to the CPU reference except (by +-1) at elements within 2^-18 of a rounding tie;
    the count of such elements is <= 0.1 % of a row.  -> None; prints the count."""
    from valley_amd import ops
    for (N, K) in wq_ref.QUANT_SHAPES:
        w = wq_ref.random_rows(N, K, seed + K, _half())
        q, s = wq_ref.quantize_ref(w)
        near = wq_ref.tie_distance(w, s) <= 2.0 ** -18
        assert int(near.sum(dim=1).max()) <= max(0, int(0.001 * K)), "the reference itself is not inside the cap: pick another seed"
        gq, gs = ops.wq_quantize(w.cuda())
        gq, gs = gq.cpu(), gs.cpu()
        assert torch.equal(_bits(gs), _bits(s)), (N, K)
        diff = (gq.to(torch.int32) - q.to(torch.int32)).abs()
        assert int(diff.max()) <= 1 and not bool((diff > 0)[~near].any()), (N, K, int(diff.max()))
        print(f"wq quantizer ({N}, {K}): {int((diff > 0).sum())} elements differ from the reference, {int(near.sum())} within 2^-18 of a tie")
        assert int((diff > 0).sum(dim=1).max()) <= int(0.001 * K)
        assert int(gq.min()) >= -127
        s64 = gs.to(torch.float64)[:, None]
        err = (gq.to(torch.float64) * s64 - w.to(torch.float64)).abs()
        assert bool((err <= s64 / 2 * (1 + 2.0 ** -20)).all())
        amax_at = w.to(torch.float32).abs().argmax(dim=1)
        assert bool((gq[torch.arange(N), amax_at].abs() == 127).all())


def _combos():
    """(epilogue, out dtype or None for 16-bit, residual?)"""
    from valley_amd import ops
    return [(ops.EPI_NONE, None, False), (ops.EPI_NONE, None, True), (ops.EPI_NONE, torch.float32, False),
            (ops.EPI_NONE, torch.float32, True), (ops.EPI_SWIGLU, None, False)]


def gemv_exact(N, K):
    """M = 1 .. 8, every epilogue / output / residual combination: bit-identical to ops.gemv on the dequantized weights and, for
    EPI_NONE, to the float64 sum rounded to the output type; guard rows and columns untouched."""
    from valley_amd import ops
    H = _half()
    w, q, s = wq_ref.exact_weights(N, K, seed=3 * N + K, dtype=H)
    wd, qd, sd = w.cuda(), q.cuda(), s.cuda()
    w64 = q.to(torch.float64) * s.to(torch.float64)[:, None]
    for M, (epi, od, use_res) in itertools.product(range(1, 9), _combos()):
        a = wq_ref.exact_activations(M, K, seed=M + K, dtype=H)
        r = wq_ref.exact_residual(M, N, seed=M + N) if use_res else None
        ad, rd = a.cuda(), (r.cuda() if use_res else None)
        No = N // 2 if epi == ops.EPI_SWIGLU else N
        dt = H if od is None else od
        buf, out = _guarded(M, No, dt)
        buf2, out2 = _guarded(M, No, dt)
        ops.wq_gemv(ad, qd, sd, residual=rd, epilogue=epi, out=out)
        ops.gemv(ad, wd, residual=rd, epilogue=epi, out=out2)
        tag = (N, K, M, epi, str(dt), use_res)
        assert torch.equal(_bits(out), _bits(out2)), tag
        assert _guards_intact(buf, M, No), tag
        if epi == ops.EPI_NONE:
            ref = a.to(torch.float64) @ w64.T
            if use_res:
                ref = ref + r.to(torch.float64)
            ref = ref.to(torch.float32).to(dt)                 # (exact in fp32: integer multiples of 2^e below 2^24 * 2^e)
            assert torch.equal(_bits(out.cpu()), _bits(ref)), tag
    # one case through non-contiguous activations and residual (rows of wider buffers)
    M = 5
    a = wq_ref.exact_activations(M, K, seed=99, dtype=H)
    r = wq_ref.exact_residual(M, N, seed=98)
    abig = torch.zeros((M, K + 8), dtype=H, device="cuda")
    rbig = torch.zeros((M, N + 5), dtype=torch.float32, device="cuda")
    abig[:, :K], rbig[:, :N] = a.cuda(), r.cuda()
    buf, out = _guarded(M, N, H)
    ops.wq_gemv(abig[:, :K], qd, sd, residual=rbig[:, :N], out=out)
    ref = (a.to(torch.float64) @ w64.T + r.to(torch.float64)).to(torch.float32).to(H)
    assert torch.equal(_bits(out.cpu()), _bits(ref)) and _guards_intact(buf, M, N)


def _half_ulp(y, dt):
    """Half an ulp of ``dt`` at the real value y (float64 tensor)."""
    mant, emin = {torch.float32: (23, -126), torch.bfloat16: (7, -126), torch.float16: (10, -14)}[dt]
    e = torch.floor(torch.log2(y.abs().clamp_min(2.0 ** -140))).clamp_min(emin)
    return torch.pow(torch.tensor(2.0, dtype=torch.float64), e - mant - 1)


def gemv_random(N, K):
    """Gaussian activations, random q and fp32 scales against float64: |err| <= (K + 4) 2^-24 s_n sum_k |a q| + half an ulp of the
    output type at the true value (any fp32 summation order, then one output rounding); EPI_NONE, both output types, with and
    without residual (the bound is the linear form's)."""
    from valley_amd import ops
    H = _half()
    g = torch.Generator().manual_seed(5 * N + K)
    q = torch.randint(-127, 128, (N, K), generator=g, dtype=torch.int32).to(torch.int8)
    s = (torch.rand((N,), generator=g) + 0.5) * 1e-3
    for M in (1, 2, 3, 8):
        a = torch.randn((M, K), generator=g).to(H)
        r = torch.randn((M, N), generator=g) * 0.05
        prod = a.to(torch.float64)[:, None, :] * q.to(torch.float64)[None]                # [M, N, K]
        y = prod.sum(-1) * s.to(torch.float64)
        mag = prod.abs().sum(-1) * s.to(torch.float64)
        for od, use_res in itertools.product((None, torch.float32), (False, True)):
            dt = H if od is None else od
            out = ops.wq_gemv(a.cuda(), q.cuda(), s.cuda(), residual=r.cuda() if use_res else None, out_dtype=dt)
            ref = y + r.to(torch.float64) if use_res else y
            bound = (K + 4) * 2.0 ** -24 * mag + _half_ulp(ref, dt)
            err = (out.cpu().to(torch.float64) - ref).abs()
            assert bool((err <= bound).all()), (N, K, M, str(dt), use_res, float((err / bound).max()))


def row_independence(N, K):
    """Row 0's output bits for M = 1 .. 8, whatever the other rows hold."""
    from valley_amd import ops
    H = _half()
    g = torch.Generator().manual_seed(N + K)
    q = torch.randint(-127, 128, (N, K), generator=g, dtype=torch.int32).to(torch.int8).cuda()
    s = ((torch.rand((N,), generator=g) + 0.5) * 1e-3).cuda()
    row0 = torch.randn((1, K), generator=g).to(H)
    for epi in (ops.EPI_NONE, ops.EPI_SWIGLU):
        first = None
        for M in range(1, 9):
            a = torch.cat([row0, (torch.randn((M - 1, K), generator=g) * (M + 1)).to(H)], 0).cuda()
            out = ops.wq_gemv(a, q, s, epilogue=epi)
            first = out[0].clone() if first is None else first
            assert torch.equal(_bits(out[0]), _bits(first)), (N, K, M, epi)


def fused_norm():
    """wq_gemv_rmsnorm == rmsnorm + wq_gemv bit for bit; refused outside its range without a launch."""
    from valley_amd import lib, ops
    H = _half()
    g = torch.Generator().manual_seed(77)
    # N = 11008 at K = 2048: 5504 row pairs, more than the resident workgroups take in one trip (8 pairs each, at most two workgroups
    # per CU), so the grid is capped and waves go round the pair loop again on rows that the register prefetch loaded a trip earlier
    for M, K, N in list(itertools.product((1, 2), (2048, 4112, 6144), (6, 34))) + [(1, 2048, 11008), (2, 2048, 11008)]:
        q = torch.randint(-127, 128, (N, K), generator=g, dtype=torch.int32).to(torch.int8).cuda()
        s = ((torch.rand((N,), generator=g) + 0.5) * 1e-3).cuda()
        h = (torch.randn((M, K), generator=g) * 3).cuda()
        gamma = (torch.rand((K,), generator=g) + 0.5).cuda()
        r = torch.randn((M, N), generator=g).cuda()
        x = ops.rmsnorm(h, gamma, 1e-5)
        for epi, od, use_res in _combos():
            No = N // 2 if epi == ops.EPI_SWIGLU else N
            dt = H if od is None else od
            buf, out = _guarded(M, No, dt)
            ops.wq_gemv_rmsnorm(h, gamma, 1e-5, q, s, residual=r if use_res else None, epilogue=epi, out=out)
            ref = ops.wq_gemv(x, q, s, residual=r if use_res else None, epilogue=epi, out_dtype=dt)
            assert torch.equal(_bits(out), _bits(ref)), (M, K, N, epi, str(dt), use_res)
            assert _guards_intact(buf, M, No)
    assert not ops.wq_gemv_rmsnorm_ok(3, 4096) and not ops.wq_gemv_rmsnorm_ok(1, 2032) and not ops.wq_gemv_rmsnorm_ok(1, 6160)
    for M, K in ((3, 4096), (1, 2032), (1, 6160)):
        q = torch.zeros((6, K), dtype=torch.int8, device="cuda")
        s = torch.ones((6,), device="cuda")
        buf, out = _guarded(M, 6, H)
        try:
            ops.wq_gemv_rmsnorm(torch.ones((M, K), device="cuda"), torch.ones((K,), device="cuda"), 1e-5, q, s, out=out)
        except lib.ValleyHipError as e:
            assert "vly_wq_gemv_rmsnorm" in str(e) and "unsupported" in str(e)
        else:
            raise AssertionError(f"vly_wq_gemv_rmsnorm took M={M} K={K}")
        torch.cuda.synchronize()
        assert bool((buf == SENT).all())


def rejected_shapes():
    from valley_amd import lib, ops
    H = _half()
    for M, N, K, epi in ((1, 6, 24, ops.EPI_NONE), (9, 6, 32, ops.EPI_NONE), (2, 7, 32, ops.EPI_SWIGLU)):
        a = torch.ones((M, K), dtype=H, device="cuda")
        q = torch.ones((N, K), dtype=torch.int8, device="cuda")
        s = torch.ones((N,), device="cuda")
        No = N // 2 if epi == ops.EPI_SWIGLU else N
        buf = torch.full((M + 1, No + 3), SENT, dtype=H, device="cuda")
        try:
            ops.wq_gemv(a, q, s, epilogue=epi, out=buf[:M, :No])
        except lib.ValleyHipError as e:
            assert "vly_wq_gemv" in str(e) and len(str(e)) > 40, str(e)
        else:
            raise AssertionError(f"vly_wq_gemv took M={M} N={N} K={K} epi={epi}")
        torch.cuda.synchronize()
        assert bool((buf == SENT).all())


def run_all():
    quantizer_exact()
    quantizer_random()
    for (N, K) in wq_ref.SHAPES:
        gemv_exact(N, K)
        gemv_random(N, K)
        row_independence(N, K)
    fused_norm()
    rejected_shapes()
