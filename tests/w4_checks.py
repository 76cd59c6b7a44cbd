"""Kernel-level checks of libvalley_hip_w4.so on the bound 16-bit storage type (runtime.HALF): called by tests/test_w4_gpu.py on
the bf16 library and by tests/w4_worker.py in a child process on the fp16 library.  Every function asserts; none returns."""
import itertools

import torch

from tests import w4_ref
from tests.wq_checks import SENT, _bits, _guarded, _guards_intact, _half, _half_ulp


def quantizer_exact():
    from valley_amd import ops
    for (N, K) in w4_ref.QUANT_SHAPES:
        w, q, s = w4_ref.exact_weights(N, K, seed=100 + N, dtype=_half())
        gq, gs = ops.w4_quantize(w.cuda())
        assert gq.dtype == torch.uint8 and tuple(gq.shape) == (N, K // 2) and tuple(gs.shape) == (N, K // 128)
        assert torch.equal(_bits(gs.cpu()), _bits(s)), (N, K)
        assert torch.equal(w4_ref.unpack(gq), q) and torch.equal(gq.cpu(), w4_ref.pack(q)), (N, K)
    # all-zero groups between live ones: s = 1, q = 0 there
    w, q, s = w4_ref.exact_weights(3, 512, seed=5, dtype=_half())
    w[:, 128:256] = 0
    w[1] = 0
    gq, gs = ops.w4_quantize(w.cuda())
    rq, rs = w4_ref.quantize_ref(w)
    assert torch.equal(w4_ref.unpack(gq), rq) and torch.equal(_bits(gs.cpu()), _bits(rs))
    assert bool((gs.cpu()[:, 1] == 1.0).all()) and bool((gs.cpu()[1] == 1.0).all()) and int(w4_ref.unpack(gq)[1].abs().max()) == 0
    # a strided source (rows of a wider buffer)
    w, q, s = w4_ref.exact_weights(6, 1152, seed=7, dtype=_half())
    big = torch.zeros((6, 1160), dtype=_half(), device="cuda")
    big[:, :1152] = w.cuda()
    gq, gs = ops.w4_quantize(big[:, :1152])
    assert torch.equal(w4_ref.unpack(gq), q) and torch.equal(_bits(gs.cpu()), _bits(s))


def quantizer_random(seed=12):
    """Random rows: the scale bit for bit and q equal to the CPU reference EVERYWHERE (no element of these rows is within 2^-16 of
    a rounding tie — asserted on the CPU first — and the two fp32 roundings move w / s by far less)."""
    from valley_amd import ops
    for (N, K) in w4_ref.QUANT_SHAPES:
        w = w4_ref.random_rows(N, K, seed + K, _half())
        q, s = w4_ref.quantize_ref(w)
        dist = float(w4_ref.tie_distance(w, s).min())
        print(f"w4 quantizer ({N}, {K}): smallest distance to a rounding tie {dist:.3e}")
        assert dist >= 2.0 ** -16, "the reference rows hold a near-tie: pick another seed"
        gq, gs = ops.w4_quantize(w.cuda())
        gq, gs = w4_ref.unpack(gq), gs.cpu()
        assert torch.equal(_bits(gs), _bits(s)), (N, K)
        assert torch.equal(gq, q), (N, K, int((gq != q).sum()))
        assert int(gq.min()) >= -7


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
    w, q, s = w4_ref.exact_weights(N, K, seed=3 * N + K, dtype=H)
    wd, qd, sd = w.cuda(), w4_ref.pack(q).cuda(), s.cuda()
    w64 = q.to(torch.float64) * w4_ref.expand(s).to(torch.float64)
    for M, (epi, od, use_res) in itertools.product(range(1, 9), _combos()):
        a = w4_ref.exact_activations(M, K, seed=M + K, dtype=H)
        r = w4_ref.exact_residual(M, N, seed=M + N) if use_res else None
        ad, rd = a.cuda(), (r.cuda() if use_res else None)
        No = N // 2 if epi == ops.EPI_SWIGLU else N
        dt = H if od is None else od
        buf, out = _guarded(M, No, dt)
        buf2, out2 = _guarded(M, No, dt)
        ops.w4_gemv(ad, qd, sd, residual=rd, epilogue=epi, out=out)
        ops.gemv(ad, wd, residual=rd, epilogue=epi, out=out2)
        tag = (N, K, M, epi, str(dt), use_res)
        assert torch.equal(_bits(out), _bits(out2)), tag
        assert _guards_intact(buf, M, No), tag
        if epi == ops.EPI_NONE:
            ref = a.to(torch.float64) @ w64.T
            if use_res:
                ref = ref + r.to(torch.float64)
            ref = ref.to(torch.float32).to(dt)                 # (exact in fp32: integer multiples of 2^-8 below 2^16)
            assert torch.equal(_bits(out.cpu()), _bits(ref)), tag
    # one case through non-contiguous activations and residual (rows of wider buffers)
    M = 5
    a = w4_ref.exact_activations(M, K, seed=99, dtype=H)
    r = w4_ref.exact_residual(M, N, seed=98)
    abig = torch.zeros((M, K + 8), dtype=H, device="cuda")
    rbig = torch.zeros((M, N + 5), dtype=torch.float32, device="cuda")
    abig[:, :K], rbig[:, :N] = a.cuda(), r.cuda()
    buf, out = _guarded(M, N, H)
    ops.w4_gemv(abig[:, :K], qd, sd, residual=rbig[:, :N], out=out)
    ref = (a.to(torch.float64) @ w64.T + r.to(torch.float64)).to(torch.float32).to(H)
    assert torch.equal(_bits(out.cpu()), _bits(ref)) and _guards_intact(buf, M, N)


def gemv_random(N, K):
    """Gaussian activations, random q and fp32 scales against float64:
    |err| <= (K + 4) 2^-24 sum_k s_g |a| (|q| + c) + half an ulp of the output type at the true value, c the header's offset
    (any fp32 order over at most K + 4 roundings per term, then one output rounding); EPI_NONE, both output types, with and
    without residual."""
    from valley_amd import ops
    H = _half()
    c = w4_ref.OFFSET[H]
    g = torch.Generator().manual_seed(5 * N + K)
    q, packed, s = w4_ref.random_quantized(N, K, g)
    s64 = w4_ref.expand(s).to(torch.float64)
    for M in (1, 2, 3, 8):
        a = torch.randn((M, K), generator=g).to(H)
        r = torch.randn((M, N), generator=g) * 0.05
        a64 = a.to(torch.float64)
        y = a64 @ (q.to(torch.float64) * s64).T
        mag = a64.abs() @ ((q.to(torch.float64).abs() + c) * s64).T
        for od, use_res in itertools.product((None, torch.float32), (False, True)):
            dt = H if od is None else od
            out = ops.w4_gemv(a.cuda(), packed.cuda(), s.cuda(), residual=r.cuda() if use_res else None, out_dtype=dt)
            ref = y + r.to(torch.float64) if use_res else y
            bound = (K + 4) * 2.0 ** -24 * mag + _half_ulp(ref, dt)
            err = (out.cpu().to(torch.float64) - ref).abs()
            print(f"w4 gemv random ({N}, {K}) M={M} {dt} res={use_res}: max err / bound {float((err / bound).max()):.3e}")
            assert bool((err <= bound).all()), (N, K, M, str(dt), use_res, float((err / bound).max()))


def row_independence(N, K):
    """Row 0's output bits for M = 1 .. 8, whatever the other rows hold."""
    from valley_amd import ops
    H = _half()
    g = torch.Generator().manual_seed(N + K)
    _q, packed, s = w4_ref.random_quantized(N, K, g)
    packed, s = packed.cuda(), s.cuda()
    row0 = torch.randn((1, K), generator=g).to(H)
    for epi in (ops.EPI_NONE, ops.EPI_SWIGLU):
        first = None
        for M in range(1, 9):
            a = torch.cat([row0, (torch.randn((M - 1, K), generator=g) * (M + 1)).to(H)], 0).cuda()
            out = ops.w4_gemv(a, packed, s, epilogue=epi)
            first = out[0].clone() if first is None else first
            assert torch.equal(_bits(out[0]), _bits(first)), (N, K, M, epi)


def fused_norm():
    """w4_gemv_rmsnorm == rmsnorm + w4_gemv bit for bit; refused outside its range without a launch."""
    from valley_amd import lib, ops
    H = _half()
    g = torch.Generator().manual_seed(77)
    # N = 11008 at K = 2048: 5504 row pairs, more than the resident workgroups take in one trip (8 pairs each, two workgroups per
    # CU), so the grid is capped and waves go round the pair loop again on rows that the register prefetch loaded a trip earlier
    for M, K, N in list(itertools.product((1, 2), (2048, 4224, 6144), (6, 34))) + [(1, 2048, 11008), (2, 2048, 11008)]:
        _q, packed, s = w4_ref.random_quantized(N, K, g)
        packed, s = packed.cuda(), s.cuda()
        h = (torch.randn((M, K), generator=g) * 3).cuda()
        gamma = (torch.rand((K,), generator=g) + 0.5).cuda()
        r = torch.randn((M, N), generator=g).cuda()
        x = ops.rmsnorm(h, gamma, 1e-5)
        for epi, od, use_res in _combos():
            No = N // 2 if epi == ops.EPI_SWIGLU else N
            dt = H if od is None else od
            buf, out = _guarded(M, No, dt)
            ops.w4_gemv_rmsnorm(h, gamma, 1e-5, packed, s, residual=r if use_res else None, epilogue=epi, out=out)
            ref = ops.w4_gemv(x, packed, s, residual=r if use_res else None, epilogue=epi, out_dtype=dt)
            assert torch.equal(_bits(out), _bits(ref)), (M, K, N, epi, str(dt), use_res)
            assert _guards_intact(buf, M, No)
    assert not ops.w4_gemv_rmsnorm_ok(3, 4096) and not ops.w4_gemv_rmsnorm_ok(1, 1920) and not ops.w4_gemv_rmsnorm_ok(1, 6272)
    for M, K in ((3, 4096), (1, 1920), (1, 6272)):
        packed = torch.full((6, K // 2), 0x88, dtype=torch.uint8, device="cuda")
        s = torch.ones((6, K // 128), device="cuda")
        buf, out = _guarded(M, 6, H)
        try:
            ops.w4_gemv_rmsnorm(torch.ones((M, K), device="cuda"), torch.ones((K,), device="cuda"), 1e-5, packed, s, out=out)
        except lib.ValleyHipError as e:
            assert "vly_w4_gemv_rmsnorm" in str(e) and "unsupported" in str(e)
        else:
            raise AssertionError(f"vly_w4_gemv_rmsnorm took M={M} K={K}")
        torch.cuda.synchronize()
        assert bool((buf == SENT).all())


def rejected_shapes():
    from valley_amd import lib, ops
    H = _half()
    for M, N, K, epi in ((1, 6, 192, ops.EPI_NONE), (9, 6, 256, ops.EPI_NONE), (2, 7, 256, ops.EPI_SWIGLU)):
        a = torch.ones((M, K), dtype=H, device="cuda")
        packed = torch.full((N, K // 2), 0x99, dtype=torch.uint8, device="cuda")
        s = torch.ones((N, K // 128), device="cuda")
        No = N // 2 if epi == ops.EPI_SWIGLU else N
        buf = torch.full((M + 1, No + 3), SENT, dtype=H, device="cuda")
        try:
            ops.w4_gemv(a, packed, s, epilogue=epi, out=buf[:M, :No])
        except lib.ValleyHipError as e:
            assert "vly_w4_gemv" in str(e) and len(str(e)) > 40, str(e)
        else:
            raise AssertionError(f"vly_w4_gemv took M={M} N={N} K={K} epi={epi}")
        torch.cuda.synchronize()
        assert bool((buf == SENT).all())
    w = torch.ones((4, 192), dtype=H, device="cuda")                    # the quantizer: K % 128
    try:
        ops.w4_quantize(w)
    except lib.ValleyHipError as e:
        assert "vly_w4_quantize_rows" in str(e)
    else:
        raise AssertionError("vly_w4_quantize_rows took K=192")


def run_all():
    quantizer_exact()
    quantizer_random()
    for (N, K) in w4_ref.SHAPES:
        gemv_exact(N, K)
        gemv_random(N, K)
        row_independence(N, K)
    fused_norm()
    rejected_shapes()
