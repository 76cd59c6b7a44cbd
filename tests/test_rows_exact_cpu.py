"""The row oracle is right and it bites (tests/row_oracle.py; no GPU).  Every kernel is emulated in torch on the CPU in its own fp32
order (lane partials, the 64-lane butterfly, the four waves of the row kernel; frames added in order; fl(1 / T) multiplied in) and the
emulation passes the oracle; one mutation per check does not: a one-pass variance on the mean-1000 row, a truncating store, the two
deltas added in the other order, the CLS row of the next frame, the last chunk of H = 520 dropped, a write into the first guard
row, a mean over T - 1, x_all left untransposed, the other clip's CLS rows, a key rotated into the next cache row.  The grid cases are
shown to be exact in any order, the 1e-3 cap to hold for the torch fp32 formula on every norm shape, the dispatch mirror to agree with
launch_norm's text — and the one place where the oracle had to be mended is shown: one 16-bit ulp alone cannot hold at outputs near
zero, for the torch fp32 formula either."""
import pytest
import torch

from tests import row_oracle as R

HALVES = [torch.bfloat16, torch.float16]
IDS = ["bf16", "fp16"]


def fails(fn, *a, **k) -> bool:
    try:
        fn(*a, **k)
    except AssertionError:
        return True
    return False


def cpu_case(branch, M, D, half) -> R.NormCase:
    """The large-M shapes on a 130-row slice (the rows repeat with period 131 anyway); the kernel the emulation follows is the
    branch's."""
    return R.NormCase(min(M, 130), D, half)


# ---- the dispatch mirror ----------------------------------------------------------------------------------------------------------------
def test_dispatch_mirror_is_launch_norms_condition():
    src = R.norm_dispatch_in_source()
    assert src["row"] == (64, 2048, 4096) and src["ladder"] == [(4, 4), (8, 8), (16, 16), (20, 20)] and src["last"] == 32
    assert src["nv"] and src["limits"] and src["rows_per_block"] == R.ROWS_PER_BLOCK == 2
    for M in (1, 64, 65, 4096, 4097):
        for D in range(4, 8193, 4):
            row = M <= src["row"][0] or (D >= src["row"][1] and M <= src["row"][2])
            nv = (D // 4 + 63) // 64
            want = "row" if row else "norm_kernel<%d>" % next((k for n, k in src["ladder"] if nv <= n), src["last"])
            assert R.norm_branch(M, D) == want, (M, D)
    seen = set()
    for branch, M, D in R.NORM_SHAPES:
        assert R.norm_branch(M, D) == branch
        seen.add(branch)
        if branch != "row":
            assert M % R.ROWS_PER_BLOCK == 1                                    # the last block holds one row
    assert seen == {"row", "norm_kernel<4>", "norm_kernel<8>", "norm_kernel<16>", "norm_kernel<20>", "norm_kernel<32>"}
    assert all(any(D % 256 for b, _m, D in R.NORM_SHAPES if b == br) for br in seen)       # a partial tail on every branch


# ---- norms ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("half", HALVES, ids=IDS)
@pytest.mark.parametrize("branch,M,D", R.NORM_SHAPES, ids=[f"{b}-{M}x{D}" for b, M, D in R.NORM_SHAPES])
def test_norm_emulation_passes_and_mutations_fail(branch, M, D, half):
    case = cpu_case(branch, M, D, half)
    threads = 256 if branch == "row" else 64
    for form in R.NORM_FORMS:
        R.check_norm(case, form, *R.emu_norm(case, form, threads))
        if form.endswith("only"):
            if form == "add2_only":
                assert fails(R.check_norm, case, form, *R.emu_norm(case, form, threads, swap=True))
            continue
        assert fails(R.check_norm, case, form, *R.emu_norm(case, form, threads, trunc=True)), f"{form}: a truncating store passes"
        if form.startswith("add2"):
            assert fails(R.check_norm, case, form, *R.emu_norm(case, form, threads, swap=True)), f"{form}: (h + d1) + d0 passes"
        if not form.endswith("rms") and "big" in case.planted:
            assert fails(R.check_norm, case, form, *R.emu_norm(case, form, threads, one_pass=True)), f"{form}: a one-pass variance passes"


@pytest.mark.parametrize("half", HALVES, ids=IDS)
def test_the_order_of_the_two_deltas_matters_where_it_was_planted(half):
    case = R.NormCase(5, 8, half)
    r = case.order_row
    h, d0, d1 = case.xu[r, 0], case.d0u[r, 0].float(), case.d1u[r, 0].float()
    assert float((h + d0) + d1) == 1.0 + 2.0 ** -23 and float((h + d1) + d0) == 1.0 + 2.0 ** -22
    good = R.emu_norm(case, "add2_only", 64)[0]
    bad = R.emu_norm(case, "add2_only", 64, swap=True)[0]
    row = int((case.idx == r).nonzero()[0])
    assert float(good[row, 0]) != float(bad[row, 0])


@pytest.mark.parametrize("half", HALVES, ids=IDS)
def test_the_cap_holds_for_the_torch_fp32_formula_on_every_norm_shape(half):
    worst = 0.0
    for branch, M, D in R.NORM_SHAPES:
        case = cpu_case(branch, M, D, half)
        for form in ("ln16+32", "rms", "add_ln", "add2_rms"):
            x = case.h_after(form)
            x = (case.xu if x is None else x)[case.idx]
            y = R.rms32(x, case.gamma, R.RMS_EPS) if form.endswith("rms") else R.ln32(x, case.gamma, case.beta, R.LN_EPS)
            res = R.check_norm(case, form, x if form.startswith("add") else None, y.to(half), y if form == "ln16+32" else None)
            worst = max(worst, res["share"])
            assert res["share"] <= 0.5 * R.CAP, (M, D, form, res)
    print("largest share of elements differing from ref64.to(HALF):", worst)


def test_one_ulp_alone_cannot_hold_near_zero():
    """Why check_norm adds the fp32 rule's bound to the ulp: the torch fp32 LayerNorm, rounded once, is more than one 16-bit ulp
    from ref64.to(HALF) at some output — and only at outputs below 1e-3, where the ulp is below any fp32 evaluation's error."""
    hits = []
    for M, D in ((64, 8192), (70, 2048), (130, 5120)):
        for half in HALVES:
            case = R.NormCase(M, D, half)
            ref = R.ln64(case.xu, case.gamma, case.beta, R.LN_EPS)
            got = R.ln32(case.xu, case.gamma, case.beta, R.LN_EPS).to(half)
            want = ref.to(half)
            miss = (got.double() - want.double()).abs() > R.ulp(want.double(), half)
            hits += want[miss].abs().tolist()
    print(len(hits), "elements miss one ulp; the largest has magnitude", max(hits) if hits else None)
    assert hits and max(hits) < 1e-3


def test_planted_rows_and_the_rules_numbers():
    case = R.NormCase(70, 2048, torch.bfloat16)
    assert set(case.planted) == {"big", "zero", "last", "const"} and len(set(case.planted.values())) == 4
    x = case.xu[case.idx]
    assert bool((x[case.planted["zero"]] == 0).all()) and bool((x[case.planted["const"]] == 7.25).all())
    last = x[case.planted["last"]]
    assert float(last[-1]) != 0 and bool((last[:-1] == 0).all())
    big = x[case.planted["big"]]
    assert float(big.double().mean()) == 1000.0 and 0.9 < float(big.double().std()) < 1.3
    for perm in (torch.arange(2048), torch.arange(2048).flip(0), torch.randperm(2048)):      # its sums are exact in any order
        s = torch.zeros(())
        for v in big[perm]:
            s = s + v
        assert float(s) == 2048000.0
    for form in ("add_ln", "add2_rms"):
        assert float(case.h_after(form)[case.urow["big"]].double().mean()) == 1000.0
    _, e, eb = case.truth("ln16")
    assert 1e-7 < e < 5e-6 and 0 < eb < 2.5e-6
    assert R.NormCase(1, 4, torch.float16).planted == {} and list(R.NormCase(3, 1028, torch.float16).planted) == ["big", "zero"]
    for M, D in R.NORM_F32_SHAPES:
        c = R.NormCase(M, D, torch.bfloat16)
        form = "ln16"
        ref, e, eb = c.truth(form)
        y = R.ln32(c.xu, c.gamma, c.beta, R.LN_EPS)[c.idx]
        R.assert_f32(y, ref[c.idx], R.f32_bounds(c, e, eb, "cpu"), "torch fp32")
        Kp = (D + 63) // 64 * 64 + 64
        hi = y.to(torch.bfloat16)
        lo = (y - hi.float()).to(torch.bfloat16)
        o3 = torch.zeros((M, 3 * Kp), dtype=torch.bfloat16)
        o3[:, :D], o3[:, Kp:Kp + D], o3[:, 2 * Kp:2 * Kp + D] = hi, hi, lo
        R.split3_check(o3, ref[c.idx], D, Kp, max(e, eb), "split3 emulation")
        o3[:, 2 * Kp:2 * Kp + D] = 0
        assert fails(R.split3_check, o3, ref[c.idx], D, Kp, max(e, eb), "lo dropped")
        o3[:, 2 * Kp:2 * Kp + D] = lo
        o3[0, D] = 1.0
        assert fails(R.split3_check, o3, ref[c.idx], D, Kp, max(e, eb), "pad written")


# ---- guards ---------------------------------------------------------------------------------------------------------------------------
def test_a_write_into_the_first_guard_row_is_seen():
    for H in R.SPLICE_H:
        emb, vis = R.splice_tables(H, torch.bfloat16)
        rmap = R.splice_map(5)
        R.assert_guards(R.emu_splice(rmap, emb, vis), 5, H, "clean")
        assert fails(R.assert_guards, R.emu_splice(rmap, emb, vis, stray=True), 5, H, "stray")
    buf, view = R.guarded(3, 12, torch.bfloat16, device="cpu")
    assert buf.shape == (6, 24) and view.shape == (3, 12)
    buf[1, 12] = 0
    assert fails(R.assert_guards, buf, 3, 12, "guard column")


# ---- RoPE ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("half", HALVES + [torch.float32], ids=IDS + ["f32"])
@pytest.mark.parametrize("shape", R.ROPE_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_rope_emulation_passes_and_mutations_fail(shape, half):
    B, S, heads, past, ctx_max = shape
    qkv0 = R.rope_inputs(B, S, heads, half)
    R.check_rope(shape, qkv0, *R.emu_rope(shape, qkv0, past), past)
    assert S * heads * B * 8 % 256 != 0 or shape != R.ROPE_SHAPES[2]            # 528 lane-units: a partial last block
    if past + S < ctx_max:
        assert fails(R.check_rope, shape, qkv0, *R.emu_rope(shape, qkv0, past, off_rows=1), past)     # the next cache row
    if past > 0:
        assert fails(R.check_rope, shape, qkv0, *R.emu_rope(shape, qkv0, past - 1), past)             # rotated by the wrong position
    q, kc, vc = R.emu_rope(shape, qkv0, past)
    kc[B - 1, heads - 1, (past + S) % ctx_max if past + S < ctx_max else 0, 127] = 0.0                # one element outside the rows
    if ctx_max > S:
        assert fails(R.check_rope, shape, qkv0, q, kc, vc, past)
    q, kc, vc = R.emu_rope(shape, qkv0, past)
    vc[0, 0, past, 5] = vc[0, 0, past, 6]                                                             # v not copied exactly
    assert fails(R.check_rope, shape, qkv0, q, kc, vc, past)
    if half != torch.float32:
        q, kc, vc = R.emu_rope(shape, qkv0, past)
        k = kc[:, :, past:past + S]
        kc[:, :, past:past + S] = torch.where(k > 0, torch.nextafter(torch.nextafter(k, k * 2), k * 2), k)   # two ulps up
        assert fails(R.check_rope, shape, qkv0, q, kc, vc, past)
    # the device position's clamp, as the kernel computes it
    assert min(ctx_max + 1000, ctx_max - S) == ctx_max - S and all(s[3] + s[1] <= s[4] for s in R.ROPE_SHAPES)


# ---- pooling, scores --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("half", HALVES + [torch.float32], ids=IDS + ["f32"])
@pytest.mark.parametrize("B,T,W", R.POOL_SHAPES)
def test_pool_emulation_passes_and_mutations_fail(B, T, W, half):
    feats = R.pool_feats(B, T, W)
    sc = R.pool_scores(B, T)
    assert float(sc.max()) == 40.0 and (T == 1 or float(sc.min()) == -40.0)
    for mode in (R.POOL_MEAN, R.POOL_MAX, R.POOL_IMPORTANCE):
        s = sc if mode == R.POOL_IMPORTANCE else None
        R.check_pool(feats, mode, s, R.emu_pool(feats, mode, s, half))
        if T > 1:
            assert fails(R.check_pool, feats, mode, s, R.emu_pool(feats, mode, s, half, cls_shift=1)), "the next frame's CLS row passes"
        if half != torch.float32 and mode == R.POOL_MEAN:                       # (where the mean is a storage number, truncation is the identity)
            bad = R.emu_pool(feats, mode, s, half, trunc=True)
            if not torch.equal(bad, R.emu_pool(feats, mode, s, half)):
                assert fails(R.check_pool, feats, mode, s, bad), "a truncating store passes"
            else:
                assert T in (1, 2) or half == torch.bfloat16 and T == 1
    if T > 1:
        assert fails(R.check_pool, feats, R.POOL_MEAN, None, R.emu_pool(feats, R.POOL_MEAN, None, half, mean_div=T - 1)), "a mean over T - 1 passes"
    # the grid makes the mean's sum exact in any order: forwards, backwards and pairwise agree with float64
    p = feats[:, :, 1:]
    fwd = sum(p[:, t] for t in range(T))
    bwd = sum(p[:, t] for t in reversed(range(T)))
    assert torch.equal(fwd.double(), p.double().sum(1)) and torch.equal(bwd, fwd) and torch.equal(p.sum(1), fwd)
    assert (B * (256 + T) * (W // 4)) % 256 != 0 or (B, T, W) != (1, 3, 12)


@pytest.mark.parametrize("with_bias", [True, False])
@pytest.mark.parametrize("F,W", R.SCORE_SHAPES)
def test_scores_are_exact_in_any_order(F, W, with_bias):
    feats, w, bias, truth = R.score_case(F, W, with_bias)                      # (asserts the partial-sum bound)
    x = feats[:, 1:].reshape(F, -1)
    b = bias if with_bias else torch.zeros(1)
    prod = x * w
    assert torch.equal((x.double() * w.double()).float(), prod)
    for order in (torch.arange(256 * W), torch.arange(256 * W).flip(0), torch.randperm(256 * W)):
        lanes = prod[:, order].reshape(F, -1, 4).sum(-1)                        # float4 dot, then strided lane partials, then the rest
        pad = (-lanes.shape[1]) % 1024
        part = torch.nn.functional.pad(lanes, (0, pad)).view(F, -1, 1024).sum(1)
        assert torch.equal((part.sum(1) + b).double(), truth) and torch.equal((b + part.flip(1).cumsum(1)[:, -1]).double(), truth)
    n4 = 64 * W
    assert (W == 68) == (0 < n4 - 4096 < 1024) and (W == 4) == (n4 < 1024)      # W = 68: the four-way loop once, then the tail


# ---- splice, cast, patchify, ViT embedding ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H", R.SPLICE_H)
def test_splice_cases_and_the_dropped_chunk(H):
    for half in HALVES + [torch.float32]:
        emb, vis = R.splice_tables(H, half)
        for R_ in R.SPLICE_R:
            rmap = R.splice_map(R_)
            want = R.splice_truth(rmap, emb, vis)
            R.assert_bits(R.emu_splice(rmap, emb, vis)[:R_], want, "emulation")
            assert fails(R.assert_bits, R.emu_splice(rmap, emb, vis, drop_last_chunk=True)[:R_], want, "dropped chunk")
            assert not (R.splice_map(R_, tokens_only=True) < 0).any()
    m = R.splice_map(9).tolist()
    V, NV = R.SPLICE_V, R.SPLICE_NV
    assert {0, V - 1, -1, -NV} <= set(m) and m.count(V - 1) == 2 and m.count(-NV) == 2
    assert (520 // 8) == 65 and {len(R.splice_map(r)) for r in R.SPLICE_R} == {1, 4, 5, 9}


@pytest.mark.parametrize("half", HALVES, ids=IDS)
def test_cast_values_hold_the_edges_and_truncation_fails(half):
    fi = torch.finfo(half)
    for n in (8, 2056):
        x = R.cast_values(n, half)
        y = x.to(half)
        assert x.numel() == n and bool(torch.isnan(y).any()) and bool(torch.isinf(y[~torch.isinf(x)]).any())
        R.assert_bits(y, x.to(half), "cast")
        assert fails(R.assert_bits, R.truncate(x, half), y, "truncation")
    x = R.cast_values(2056, half)
    y = x.to(half).float()
    one = float(torch.tensor(1.0 + fi.eps))
    assert float(y[0]) == 1.0 and float(y[1]) == one + fi.eps and float(y[2]) == -1.0       # ties: to even, down and up
    assert float(y[4]) == one and float(y[5]) == 1.0                                        # just above / below the tie
    assert float(y[6]) == fi.max and float(y[8]) == float("inf") and float(y[9]) == fi.max  # the first value that overflows, the last that does not
    assert str(float(y[11])) == "-0.0" and (2056 // 8) % 256 == 1
    if half == torch.float16:
        assert float(y[16]) == 2.0 ** -24 and float(y[17]) == 0.0 and float(y[19]) == 2.0 ** -24 and float(y[20]) == 2.0 ** -23


@pytest.mark.parametrize("F", [1, 3])
def test_patchify_truth_is_the_convolutions_unfold(F):
    for dtype, kp in ((torch.float32, 592), (torch.bfloat16, 640), (torch.float16, 640)):
        img = R.patch_image(F, dtype)
        cols = torch.nn.functional.unfold(R.patch_image(F, torch.float32), kernel_size=14, stride=14).transpose(1, 2).reshape(F * 256, 588)
        out = torch.zeros((F * 256, kp), dtype=torch.float32)
        out[:, :588] = cols
        if dtype != torch.float32:
            v = out.long() & 0xFFFF
            o16 = (v - ((v & 0x8000) << 1)).to(torch.int16).view(dtype).clone()
            o16[:, 588:] = 0
            out = o16
            assert torch.equal(img.view(torch.int16).long() & 0xFFFF, torch.arange(img.numel()).view(img.shape) & 0xFFFF)
        R.check_patchify(out, F)
        bad = out.clone()
        bad[:, 0:14], bad[:, 14:28] = out[:, 14:28], out[:, 0:14]                            # two kernel rows swapped
        assert fails(R.check_patchify, bad, F)
        bad = out.clone()
        bad[F * 256 - 1, kp - 1] = 1.0
        assert fails(R.check_patchify, bad, F)
        bad = out.roll(1, 0)                                                                 # every patch one row late
        assert fails(R.check_patchify, bad, F)


@pytest.mark.parametrize("F", [1, 3])
def test_vit_embed_emulation_passes_and_mutations_fail(F):
    po, cls, pos, gm, bt = R.vit_embed_case(F)
    emb = torch.cat([cls.expand(F, 1, 1024), po.view(F, 256, 1024)], 1) + pos[None]
    mean, rstd = R.emu_norm_stats(emb.view(F * 257, 1024), 64, False, R.LN_EPS)
    h = (emb.view(F * 257, 1024) - mean) * rstd * gm + bt
    R.check_vit_embed(F, h)
    late = torch.cat([cls.expand(F, 1, 1024), po.view(F, 256, 1024).roll(1, 1)], 1) + pos[None]   # patch t - 2 in row t
    assert fails(R.check_vit_embed, F, R.ln32(late, gm, bt, R.LN_EPS).view(F * 257, 1024))
    nopos = torch.cat([cls.expand(F, 1, 1024), po.view(F, 256, 1024)], 1) + pos[None].roll(1, 1)
    assert fails(R.check_vit_embed, F, R.ln32(nopos, gm, bt, R.LN_EPS).view(F * 257, 1024))
    mean, rstd = R.emu_norm_stats(emb.view(F * 257, 1024), 64, False, R.LN_EPS, one_pass=True)
    R.check_vit_embed(F, (emb.view(F * 257, 1024) - mean) * rstd * gm + bt)                   # (unit-scale rows: a one-pass variance is fine here)


# ---- temporal-transformer glue ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("st", HALVES + [torch.float32], ids=IDS + ["f32"])
@pytest.mark.parametrize("B,T,H", R.DELTA_SHAPES)
def test_delta_emulation_passes_and_mutations_fail(B, T, H, st):
    feats, pos, delta, mean_in = R.delta_case(B, T, H)
    twin = st == torch.float32

    def prep(wrong_t=False, mean_div=0, last=None):
        x, xl, _ = R.delta_prep_truth(feats, pos, wrong_t)
        m = torch.zeros((B, 256, H))
        for t in range(T):
            m = m + feats[:, t, 1:]
        m = m * (torch.ones(()) / float(mean_div or T))
        if last is not None:
            xl = (feats[:, last, 1:] + pos[last]).reshape(B * 256, H)
        return x.to(st), (None if twin else xl.to(st)), xl, m.reshape(B * 256, H)

    R.check_delta_prep(feats, pos, *prep())
    if T > 1:
        assert fails(R.check_delta_prep, feats, pos, *prep(wrong_t=True)), "x_all indexed (b, t, p) passes"
        assert fails(R.check_delta_prep, feats, pos, *prep(mean_div=T - 1)), "a mean over T - 1 passes"
        assert fails(R.check_delta_prep, feats, pos, *prep(last=T - 2)), "x_last of frame T - 2 passes"
    good = R.delta_finish_truth(feats, delta, mean_in).to(st)
    R.check_delta_finish(feats, delta, mean_in, good)
    if T > 1:
        assert fails(R.check_delta_finish, feats, delta, mean_in, R.delta_finish_truth(feats, delta, mean_in, cls_shift=1).to(st)), "the next frame's CLS row passes"
    if B > 1:
        assert fails(R.check_delta_finish, feats, delta, mean_in, R.delta_finish_truth(feats, delta, mean_in, clip_shift=1).to(st)), "the other clip's CLS rows pass"
    if not twin:
        assert fails(R.check_delta_finish, feats, delta, mean_in, R.truncate(R.delta_finish_truth(feats, delta, mean_in), st)), "a truncating store passes"
    assert any(b > 1 for b, _, _ in R.DELTA_SHAPES)
