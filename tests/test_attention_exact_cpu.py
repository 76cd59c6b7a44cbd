"""The attention oracle has teeth (tests/attention_oracle.py; no GPU): the three checks pass on the fp64 reference rounded to the 16-bit
storage type and fail on references with a planted mask error — causal off by one either way, a padded key let in, the newest key
dropped, the key at a 64 / 512 boundary dropped, 16 keys at a chunk start dropped, the cache row at kv_len counted, the ViT padding
counted — on every case whose shape can express the error.  The same errors on the random-data decode cases of
tests/test_kernels_gpu.py are classified against those tests' two limits: max-abs sees no one-key error in a long row, rel-L2 sees most
but not all (test_what_the_random_data_tolerances_see_of_a_mask_error).  The gap and distinct-code conditions of check (a)
are asserted here for every case the GPU module runs.

The mask logic does not depend on the head, and every "launch" here is a dense fp64 softmax: the proofs run the GPU module's cases
with at most two heads and the thinned cut points of the invisibility check; the conditions are asserted on the cases as they are."""
import pytest
import torch

from tests import attention_oracle as AO

HALF = torch.bfloat16               # (the constructions hold integers up to 64 and 0 / 1: exact in fp16 as well; fp16 is parametrised below)


def _cpu(case: AO.Case) -> AO.Case:
    c = AO.Case(**{**case.__dict__, "heads": min(case.heads, 2)})
    return c


def _ids(cases):
    return [c.name for c in cases]


LLAMA_CASES = AO.prefill_cases() + AO.decode_uniform_cases() + AO.decode_rows_cases()


def _run(dtype, vis=None):
    return lambda inp: AO.reference(inp, vis).to(dtype)


def _checks(case, dtype, vis=None):
    """name -> None (passed) or the assertion's message."""
    res = {}
    for name, fn in (("pointer", lambda: AO.check_pointer(case, _run(dtype, vis), dtype, rounds=1)),
                     ("invisible", lambda: AO.check_invisible(case, _run(dtype, vis), dtype, cuts=AO.thin_cuts(case.S))),
                     ("count", lambda: AO.check_count(case, _run(dtype, vis), dtype))):
        try:
            fn()
            res[name] = None
        except AssertionError as e:
            res[name] = str(e)
    return res


@pytest.mark.parametrize("n", range(len(LLAMA_CASES)), ids=_ids(LLAMA_CASES))
def test_reference_passes_and_every_mutation_is_caught(n):
    case = LLAMA_CASES[n]
    c = _cpu(case)
    dtype = torch.float16 if n % 2 else torch.bfloat16           # (odd cases of the list on fp16, even ones on bf16)
    res = _checks(c, dtype)
    assert all(v is None for v in res.values()), res
    muts = AO.mutations(c)
    assert "newest_key_dropped" in muts and "causal_minus_one" in muts and "sixteen_keys_of_a_chunk_start_dropped" in muts
    for name, vis in muts.items():
        res = _checks(c, dtype, vis)
        caught = [k for k, v in res.items() if v is not None]
        assert caught, f"{case.name}: mutation {name} passed all three checks"
        assert "count" in caught or "invisible" in caught, (name, caught)


def test_mutations_are_expressible_somewhere():
    """Every mutation of the issue is expressed by some case (a list whose shapes dodge a mutation proves nothing about it)."""
    seen = set()
    for c in LLAMA_CASES:
        seen.update(k.split("_at_a_")[-1] if "_at_a_" in k else k for k in AO.mutations(_cpu(c)))
    for want in ("causal_plus_one", "causal_minus_one", "padded_key_let_in", "newest_key_dropped", "64_boundary_dropped", "512_boundary_dropped",
                 "sixteen_keys_of_a_chunk_start_dropped", "key_at_kv_len_counted"):
        assert want in seen, want


@pytest.mark.parametrize("case", LLAMA_CASES, ids=_ids(LLAMA_CASES))
def test_gap_and_distinct_codes_of_every_gpu_case(case):
    """Check (a)'s conditions on the case as the GPU runs it (all heads, every round, both storage types): build_pointer asserts
    G >= 160 (+ the rotation's slack on the fused kernels) from the operands; the code table's rows are pairwise distinct and a cache
    never wraps around it."""
    assert case.ctx_max <= AO.code_table(AO.D).shape[0]
    for dtype in (torch.bfloat16, torch.float16):
        for rnd in range(AO.pointer_rounds(case)):
            inp = AO.build_pointer(case, dtype, "cpu", rnd)
            live = case.live_rows()
            assert bool((inp.q.float().abs().amax(-1) > 0)[live].all())
            if not case.fused:
                assert bool((inp.k.float().abs() == 1).all()) and bool((inp.q.float().abs()[live] == AO.GAMMA).all())


def test_candidates_walk_the_seams():
    """The targets of a long row: its own position, the first valid key after the padding, the last and the first key of every 64-key
    tile (= every chunk and split boundary of the decode kernels), and over the rounds every one of them is some head's target."""
    case = [c for c in AO.decode_rows_cases() if c.name == "rows-8x40"][0]
    vis = case.vis()
    c = AO.candidates(case, vis[0], 0, 0)                       # row 0: position 1300, 600 padded keys
    assert c[0] == 1300 and c[1] == 600 and 0 not in c and {639, 640, 1023, 1024, 1279, 1280}.issubset(c) and min(c) == 600
    c5 = AO.candidates(case, vis[5], 5, 0)                      # row 5: position 1025, 70 padded keys
    assert {1025, 70, 511, 512, 1023, 1024}.issubset(c5)
    for case in LLAMA_CASES:                                    # every case: every candidate of every row's last query is some head's target
        vis = case.vis()
        hit = [set() for _ in range(case.B)]
        for rnd in range(AO.pointer_rounds(case)):
            t = AO.pick_targets(case, rnd)
            for b in range(case.B):
                hit[b].update(t[b, case.S - 1].tolist())
        for b in range(case.B):
            want = set(AO.candidates(case, vis[b], b, case.S - 1))
            assert not want or hit[b] == want, (case.name, b, sorted(want - hit[b]))
    assert AO.cut_points(130) == [14, 15, 16, 30, 31, 32, 46, 47, 48, 62, 63, 64, 78, 79, 80, 94, 95, 96, 110, 111, 112, 126, 127, 128, 129]


# ---- ViT -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("F", [1, 17])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_vit_reference_passes_and_counted_padding_is_caught(F, dtype):
    ok = lambda qkv: AO.vit_reference(qkv).to(dtype)
    AO.vit_check_pointer(F, ok, dtype)
    AO.vit_check_count(F, ok, dtype)
    AO.vit_check_invisible(F, ok, dtype)
    for pad in (1, 15, 31):                                     # key 257 alone; the 272 keys of the score tiles; the 288 of the PV chunks
        with pytest.raises(AssertionError):
            AO.vit_check_count(F, lambda qkv: AO.vit_reference(qkv, pad).to(dtype), dtype)

    def next_head(qkv):                                         # a head that reads its neighbour's V: pointer and invisibility both see it
        q, k, v = AO.vit_unpack(qkv)
        return AO.vit_reference(AO.vit_pack(q, k, v.roll(1, 2))).to(dtype)
    with pytest.raises(AssertionError):
        AO.vit_check_pointer(F, next_head, dtype)
    with pytest.raises(AssertionError):
        AO.vit_check_invisible(F, next_head, dtype)


def test_vit_gap_of_every_gpu_case():
    for F in AO.VIT_FRAMES:
        AO.vit_build_pointer(F, torch.bfloat16)                 # asserts G >= 160 per (frame, head); +-1 and +-64: the same in fp16
    t = AO.vit_targets(1)[0]
    assert {0, 15, 16, 240, 255, 256}.issubset(set(t.flatten().tolist())) and bool((t[256] == 256).any())


# ---- delta attention -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nseq,T,H,nhead", AO.DELTA_SHAPES)
def test_delta_reference_passes_and_a_dropped_key_is_caught(nseq, T, H, nhead):
    for dtype in (torch.bfloat16, torch.float32):
        q, kv, want = AO.delta_build_pointer(nseq, T, H, nhead, dtype)
        assert torch.equal(AO.delta_reference(q, kv, T, nhead).to(dtype), want)
        q0, kv0, want0 = AO.delta_build_count(nseq, T, H, nhead, dtype)
        got = AO.delta_reference(q0, kv0, T, nhead)
        assert bool(((got - want0).abs() <= AO.ulp(want0, dtype) * (want0 != 0)).all())
        if T > 1:
            bad = AO.delta_reference(q0, kv0, T, nhead, drop_last=True)
            assert not bool(((bad - want0).abs() <= 4 * AO.ulp(want0, dtype) * (want0 != 0)).all())
            assert not torch.equal(AO.delta_reference(q, kv, T, nhead, drop_last=True).to(dtype), want)


# ---- why: the same mistakes on the random-data cases of tests/test_kernels_gpu.py --------------------------------------------------
def _randn(shape, seed, dtype):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return torch.randn(shape, generator=g).to(dtype)


# (rel-L2 seen, max-abs seen) by the limits of test_decode_attention_fused_equals_rope_then_attention: rel-L2 < 0.512 EPS, max-abs <= 2.56 EPS
SEEN = {
    511: {"key_64_dropped": (True, False), "newest_key_dropped": (True, False), "key_at_kv_len_counted": (False, False)},
    700: {"key_64_dropped": (True, False), "key_512_dropped": (True, False), "newest_key_dropped": (True, True),
          "sixteen_keys_from_512_dropped": (True, True), "key_at_kv_len_counted": (True, False), "padded_key_let_in": (True, False)},
    1300: {"key_64_dropped": (False, False), "key_512_dropped": (True, False), "key_1024_dropped": (True, False),
           "newest_key_dropped": (True, False), "sixteen_keys_from_512_dropped": (True, False), "sixteen_keys_from_1024_dropped": (True, False),
           "key_at_kv_len_counted": (False, False)},
}


@pytest.mark.parametrize("B,past,heads,pad", [(1, 511, 3, 0), (3, 700, 2, 600), (1, 1300, 1, 0)])
def test_what_the_random_data_tolerances_see_of_a_mask_error(B, past, heads, pad):
    """test_decode_attention_fused_equals_rope_then_attention's cases at past >= 511 (seeded randn K, V, q of the same scale, bf16, the cache
    row behind the new token zero as there; without the rotation, which does not change the distribution): the fp64 reference with a
    planted mask error against the unmutated one, over every row, in that test's two measures and against its two limits.  With one new
    token, causal + 1 and "the row at kv_len counted" are the same error.  Measured (rel-L2, max-abs; units of EPS; limits 0.512, 2.56):
        past  511: key 64 dropped 1.65, 0.53; newest dropped 2.77, 0.75; row kv_len counted 0.16, 0.03
        past  700 (row 0 sees 101 keys behind 600 padded ones): key 64 1.55, 0.79; key 512 2.13, 1.19; newest 12.1, 7.39; sixteen keys
                   from 512 9.97, 3.47; row kv_len counted 0.70, 0.31; padded key 599 let in 1.40, 0.81
        past 1300: key 64 0.31, 0.04; key 512 2.58, 0.34; key 1024 2.60, 0.34; newest 1.23, 0.22; sixteen keys from 512 6.07, 0.90;
                   from 1024 11.3, 1.74; row kv_len counted 0.06, 0.01
    So the max-abs limit sees none of the one-key errors in a long row (only the short padded row's), the rel-L2 limit sees most of them
    but not all (key 64 at past 1300, the row at kv_len at 511 and 1300 pass both).  Asserted per error: on which side of each limit it
    falls (SEEN).  What those tests lack is therefore less the tolerance than the reference — they compare one kernel with another, which
    share their masking code — and shapes on the kernels' seams; the exact checks see every one of these errors at any length."""
    EPS = 2.0 ** -7
    case = AO.Case("random", B, 1, [past] * B, heads, past + 2, [pad], full_valid=True)
    k, v = _randn((B, heads, past + 2, 128), 30, HALF), _randn((B, heads, past + 2, 128), 31, HALF)
    k[:, :, past + 1] = 0
    v[:, :, past + 1] = 0
    inp = AO.Inputs(case, _randn((B, 1, heads, 128), 32, HALF), k, v, case.valid_buffer("cpu"))
    ref = AO.reference(inp)
    j = torch.arange(case.ctx_max)[None, None, :]
    row0 = (torch.arange(B) == 0)[:, None, None]
    vis = case.vis()
    muts = {"key_64_dropped": vis & (j != 64), "key_512_dropped": vis & (j != 512), "key_1024_dropped": vis & (j != 1024),
            "newest_key_dropped": vis & (j != past), "sixteen_keys_from_512_dropped": vis & ~((j >= 512) & (j < 528)),
            "sixteen_keys_from_1024_dropped": vis & ~((j >= 1024) & (j < 1040)), "key_at_kv_len_counted": vis | (j == past + 1),
            "padded_key_let_in": vis | ((j == pad - 1) & row0)}
    muts = {n: m for n, m in muts.items() if bool((m != vis).any()) and not (n.startswith("sixteen") and past < 528)}
    assert set(muts) == set(SEEN[past])
    for name, mut in muts.items():
        got = AO.reference(inp, mut)
        rel = float((got - ref).norm() / ref.norm()) / EPS
        mab = float((got - ref).abs().max()) / EPS
        print(f"past {past} {name}: rel-L2 {rel:.2f} EPS, max-abs {mab:.2f} EPS")
        assert (rel >= 0.512, mab > 2.56) == SEEN[past][name], (name, rel, mab)
    # ... and the exact checks see each of them at the same shape (one head: the mask does not depend on it)
    c2 = AO.Case("random-exact", B, 1, [past] * B, 1, past + 2, [pad], full_valid=True)
    for name, mut in muts.items():
        res = _checks(c2, HALF, mut)
        assert any(r is not None for r in res.values()), name
