"""The decode GEMV oracle checked on the CPU (tests/gemv_oracle.py): its case builders meet their exactness bounds, planted edges
sit where a plain float64 product says, the exact norm prologue survives a perturbed rsqrt in both 16-bit types, and the dispatch
mirror agrees with the source text and its comments' worked examples and reaches every branch through the listed cases."""
import pytest
import torch

from tests import gemv_oracle as G
from tests.test_gemm_exact_gpu import EDGES, Case


def test_mirror_rests_on_the_source_text():
    facts = G.dispatch_in_source()
    assert all(facts.values()), {k: v for k, v in facts.items() if not v}


def test_mirror_agrees_with_the_worked_examples():
    # gemv_kernel's comment: N = 5120 (o / down of the 13B decoder) takes four rows at K = 13824, two at K = 5120 (K >= 8192 as well)
    assert G.gemv_branch(1, 5120, 13824, 256) == "gemv_kernel<MR=1,KS=4,NR=4>"
    assert G.gemv_branch(2, 5120, 13824, 256) == "gemv_kernel<MR=2,KS=4,NR=4>"
    assert G.gemv_branch(1, 5120, 5120, 256) == "gemv_kernel<MR=1,KS=4,NR=2>"
    assert G.gemv_branch(1, 13824, 5120, 256) == "gemv_kernel<MR=1,KS=4,NR=2>"
    assert G.gemv_branch(1, 1000, 1024, 256) == "gemv_kernel<MR=1,KS=1,NR=2>"
    # launch_mfma_rows: half8 for (N + 15) / 16 < 768 and K % 128 == 0, by shape only
    for cus in G.CU_COUNTS:
        assert G.gemv_branch(8, 12272, 128, cus) == "gemv_mfma2<HALF8>" and G.gemv_branch(8, 12273, 128, cus) == "gemv_mfma2<16>"
        assert G.gemv_branch(8, 1000, 192, cus) == "gemv_mfma2<16>" and G.gemv_branch(9, 1000, 1024, cus) == "gemv_mfma2<BIGM>"
        assert G.gemv_branch(8, 1000, 1024, cus, mfma_env=0) == "gemv_kernel<MR=8,KS=1,NR=2>"
        assert G.gemv_branch(9, 1000, 1024, cus, mfma_env=0) == "gemv_mfma2<BIGM>"          # the switch covers M <= 8 only
        assert G.gemv_branch(9, 1001, 1024, cus, blockers=G.mfma_blockers(9, 1001, 1024)) == "refused"
        assert G.gemv_branch(3, 1000, 1024, cus, mfma_env=1) == "gemv_mfma"
        assert G.gemv_branch(1, 9, 2048, cus, rows_pin=4) == "gemv_kernel<MR=1,KS=4,NR=4>"
        assert G.gemv_branch(1, 7, 2048, cus, rows_pin=4) == "gemv_kernel<MR=1,KS=4,NR=2>"  # N >= 8
        assert G.gemv_branch(1, 20 * cus, 8192, cus, rows_pin=2) == "gemv_kernel<MR=1,KS=4,NR=2>"


@pytest.mark.parametrize("cus", G.CU_COUNTS)
def test_four_rows_exactly_between_sixteen_and_twenty_per_cu(cus):
    """The natural rule at K = 8192 selects four rows for N in (16 CUs, 20 CUs] and nowhere else up to 24 CUs."""
    for N in range(8, 24 * cus + 1):
        assert G.four_rows(N, 8192, cus) == (16 * cus < N <= 20 * cus), N
    for s in G.four_row_shapes(cus) + G.epilogue_shapes(cus)[1:]:
        assert {G.gemv_branch(M, s.N, s.K, cus) for M in s.Ms} == {"gemv_kernel<MR=1,KS=4,NR=4>", "gemv_kernel<MR=2,KS=4,NR=4>"}
    for s in G.split_shapes():
        assert {G.gemv_branch(M, s.N, s.K, cus) for M in s.Ms} == {"gemv_kernel<MR=1,KS=4,NR=2>", "gemv_kernel<MR=2,KS=4,NR=2>"}


@pytest.mark.parametrize("cus", G.CU_COUNTS)
def test_listed_cases_reach_every_branch(cus):
    got = G.listed_branches(cus)
    for row, kernels in G.TABLE_ROWS.items():
        for k in kernels:
            assert k in got, f"{row}: no listed case selects {k} at {cus} CUs"


def test_fallback_cases_are_kept_off_the_matrix_cores_for_their_reason():
    for N, K, layout, reason in G.FALLBACK:
        for M in G.FALLBACK_MS:
            blk = G.mfma_blockers(M, N, K, ldc=N + 5 if layout == "ldc" else None, c_ptr=2 if layout == "offset" else 0, out32=layout != "offset")
            assert reason in blk, (N, K, layout, blk)
            assert G.gemv_branch(M, N, K, 256, out32=layout != "offset", blockers=blk) == \
                f"gemv_kernel<MR={4 if M <= 4 else 8},KS={4 if K >= 2048 else 1},NR=2>"
    assert G.mfma_blockers(8, 1000, 1024) == [] and G.mfma_blockers(8, 1000, 1024, res_ptr=32, ldr=1024) == []
    assert G.mfma_blockers(8, 1000, 1024, res_ptr=32, ldr=1001) == ["residual alignment"]


@pytest.mark.parametrize("cus", G.CU_COUNTS)
def test_norm_grid_edges(cus):
    """One trip with a ragged last group, a second trip for block 0 only, three trips, four trips: both halves of red[] and both ways
    out of the loop."""
    one, two, three, four = (G.norm_plan(1, N, 2048, cus) for N in (8 * cus - 2, 8 * cus + 2, 16 * cus + 6, 24 * cus + 3))
    assert one.grid == two.grid == cus
    assert set(one.reduces) == {1} and one.exits == {"break"}
    assert two.reduces[0] == 2 and set(two.reduces[1:]) == {1} and two.exits == {"end", "break"}
    assert three.reduces[:3] == (3, 3, 3) and set(three.reduces) == {3, 2} and "break" in three.exits
    assert four.reduces[:2] == (4, 4) and set(four.reduces) == {4, 3} and four.exits == {"end", "break"}
    assert G.norm_plan(2, 6, 2048, cus) == G.NormPlan("gemv_norm_kernel<MR=2,CH=2,PRO=0>", 1, (1,), frozenset({"break"}))
    assert G.norm_plan(1, 6, 4096, cus).kernel.endswith("CH=2,PRO=0>") and G.norm_plan(1, 6, 4104, cus).kernel.endswith("CH=3,PRO=0>")
    for M, K in ((3, 2048), (1, 2040), (1, 6152), (1, 2052)):
        assert G.norm_plan(M, 6, K, cus).kernel == "refused"


@pytest.mark.parametrize("M", [1, 2])
@pytest.mark.parametrize("N,K", [(6, 2048), (1001, 2056), (10, 13824)])
def test_case_builder_meets_its_bound_and_plants_where_the_product_says(M, N, K):
    for has_b, has_r in ((False, False), (True, True)):
        c = Case(M, N, K, 61 + M, has_b, has_r)                      # (asserts 16 * 4 * K + 64 < 2^21 itself)
        truth = c.a.double() @ c.w.double().t()
        if has_b:
            truth = truth + c.bias.double()
        if has_r:
            truth = truth + c.res.double()
        assert torch.equal(truth, c.truth) and len(c.pairs) == M
        for p, (rr, cc) in enumerate(c.pairs):
            assert float(truth[rr, cc]) == EDGES[p]
    assert 16 * 4 * 13824 + 64 < G.EXACT_LIMIT


@pytest.mark.parametrize("M", [1, 2])
@pytest.mark.parametrize("N,K", [(6, 2048), (1001, 2056), (64, 4096), (6, 4104), (258, 5120), (6, 6136), (7, 6144)])
def test_norm_case_is_exact_under_a_perturbed_rsqrt(M, N, K):
    for seed, has_b, has_r in ((3, False, False), (4, True, True)):
        c = G.NormCase(M, N, K, seed, has_b, has_r)                  # (asserts the counts, the sum of squares 4 K and the bounds)
        assert c.eps == (1e-5 if seed % 2 else 1e-6)
        # the sum of squares is 4 K in fp32 in any order
        for perm in (torch.arange(K), torch.randperm(K, generator=torch.Generator().manual_seed(K))):
            hp = c.h[:, perm]
            assert torch.equal((hp * hp).cumsum(-1)[:, -1], torch.full((M,), 4.0 * K))
        for dtype in (torch.bfloat16, torch.float16):
            for steps in range(-3, 4):
                x = G.perturbed_norm_x(c.h, c.gamma, c.eps, steps, dtype)
                assert torch.equal(x.double(), c.x64), (dtype, steps)
        # the planted edges, by a plain float64 product of what the kernel is given
        truth = c.x64 @ c.w.double().t()
        if has_b:
            truth = truth + c.bias.double()
        if has_r:
            truth = truth + c.res.double()
        assert torch.equal(truth, c.truth)
        assert len(c.planted) == min(len(EDGES), max(1, N // 2), len({N - 1, 0, N - 2, 1, N // 2, N - 3, N // 3, 2, N - 4, N // 4, N // 5, 3}))
        for p, (rr, cc) in enumerate(c.planted):
            assert float(truth[rr, cc]) == EDGES[p], (p, rr, cc)
        if M == 2:
            assert not torch.equal(c.h[0].abs(), c.h[1].abs())           # every row its own shuffle
    sw = G.NormCase(M, 258, K, 5, False, False, True, 2, 1)
    assert float(sw.gamma.abs().max()) <= 2 and float(sw.w.double().abs()[~torch.isin(torch.arange(258), torch.tensor([c for _, c in sw.planted]))].max()) <= 1


@pytest.mark.parametrize("heads", G.MERGE_HEADS)
def test_merge_case_is_exact(heads):
    c = G.MergeCase(2, 1001, heads, 9, True, True)
    p = c.partials.double()
    assert bool((p[..., 0] == p[..., :1, 0]).all()) and bool((p[..., 1] == 0.5).all())
    # the merge, as written in the kernel: weights 2^(m - max) = 1, L = 2
    x = (p[..., 4:].sum(2) / p[..., 1].sum(2)[..., None]).reshape(2, heads * 128)
    assert torch.equal(x, c.x64) and torch.equal(x @ c.w.double().t() + c.bias.double() + c.res.double(), c.truth)
