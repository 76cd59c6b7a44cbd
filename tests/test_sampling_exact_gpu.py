"""vly_argmax on the MI355X against the sampling oracle (tests/sampling_oracle.py): exact kept sets and draws at every radix edge.
Every assertion is exact equality of token ids; the margins that make that possible were asserted on the host when the rows were
built.  Every launch has its padding columns and a guard row after the last row poisoned (+inf, 3e38, NaN) and guard entries after
the M outputs that must keep their sentinel.  One more test replays DecodeSession(sampling=True)'s draws on the host with the
counter DESIGN.md states (c = pos + 1)."""
import time

import numpy as np
import pytest
import torch

from tests import sampling_oracle as O

pytestmark = pytest.mark.gpu
GUARD = 4


def launch(case) -> np.ndarray:
    from valley_amd import ops
    d = torch.device("cuda:0")
    L = O.layout(case)
    M, N, ld, off = len(case.entries), case.N, case.ld, case.offset
    flat = torch.empty(off + (M + 1) * ld, dtype=torch.float32, device=d)
    flat[:off] = float("nan")
    body = flat[off:].view(M + 1, ld)
    body.copy_(torch.from_numpy(O.poison(ld, start=-N)).to(d).expand(M + 1, ld))          # column N holds +inf
    x = body[:M, :N]
    x.copy_(torch.from_numpy(L["uniq"]).to(d)[torch.from_numpy(L["index"]).to(d)])
    assert x.data_ptr() % 16 == (4 * off) % 16 and x.stride(0) == ld
    outbuf = torch.full((M + GUARD,), O.SENTINEL, dtype=torch.int32, device=d)
    out = outbuf[:M]
    if case.null:
        ops.argmax(x, out=out)
    else:
        sp = ops.sampling_rows(L["T"], L["k"], L["p"], L["seed"], device=d)
        ops.argmax(x, out=out, sampling=sp, ctr=torch.from_numpy(L["ctr"]).to(d), ctr_add=O.CTR_ADD)
    got = outbuf.cpu().numpy()
    assert (got[M:] == O.SENTINEL).all(), f"{case.name}: an output past row M - 1 was written"
    return got[:M]


def run(family: str) -> None:
    t0 = time.perf_counter()
    cases = O.FAMILIES[family]()
    t1 = time.perf_counter()
    assert 1 <= len(cases) <= 2                                  # at most two launches per test
    for case in cases:
        O.check(case, launch(case))
    torch.cuda.synchronize()
    print(f"family {family}: {sum(len(c.entries) for c in cases)} probes, host search {t1 - t0:.2f} s, launches {time.perf_counter() - t1:.2f} s")


def test_top_k_boundary_at_each_of_the_four_digits():
    run("A")


def test_sign_fold_cut_beside_the_zeros_and_the_zero_tie_group():
    run("B")


def test_denormal_scores_are_not_flushed():
    run("B denormal")


def test_boundary_tie_groups_of_2_65_and_1025_are_kept_whole():
    run("C")


def test_edge_values_of_k_and_k_against_the_candidate_count():
    run("D")


def test_top_p_cut_at_each_of_the_four_digits_and_the_edges_of_p():
    run("E")


def test_top_p_mass_is_taken_over_the_top_k_survivors():
    run("F")


@pytest.mark.parametrize("N", O.WIDTHS)
def test_widths_strides_and_unaligned_rows(N):
    run(f"G {N}")


@pytest.mark.parametrize("N", [4097, 32769])
def test_fallbacks_return_the_first_maximum_of_the_logits(N):
    run(f"H {N}")


@pytest.mark.parametrize("N", [4096, 4097, 32769])
def test_all_nan_row_gives_token_0_on_every_entry_path(N):
    run(f"H NaN {N}")


def test_greedy_first_maximum_on_the_float4_path():
    run("greedy aligned")


def test_greedy_first_maximum_on_the_unaligned_scalar_loop():
    run("greedy unaligned")


# ---- the counter contract ---------------------------------------------------------------------------------------------------------------
SESSION = dict(T=[0.7, 1.0, 1.5, 0.9], k=[0, 50, 0, 40], p=[0.9, 1.0, 1.0, 0.95], seed=[11, 12, 13, 14])


@pytest.mark.parametrize("use_graph", [True, False], ids=["graph", "eager"])
def test_decode_session_draws_with_counter_pos_plus_1(use_graph):
    """Eight steps of DecodeSession(sampling=True): each row's token is the host replay of that step's sess.logits at c = pos + 1
    (decode: sampling).  A (step, row) pair is checked when the host's winner leads by >= 1e-3 and no top-p mass is
    within 1e-4 of p; at least 24 of the 32 pairs must be, and every checked pair matches exactly."""
    from valley_amd import ops
    from valley_amd.decode import DecodeSession
    from tests.test_sampling_gpu import small_llama
    ll = small_llama()
    B, S, steps = 4, 40, 8
    g = torch.Generator(device="cuda").manual_seed(21)
    cache = ll.new_cache(B, S + steps + 2)
    h = torch.randn((B * S, ll.H), generator=g, device="cuda") * 0.02
    x = ll.forward(h, B, S, cache)
    first = ll.logits(x.view(B, S, -1)[:, -1].contiguous())[:, :ll.V].argmax(-1)
    sess = DecodeSession(ll, cache, use_graph=use_graph, sampling=True)
    sess.sample.copy_(ops.sampling_rows(SESSION["T"], SESSION["k"], SESSION["p"], SESSION["seed"], device="cuda:0"))
    sess.begin(first)
    checked = 0
    for step in range(steps):
        pos = int(sess.pos[0])
        tok = sess.step().cpu().tolist()
        logits = sess.logits[:, :ll.V].cpu().numpy()
        assert int(sess.pos[0]) == pos + 1 == S + step + 1
        for r in range(B):
            want, ok = O.replay(logits[r], SESSION["T"][r], SESSION["k"][r], SESSION["p"][r], SESSION["seed"][r], pos + 1)
            if ok:
                assert tok[r] == want, (step, r, tok[r], want)
                checked += 1
    sess.check()
    print(f"counter contract ({'graph' if use_graph else 'eager'}): {checked} of {steps * B} pairs checked")
    assert checked >= 24
