"""The beam and processor oracle without a GPU (tests/beam_oracle.py): the expectations against torch and transformers, every
case's edge asserted from its radix trace, the mirror constants against the source text, and a numpy emulation of the kernels (the
two descents, the collect and rank, the merge by binary search, the selection, the processors with their bitmap) that passes every
case while each planted error fails the cases named for it."""
import os
import re

import numpy as np
import pytest
import torch

from tests import beam_oracle as O
from tests import logits_ref

STALE = (0, O.SENTINEL)                   # what a list slot the collect step never wrote is modelled to hold


# ---- constants and dispatch ---------------------------------------------------------------------------------------------------------
def test_mirror_constants_equal_the_source_text():
    c = O.source_constants()
    want = dict(MAX_K=64, MAX_NB=16, ROW_THREADS=1024, REG_J=32, PROC_MAX_V=1 << 18, RO_VECS=2048, RO_MAX_R=128, G_STAGE=8192, G_POS=64)
    assert {k: c[k] for k in want} == want
    assert (O.MAX_K, O.MAX_NB, O.ROW_THREADS, O.REG_J, O.PROC_MAX_V, O.RO_VECS, O.RO_MAX_R, O.G_STAGE, O.G_POS) == tuple(want.values())
    inc = open(os.path.join(O.CSRC, "beam_rows.inc")).read()
    assert inc.count(O.DISPATCH_TEXT) == 1 and inc.count("REG_J * ROW_THREADS") == 1       # the one dispatch kernel_of mirrors
    after = inc[inc.index(O.DISPATCH_TEXT):]
    assert after.index("beam_rows_kernel<true, LSE>") < after.index("beam_rows_kernel<false, LSE>")
    beam = open(os.path.join(O.CSRC, "beam.hip")).read()
    assert "R * 128 * elem_bytes > RO_VECS * 16" in beam and "const int P = RO_VECS / (n * vpp);" in beam
    assert re.search(r"for \(int lev = 0; lev < 3; \+\+lev\) \{\s+// indices < 2\^24", inc)
    assert O.ROW_THREADS == O.MAX_NB * O.MAX_K


def test_kernel_of_names_the_intended_form():
    assert [O.kernel_of(V) for V in (64, 1025, 32768, 32769, 66000)] == ["reg", "reg", "reg", "stream", "stream"]
    names = O.candidate_case_names()
    for n in names:                                                       # every register-form case has a streaming twin
        base, V = n.split("@")
        if O.kernel_of(int(V)) == "reg" and base != "k_equals_v":
            assert any(m.startswith(base + "@") and O.kernel_of(int(m.split("@")[1])) == "stream" for m in names), n
    assert {int(n.split("@")[1]) for n in names} == set(O.WIDTHS)
    assert O.reorder_run(128, 2) == 1 and O.reorder_run(64, 4) == 1 and O.reorder_run(5, 2) == 25


# ---- the expectations ---------------------------------------------------------------------------------------------------------------
def test_expected_candidates_by_hand():
    z = np.zeros
    s = np.array([[-1, -3, -1, -2], [-1, -5, -0.5, -9]], dtype=np.float32)
    sc, tok, beam, hit = O.expected_candidates(s, z(2, dtype=np.float32), 1, 2, 4, [0])
    assert tok.tolist() == [2, 0, 2, 0] and beam.tolist() == [1, 0, 0, 1] and hit.tolist() == [0, 1, 0, 1]
    assert sc.view(np.float32).tolist() == [-0.5, -1, -1, -1]
    s = np.array([[0, -1], [0, -1], [5, 4], [-70, 3]], dtype=np.float32)  # two prompts; -70 - 1e9 rounds to -1e9 - 64
    sc, tok, beam, hit = O.expected_candidates(s, np.array([-1e9, 0, -1e9, -1e9], dtype=np.float32), 2, 2, 2, [])
    assert tok.tolist() == [0, 1, 0, 1] and beam.tolist() == [1, 1, 2, 2] and not hit.any()
    assert sc.view(np.float32).tolist() == [0, -1, -1e9, -1e9]
    s = np.array([[np.nan, -0.0, 0.0]], dtype=np.float32)
    sc, tok, beam, hit = O.expected_candidates(s, z(1, dtype=np.float32), 1, 1, 3, [2, 7])
    assert tok.tolist() == [1, 2, 0] and sc.tolist() == [0, 0, 0xffffffff] and hit.tolist() == [0, 1, 0]


def test_expected_candidates_equal_a_stable_torch_sort():
    """On the float64 values of the fp32 sums; NaN aside (torch sorts it first), a stable descending sort has the kernel's order."""
    n = 0
    for c in O.candidate_cases() + O.lse_cases():
        acc = O.acc_of(c.scores, c.running)
        if np.isnan(acc).any():
            continue
        flat = torch.from_numpy(acc.astype(np.float64)).view(c.B, c.nb * c.V)
        order = torch.sort(flat, dim=1, descending=True, stable=True)[1][:, :c.K]
        sc, tok, beam, _ = O.expected_candidates(c.scores, c.running, c.B, c.nb, c.K, c.eos)
        assert tok.tolist() == (order % c.V).reshape(-1).tolist(), c.name
        assert beam.tolist() == (order // c.V + torch.arange(c.B)[:, None] * c.nb).reshape(-1).tolist(), c.name
        val = torch.take_along_dim(flat, order, 1).reshape(-1).numpy()
        assert np.array_equal(sc.view(np.float32).astype(np.float64), val), c.name                # (-0 == +0 here)
        n += 1
    assert n >= 70


def test_expected_select_by_hand():
    score = np.array([-1, -2, -3, -4, -0.0, 0.0, np.nan, -5], dtype=np.float32)
    hit = np.array([1, 0, 0, 1, 0, 0, 0, 0], dtype=np.uint8)
    tok, parent, run = O.expected_select(score, np.arange(8), np.arange(8) + 10, hit, 2, 2)
    assert tok.tolist() == [1, 2, 4, 5] and parent.tolist() == [11, 12, 14, 15]
    assert run.view(np.float32).tolist()[:2] == [-2, -3] and run.tolist()[2:] == [0x80000000, 0]


@pytest.mark.parametrize("name", [c.name for c in O.process_cases() if not c.foreign])
def test_expected_process_equals_transformers(name):
    c = O.case_by_name(name, "proc")
    want, hist = c.expected()
    for r in range(c.R):
        pen, n, m = c.params[r]
        ln = max(0, min(c.lengths()[r], c.hist.shape[1]))
        row = torch.from_numpy(c.x[r].copy())
        if c.lse is not None:
            row = row - float(c.lse[r])
        if ln == 0:                                                       # (transformers has no empty sequence: only the EOS mask applies)
            if m > 0:
                row[[t for t in c.eos if 0 <= t < c.V]] = -float("inf")
        else:
            procs = logits_ref.hf_processors(float(pen), n, m, None, eos=[t for t in c.eos] or None)
            if len(procs):
                row = procs(torch.from_numpy(hist[r, :ln].astype(np.int64))[None], row[None])[0]
        assert np.array_equal(row.numpy().view(np.uint32), want[r].view(np.uint32)), (name, r)


def test_expected_reorder_is_index_select():
    g = np.random.default_rng(1)
    cache = g.integers(-9, 9, size=(6, 2, 10, 128)).astype(np.int16)
    parent = [3, 1, 0, 0, -1, 6]
    out = O.expected_reorder(cache, parent, 2, 40)
    sel = torch.from_numpy(cache).index_select(0, torch.tensor([3, 1, 0, 0, 4, 5])).numpy()
    assert np.array_equal(out[:, :, 2:], sel[:, :, 2:]) and np.array_equal(out[:, :, :2], cache[:, :, :2])
    assert np.array_equal(O.expected_reorder(cache, parent, 5, 5), cache)


# ---- edges ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", O.candidate_case_names() + [c.name for c in O.lse_cases()])
def test_every_case_reaches_the_edge_it_is_named_after(name):
    c = O.case_by_name(name, "lse" if name.startswith("lse_") else "cand")
    c.check_edge()
    assert c.nb <= O.MAX_NB and c.nb <= c.K <= O.MAX_K and c.K <= c.V and c.ld >= c.V


def test_the_tie_descent_selects_every_index_digit_somewhere():
    top, mid, low = set(), set(), set()
    for c in O.candidate_cases():
        for t in c.traces():
            if t.idx_digits:
                top.add(t.idx_digits[0]), mid.add(t.idx_digits[1]), low.add(t.idx_digits[2])
    assert {0, 1} <= top and {0, 1, 255} <= mid and {0, 255} <= low


def test_process_cases_walk_their_loops_more_than_once():
    cs = {c.name: c for c in O.process_cases()}
    assert sorted({c.lengths()[0] for c in cs.values() if c.name.startswith("len")} & {1023, 1024, 1025, 2049}) == [1023, 1024, 1025, 2049]
    for name in ("len1024_v32769", "len2049_v262144"):
        c = cs[name]
        ids = c.hist[0, :c.lengths()[0]]
        words = set((ids[(ids >= 0) & (ids < c.V)] >> 5).tolist())
        assert {0, 1023, 1024, (c.V + 31) // 32 - 1} <= words, name             # both sides of the first trip of the bitmap zeroing
    c = cs["len2049_v262144"]
    ids = c.hist[0, :2049]
    late = set(ids[O.ROW_THREADS:].tolist()) - set(ids[:O.ROW_THREADS].tolist())
    assert any(0 <= t < c.V for t in late)                                # an id only the second trip of the penalty walk meets
    x, _ = c.expected()
    assert np.isneginf(x[0, c.V // 5]) and np.isneginf(x[0, c.V // 5 + 7])    # banned by a window before and one after position 1024
    f = cs["foreign_ids"]
    assert all(any(t < 0 or t >= f.V for t in row[:ln]) for row, ln in zip(f.hist.tolist(), f.lengths()))


# ---- the emulation ------------------------------------------------------------------------------------------------------------------------
def emulate_row(keys, K, mut=None):
    """One workgroup of beam_rows_kernel up to its sorted list: descents, collect (index <= icut), rank by (key, index)."""
    t = O.radix_trace(keys, K, index_levels=2 if mut == "two_index_levels" else 3, reduce_rem=mut != "rem_not_reduced")
    i = np.arange(len(keys))
    cut = i < t.icut if mut == "icut_strict" else i <= t.icut
    sel = np.flatnonzero((keys > np.uint32(t.thr)) | ((keys == np.uint32(t.thr)) & cut))[:K]
    ck = np.full(K, STALE[0], dtype=np.uint32)
    ci = np.full(K, STALE[1], dtype=np.int64)
    ck[:len(sel)], ci[:len(sel)] = keys[sel], sel
    rank = ((ck[None, :] > ck[:, None]) | ((ck[None, :] == ck[:, None]) & (ci[None, :] < ci[:, None]))).sum(1)
    lk, lt = np.full(K, STALE[0], dtype=np.uint32), np.full(K, STALE[1], dtype=np.int64)
    lk[rank[rank < K]], lt[rank[rank < K]] = ck[rank < K], ci[rank < K]
    return lk, lt


def emulate_candidates(c, mut=None):
    key_fn = (lambda s: O.okey(s, zero_apart=True)) if mut == "zero_apart" else (lambda s: O.okey(s, nan_high=True)) if mut == "nan_high" \
        else O.okey
    keys = key_fn(O.acc_of(c.scores, c.running))
    K, nb = c.K, c.nb
    out = [np.full(c.B * K, O.SENTINEL, dtype=np.int64) for _ in range(4)]
    for b in range(c.B):
        lists = [emulate_row(keys[b * nb + j], K, mut) for j in range(nb)]
        for jt in range(nb):
            for pos in range(K):
                k = lists[jt][0][pos]
                rank = pos
                for j in range(nb):
                    if j == jt:
                        continue
                    ge = {"merge_le": j <= jt, "merge_gt": j > jt}.get(mut, j < jt)
                    lk, lo, hi = lists[j][0], 0, K
                    while lo < hi:                                       # first position whose key is not better (lists descend)
                        mid = (lo + hi) >> 1
                        if (lk[mid] >= k) if ge else (lk[mid] > k):
                            lo = mid + 1
                        else:
                            hi = mid
                    rank += lo
                if rank < K:
                    o = b * K + rank
                    tkn = int(lists[jt][1][pos])
                    out[0][o], out[1][o], out[2][o] = int(O.okey_value(np.uint32(k)).view(np.uint32)), tkn, b * nb + jt
                    out[3][o] = int(any(e == tkn for e in c.eos))
    return out


def candidates_agree(c, mut=None):
    want = O.expected_candidates(c.scores, c.running, c.B, c.nb, c.K, c.eos)
    return all(np.array_equal(np.asarray(g, dtype=np.int64), np.asarray(w).astype(np.int64)) for g, w in zip(emulate_candidates(c, mut), want))


@pytest.mark.parametrize("name", O.candidate_case_names() + [c.name for c in O.lse_cases()])
def test_emulated_kernel_passes_every_candidate_case(name):
    assert candidates_agree(O.case_by_name(name, "lse" if name.startswith("lse_") else "cand"))


CAND_MUTANTS = {
    "icut_strict": ["ties_in_one_block@1025", "ties_straddle_255@1025", "ties_straddle_65535@66000", "ties_rem_1@32769",
                    "whole_row_constant@1024", "whole_row_all_nan@66000", "collapse_both_rows@32769"],
    "two_index_levels": ["ties_in_one_block@1025", "ties_straddle_255@32769", "ties_straddle_65535@66000", "collapse_both_rows@1025"],
    "merge_gt": ["merge_same_token_across_beams@97", "merge_equal_keys@32769", "limit_nb16_k64@1025"],
    "rem_not_reduced": ["digit2_ff@1025", "digit1_ff@32769", "negative_kth@32769", "ties_rem_n_eq_minus_1@1025"],
    "zero_apart": ["signed_zero_thr@1025", "signed_zero_thr@32769"],
    "nan_high": ["nan_row_short_of_k@1025", "nan_prompt_short_of_k@32769", "whole_row_all_nan@1024", "three_prompts@1025"],
}


@pytest.mark.parametrize("mut", list(CAND_MUTANTS))
def test_planted_selection_errors_fail_their_cases(mut):
    for name in CAND_MUTANTS[mut]:
        assert not candidates_agree(O.case_by_name(name), mut), (mut, name)


def test_the_merge_rule_j_le_jt_is_the_rule_j_lt_jt():
    """The merge skips its own list (``if (j == jt) continue``) before it takes ``ge = j < jt``: written as ``j <= jt`` the rule is
    the same function, so no case can tell the two apart.  The rule that can be wrong is the direction, ``merge_gt`` above."""
    for name in CAND_MUTANTS["merge_gt"] + ["merge_strict_interleave@97", "k_equals_v@64"]:
        assert candidates_agree(O.case_by_name(name), "merge_le"), name


def emulate_select(c):
    s = c.score.view(np.float32).reshape(c.B, c.K)
    out = [np.full(c.B * c.nb, O.SENTINEL, dtype=np.int64) for _ in range(3)]
    for b in range(c.B):
        with np.errstate(invalid="ignore"):
            v = (s[b] + c.hit.reshape(c.B, c.K)[b].astype(np.float32) * O.NEG_RUN).astype(np.float32)
        vk = O.okey(v)
        for t in range(c.K):
            rank = sum(1 for j in range(c.K) if vk[j] > vk[t] or (vk[j] == vk[t] and j < t))
            if rank < c.nb:
                o = b * c.nb + rank
                out[0][o], out[1][o], out[2][o] = c.token[b * c.K + t], c.beam[b * c.K + t], int(v[t:t + 1].view(np.uint32)[0])
    return out


@pytest.mark.parametrize("name", [c.name for c in O.select_cases()])
def test_emulated_selection_passes_every_case(name):
    c = O.case_by_name(name, "select")
    want = O.expected_select(c.score, c.token, c.beam, c.hit, c.B, c.nb)
    for g, w in zip(emulate_select(c), want):
        assert np.array_equal(g, np.asarray(w).astype(np.int64)), name
    assert c.nb <= c.K <= O.MAX_K and c.nb <= O.MAX_NB


def test_select_cases_reach_their_edges():
    cs = {c.name: c for c in O.select_cases()}
    assert cs["limit_k64_nb16"].K == O.MAX_K and cs["limit_k64_nb16"].nb == O.MAX_NB and cs["k_equals_nb"].K == cs["k_equals_nb"].nb
    c = cs["every_candidate_hit"]
    tok, _, run = O.expected_select(c.score, c.token, c.beam, c.hit, c.B, c.nb)
    assert c.hit.all() and len(np.unique(run)) <= 4 and tok.tolist() == c.token.reshape(c.B, c.K)[:, :c.nb].reshape(-1).tolist()
    z = cs["signed_zeros"]
    assert O.expected_select(z.score, np.arange(8), z.beam, z.hit, 1, 4)[0].tolist() == [0, 1, 2, 3]
    n = cs["nan_ranks_last"]
    assert O.expected_select(n.score, np.arange(8), n.beam, n.hit, 1, 4)[0].tolist() == [1, 2, 4, 5]


def emulate_process(c, mut=None):
    """logits_process_kernel thread by thread (tid-major: another order than the reference's), with its bitmap of seen ids."""
    T = O.ROW_THREADS
    x = c.x.copy()
    hist = c.hist.copy()
    hist_ld = hist.shape[1]
    for r in range(c.R):
        pen, n, m = np.float32(c.params[r][0]), int(c.params[r][1]), int(c.params[r][2])
        ln = min(c.lengths()[r], hist_ld)
        append = c.tok is not None and ln >= 1
        row = x[r]
        if append:
            hist[r, ln - 1] = c.tok[r]
        ids = hist[r].astype(np.int64)
        if c.lse is not None:
            row[:] = row - np.float32(c.lse[r])
        if pen != np.float32(1.0) and ln > 0:
            words = (c.V + 31) >> 5
            seen = np.full(words, 0xffffffff, dtype=np.uint64)             # LDS is not zero when a workgroup starts
            seen[:min(words, 1024) if mut == "bitmap_first_trip" else words] = 0
            for tid in range(min(T, ln)):
                for i in range(tid, ln, T):
                    t = int(ids[i])
                    if 0 <= t < c.V:
                        bit = 1 << (t & 31)
                        old = int(seen[t >> 5])
                        seen[t >> 5] = old | bit
                        if not (old & bit) or mut == "per_occurrence":
                            with np.errstate(all="ignore"):
                                row[t] = row[t] * pen if row[t] < 0 else row[t] / pen
        if n > 0 and ln >= n:
            p0 = ln - n + 1
            for i in range(ln):
                if (i + n < ln) if mut == "window_bound" else (i + n <= ln):
                    if all(ids[i + k] == ids[p0 + k] for k in range(n - 1)):
                        t = int(ids[i + n - 1])
                        if 0 <= t < c.V:
                            row[t] = -np.inf
        if ln < m:
            for t in c.eos:
                if 0 <= t < c.V:
                    row[t] = -np.inf
    return x, hist


def process_agrees(c, mut=None):
    (gx, gh), (wx, wh) = emulate_process(c, mut), c.expected()
    return np.array_equal(gx.view(np.uint32), wx.view(np.uint32)) and np.array_equal(gh, wh)


@pytest.mark.parametrize("name", [c.name for c in O.process_cases()])
def test_emulated_processors_pass_every_case(name):
    assert process_agrees(O.case_by_name(name, "proc"))


PROC_MUTANTS = {
    "per_occurrence": ["one_id_2049_times", "len2049_v262144", "log_softmax_then_penalty"],
    "window_bound": ["ngram_banned_id_is_the_appended_token", "ngram_n_equals_len_periodic", "ngram_n1_nlen_nlen_plus_1"],
    "bitmap_first_trip": ["len1024_v32769", "len1025_v262144", "len2049_v262144", "one_id_2049_times"],
}


@pytest.mark.parametrize("mut", list(PROC_MUTANTS))
def test_planted_processor_errors_fail_their_cases(mut):
    for name in PROC_MUTANTS[mut]:
        assert not process_agrees(O.case_by_name(name, "proc"), mut), (mut, name)
    if mut == "bitmap_first_trip":
        assert process_agrees(O.case_by_name("len1023_v32768", "proc"), mut)       # 1024 words: one trip is the whole bitmap
