"""GPU checks of batched prompt-lookup speculation (include/valley_hip_spec_rows.h, valley_amd.spec.SpecRowsSession,
ContinuousBatcher(prompt_lookup_num_tokens=k)):

* vly_spec_rows_attention and vly_spec_rows_rope_kv bit for bit against vly_spec_attention / vly_rope_kv of each sequence alone,
  the attention's independence of S, of the sequence's index and of its neighbours' positions, and dead rows (positions behind the
  cache's end) that store nothing;
* vly_spec_rows_draft, _accept and _counters against tests/spec_rows_ref.py, exactly, and the draft and the acceptance of ONE
  sequence against vly_spec_draft / vly_spec_accept on the same tables, buffer for buffer (both call csrc/spec_lookup.inc);
* SpecRowsSession with forced drafts against SpecDecodeSession of each sequence alone, and the speculating batcher against the
  plain one, token for token (greedy and seeded).

Shapes: heads = 2, ctx_max = 384 — six 64-key blocks, so two of the four splits visit two blocks each."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import attention_oracle as AO
from tests import golden_cfg as G
from tests import spec_rows_ref as RR
from valley_amd.runtime import HALF

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
HEADS, CTX, HQ = 2, 384, 256
POSITIONS = [0, 1, 62, 63, 64, 127, 128, 255, 256, 300]
# positions of the three sequences per launch; sequence 1's key_valid masks the whole first block, so it sits behind it
TRIPLES = [(0, 64, 1), (62, 127, 63), (128, 255, 256), (300, 300, 64), (1, 128, 0)]


@pytest.fixture(scope="module", autouse=True)
def no_gemm_trials_in_this_module():
    """The online GEMM tuner decides a shape over its first ~150 calls in a process, each trial call running another candidate
    (valid results that differ by fp32 summation order).  The prefills here compare a request served two ways, so every prefill
    of a shape must run the SAME kernel (ops.TUNE_ONLINE = False: the table's choice or the static tile) — and the tuner's
    tables stay as this module found them, so the prefills of the files that run behind it start from the point they always did."""
    from valley_amd import ops
    mp = pytest.MonkeyPatch()
    mp.setattr(ops, "TUNE_ONLINE", False)
    yield
    mp.undo()


# ---- inputs shared by the attention and RoPE checks: built once, never modified ---------------------------------------------
@pytest.fixture(scope="module")
def world():
    return make_world()


def make_world():
    g = torch.Generator().manual_seed(5)
    k = torch.randn((3, HEADS, CTX, 128), generator=g).to(HALF).to(DEV)
    v = torch.randn((3, HEADS, CTX, 128), generator=g).to(HALF).to(DEV)
    q = torch.randn((3, 8, 3 * HQ), generator=g).to(HALF).to(DEV)     # per sequence: the q | k | v rows of up to 8 queries
    valid = torch.ones((3, CTX), dtype=torch.uint8)
    j = torch.arange(CTX)
    valid[0, (j % 37 == 5)] = 0                                  # holes
    valid[1, :64] = 0                                            # a fully masked first block ...
    valid[1, (j % 29 == 3)] = 0                                  # ... and holes behind it
    valid[2, (j % 41 == 7)] = 0
    cos, sin = (t.to(DEV) for t in AO.rope_tables(CTX))
    return {"k": k, "v": v, "q": q, "valid": valid.to(DEV), "cos": cos, "sin": sin}


def pos_tensor(pos):
    return torch.tensor(list(pos), dtype=torch.int32, device=DEV)


def rows_attention(w, order, pos, S, rows=None):
    """One vly_spec_rows_attention launch over the world's sequences ``order`` at ``pos`` with S queries each (the world's q rows
    ``rows[i]`` of each sequence, default 0 .. S - 1); caches and tickets checked; -> out [B, S, heads * 128]."""
    from valley_amd import ops
    B = len(order)
    rows = rows or [list(range(S))] * B
    qkv = torch.stack([w["q"][s][r] for s, r in zip(order, rows)]).reshape(B * S, 3 * HQ).contiguous()
    k, v, valid = w["k"][list(order)].contiguous(), w["v"][list(order)].contiguous(), w["valid"][list(order)].contiguous()
    k0, v0 = k.clone(), v.clone()
    scratch = ops.spec_rows_scratch(B, S, HEADS, DEV)
    out = ops.spec_rows_attention(qkv, k, v, valid, B, S, HEADS, pos_tensor(pos), scratch)
    assert torch.equal(AO.bits(k), AO.bits(k0)) and torch.equal(AO.bits(v), AO.bits(v0)), "the caches are read-only"
    assert int(scratch[1].abs().sum()) == 0, "ticket counters not back at zero"
    return out.view(B, S, HQ)


def single_attention(w, s, p, S, rows=None):
    """What vly_spec_attention writes for sequence ``s`` alone at position ``p``."""
    from valley_amd import ops
    rows = rows or list(range(S))
    qkv = w["q"][s][rows].contiguous()
    scratch = ops.spec_scratch(1, S, HEADS, DEV)
    out = ops.spec_attention(qkv, w["k"][s:s + 1].contiguous(), w["v"][s:s + 1].contiguous(), w["valid"][s:s + 1].contiguous(), 1, S, HEADS,
                             p, scratch)
    assert int(scratch[1].abs().sum()) == 0
    return out.view(S, HQ)


def attention_bit_equality(w):
    seen = set()
    for S in (1, 2, 4, 8):
        for pos in TRIPLES:
            got = rows_attention(w, (0, 1, 2), pos, S)
            for b, p in enumerate(pos):
                want = single_attention(w, b, p, S)
                assert torch.equal(AO.bits(got[b]), AO.bits(want)), (S, pos, b)
                assert bool(got[b].float().isfinite().all())
                seen.add(p)
    assert seen == set(POSITIONS)
    return len(seen)


def attention_position_invariance(w):
    """The row of (sequence, absolute position P, q row) is the same bits whatever S, the sequence's index in the launch and its
    neighbours' positions are."""
    for pos in TRIPLES:
        base = rows_attention(w, (0, 1, 2), pos, 8)
        # S = 4 from the third query on, the sequences permuted: sequence s sits at index order.index(s), beside other neighbours
        order = (2, 0, 1)
        got = rows_attention(w, order, [pos[s] + 2 for s in order], 4, rows=[[2, 3, 4, 5]] * 3)
        for i, s in enumerate(order):
            assert torch.equal(AO.bits(got[i]), AO.bits(base[s, 2:6])), (pos, s, "S = 4, permuted")
        # S = 1, two sequences only, the neighbour somewhere else
        for s, other in ((0, 2), (1, 0), (2, 1)):
            for r in (0, 7):
                got = rows_attention(w, (other, s), [70, pos[s] + r], 1, rows=[[0], [r]])
                assert torch.equal(AO.bits(got[1, 0]), AO.bits(base[s, r])), (pos, s, r, "S = 1")


def test_attention_rows_are_the_single_sequence_rows(world):
    assert attention_bit_equality(world) == len(POSITIONS)


def test_attention_position_invariance(world):
    attention_position_invariance(world)


def rope_bit_equality(w):
    from valley_amd import ops
    g = torch.Generator().manual_seed(9)
    for S in (1, 2, 4, 8):
        for pos in TRIPLES:
            qkv = torch.randn((3 * S, 3 * HQ), generator=g).to(HALF).to(DEV)
            k = torch.full((3, HEADS, CTX, 128), 0.25, dtype=HALF, device=DEV)
            v = torch.full((3, HEADS, CTX, 128), -0.5, dtype=HALF, device=DEV)
            got_q, got_k, got_v = qkv.clone(), k.clone(), v.clone()
            ops.spec_rows_rope_kv(got_q, got_k, got_v, w["cos"], w["sin"], 3, S, HEADS, pos_tensor(pos))
            for b, p in enumerate(pos):
                q1, k1, v1 = qkv[b * S:(b + 1) * S].clone(), k[b:b + 1].clone(), v[b:b + 1].clone()
                ops.rope_kv(q1, k1, v1, w["cos"], w["sin"], 1, S, HEADS, p)
                assert torch.equal(AO.bits(got_q[b * S:(b + 1) * S]), AO.bits(q1)), (S, pos, b, "qkv")
                assert torch.equal(AO.bits(got_k[b]), AO.bits(k1[0])) and torch.equal(AO.bits(got_v[b]), AO.bits(v1[0])), (S, pos, b, "cache")
                assert not torch.equal(AO.bits(got_k[b, :, p:p + S]), AO.bits(k[b, :, p:p + S]))     # (it did write there)


def test_rope_rows_are_the_single_sequence_rows(world):
    rope_bit_equality(world)


def test_dead_rows_store_nothing(world):
    """Sequences at ctx_max - 1, ctx_max - 2 and beyond the end (brought back to ctx_max - 1), S = 4: 1, 2 and 1 live rows.  The
    caches sit between guard sequences, qkv and out between guard rows, all filled with a sentinel; after the RoPE and the
    attention everything but the live positions is bit for bit what it was, the live ones are the single-sequence kernels', and
    every output is finite."""
    from valley_amd import ops
    w, S, B = world, 4, 3
    pos = [CTX - 1, CTX - 2, CTX + 5]
    live = [1, 2, 1]
    g = torch.Generator().manual_seed(3)
    big_k = torch.full((B + 2, HEADS, CTX, 128), 1.5, dtype=HALF, device=DEV)
    big_v = torch.full((B + 2, HEADS, CTX, 128), -2.5, dtype=HALF, device=DEV)
    big_k[1:B + 1] = w["k"]
    big_v[1:B + 1] = w["v"]
    big_q = torch.full((B * S + 4, 3 * HQ), 3.0, dtype=HALF, device=DEV)
    big_q[2:B * S + 2] = torch.randn((B * S, 3 * HQ), generator=g).to(HALF).to(DEV)
    big_o = torch.full((B * S + 4, HQ), 7.0, dtype=HALF, device=DEV)
    k, v, qkv, out = big_k[1:B + 1], big_v[1:B + 1], big_q[2:B * S + 2], big_o[2:B * S + 2]
    want_k, want_v, want_q = big_k.clone(), big_v.clone(), big_q.clone()
    for b in range(B):                                           # the live rows, by the single-sequence kernel
        p, n = min(pos[b], CTX - 1), live[b]
        assert [RR.dead(pos[b], j, CTX) for j in range(S)] == [False] * n + [True] * (S - n)
        q1, k1, v1 = qkv[b * S:b * S + n].clone(), k[b:b + 1].clone(), v[b:b + 1].clone()
        ops.rope_kv(q1, k1, v1, w["cos"], w["sin"], 1, n, HEADS, p)
        want_q[2 + b * S:2 + b * S + n] = q1
        want_k[1 + b] = k1[0]
        want_v[1 + b] = v1[0]
    posd = pos_tensor(pos)
    ops.spec_rows_rope_kv(qkv, k, v, w["cos"], w["sin"], B, S, HEADS, posd)
    assert torch.equal(AO.bits(big_q), AO.bits(want_q)), "qkv: only the q of live rows may change"
    assert torch.equal(AO.bits(big_k), AO.bits(want_k)) and torch.equal(AO.bits(big_v), AO.bits(want_v)), "caches: only live positions"
    assert posd.tolist() == pos
    valid = torch.ones((B, CTX), dtype=torch.uint8, device=DEV)
    scratch = ops.spec_rows_scratch(B, S, HEADS, DEV)
    ops.spec_rows_attention(qkv, k, v, valid, B, S, HEADS, posd, scratch, out=out)
    assert torch.equal(AO.bits(big_q), AO.bits(want_q)) and torch.equal(AO.bits(big_k), AO.bits(want_k)) and \
        torch.equal(AO.bits(big_v), AO.bits(want_v)), "the attention reads only"
    assert bool((big_o[:2] == 7.0).all()) and bool((big_o[-2:] == 7.0).all()) and int(scratch[1].abs().sum()) == 0
    assert bool(out.float().isfinite().all())
    for b in range(B):
        p, n = min(pos[b], CTX - 1), live[b]
        one = ops.spec_attention(qkv[b * S:b * S + n].contiguous(), k[b:b + 1].contiguous(), v[b:b + 1].contiguous(), valid[b:b + 1], 1, n,
                                 HEADS, p, ops.spec_scratch(1, n, HEADS, DEV))
        assert torch.equal(AO.bits(out[b * S:b * S + n]), AO.bits(one)), (b, "live rows")


# ---- draft, accept and counters ---------------------------------------------------------------------------------------------------
GUARD = 12


def guarded(values, fill=-99):
    a = np.asarray(values, dtype=np.int64)
    t = torch.full((a.size + 2 * GUARD,), fill, dtype=torch.int32)
    t[GUARD:GUARD + a.size] = torch.from_numpy(a.reshape(-1)).to(torch.int32)
    t = t.to(DEV)
    return t, t[GUARD:GUARD + a.size].view(a.shape)


def guards_intact(bufs):
    for name, (t, _view) in bufs.items():
        assert bool((t[:GUARD] == -99).all()) and bool((t[-GUARD:] == -99).all()), f"{name}: a guard word changed"


def run_draft(hist, lengths, k, n, eos=(), live=None, lookup=True, vocab=0, len_add=1):
    from valley_amd import ops
    B = hist.shape[0]
    before_d = np.arange(50, 50 + B * k).reshape(B, k)
    before_dl = [9] * B
    bufs = {"hist": guarded(hist), "pos": guarded([length - len_add for length in lengths]), "draft": guarded(before_d),
            "dl": guarded(before_dl), "tok": guarded(np.full((B * (k + 1),), -5))}
    lv = None if live is None else torch.tensor(live, dtype=torch.uint8, device=DEV)
    e = torch.tensor(list(eos), dtype=torch.int32, device=DEV) if len(eos) else None
    ops.spec_rows_draft(bufs["hist"][1], bufs["pos"][1], len_add, k, n, bufs["draft"][1], bufs["dl"][1], bufs["tok"][1], live=lv, eos=e,
                        vocab=vocab, lookup=lookup)
    guards_intact(bufs)
    assert bufs["hist"][1].tolist() == hist.tolist() and bufs["pos"][1].tolist() == [length - len_add for length in lengths]
    got = (bufs["draft"][1].tolist(), bufs["dl"][1].tolist(), bufs["tok"][1].view(B, k + 1).tolist())
    want = RR.draft_rows(hist, lengths, k, n, eos, vocab=vocab, live=live, lookup=lookup, draft=before_d, draft_len=before_dl)
    assert got == want, (lengths, k, n, eos, live, lookup, got, want)
    return got


def history(lengths, seed, V=4):
    g = np.random.default_rng(seed)
    h = np.full((len(lengths), CTX), 7777, dtype=np.int64)
    for b, length in enumerate(lengths):
        h[b, :length] = g.integers(0, V, size=length)
        tail = h[b, max(0, length - 8):length]                    # poison behind the end: a scan past it would match here
        room = min(CTX - length, 2 * len(tail))
        h[b, length:length + room] = np.tile(tail, 2)[:room]
    return h


def test_draft_rows_match_the_reference():
    for lengths in ([1], [CTX], [CTX, 1], [2, 383, 100], [300, 1, CTX, 65], [CTX - 2, CTX - 1, 3, 257]):
        B = len(lengths)
        for seed in range(2):
            h = history(lengths, 100 * seed + B)
            for k in (1, 3, 7):
                for n in (1, 2, 8):
                    for eos in ((), (3,), (0, 3)):
                        run_draft(h, lengths, k, n, eos)
    # the device position and the host's addend share the length
    run_draft(history([200, 300], 5), [200, 300], 3, 2, len_add=2)
    # a sequence that is not live: no draft, rows of token 0, its draft row kept; its neighbours as ever
    for live in ([1, 0, 1], [0, 1, 1], [0, 0, 0]):
        d, dl, tok = run_draft(history([120, 250, 380], 6), [120, 250, 380], 3, 2, live=live)
        for b in range(3):
            if not live[b]:
                assert dl[b] == 0 and tok[b] == [0] * 4 and d[b] == [50 + 3 * b, 51 + 3 * b, 52 + 3 * b]
    # a planted match per sequence, cropped by an EOS in one and by the end of the cache in another
    h = np.tile(np.arange(1000, 1000 + CTX), (3, 1))
    for b, (length, cont) in enumerate(((200, [21, 22, 23, 24]), (300, [31, 5, 33, 34]), (CTX - 2, [41, 42, 43, 44]))):
        h[b, 50:52] = [11, 12]
        h[b, 52:56] = cont
        h[b, length - 2:length] = [11, 12]
    d, dl, tok = run_draft(h, [200, 300, CTX - 2], 4, 2, eos=(5,))
    assert dl == [4, 1, 2] and tok[0] == [12, 21, 22, 23, 24] and tok[1] == [12, 31, 12, 12, 12] and tok[2] == [12, 41, 42, 12, 12]
    # lookup = 0: the caller's drafts (run_draft's tables hold 50 ..., length 9 -> k, capped at the cache's end)
    d, dl, tok = run_draft(h, [200, CTX - 1, CTX], 3, 2, lookup=False)
    assert dl == [9, 9, 9] and d == [[50, 51, 52], [53, 54, 55], [56, 57, 58]]
    assert tok[0] == [12, 50, 51, 52] and tok[1][1:] == [53] + [tok[1][0]] * 2 and tok[2][1:] == [tok[2][0]] * 3


def run_accept(am, draft, dl, k, hist, pos, stats, live=None):
    from valley_amd import ops
    B = hist.shape[0]
    emit0, tok0 = np.full((B, k + 2), -3), np.full((B * (k + 1),), -3)
    bufs = {"am": guarded(am), "draft": guarded(draft), "dl": guarded(dl), "hist": guarded(hist), "pos": guarded(pos),
            "emit": guarded(emit0), "tok": guarded(tok0), "stats": guarded(stats)}
    lv = None if live is None else torch.tensor(live, dtype=torch.uint8, device=DEV)
    ops.spec_rows_accept(bufs["am"][1], bufs["draft"][1], bufs["dl"][1], k, bufs["hist"][1], bufs["pos"][1], bufs["emit"][1], bufs["tok"][1],
                         bufs["stats"][1], live=lv)
    guards_intact(bufs)
    for name, src in (("am", am), ("draft", draft), ("dl", dl)):
        assert bufs[name][1].tolist() == np.asarray(src).tolist(), f"{name} is an input"
    ns, h, emit, tok, st, p = RR.accept_rows(am, np.asarray(draft), dl, k, hist, pos, np.asarray(stats), live=live, emit=emit0, tok=tok0)
    got = {name: bufs[name][1].tolist() for name in ("hist", "emit", "tok", "stats", "pos")}
    assert got == {"hist": h.tolist(), "emit": emit, "tok": tok, "stats": st, "pos": p}, (dl, pos, live)
    return ns


def test_accept_all_pairs_on_one_row_beside_busy_neighbours():
    k, B = 3, 3
    am = np.array([[10, 11, 12, 13], [20, 21, 22, 23], [30, 31, 32, 33]])
    hist = np.full((B, 64), -7)
    pairs = 0
    for row in range(B):
        for dl in range(k + 1):
            for m in range(dl + 1):                              # the first wrong draft: m of dl accepted
                draft = np.array([[a if i != (m if b == row else 1) else 99 for i, a in enumerate(am[b][:k])] for b in range(B)])
                dls = [dl if b == row else 3 for b in range(B)]
                ns = run_accept(am.reshape(-1), draft, dls, k, hist, [20, 40, 59], [[3, 4, 5], [0, 0, 0], [7, 8, 9]])
                assert ns[row] == m and [ns[b] for b in range(B) if b != row] == [1, 1]
                pairs += 1
    assert pairs == 3 * 10


def test_accept_at_the_end_of_the_cache_and_rows_that_are_not_live():
    k = 3
    for B in (1, 2, 4):
        am = np.arange(30, 30 + B * (k + 1))
        draft = am.reshape(B, k + 1)[:, :k].copy()               # every draft right
        for pos in ([21, 20, 23, 22][:B], [23, 0, 19, 21][:B]):  # hist has 24 columns: drafts partly, wholly, not at all inside
            for live in (None, [1, 0, 1, 0][:B], [0] * B):
                ns = run_accept(am, draft, [3] * B, k, np.full((B, 24), -7), pos, np.zeros((B, 3), dtype=np.int64), live=live)
                for b in range(B):
                    assert ns[b] == (None if live is not None and not live[b] else min(3, 24 - (pos[b] + 1)))
    assert run_accept(np.arange(8), [[0, 1, 2], [4, 5, 6]], [50, -4], k, np.full((2, 24), -7), [2, 2], np.zeros((2, 3)))[:2] == [3, 0]


def test_counters_rows():
    from valley_amd import ops
    for pos, k in (([0], 7), ([5, 300], 3), ([CTX - 1, CTX, -3, 17], 1), ([CTX + 9, 2], 2)):
        t, view = guarded(np.full((len(pos) * (k + 1),), -3))
        ops.spec_rows_counters(pos_tensor(pos), k, CTX, view)
        guards_intact({"ctr": (t, view)})
        assert view.tolist() == RR.counters(pos, k, CTX), (pos, k)


# ---- one sequence: the rows kernels against the single-sequence kernels (both call csrc/spec_lookup.inc) ---------------------------
WIDE = 1030                                                      # columns: a thread's second window start (t + 1024) exists


def twin_draft(hist, length, k, n, eos=(), vocab=0, lookup=True, len_add=1):
    """vly_spec_rows_draft at B = 1 and vly_spec_draft on the same tables: every output buffer equal, and equal to the reference."""
    from valley_amd import ops
    hist = np.asarray(hist).reshape(1, -1)
    before_d, before_dl = np.arange(50, 50 + k), [9]
    e = torch.tensor(list(eos), dtype=torch.int32, device=DEV) if len(eos) else None
    out = []
    for rows in (True, False):
        bufs = {"hist": guarded(hist if rows else hist[0]), "pos": guarded([length - len_add]),
                "draft": guarded(before_d.reshape(1, k) if rows else before_d), "dl": guarded(before_dl), "tok": guarded(np.full((k + 1,), -5))}
        fn = ops.spec_rows_draft if rows else ops.spec_draft
        fn(bufs["hist"][1], bufs["pos"][1], len_add, k, n, bufs["draft"][1], bufs["dl"][1], bufs["tok"][1], eos=e, vocab=vocab, lookup=lookup)
        guards_intact(bufs)
        assert bufs["hist"][1].reshape(-1).tolist() == hist[0].tolist() and bufs["pos"][1].tolist() == [length - len_add]
        out.append({name: bufs[name][1].reshape(-1).tolist() for name in ("draft", "dl", "tok")})
    d, dl, tok = RR.draft_rows(hist, [length], k, n, eos, vocab=vocab, lookup=lookup, draft=before_d, draft_len=before_dl)
    want = {"draft": d[0], "dl": dl, "tok": tok[0]}
    assert out[0] == out[1] == want, (length, k, n, eos, vocab, lookup, len_add, out, want)
    return want


def test_rows_draft_of_one_sequence_is_the_single_sequence_draft():
    g = np.random.default_rng(11)
    dense = g.integers(0, 4, size=WIDE)                          # four ids: every n-gram size finds a match early
    for length in (1, 2, 1029, 1030):
        for k in (1, 7):
            for n in (1, 8):
                twin_draft(dense, length, k, n)
                twin_draft(dense, length, k, n, eos=(3,))
    twin_draft(dense, 1029, 7, 8, len_add=2)
    for length in (1029, 1030):                                  # the caller's draft (9 tokens claimed), capped at the cache's end
        assert twin_draft(dense, length, 7, 8, lookup=False)["tok"][1:] == [50] * (WIDE - length) + [int(dense[length - 1])] * (7 - (WIDE - length))
    # one match, at a window start >= 1024: only the second round of the search (t + 1024) finds it
    # (1029 of 1030 columns known: the end of the cache leaves room for one drafted token)
    far = np.arange(1000, 1000 + WIDE)
    far[1024:1026] = far[1027:1029] = [11, 12]
    for k in (1, 7):
        for n in (8, 1):                                         # [11, 12] at start 1024; the 1-gram [12] at start 1025
            assert twin_draft(far, 1029, k, n) == {"draft": [2026] + [12] * (k - 1), "dl": [1], "tok": [12, 2026] + [12] * (k - 1)}
    assert twin_draft(far, 1030, 7, 8)["dl"] == [0]              # the sequence ends on [11, 12, 2029]: nothing matches
    # ... and the same n-gram at a start < 1024 as well: the earlier one wins
    both = far.copy()
    both[50:52] = [11, 12]
    assert twin_draft(both, 1029, 7, 8)["tok"] == [12, 1052] + [12] * 6
    assert twin_draft(both, 1029, 7, 8, eos=(2026,))["dl"] == [1]
    assert twin_draft(both, 1029, 7, 8, eos=(1052,)) == {"draft": [12] * 7, "dl": [0], "tok": [12] * 8}       # cropped by an EOS
    assert twin_draft(both, 1029, 7, 8, vocab=1053)["dl"] == [1]
    assert twin_draft(both, 1029, 7, 8, vocab=1052)["tok"] == [12] * 8                                        # ... by the vocabulary


def test_rows_accept_of_one_sequence_is_the_single_sequence_accept():
    from valley_amd import ops
    k = 3
    am = np.array([10, 11, 12, 13])
    pairs = 0
    for pos in (0, 19, 20, 21, 22, 23):                          # hist has 24 columns: drafts wholly, partly, not at all inside
        for dl in range(k + 1):
            for m in range(dl + 1):                              # the first wrong draft: m of dl accepted
                draft = np.array([a if i != m else 99 for i, a in enumerate(am[:k])])
                hist, stats = np.full((1, 24), -7), np.array([[3, 4, 5]])
                out = []
                for rows in (True, False):
                    flat = (lambda a: a) if rows else (lambda a: np.asarray(a).reshape(-1))
                    bufs = {"am": guarded(am), "draft": guarded(flat(draft.reshape(1, k))), "dl": guarded([dl]), "hist": guarded(flat(hist)),
                            "pos": guarded([pos]), "emit": guarded(flat(np.full((1, k + 2), -3))), "tok": guarded(np.full((k + 1,), -3)),
                            "stats": guarded(flat(stats))}
                    fn = ops.spec_rows_accept if rows else ops.spec_accept
                    fn(*(bufs[name][1] for name in ("am", "draft", "dl")), k, *(bufs[name][1] for name in ("hist", "pos", "emit", "tok", "stats")))
                    guards_intact(bufs)
                    assert bufs["am"][1].tolist() == am.tolist() and bufs["draft"][1].reshape(-1).tolist() == draft.tolist() and bufs["dl"][1].tolist() == [dl]
                    out.append({name: bufs[name][1].reshape(-1).tolist() for name in ("hist", "emit", "tok", "stats", "pos")})
                ns, h, emit, tok, st, p = RR.accept_rows(am, draft, [dl], k, hist, [pos], stats, emit=np.full((1, k + 2), -3), tok=[-3] * (k + 1))
                want = {"hist": h.reshape(-1).tolist(), "emit": emit[0], "tok": tok, "stats": st[0], "pos": p}
                assert out[0] == out[1] == want, (pos, dl, m, out, want)
                assert ns[0] == min(m, max(0, 24 - (pos + 1))) and want["tok"][0] == am[ns[0]]
                pairs += 1
    assert pairs == 6 * 10


# ---- the session ---------------------------------------------------------------------------------------------------------------
NEW = 16
REPEAT = [7, 8, 9] * 6                                           # a prompt whose continuation the lookup can find


@pytest.fixture(scope="module")
def golden():
    """The golden model and three prompts of different lengths (one left-padded, one text-only and repetitive); built once."""
    from tests.test_model_gpu import build_golden_model
    model = build_golden_model()
    T = G.GCFG["T"]
    img = torch.from_numpy(G.golden_pixels(T, "mixed")).view(1, T, 3, 224, 224).cuda()
    ids, mask = G.golden_ids("main")
    prompts = {"decode2": (torch.from_numpy(G.golden_ids("decode2")[0]).cuda(), None, img),
               "main1": (torch.from_numpy(ids[1:2]).cuda(), torch.from_numpy(mask[1:2]).cuda(), img),
               "repeat": (torch.tensor([REPEAT], dtype=torch.long).cuda(), None, None)}
    return model, prompts


def forced_tokens_single(model, prompt, k, truth_fn):
    """SpecDecodeSession of one sequence alone with forced drafts: per step, what ``truth_fn(tokens so far)`` drafts."""
    from valley_amd import ops
    from valley_amd.spec import SpecDecodeSession
    ids, mask, img = prompt
    ll = model.get_model().llama
    cache = ll.new_cache(1, ids.shape[1] + NEW + 16)
    out = model(input_ids=ids, images=img, attention_mask=mask, past_key_values=cache, use_cache=True)
    first = ops.argmax(out.logits[:, -1, :].contiguous())
    sess = SpecDecodeSession(ll, cache, k, use_graph=True, lookup=False)
    sess.begin(first, prompt_ids=ids[0])
    new, steps = [int(first[0])], []
    while len(new) < NEW:
        sess.draft.copy_(torch.tensor(truth_fn(new, k), dtype=torch.int32))
        sess.draft_len.fill_(k)
        got = sess.step()
        steps.append(len(got))
        new += got
    sess.check()
    return new, steps


@pytest.fixture(scope="module")
def greedy_truth(golden):
    model, prompts = golden
    truth = {}
    for name, (ids, mask, img) in prompts.items():
        seq = model.generate(ids, images=img, attention_mask=mask, max_new_tokens=NEW + 12, use_graph=True)
        truth[name] = seq[0, ids.shape[1]:].tolist()
    return truth


@pytest.mark.parametrize("use_graph", [True, False], ids=["graph", "eager"])
@pytest.mark.parametrize("k", [1, 3])
def test_session_forced_drafts_match_each_sequence_alone(golden, greedy_truth, k, use_graph):
    """Two sequences of different prompt lengths in one SpecRowsSession; sequence 0 is drafted the truth with its second draft
    wrong (one accepted per step for k = 3, all for k = 1), sequence 1 the truth with its first draft wrong every other step."""
    from valley_amd.spec import SpecRowsSession
    model, prompts = golden
    names = ["decode2", "main1"]
    V = G.GCFG["vocab"]

    def drafter(name, which):
        truth = greedy_truth[name]

        def fn(new, kk):
            nxt = truth[len(new):len(new) + kk]
            wrong = 1 if which == 0 else (0 if len(new) % 2 else kk)
            return [t if i != wrong else (t + 1) % V for i, t in enumerate(nxt)]
        return fn

    want = [forced_tokens_single(model, prompts[n], k, drafter(n, i)) for i, n in enumerate(names)]
    ll = model.get_model().llama
    depth = max(prompts[n][0].shape[1] for n in names) + NEW + 16
    cache = ll.new_cache(2, depth)
    cache.key_valid = torch.ones((2, depth), dtype=torch.uint8, device=ll.device)
    sess = SpecRowsSession(ll, cache, k, use_graph=use_graph, lookup=False)
    new = []
    for b, n in enumerate(names):
        ids, mask, img = prompts[n]
        row = type(cache).rows_of(cache, b, b + 1)
        out = model(input_ids=ids, images=img, attention_mask=mask, past_key_values=row, use_cache=True)
        first = int(out.logits[0, -1].argmax())
        sess.set_sequence(b, ids.shape[1], first, prompt_ids=ids[0])
        new.append([first])
    steps = [[], []]
    while min(len(x) for x in new) < NEW:
        for b, n in enumerate(names):
            if len(new[b]) < NEW:
                sess.draft[b].copy_(torch.tensor(drafter(n, b)(new[b], k), dtype=torch.int32))
                sess.draft_len[b:b + 1].fill_(k)
            elif int(sess.live[b]):
                sess.release(b)                                  # done: it rides along, unread
        got = sess.step()
        assert set(got) == {b for b in range(2) if len(new[b]) < NEW}
        for b, toks in got.items():
            steps[b].append(len(toks))
            new[b] += toks
        sess.check()
    for b, n in enumerate(names):
        if new[b] != want[b][0]:                                 # report the logits of the first difference's row
            print(n, "rows", new[b], "alone", want[b][0])
        assert new[b] == want[b][0] and steps[b] == want[b][1], (n, k)
        assert new[b][:NEW] == greedy_truth[n][:NEW]
        s = sess.speculation(b)
        assert s["steps"] == len(steps[b]) and s["steps"] + s["accepted"] == len(new[b]) - 1 and s["drafted"] == k * s["steps"]
        assert sess.hist[b, prompts[n][0].shape[1]:prompts[n][0].shape[1] + len(new[b])].tolist() == new[b]


# ---- the batcher ------------------------------------------------------------------------------------------------------------------
def serve(model, prompts, plan, spec, sampling, slots, ctx_max, steps=60):
    """Run ``plan`` — [(prompt name, join step, tokens wanted or None: until its slot is full, add() kwargs)] — on a batcher;
    -> (tokens per request, speculation per request or None, the slots used).  A request leaves once it has its tokens."""
    from valley_amd.serving import ContinuousBatcher
    cb = ContinuousBatcher(model, slots=slots, ctx_max=ctx_max, sampling=sampling, **spec)
    got, slot_of, done, stats = {}, {}, set(), {}
    for step in range(steps):
        for r, (name, at, n, kw) in enumerate(plan):
            if at == step:
                ids, mask, img = prompts[name]
                slot_of[r] = cb.add(ids, images=img, attention_mask=mask, **kw)
                got[r] = [int(cb.sess.tok[slot_of[r] * (spec.get("prompt_lookup_num_tokens", 0) + 1)])]
        for r, s in slot_of.items():
            n = plan[r][2]
            if r not in done and n is not None and len(got[r]) >= n:
                stats[r] = cb.speculation(s) if spec else None
                cb.release(s)
                done.add(r)
        if len(done) == len(plan):
            break
        toks = cb.step()
        for s in cb.full:                                        # released by the batcher: its cache rows are full
            r = next(r for r, s2 in slot_of.items() if s2 == s and r not in done)
            stats[r] = cb.speculation(s) if spec else None
            done.add(r)
        for r, s in slot_of.items():
            if r not in done and s in toks:
                got[r] += toks[s] if spec else [toks[s]]
    assert len(done) == len(plan), (done, {r: len(t) for r, t in got.items()})
    return got, stats, slot_of


def batcher_plan(sampling):
    kw = (lambda seed: dict(temperature=0.8, top_k=50, seed=seed)) if sampling else (lambda seed: {})
    # request 2 leaves mid-run and request 3 reuses its slot; request 4 (slots permitting) runs to the end of its cache
    return [("repeat", 0, 14, kw(11)), ("decode2", 1, 12, kw(12)), ("main1", 2, 5, kw(13)), ("repeat", 9, 10, kw(14))]


def batcher_matches_plain(model, prompts, slots, k, sampling):
    """Every request's tokens from the speculating batcher == the plain batcher's, the counters add up, and a request that runs to
    the end of its slot's cache gets its last tokens from steps with dead rows."""
    plan = batcher_plan(sampling)[:4 if slots >= 4 else 2]
    if slots == 2:                                               # two slots: request 1 leaves early and request 2 reuses its slot
        plan[1] = (plan[1][0], 1, 4, plan[1][3])
        plan.append(("repeat", 6, 9, dict(temperature=0.8, top_k=50, seed=15) if sampling else {}))
    ctx_max = 320
    spec = dict(prompt_lookup_num_tokens=k, max_matching_ngram_size=2)
    want, _, slots_plain = serve(model, prompts, plan, {}, sampling, slots, ctx_max)
    got, stats, slots_spec = serve(model, prompts, plan, spec, sampling, slots, ctx_max)
    accepted = 0
    for r in range(len(plan)):
        n = plan[r][2]
        assert got[r][:n] == want[r][:n], (slots, k, sampling, r, got[r], want[r])
        assert stats[r]["steps"] + stats[r]["accepted"] == len(got[r]) - 1 and stats[r]["accepted"] <= stats[r]["drafted"] <= k * stats[r]["steps"]
        accepted += stats[r]["accepted"]
    assert len(set(slots_spec.values())) < len(plan)              # a released slot was reused
    return accepted, stats


@pytest.mark.parametrize("sampling", [False, True], ids=["greedy", "seeded"])
@pytest.mark.parametrize("slots,k", [(2, 3), (4, 1)])
def test_batcher_speculation_is_the_plain_batcher(golden, slots, k, sampling):
    model, prompts = golden
    accepted, stats = batcher_matches_plain(model, prompts, slots, k, sampling)
    print(f"slots={slots} k={k} sampling={sampling}: {stats}")
    if not sampling:
        assert stats[0]["accepted"] > 0, "the repetitive prompt: at least one draft accepted"


@pytest.mark.parametrize("sampling", [False, True], ids=["greedy", "seeded"])
@pytest.mark.parametrize("slots,k", [(2, 3), (4, 1)])
def test_batcher_runs_a_request_to_the_end_of_its_cache(golden, slots, k, sampling):
    """ctx_max = the prompt + 7: the request gets 7 tokens from steps and is then released as full.  Its last three tokens come
    from steps whose rows (position + j >= ctx_max) are partly dead — with k = 3 the step at ctx_max - 3 has one dead row, the
    next ones more — and equal the plain batcher's; a neighbour decodes beside it throughout."""
    model, prompts = golden
    S = prompts["decode2"][0].shape[1]
    kw = (lambda seed: dict(temperature=0.8, top_k=50, seed=seed)) if sampling else (lambda seed: {})
    plan = [("decode2", 0, None, kw(21)), ("repeat", 0, 9, kw(22))]
    spec = dict(prompt_lookup_num_tokens=k)
    want, _, _ = serve(model, prompts, plan, {}, sampling, slots, S + 7)
    got, stats, _ = serve(model, prompts, plan, spec, sampling, slots, S + 7)
    assert len(want[0]) == 8 and got[0] == want[0], (got[0], want[0])     # the first token + 7 from steps
    assert got[1][:9] == want[1][:9]
    assert stats[0]["steps"] + stats[0]["accepted"] == 7


def test_batcher_speculation_on_the_int8_engine():
    from tests.test_model_gpu import build_golden_model
    model = build_golden_model()
    model.quantize_decode_weights("int8")
    T = G.GCFG["T"]
    img = torch.from_numpy(G.golden_pixels(T, "mixed")).view(1, T, 3, 224, 224).cuda()
    prompts = {"decode2": (torch.from_numpy(G.golden_ids("decode2")[0]).cuda(), None, img),
               "repeat": (torch.tensor([REPEAT], dtype=torch.long).cuda(), None, None)}
    plan = [("repeat", 0, 12, {}), ("decode2", 1, 3, {}), ("repeat", 5, 6, {})]       # request 2 reuses request 1's slot
    want, _, _ = serve(model, prompts, plan, {}, False, 2, 320)
    got, stats, _ = serve(model, prompts, plan, dict(prompt_lookup_num_tokens=3), False, 2, 320)
    for r in range(3):
        assert got[r][:plan[r][2]] == want[r][:plan[r][2]], (r, got[r], want[r])
        assert stats[r]["steps"] + stats[r]["accepted"] == len(got[r]) - 1


# ---- the fp16 storage type, and a run that never speculates -------------------------------------------------------------------
def _worker(mode, env_extra):
    env = {k: v for k, v in os.environ.items() if k not in ("VALLEY_PRECISION", "VALLEY_SPEC_ATTN")}
    env.update(env_extra)
    env["VALLEY_TUNE_ONLINE"] = "0"                              # as in this module: every prefill of a shape runs the same kernel
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "spec_rows_worker.py"), mode], capture_output=True, text=True, env=env,
                       timeout=600)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    return json.loads(p.stdout.strip().splitlines()[-1])


def test_spec_rows_on_the_fp16_library():
    res = _worker("fp16", {"VALLEY_PRECISION": "fp16"})
    assert res["ok"] and res["storage"] == 1 and res["positions"] == len(POSITIONS) and res["accepted"] >= 0


def test_a_plain_batcher_never_loads_the_rows_library():
    res = _worker("off", {})
    assert res["ok"] and res["tokens"] == 4 and res["rows_lib_loaded"] is False
