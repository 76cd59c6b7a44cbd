"""Token constraints on the MI355X: vly_constrain_apply against the reference of tests/constrain_ref.py (pinned to
transformers by tests/test_constrain_cpu.py) — exact: every value, and the bits of every entry no rule touched — a captured
launch replayed with new rows, tables and lengths, and generate() / ContinuousBatcher end to end on the golden model against
the reference loop with transformers' own processors over the HIP forward's logits."""
import os
import subprocess
import sys

import pytest
import torch

from tests import constrain_ref as CR
from tests import golden_cfg as G
from tests import logits_ref
from tests.test_logits_process_gpu import beam_stepper, greedy_stepper, inputs

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EOS = [2, 5]
FLAG = {"bad": 1, "trie": 2, "forced": 4, "suppress": 8, "begin": 16}


def dev():
    return torch.device("cuda:0")


def scores(R, V, ld, seed):
    """Random logits with a -inf, a -0.0 and a NaN per row where they fit, NaN in the padding columns."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn((R, ld), generator=g) * 3
    x[:, V:] = float("nan")
    for r in range(R):
        if V > 40:
            x[r, 7 + r], x[r, 20 + r], x[r, 30 + r] = float("-inf"), -0.0, float("nan")
    return x


def check(x, hist, lens, spec, V, bad=None, sup=None, beg=None, eos=EOS, tries=(), length="rows", len_add=0, len_dev=None):
    """Launch on rows described by ``spec`` — per row {"on": rule names, "begin", "max_length", "trie": index into tries} — and
    compare with the reference.  ``lens``: the rows' lengths AFTER len_add and the clamp; ``len_dev``: what the device holds."""
    from valley_amd import ops
    R, ld = x.shape
    eos = [e for e in eos if e < V] or [0]
    cap = {"trie": max([len(ops.pack_trie(t, V)) for t in tries], default=0), "trie_slots": max(1, len(tries))}
    tables = ops.constraint_tables(bad, sup, beg, eos=eos or None, V=V, capacity=cap, device=dev())
    roots = [ops.constraint_trie(tables, i, t) for i, t in enumerate(tries)]
    rows = ops.constraint_rows(tables, R, begin=[s.get("begin", 0) for s in spec], max_length=[s.get("max_length", 0) for s in spec],
                               trie_root=[roots[s["trie"]] if "trie" in s else -1 for s in spec],
                               flags=[sum(FLAG[n] for n in s["on"]) for s in spec], device=dev())
    if len_dev is None:
        len_dev = torch.tensor([n - len_add for n in lens] if length == "rows" else [lens[0] - len_add], dtype=torch.int32)
    xd = x.to(dev())
    ops.constrain(xd[:, :V], rows, tables, hist.to(dev()), None if length == "none" else len_dev.to(dev()), len_add)
    got = xd.cpu()
    assert CR.same_bits(got[:, V:], x[:, V:])                                         # the padding columns are never touched
    for r, s in enumerate(spec):
        on = s["on"]
        want = CR.constrain_row(x[r, :V], hist[r, :lens[r]].tolist(), bad_words=bad if "bad" in on else None,
                                allowed=tries[s["trie"]] if "trie" in on and "trie" in s else None,
                                max_length=s.get("max_length", 0) if "forced" in on else 0, suppress=(sup or []) if "suppress" in on else None,
                                begin_suppress=(beg or []) if "begin" in on else None, begin=s.get("begin", 0), eos=eos)
        assert CR.same_values(got[r, :V], want), (r, s)
        keep = torch.isfinite(want) & (want == x[r, :V])
        assert torch.equal(got[r, :V][keep].view(torch.int32), x[r, :V][keep].view(torch.int32)), (r, s)   # untouched: bit for bit
        if not on:
            assert CR.same_bits(got[r], x[r])                                         # a neutral row is not written
    return got


# ---- shapes and lengths -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("V", [1, 63, 1025, 32000, 32003])
@pytest.mark.parametrize("R", [1, 3, 8])
def test_shapes(V, R):
    g = torch.Generator().manual_seed(V + R)
    ld, hist_ld = V + 5, 40
    x = scores(R, V, ld, seed=V * 10 + R)
    hist = torch.randint(0, min(V, 6), (R, hist_ld), generator=g, dtype=torch.int32)
    lens = [int(torch.randint(3, hist_ld + 1, (1,), generator=g)) for _ in range(R)]
    ids = lambda n: torch.randint(0, V, (n,), generator=g).tolist()                   # noqa: E731
    bad = [[t] for t in ids(3)] + [ids(2) for _ in range(3)] + [hist[0, lens[0] - 2:lens[0]].tolist() + ids(1)]
    tries = [[ids(2), ids(1), ids(3)], [hist[R - 1, lens[R - 1] - 1:lens[R - 1]].tolist() + ids(2), ids(1)]]
    names = ["bad", "suppress", "begin", "trie", "forced"]
    spec = []
    for r in range(R):
        on = [n for i, n in enumerate(names) if (r + i) % 2 == 0 or R == 1] if r != 1 else []      # row 1 is neutral
        s = {"on": on, "begin": lens[r] - (r % 2), "max_length": lens[r] + 1 + (r % 3 == 2)}
        if "trie" in on:
            s["trie"] = r % 2 if r != R - 1 else 1
        spec.append(s)
    spec[R - 1]["begin"] = lens[R - 1] - 1                                            # the last row stands one id into its trie
    check(x, hist, lens, spec, V, bad=bad, sup=ids(4) + [V - 1], beg=ids(2), tries=tries)


@pytest.mark.parametrize("length,len_add", [("rows", 0), ("rows", 1), ("one", 0), ("one", 1), ("none", 9)])
def test_length_sources(length, len_add):
    V, R, hist_ld = 300, 3, 24
    x = scores(R, V, V + 3, seed=len_add)
    hist = torch.randint(0, 5, (R, hist_ld), dtype=torch.int32, generator=torch.Generator().manual_seed(2))
    lens = [9, 14, 20] if length == "rows" else [9, 9, 9]
    spec = [{"on": ["bad", "begin", "forced", "trie"], "begin": n - 1, "max_length": n + 1, "trie": 0} for n in lens]
    spec[1]["begin"] = lens[1]                                                        # begin-suppress fires; so does the forced EOS
    spec[0]["max_length"], spec[2]["max_length"] = lens[0] + 2, lens[2] + 2           # one step before the forced EOS
    bad = [hist[0, lens[0] - 3:lens[0]].tolist() + [77], [3, 78]]
    tries = [[[0, 10], [1, 11], [2, 12], [3, 13], [4, 14], [4]]]
    check(x, hist, lens, spec, V, bad=bad, beg=[4, 6], tries=tries, length=length, len_add=len_add)


def test_length_is_clamped_at_the_history_width():
    V, hist_ld = 300, 16
    x = scores(2, V, V, seed=3)
    hist = torch.randint(0, 5, (2, hist_ld), dtype=torch.int32, generator=torch.Generator().manual_seed(4))
    spec = [{"on": ["bad", "forced"], "begin": 3, "max_length": hist_ld + 1}, {"on": ["bad", "forced"], "begin": 3, "max_length": 31}]
    bad = [hist[0, hist_ld - 2:].tolist() + [77], hist[1, hist_ld - 4:].tolist() + [78]]
    # the device holds 30 and 1000: both rows are read as 16 ids; row 0's forced EOS fires at the clamped length, row 1's
    # (max_length - 1 = 30, the unclamped value) does not
    check(x, hist, [hist_ld, hist_ld], spec, V, bad=bad, len_add=1, len_dev=torch.tensor([29, 999], dtype=torch.int32))


# ---- bad words ----------------------------------------------------------------------------------------------------------------
def test_bad_words():
    V, hist_ld, R = 5000, 80, 6
    g = torch.Generator().manual_seed(11)
    x = scores(R, V, V + 1, seed=12)
    hist = torch.randint(10, 4000, (R, hist_ld), generator=g, dtype=torch.int32)
    hist[4, :12] = 0                                                                  # row 4: left padding
    lens = [70, 64, 63, 5, 12, 70]
    tail = lambda r, n: hist[r, lens[r] - n:lens[r]].tolist()                         # noqa: E731
    bad = [[4001], tail(0, 1) + [4002], tail(0, 4) + [4003], tail(0, 63) + [4004],    # lengths 1, 2, 5, 64 on row 0
           tail(1, 63) + [4005],                                                      # L == len on row 1 (64): applies
           tail(2, 63) + [4006],                                                      # L == len + 1 on row 2 (its head is the WHOLE row): skipped
           [0, 0, 0, 4007],                                                           # a match wholly in row 4's left padding
           tail(0, 1) + [4002], [4001],                                               # duplicates
           tail(0, 2) + [4002],                                                       # two words ban one token
           tail(3, 4) + [4008], tail(3, 5) + [4009],                                  # len = 5: L = 5 applies, L = 6 does not
           [2], [5], [4001, 2]]                                                       # [eos] words are dropped; a word ENDING in eos is not
    spec = [{"on": ["bad"]} for _ in range(R)]
    spec[5] = {"on": []}
    got = check(x, hist, lens, spec, V, bad=bad)
    ninf = float("-inf")
    assert got[0, 4001] == ninf and got[0, 4002] == ninf and got[0, 4003] == ninf and got[0, 4004] == ninf
    assert got[1, 4005] == ninf and got[2, 4006] == x[2, 4006] and got[4, 4007] == ninf and got[0, 4007] == x[0, 4007]
    assert got[3, 4008] == ninf and got[3, 4009] == x[3, 4009] and got[0, 2] == x[0, 2] and got[0, 5] == x[0, 5]


def test_three_thousand_bad_words():
    """More words than the workgroup has threads: three passes, the hits spread over all of them."""
    V, hist_ld = 32000, 32
    g = torch.Generator().manual_seed(13)
    x = scores(2, V, V, seed=14)
    hist = torch.randint(0, 50, (2, hist_ld), generator=g, dtype=torch.int32)
    lens = [30, 17]
    bad = [[int(a), int(b), 100 + i] for i, (a, b) in enumerate(torch.randint(0, 50, (3000, 2), generator=g).tolist())]
    for i in (0, 1023, 1024, 2047, 2048, 2999):
        bad[i][:2] = hist[i % 2, lens[i % 2] - 2:lens[i % 2]].tolist()
    got = check(x, hist, lens, [{"on": ["bad"]}] * 2, V, bad=bad)
    assert int((got[0, :V] == float("-inf")).sum()) >= 3 and int((got[1, :V] == float("-inf")).sum()) >= 3


# ---- suppress, begin-suppress, forced EOS -------------------------------------------------------------------------------------
@pytest.mark.parametrize("sup", [None, [17], [0, 299, 299, 17, 0]])
def test_suppress_lists(sup):
    """An empty table under a set flag, one id, duplicates and V - 1; begin-suppress at len == begin, begin - 1, begin + 1."""
    V = 300
    x = scores(4, V, V + 2, seed=15)
    hist = torch.zeros((4, 12), dtype=torch.int32)
    spec = [{"on": ["suppress", "begin"], "begin": b} for b in (8, 9, 7)] + [{"on": []}]
    got = check(x, hist, [8, 8, 8, 8], spec, V, sup=sup, beg=[40, 41, 299])
    assert got[0, 40] == float("-inf") and got[1, 40] == x[1, 40] and got[2, 41] == x[2, 41]


def test_forced_eos():
    V = 300
    x = scores(4, V, V, seed=16)
    hist = torch.zeros((4, 12), dtype=torch.int32)
    spec = [{"on": ["forced"], "max_length": 10}, {"on": ["forced"], "max_length": 11}, {"on": ["forced", "suppress"], "max_length": 10},
            {"on": ["forced"], "max_length": 0}]
    got = check(x, hist, [9, 9, 9, 9], spec, V, sup=[5, 6])
    assert got[0, 2] == 0 and got[0, 5] == 0 and int(torch.isfinite(got[0, :V]).sum()) == 2          # two EOS ids
    assert CR.same_bits(got[1], x[1]) and CR.same_bits(got[3], x[3])                              # max_length - 2; off
    assert got[2, 2] == 0 and got[2, 5] == float("-inf")                                          # a suppressed EOS id ends -inf


# ---- the trie -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fan", [1, 64, 65, 1500])
def test_trie_fan_out(fan):
    """Fan-out ``fan`` at the root and again one level down; rows at the root, behind the first, a middle and the last child,
    and behind an id between two children (out of the trie)."""
    V = 32003
    kids = list(range(3, 3 + 2 * fan, 2))                                             # odd ids: the even ones between them miss
    tries = [[[a, b] for a in (kids[0], kids[fan // 2], kids[-1]) for b in kids] + [[k] for k in kids]]
    firsts = [None, kids[0], kids[fan // 2], kids[-1], kids[fan // 2] + 1, kids[-1] + 2, 1]
    R = len(firsts)
    x = scores(R, V, V, seed=fan)
    hist = torch.zeros((R, 16), dtype=torch.int32)
    lens, spec = [], []
    for r, f in enumerate(firsts):
        lens.append(8 if f is None else 9)
        if f is not None:
            hist[r, 8] = f
        spec.append({"on": ["trie"], "begin": 8, "trie": 0})
    got = check(x, hist, lens, spec, V, tries=tries)
    assert int(torch.isfinite(got[0, :V]).sum()) >= fan - 3 and int(torch.isfinite(got[4, :V]).sum()) <= 2


def test_trie_depth_ends_and_leaves():
    V = 1025
    deep = list(range(100, 164))                                                      # one sequence of 64 ids
    tries = [[deep, [7], [7, 8], [7, 8, 9], [20]], [[30, 31], [40]]]
    rows = [(0, []), (0, [100]), (0, deep[:63]), (0, deep), (0, deep + [1]),          # the root; depth 1, 63, 64 (a leaf); 65 generated ids
            (0, [7]), (0, [7, 8]), (0, [7, 8, 9]), (0, [20]),                         # nodes that end a sequence AND have children; leaves
            (0, [101]), (0, deep[:63] + [5]), (0, [7, 8, 10]),                        # leaves the trie at the first / the last id
            (1, [30]), (1, []), (None, [30])]                                         # another root in the same launch; a neutral row
    R, begin = len(rows), 6
    x = scores(R, V, V + 7, seed=17)
    hist = torch.randint(0, 50, (R, 80), dtype=torch.int32, generator=torch.Generator().manual_seed(18))
    lens, spec = [], []
    for r, (t, g) in enumerate(rows):
        hist[r, begin:begin + len(g)] = torch.tensor(g, dtype=torch.int32)
        lens.append(begin + len(g))
        spec.append({"on": [], "begin": begin} if t is None else {"on": ["trie"], "begin": begin, "trie": t})
    got = check(x, hist, lens, spec, V, tries=tries)
    fin = lambda r: torch.isfinite(got[r, :V]).nonzero().view(-1).tolist()            # noqa: E731
    assert set(fin(0)) <= {100, 7, 20} and set(fin(3)) <= set(EOS) and set(fin(4)) <= set(EOS) and set(fin(5)) <= {8, *EOS}
    assert set(fin(12)) <= {31} and set(fin(13)) <= {30, 40}


# ---- capture ------------------------------------------------------------------------------------------------------------------
def test_captured_launch_replays_new_rows_tables_and_lengths():
    from valley_amd import ops
    R, V, hist_ld = 4, 32000, 48
    g = torch.Generator().manual_seed(21)
    cap = {"eos": 2, "suppress": 8, "begin": 4, "words": 400, "trie": 300, "trie_slots": 2}
    tables = ops.constraint_tables(eos=[2], V=V, capacity=cap, device=dev())
    logits = torch.empty((R, V), device=dev())
    rows = ops.constraint_rows(tables, R, flags=0, device=dev())
    hist = torch.zeros((R, hist_ld), dtype=torch.int32, device=dev())
    length = torch.zeros((R,), dtype=torch.int32, device=dev())

    def fill(k):
        """round k: other lists and counts, other tries, other rows, other lengths"""
        x = torch.randn((R, V), generator=g) * 3
        h = torch.randint(0, 6, (R, hist_ld), generator=g, dtype=torch.int32)
        lens = torch.randint(8, 40, (R,), generator=g).tolist()
        eos = [[2], [2, 5], [9]][k]
        bad = [[int(h[0, lens[0] - 1]), 100 + k]] + [[200 + i] for i in range(k * 30)]
        sup = [None, [300, 301], [302]][k]
        beg = [[400], None, [401, 402, 403]][k]
        tries = [[[1, 2, 3], [4]], [[0], [1], [2], [3], [4], [5, 5]]] if k != 1 else [[[5, 4], [5]], [[3]]]
        tables.write(bad, sup, beg, eos)
        roots = [ops.constraint_trie(tables, i, t) for i, t in enumerate(tries)]
        spec = [dict(begin=lens[r] - (r + k) % 2, max_length=lens[r] + 1 + (r + k) % 2, trie=(r + k) % 2) for r in range(R)]
        rows.copy_(ops.constraint_rows(tables, R, begin=[s["begin"] for s in spec], max_length=[s["max_length"] for s in spec],
                                       trie_root=[roots[s["trie"]] for s in spec]))
        logits.copy_(x)
        hist.copy_(h)
        length.copy_(torch.tensor(lens, dtype=torch.int32))
        want = [CR.constrain_row(x[r], h[r, :lens[r]].tolist(), bad_words=bad, allowed=tries[spec[r]["trie"]], max_length=spec[r]["max_length"],
                                 suppress=sup, begin_suppress=beg, begin=spec[r]["begin"], eos=eos) for r in range(R)]
        return torch.stack(want)

    fill(0)
    ops.constrain(logits, rows, tables, hist, length, 0)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ops.constrain(logits, rows, tables, hist, length, 0)
    for k in (1, 2, 0):
        want = fill(k)
        graph.replay()
        assert CR.same_values(logits.cpu(), want), k


# ---- generate() end to end ----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def model():
    from tests.test_model_gpu import build_golden_model
    return build_golden_model()


def ref_greedy(model, ids, mask, img, max_new, eos=None, repetition_penalty=None, **kw):
    """HF's greedy loop with HF's own processors, in its order, over the HIP forward's logits."""
    S = ids.shape[1]
    front = logits_ref.hf_processors(repetition_penalty, prompt_len=S, eos=eos)
    procs = CR.hf_constraint_processors(kw.get("bad_words_ids"), kw.get("allowed_sequences"), S + max_new if "forced_eos_token_id" in kw else 0,
                                        kw.get("suppress_tokens"), kw.get("begin_suppress_tokens"), begin=S, eos=eos, front=front)
    return logits_ref.greedy_loop(greedy_stepper(model, ids, mask, img), ids, max_new, procs, eos=eos, pad=0)


def cases(plain, S):
    """Constraints that bite on what greedy decoding says: its first token, a later token, a bigram of it."""
    E, t = 2, plain[:, S:].tolist()
    choices = [[11], [12, 13], [14, 15, 16, 17]]
    return {
        "bad_words": dict(bad_words_ids=[[t[0][0]], t[1][1:3], t[0][2:5], [E]]),
        "suppress": dict(suppress_tokens=sorted({t[0][1], t[1][2]})),
        "begin_suppress": dict(begin_suppress_tokens=sorted({t[0][0], t[1][0]})),
        "forced_eos": dict(forced_eos_token_id=E),
        "allowed": dict(allowed_sequences=choices),
        "allowed_per_row": dict(allowed_sequences=[choices, [[21, 22], [23]]]),
        "all": dict(bad_words_ids=[[18]], suppress_tokens=[12], begin_suppress_tokens=[11], forced_eos_token_id=E,
                    allowed_sequences=[[11], [12, 13], [14, 15, 16, 17, 19, 20, 21, 22], [18, 19], [30, 31, 32, 33, 34, 35, 36, 37]]),
    }


@pytest.mark.parametrize("name", ["bad_words", "suppress", "begin_suppress", "forced_eos", "allowed", "allowed_per_row", "all"])
@pytest.mark.parametrize("rp", [None, 1.3])
def test_generate_greedy_matches_reference_in_every_route(model, name, rp):
    ids, mask, img = inputs("main")
    S, new, E = ids.shape[1], 6, 2
    plain = model.generate(ids, images=img, attention_mask=mask, max_new_tokens=new)
    kw = cases(plain, S)[name]
    if rp is not None:
        kw["repetition_penalty"] = rp
    ref = ref_greedy(model, ids, mask, img, new, eos=E, **kw)
    assert not torch.equal(ref[:, :plain.shape[1]], plain[:, :ref.shape[1]])         # the constraint changed the output
    for ug in (True, False, None):
        got = model.generate(ids, images=img, attention_mask=mask, max_new_tokens=new, eos_token_id=E, pad_token_id=0, use_graph=ug, **kw)
        assert torch.equal(got, ref), (name, ug, got[:, S:], ref[:, S:])


def test_allowed_sequences_end_in_one_choice_then_eos(model):
    ids, mask, img = inputs("main")
    S, E = ids.shape[1], 2
    choices = [[11], [12, 13], [14, 15, 16, 17]]
    for ug in (True, False, None):
        got = model.generate(ids, images=img, attention_mask=mask, max_new_tokens=8, eos_token_id=E, pad_token_id=0, use_graph=ug,
                             allowed_sequences=choices)
        for r in range(ids.shape[0]):
            tail = got[r, S:].tolist()
            assert E in tail and tail[:tail.index(E)] in choices and set(tail[tail.index(E) + 1:]) <= {0}, (ug, tail)


def test_seeded_and_host_sampling_keep_the_constraints(model):
    ids, mask, img = inputs("main")
    S, E = ids.shape[1], 2
    plain = model.generate(ids, images=img, attention_mask=mask, max_new_tokens=8, do_sample=True, temperature=0.9, top_k=50, seed=11)
    banned = sorted(set(plain[:, S:].reshape(-1).tolist()) - {E})
    kw = dict(images=img, attention_mask=mask, max_new_tokens=8, do_sample=True, temperature=0.9, eos_token_id=E, pad_token_id=0,
              suppress_tokens=banned, forced_eos_token_id=E, repetition_penalty=1.2)
    outs = [model.generate(ids, use_graph=ug, top_k=50, seed=11, **kw) for ug in (True, False, None)]
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2])
    assert not torch.isin(outs[0][:, S:], torch.tensor(banned, device=ids.device)).any() and bool((outs[0][:, S:] == E).any(-1).all())
    host = []
    for ug in (True, False, None):                                                   # torch.multinomial over the constrained logits
        torch.manual_seed(3)
        host.append(model.generate(ids, use_graph=ug, **kw))
        assert not torch.isin(host[-1][:, S:], torch.tensor(banned, device=ids.device)).any() and bool((host[-1][:, S:] == E).any(-1).all())
    assert torch.equal(host[0], host[1]) and torch.equal(host[0], host[2])


def test_logprobs_stay_those_of_the_raw_logits(model):
    """token_logprobs = log_softmax(UNconstrained logits)[token], two ways.  (a) In every route: suppressing each step's
    runner-up (and banning it as a word) rewrites the logits the token is picked from but not the pick, so the sequences,
    token_logprobs and the top-2 tables must equal the unconstrained call's of the same route BIT FOR BIT; a log_softmax
    of the constrained row would move every value by -log(1 - p(runner-up)), p >= 1e-3 asserted.  (b) Where the constraints
    do change the tokens: in the generic-forward route the teacher-forced forward IS generate's own, so the values must
    meet tests/test_score_gpu.py's bound for the same comparison without constraints (1e-6 of the scale, against float64)."""
    from tests.test_score_gpu import bits, within
    ids, mask, img = inputs("main")
    S, new, E = ids.shape[1], 6, 2
    base = dict(images=img, attention_mask=mask, max_new_tokens=new, output_logprobs=True, top_logprobs=2, return_dict_in_generate=True)
    for ug in (True, False, None):
        plain = model.generate(ids, use_graph=ug, **base)
        said = set(plain.sequences[:, S:].reshape(-1).tolist())
        second = [t for t in sorted(set(plain.top_tokens[:, :, 1].reshape(-1).tolist())) if t not in said]
        assert second and float(plain.top_logprobs[:, :, 1].exp().min()) >= 1e-3
        got = model.generate(ids, use_graph=ug, suppress_tokens=second, bad_words_ids=[[t] for t in second], **base)
        assert torch.equal(got.sequences, plain.sequences), ug
        assert torch.equal(bits(got.token_logprobs), bits(plain.token_logprobs)), ug
        assert torch.equal(got.top_tokens, plain.top_tokens) and torch.equal(bits(got.top_logprobs), bits(plain.top_logprobs)), ug
    plain = model.generate(ids, images=img, attention_mask=mask, max_new_tokens=new)
    kw = dict(cases(plain, S)["all"], eos_token_id=E, pad_token_id=0)
    raw = []
    step = greedy_stepper(model, ids, mask, img)
    recorder = lambda tok: raw.append(step(tok).clone()) or raw[-1]                   # noqa: E731  (a copy: the forward may reuse its buffer)
    procs = CR.hf_constraint_processors(kw["bad_words_ids"], kw["allowed_sequences"], S + new, kw["suppress_tokens"],
                                        kw["begin_suppress_tokens"], begin=S, eos=E)
    ref = logits_ref.greedy_loop(recorder, ids, new, procs, eos=E, pad=0)
    n = ref.shape[1] - S
    want = torch.stack([torch.log_softmax(raw[i].double(), -1).gather(1, ref[:, S + i:S + i + 1])[:, 0] for i in range(n)], 1)
    done = torch.zeros_like(want, dtype=torch.bool)
    for i in range(1, n):
        done[:, i] = done[:, i - 1] | (ref[:, S + i - 1] == E)
    want = torch.where(done, torch.zeros_like(want), want)
    got = model.generate(ids, images=img, attention_mask=mask, max_new_tokens=new, use_graph=None, output_logprobs=True,
                         return_dict_in_generate=True, **kw)
    assert torch.equal(got.sequences, ref)
    within(got.token_logprobs, want.cpu().numpy(), "generic-forward route, constrained tokens: token_logprobs")
    for ug in (True, False):                                                          # the session routes: the same tokens, values recorded
        o = model.generate(ids, images=img, attention_mask=mask, max_new_tokens=new, use_graph=ug, output_logprobs=True,
                           return_dict_in_generate=True, **kw)
        assert torch.equal(o.sequences, ref) and o.token_logprobs.shape == got.token_logprobs.shape
        print(f"use_graph={ug}: max |token_logprobs - generic route's| = {float((o.token_logprobs - got.token_logprobs).abs().max()):.3e}")


def test_beams_take_bad_words_and_suppressed_tokens(model):
    ids, mask, img = inputs("main")
    S, nb, new = ids.shape[1], 2, 5
    plain = model.generate(ids, images=img, attention_mask=mask, max_new_tokens=new, num_beams=nb)
    t = plain[:, S:].tolist()
    kw = dict(bad_words_ids=[[t[0][0]], t[1][1:3]], suppress_tokens=sorted({t[0][1], t[1][0]}), begin_suppress_tokens=[t[0][2]])
    step, reorder = beam_stepper(model, ids, mask, img, nb)
    procs = CR.hf_constraint_processors(kw["bad_words_ids"], None, 0, kw["suppress_tokens"], kw["begin_suppress_tokens"], begin=S)
    ref, _ = logits_ref.beam_loop(step, reorder, ids, nb, new, procs)
    assert not torch.equal(ref.cuda(), plain)
    for ug in (True, False, None):
        got = model.generate(ids, images=img, attention_mask=mask, max_new_tokens=new, num_beams=nb, use_graph=ug, **kw)
        assert torch.equal(got, ref.cuda()), ug


def test_refusals(model):
    ids, mask, img = inputs("main")
    kw = dict(images=img, attention_mask=mask, max_new_tokens=4)
    with pytest.raises(ValueError, match="not supported with num_beams > 1"):
        model.generate(ids, num_beams=2, eos_token_id=2, allowed_sequences=[[11]], **kw)
    with pytest.raises(ValueError, match="not supported with num_beams > 1"):
        model.generate(ids, num_beams=2, eos_token_id=2, forced_eos_token_id=2, **kw)
    with pytest.raises(ValueError, match="prompt_lookup_num_tokens is not supported with token constraints"):
        model.generate(ids[:1], images=img[:1], max_new_tokens=4, prompt_lookup_num_tokens=3, suppress_tokens=[5])
    with pytest.raises(ValueError, match="needs an `eos_token_id`"):
        model.generate(ids, allowed_sequences=[[11]], **kw)
    with pytest.raises(ValueError, match="needs an `eos_token_id`"):
        model.generate(ids, forced_eos_token_id=2, **kw)
    with pytest.raises(ValueError, match="The model vocabulary size is"):
        model.generate(ids, bad_words_ids=[[model.model.llama.V]], **kw)
    from valley_amd.serving import ContinuousBatcher
    with pytest.raises(ValueError, match="does not combine with constraints=True"):
        ContinuousBatcher(model, slots=2, prompt_lookup_num_tokens=2, constraints=True, eos_token_id=2)
    with pytest.raises(ValueError, match="needs ContinuousBatcher"):
        ContinuousBatcher(model, slots=2, ctx_max=512).add(ids[:1], images=img[:1], allowed_sequences=[[11]])


def test_a_prefix_session_turn_takes_bad_words():
    from tests import suffix_cases as SC
    from tests.test_model_gpu import build_golden_model
    from tests.test_prefix_gpu import HandPrefix, copy_rows, session
    model = build_golden_model()
    T = G.GCFG["T"]
    img = torch.from_numpy(G.golden_pixels(T, "mixed")).view(1, T, 3, 224, 224).cuda()
    ids1 = torch.from_numpy(G.golden_ids("decode2")[0]).cuda()
    s = session(model, "prefill")
    seq1 = model.generate(ids1, images=img, prefix=s, max_new_tokens=SC.TURN1_NEW)
    ids2 = torch.tensor([SC.turn2_ids(ids1[0].tolist(), seq1[0, 283:].tolist())], device=ids1.device)
    plain = model.generate(ids2, images=img, prefix=HandPrefix(model, copy_rows(model, s, 289), 289), max_new_tokens=6)
    t = plain[0, ids2.shape[1]:].tolist()
    kw = dict(bad_words_ids=[[t[0]], t[2:4]], max_new_tokens=6)
    want = model.generate(ids2, images=img, prefix=HandPrefix(model, copy_rows(model, s, 289), 289), **kw)
    got = model.generate(ids2, images=img, prefix=s, **kw)
    assert s.stats["reused"] == 289 and torch.equal(got, want) and not torch.equal(got, plain)
    said = got[0, ids2.shape[1]:].tolist()
    assert said[0] != t[0] and all(said[i:i + 2] != t[2:4] for i in range(len(said) - 1))


def test_int8_engine_one_row():
    from tests.test_model_gpu import build_golden_model
    model = build_golden_model()
    model.quantize_decode_weights("int8")
    ids, mask, img = inputs("one")
    S, E, choices = ids.shape[1], 2, [[11], [12, 13], [14, 15, 16, 17]]
    plain = model.generate(ids, images=img, max_new_tokens=5)
    kw = dict(suppress_tokens=[int(plain[0, S + 1])], begin_suppress_tokens=[int(plain[0, S])], eos_token_id=E, pad_token_id=0)
    outs = [model.generate(ids, images=img, max_new_tokens=5, use_graph=ug, **kw) for ug in (True, False, None)]
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2]) and not torch.equal(outs[0][:, :plain.shape[1]], plain)
    assert int(outs[0][0, S]) != int(plain[0, S]) and int(plain[0, S + 1]) not in outs[0][0, S:].tolist()
    for ug in (True, None):
        tail = model.generate(ids, images=img, max_new_tokens=8, use_graph=ug, allowed_sequences=choices, eos_token_id=E,
                              pad_token_id=0)[0, S:].tolist()
        assert tail[:tail.index(E)] in choices


# ---- the batcher --------------------------------------------------------------------------------------------------------------
def test_batcher_requests_with_their_own_tries_equal_generate_alone(model):
    from valley_amd.serving import ContinuousBatcher
    T, E = G.GCFG["T"], 2
    img = torch.from_numpy(G.golden_pixels(T, "mixed")).view(1, T, 3, 224, 224).cuda()
    reqs = [torch.from_numpy(G.golden_ids(c)[0]).cuda() for c in ("decode2", "decode", "decode2")]
    plain = model.generate(reqs[1], images=img, max_new_tokens=3)
    second = int(plain[0, reqs[1].shape[1] + 1])                                      # what request 1 says second when nothing is banned
    o = 100 if 11 <= second <= 40 else 0                                              # (the choices keep clear of it: no row may end all -inf)
    sets = [[[o + 11], [o + 12, o + 13], [o + 14, o + 15, o + 16, o + 17]], [[o + 21, o + 22, o + 23, o + 24, o + 25], [o + 26, o + 27, o + 28]],
            [[o + 31, o + 32, o + 33, o + 34, o + 35, o + 36], [o + 37, o + 38, o + 39, o + 40]]]
    shared = dict(suppress_tokens=[o + 12, second])
    n = 8

    def alone(ids, **kw):
        out = model.generate(ids, images=img, max_new_tokens=n, eos_token_id=E, pad_token_id=0, **shared, **kw)[0, ids.shape[1]:].tolist()
        return out[:out.index(E) + 1] if E in out else out

    cb = ContinuousBatcher(model, slots=4, ctx_max=512, constraints=True, eos_token_id=E, trie_capacity=64, **shared)
    slots, got = [], []
    for i in (0, 1):
        slots.append(cb.add(reqs[i], images=img, allowed_sequences=sets[i]))
        got.append([int(cb.sess.tok[slots[-1]])])
    for step in range(n - 1):
        if step == 2:                                                                 # the third joins while the others decode
            slots.append(cb.add(reqs[2], images=img, allowed_sequences=sets[2], forced_eos_at=4))
            got.append([int(cb.sess.tok[slots[-1]])])
        toks = cb.step()
        for j, s in enumerate(slots):
            got[j].append(toks[s])
    assert len(set(slots)) == 3
    for i in (0, 1):
        want = alone(reqs[i], allowed_sequences=sets[i])
        assert got[i][:len(want)] == want and want[-1] == E and want[:-1] in sets[i], (i, got[i], want, second)
    want = model.generate(reqs[2], images=img, max_new_tokens=4, eos_token_id=E, pad_token_id=0, allowed_sequences=sets[2],
                          forced_eos_token_id=E, **shared)[0, reqs[2].shape[1]:].tolist()
    assert got[2][:4] == want and want[3] == E and want[:3] in (sets[2][0][:3], sets[2][1][:3])
    # a released and reused slot carries nothing over: no trie, no forced EOS — only the batcher's shared list
    cb.release(slots[0])
    assert cb.sess.con[slots[0]].tolist() == [0, 0, 0, -1]
    s = cb.add(reqs[1], images=img)
    assert s == slots[0]
    again = [int(cb.sess.tok[s])] + [cb.step()[s] for _ in range(3)]
    assert again == alone(reqs[1])[:4] and second not in again


def test_a_default_generation_and_batcher_never_import_the_binding():
    code = ("import sys, torch\n"
            "from tests import golden_cfg as G\n"
            "from tests.test_model_gpu import build_golden_model\n"
            "from valley_amd.serving import ContinuousBatcher\n"
            "model = build_golden_model()\n"
            "T = G.GCFG['T']\n"
            "ids = torch.from_numpy(G.golden_ids('decode')[0]).cuda()\n"
            "img = torch.from_numpy(G.golden_pixels(T, 'mixed')).view(1, T, 3, 224, 224).cuda()\n"
            "for ug in (True, None):\n"
            "    model.generate(ids, images=img, max_new_tokens=3, use_graph=ug, repetition_penalty=1.2)\n"
            "cb = ContinuousBatcher(model, slots=2, ctx_max=512, processors=True)\n"
            "cb.add(ids, images=img); cb.step()\n"
            "assert 'valley_amd.lib_constrain' not in sys.modules and 'libvalley_hip_constrain' not in open('/proc/self/maps').read()\n"
            "assert cb.sess.con is None\n"
            "print('ok')\n")
    p = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, cwd=ROOT, timeout=300)
    assert p.returncode == 0 and p.stdout.strip().endswith("ok"), p.stderr[-3000:]
