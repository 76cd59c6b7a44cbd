"""Token constraints without a GPU (include/valley_hip_constrain.h): the reference of tests/constrain_ref.py pinned to
transformers' own processor objects, per call and end to end through ``LlamaForCausalLM.generate`` on a tiny CPU Llama; the
packers of valley_amd.ops against brute force (the packed tables are read back by a python walk that follows the header's
layout); every refusal and its message; and the companion contract of the fourth build table."""
import os
import random
import re
import subprocess
import sys

import pytest
import torch

from tests import constrain_ref as CR
from tests import logits_ref
from tests.test_companions_cpu import exported, header_macro, header_symbols, header_text
from valley_amd import build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["vly_constrain_abi_version", "vly_constrain_apply", "vly_constrain_last_error"]
EOS = 7
V = 101


# ---- the build table, the exports, the lazy load ------------------------------------------------------------------------------
def test_the_fourth_table_is_the_constrain_companion():
    assert [c.name for c in build.COMPANIONS_CONSTRAIN] == ["constrain"]
    assert len(build.COMPANIONS) == 7 and [c.name for c in build.COMPANIONS_ROWS] == ["spec_rows"]
    assert [c.name for c in build.COMPANIONS_SUFFIX] == ["suffix"]
    assert build.ALL_COMPANIONS == (*build.COMPANIONS, *build.COMPANIONS_ROWS, *build.COMPANIONS_SUFFIX, *build.COMPANIONS_CONSTRAIN)
    c = build.COMPANIONS_CONSTRAIN[0]
    assert c.lib == build.LIB_CONSTRAIN == os.path.join(build.LIBDIR, "libvalley_hip_constrain.so")
    assert c.header == "valley_hip_constrain.h" and c.sources == ("constrain.hip",)
    assert c.lib not in {o.lib for o in (*build.COMPANIONS, *build.COMPANIONS_ROWS, *build.COMPANIONS_SUFFIX)}
    src = open(os.path.join(build.CSRC, c.sources[0])).read()
    assert set(re.findall(r'#include "([a-z0-9_]+\.(?:hpp|inc))"', src)) <= set(c.deps) | set(build.COMPANION_SHARED)


def test_header_binding_and_library_agree():
    build.build(verbose=False)
    from valley_amd import lib_constrain, ops
    assert header_symbols("valley_hip_constrain.h") == NAMES == sorted(lib_constrain.EXPORTS) == exported(build.LIB_CONSTRAIN)
    assert re.search(r"#define VLY_CONSTRAIN_ABI_VERSION 1\b", header_text("valley_hip_constrain.h")) and lib_constrain.ABI_VERSION == 1
    assert lib_constrain.load().vly_constrain_abi_version() == 1
    for macro, a, b in (("MAX_WORD", lib_constrain.MAX_WORD, ops.CONSTRAIN_MAX_WORD), ("MAX_DEPTH", lib_constrain.MAX_DEPTH, ops.CONSTRAIN_MAX_DEPTH),
                        ("HEADER", lib_constrain.HEADER, ops.CONSTRAIN_HEADER), ("BAD_WORDS", lib_constrain.BAD_WORDS, ops.CONSTRAIN_BAD_WORDS),
                        ("TRIE", lib_constrain.TRIE, ops.CONSTRAIN_TRIE), ("FORCED_EOS", lib_constrain.FORCED_EOS, ops.CONSTRAIN_FORCED_EOS),
                        ("SUPPRESS", lib_constrain.SUPPRESS, ops.CONSTRAIN_SUPPRESS),
                        ("BEGIN_SUPPRESS", lib_constrain.BEGIN_SUPPRESS, ops.CONSTRAIN_BEGIN_SUPPRESS)):
        assert header_macro("valley_hip_constrain.h", f"VLY_CONSTRAIN_{macro}") == a == b, macro
    assert CR.MAX_DEPTH == ops.CONSTRAIN_MAX_DEPTH and CR.MAX_WORD == ops.CONSTRAIN_MAX_WORD
    # the other libraries are what they were, and none carries the new names
    assert len(exported(build.LIB)) == 52 and not [n for n in exported(build.LIB) if "constrain" in n]
    for c in (*build.COMPANIONS, *build.COMPANIONS_ROWS, *build.COMPANIONS_SUFFIX):
        got = exported(c.lib)
        assert not [n for n in got if "constrain" in n], c.name
        assert got == header_symbols(c.header), c.name
        assert not [n for n in exported(build.LIB_CONSTRAIN) if n.startswith(f"vly_{c.name}_")], c.name
    from valley_amd import lib_logits, lib_spec_rows, lib_suffix
    assert lib_logits.load().vly_logits_abi_version() == 1 and len(lib_logits.EXPORTS) == 6
    assert lib_spec_rows.ABI_VERSION == 1 and len(lib_spec_rows.EXPORTS) == 7 and lib_suffix.ABI_VERSION == 1 and len(lib_suffix.EXPORTS) == 4


def test_bad_arguments_to_the_entry_point_return_einval():
    """No launch is made for bad arguments: -22 and a message."""
    build.build(verbose=False)
    from valley_amd import lib_constrain
    h = lib_constrain.load()
    # apply(logits, ld, V, R, rows, tables, tables_len, hist, hist_ld, len_dev, len_per_row, len_add, stream)
    assert h.vly_constrain_apply(None, 10, 10, 1, None, None, 16, None, 8, None, 0, 0, None) == -22
    assert b"vly_constrain_apply" in h.vly_constrain_last_error()
    assert h.vly_constrain_apply(64, 10, 11, 1, 64, 64, 16, 64, 8, None, 0, 0, None) == -22          # ld < V
    assert h.vly_constrain_apply(64, 1 << 19, 1 << 19, 1, 64, 64, 16, 64, 8, None, 0, 0, None) == -22   # V too wide
    assert h.vly_constrain_apply(64, 10, 10, 1, 64, 64, 15, 64, 8, None, 0, 0, None) == -22          # no room for the header
    assert b"tables_len=15" in h.vly_constrain_last_error()
    assert h.vly_constrain_apply(64, 10, 10, 1, 64, 64, 16, 64, 8, None, 1, 0, None) == -22          # per-row, no len
    assert h.vly_constrain_apply(64, 10, 10, 1, 64, 66, 16, 64, 8, None, 0, 0, None) == -22          # misaligned tables


def test_a_default_generation_never_imports_the_binding():
    """In a fresh process: the package, the model, the sessions and the batcher are imported, a generation's constraint setup
    runs with every argument at its default, and the binding's module is not even imported (the GPU suite runs a real
    default ``generate`` under the same assertion)."""
    code = ("import sys; import valley_amd.ops, valley_amd.valley_model, valley_amd.decode, valley_amd.serving\n"
            "from valley_amd import generation\n"
            "assert generation.constraint_setup((None,) * 5, 100, 4, 8, [2], 'cpu') is None\n"
            "assert 'valley_amd.lib_constrain' not in sys.modules\n"
            "from valley_amd import lib_constrain\n"
            "assert not lib_constrain.loaded() and 'libvalley_hip_constrain' not in open('/proc/self/maps').read(); print('ok')")
    p = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, cwd=ROOT)
    assert p.returncode == 0 and p.stdout.strip() == "ok", p.stderr[-2000:]


def test_generate_and_completion_name_the_five_arguments():
    import inspect
    from valley_amd.valley_model import ValleyLlamaForCausalLM
    sig = inspect.signature(ValleyLlamaForCausalLM.generate).parameters
    src = inspect.getsource(ValleyLlamaForCausalLM.completion)
    for k in ("bad_words_ids", "suppress_tokens", "begin_suppress_tokens", "forced_eos_token_id", "allowed_sequences"):
        assert k in sig and sig[k].default is None and f'"{k}"' in src
    assert "prefix_allowed_tokens_fn" not in sig


# ---- the reference equals transformers' processors ---------------------------------------------------------------------------
def random_scores(g, R):
    x = torch.randn((R, V), generator=g) * 3
    x[0, 3], x[0, 9] = float("-inf"), -0.0
    x[R - 1, 11] = float("nan")
    return x


def random_rules(rng, n_hist):
    words = [[rng.randrange(8, V) for _ in range(rng.choice([1, 1, 2, 3, 5]))] for _ in range(rng.randrange(1, 12))]
    words += [words[0], [EOS]]                                # a duplicate, and the EOS word HF drops
    seqs = [[rng.randrange(8, 14) for _ in range(rng.randrange(1, 5))] for _ in range(rng.randrange(1, 8))]
    return dict(bad_words=words, allowed=seqs, max_length=n_hist + rng.choice([1, 2]), suppress=[rng.randrange(V) for _ in range(4)] + [V - 1],
                begin_suppress=[rng.randrange(V) for _ in range(3)])


def plant(rng, ids, rules, begin):
    """make the rules bite: the history ends with a bad word's head, and continues one of the allowed sequences"""
    ids = list(ids)
    seq = rng.choice(rules["allowed"])
    k = rng.randrange(0, len(seq) + 1)
    if begin + k <= len(ids):
        ids[begin:begin + k] = seq[:k]
    return ids


@pytest.mark.parametrize("rule", ["bad_words", "allowed", "max_length", "suppress", "begin_suppress", "all"])
def test_reference_equals_transformers_per_call(rule):
    rng = random.Random(len(rule) * 31 + ord(rule[0]))
    g = torch.Generator().manual_seed(5)
    for trial in range(40):
        R, n = rng.choice([1, 3]), rng.randrange(2, 12)
        begin = rng.choice([n, n - 1, max(0, n - 3), 0])
        rules = random_rules(rng, n)
        if rule != "all":
            rules = {rule: rules[rule]}
        ids = [[rng.randrange(8, 14) for _ in range(n)] for _ in range(R)]
        if "allowed" in rules:
            ids = [plant(rng, row, rules, begin) for row in ids]
        if "bad_words" in rules and trial % 2:
            w = max(rules["bad_words"], key=len)
            if 1 < len(w) <= n:
                ids[0][n - len(w) + 1:] = w[:-1]              # row 0 ends with the longest word's head
        x = random_scores(g, R)
        procs = CR.hf_constraint_processors(rules.get("bad_words"), rules.get("allowed"), rules.get("max_length", 0), rules.get("suppress"),
                                            rules.get("begin_suppress"), begin=begin, eos=[EOS, 5])
        want = procs(torch.tensor(ids), x.clone())
        got = torch.stack([CR.constrain_row(x[r], ids[r], begin=begin, eos=[EOS, 5], **rules) for r in range(R)])
        assert CR.same_values(got, want), (rule, trial)
        untouched = torch.isfinite(got) & (got == x)          # (the forced EOS writes zeros: those are not untouched)
        assert torch.equal(got[untouched].view(torch.int32), x[untouched].view(torch.int32))   # what no rule banned keeps its bits


def test_reference_edges():
    x = torch.arange(V, dtype=torch.float32)
    # L == len applies, L == len + 1 is skipped (HF: "longer than the context, ignore")
    assert CR.constrain_row(x, [1, 2, 3], bad_words=[[9, 2, 3, 50]])[50] == 50.0          # L = 4 > len = 3
    assert CR.constrain_row(x, [1, 2, 3], bad_words=[[2, 3, 50]])[50] == float("-inf")    # L = 3 == len
    assert CR.constrain_row(x, [2, 3], bad_words=[[2, 3, 50]])[50] == 50.0                # L = len + 1
    # a leaf, a left trie and 65 generated ids allow only EOS; the root allows the first ids
    seqs = [[10, 11], [10], [12]]
    assert CR.trie_allowed(seqs, [], EOS) == [10, 12] and CR.trie_allowed(seqs, [10], EOS) == [EOS, 11]
    assert CR.trie_allowed(seqs, [12], EOS) == [EOS] and CR.trie_allowed(seqs, [13], EOS) == [EOS]
    assert CR.trie_allowed([[1] * 64], [1] * 64, EOS) == [EOS] and CR.trie_allowed([[1] * 64], [1] * 63, EOS) == [1]
    assert CR.trie_allowed([[1] * 64], [1] * 65, EOS) == [EOS]
    # forced EOS, then a suppressed EOS id ends -inf
    y = CR.constrain_row(x, [1, 2, 3], max_length=5, eos=[EOS, 5])
    assert torch.equal(y, x)
    y = CR.constrain_row(x, [1, 2, 3, 4], max_length=5, eos=[EOS, 5], suppress=[5])
    assert y[EOS] == 0 and y[5] == float("-inf") and int(torch.isfinite(y).sum()) == 1


# ---- the packers against brute force ------------------------------------------------------------------------------------------
def walk_packed(buf, root, generated, V):
    """The allowed ids behind ``generated`` as the table says, by the header's layout (valley_hip_constrain.h)."""
    n_eos, off_eos, off_trie = buf[0], buf[4], buf[8]
    eos = buf[off_eos:off_eos + n_eos]
    if len(generated) > 64:
        return sorted(set(eos))
    p = root
    for t in generated:
        n = buf[off_trie + p]
        pairs = [(buf[off_trie + p + 2 + 2 * i], buf[off_trie + p + 3 + 2 * i]) for i in range(n)]
        assert [a for a, _ in pairs] == sorted({a for a, _ in pairs})         # sorted by token, no duplicates
        nxt = dict(pairs).get(t)
        if nxt is None:
            return sorted(set(eos))
        p = nxt
    n, ends = buf[off_trie + p], buf[off_trie + p + 1]
    out = {buf[off_trie + p + 2 + 2 * i] for i in range(n)}
    if ends or not out:
        out |= set(eos)
    return sorted(out)


def test_trie_packer_against_brute_force():
    from valley_amd import ops
    rng = random.Random(3)
    for trial in range(30):
        sets = []
        for _ in range(3):                                    # three tries side by side, as a batcher's slots hold them
            seqs = [[rng.randrange(0, 6) for _ in range(rng.randrange(1, 6))] for _ in range(rng.randrange(1, 12))]
            seqs += [seqs[0], seqs[0][:1], seqs[0] + [3, 4]]  # a duplicate, a prefix of another, an extension (shared prefix)
            sets.append(seqs)
        cap = max(len(ops.pack_trie(s, V)) for s in sets)
        t = ops.constraint_tables(eos=[EOS, 5], V=V, capacity={"trie": cap, "trie_slots": 3})
        roots = [ops.constraint_trie(t, i, s) for i, s in enumerate(sets)]
        assert roots == [0, cap, 2 * cap]
        buf = t.buf.tolist()
        assert buf[8] == t.off["trie"] and buf[10] == 3 * cap and len(buf) == t.off["trie"] + 3 * cap
        for root, seqs in zip(roots, sets):
            prefixes = {tuple(s[:k]) for s in seqs for k in range(len(s) + 1)}
            for g in list(prefixes) + [(9,), tuple(seqs[0]) + (0, 0, 0, 0, 0, 0)] + [p + (7,) for p in list(prefixes)[:5]]:
                assert walk_packed(buf, root, list(g), V) == CR.trie_allowed(seqs, list(g), [EOS, 5]), (trial, g)
    # a node of 1500 children, a chain of 64
    wide = ops.pack_trie([[i] for i in range(1500, 0, -1)], 2000)
    assert wide[0] == 1500 and wide[2:3002:2] == list(range(1, 1501)) and len(wide) == 2 + 2 * 1500 + 2 * 1500
    deep = ops.pack_trie([[3] * 64], V)
    assert len(deep) == 65 * 2 + 64 * 2 and deep[-2:] == [0, 1]


def test_bad_word_packer_against_its_input():
    from valley_amd import ops
    rng = random.Random(4)
    for _ in range(20):
        words = [[rng.randrange(0, V) for _ in range(rng.choice([1, 1, 2, 5, 64]))] for _ in range(rng.randrange(1, 40))]
        words += [words[0], [EOS], [5]]
        t = ops.constraint_tables(bad_words_ids=words, suppress_tokens=[1, 1, V - 1], begin_suppress_tokens=[0], eos=[EOS, 5], V=V)
        buf = t.buf.tolist()
        n_eos, n_sup, n_beg, n_words, off_eos, off_sup, off_beg, off_w = buf[:8]
        assert buf[off_eos:off_eos + n_eos] == [EOS, 5] and buf[off_sup:off_sup + n_sup] == [1, 1, V - 1] and buf[off_beg:off_beg + n_beg] == [0]
        got = [tuple(buf[off_w + buf[off_w + 2 * i]:off_w + buf[off_w + 2 * i] + buf[off_w + 2 * i + 1]]) for i in range(n_words)]
        want = list(dict.fromkeys(tuple(w) for w in words if w not in ([EOS], [5])))
        assert got == want and buf[9] == 2 * n_words + sum(len(w) for w in want) and len(buf) == off_w + buf[9]
        assert t.flags() == ops.CONSTRAIN_BAD_WORDS | ops.CONSTRAIN_SUPPRESS | ops.CONSTRAIN_BEGIN_SUPPRESS
    # rewriting in place: new contents, new counts, the same storage
    ptr = t.buf.data_ptr()
    t.write(suppress_tokens=[4], eos=[EOS])
    assert t.buf.data_ptr() == ptr and t.buf[:4].tolist() == [1, 1, 0, 0] and t.flags() == ops.CONSTRAIN_SUPPRESS


def test_constraint_rows():
    from valley_amd import ops
    t = ops.constraint_tables(suppress_tokens=[4], eos=[EOS], V=V, capacity={"trie": 40, "trie_slots": 2})
    root = ops.constraint_trie(t, 1, [[1, 2], [3]])
    rows = ops.constraint_rows(t, 3, begin=[4, 5, 6], max_length=[0, 9, 0], trie_root=[-1, root, -1])
    S, T, F = ops.CONSTRAIN_SUPPRESS, ops.CONSTRAIN_TRIE, ops.CONSTRAIN_FORCED_EOS
    assert rows.dtype == torch.int32 and rows.tolist() == [[S, 4, 0, -1], [S | T | F, 5, 9, 40], [S, 6, 0, -1]]
    assert ops.constraint_rows(t, 2, flags=0).tolist() == [[0, 0, 0, -1]] * 2
    for bad in (dict(begin=-1), dict(max_length=-2), dict(trie_root=80), dict(trie_root=-2), dict(begin=[1, 2])):
        with pytest.raises(ValueError, match="constraint_rows"):
            ops.constraint_rows(t, 3, **bad)


# ---- refusals -------------------------------------------------------------------------------------------------------------------
def message(fn):
    with pytest.raises(ValueError) as e:
        fn()
    return str(e.value)


def test_refusals_and_their_messages():
    from transformers.generation.logits_process import NoBadWordsLogitsProcessor
    from valley_amd import generation, lib_constrain, ops
    lib_constrain.reset()
    tables = lambda **kw: ops.constraint_tables(V=V, **kw)    # noqa: E731
    # HF's own messages where HF checks
    for bad in ([], "x", [1, 2], [[1], 2], [[1, -2]], [[1.5]]):
        assert message(lambda: tables(bad_words_ids=bad)) == message(lambda: NoBadWordsLogitsProcessor(bad, EOS))
    p = NoBadWordsLogitsProcessor([[1, V + 3], [V]], EOS)
    assert message(lambda: tables(bad_words_ids=[[1, V + 3], [V]])) == message(lambda: p(torch.zeros((1, 2), dtype=torch.long), torch.zeros((1, V))))
    assert message(lambda: tables(bad_words_ids=[[1], []])) == "Each list in `bad_words_ids` has to be a non-empty list of positive integers, but is [[1], []]."
    assert message(lambda: tables(bad_words_ids=[[1] * 65])) == "a bad word holds at most 64 tokens, got one of 65"
    tables(bad_words_ids=[[1] * 64])
    for name in ("suppress_tokens", "begin_suppress_tokens"):
        assert message(lambda: tables(**{name: []})) == f"`{name}` has to be a non-empty list of integers, but is []."
        assert message(lambda: tables(**{name: 3})) == f"`{name}` has to be a non-empty list of integers, but is 3."
        assert message(lambda: tables(**{name: [1, -1]})) == f"`{name}` has to be a list of positive integers, but is [1, -1]."
        assert message(lambda: tables(**{name: [1, True]})) == f"`{name}` has to be a list of positive integers, but is [1, True]."
        assert message(lambda: tables(**{name: [V, 2, V + 1]})) == f"The model vocabulary size is {V}, but `{name}` holds the ids [{V}, {V + 1}]"
    assert message(lambda: tables(eos=[V])) == f"The model vocabulary size is {V}, but `eos_token_id` holds the ids [{V}]"
    assert "V (the vocabulary size) is required" in message(lambda: ops.constraint_tables(suppress_tokens=[1]))
    # allowed sequences
    t = tables(eos=EOS, capacity={"trie": 14})
    assert message(lambda: ops.constraint_trie(t, 0, [])) == "`allowed_sequences` has to be a non-empty list of lists, but is []."
    assert message(lambda: ops.constraint_trie(t, 0, [[1], []])) == \
        "Each sequence in `allowed_sequences` has to be a non-empty list of positive integers, but is []."
    assert message(lambda: ops.constraint_trie(t, 0, [[1, -3]])) == \
        "Each sequence in `allowed_sequences` has to be a non-empty list of positive integers, but is [1, -3]."
    assert message(lambda: ops.constraint_trie(t, 0, [[1, V]])) == f"The model vocabulary size is {V}, but `allowed_sequences` holds the ids [{V}]"
    assert message(lambda: ops.constraint_trie(t, 0, [[2] * 65])) == "an allowed sequence holds at most 64 tokens, got one of 65"
    assert message(lambda: ops.constraint_trie(t, 1, [[2]])) == "constraint_trie: slot 1 of 1"
    # capacities
    assert message(lambda: ops.constraint_trie(t, 0, [[1, 2, 3], [4]])) == "constraint_tables: the trie takes 18 words, a slot's capacity is 14"
    ops.constraint_trie(t, 0, [[1, 2], [4]])
    assert message(lambda: tables(bad_words_ids=[[1, 2], [3]], capacity={"words": 6})) == \
        "constraint_tables: the words table takes 7 words, its capacity is 6"
    assert message(lambda: tables(suppress_tokens=[1, 2], capacity={"suppress": 1})) == \
        "constraint_tables: the suppress table takes 2 words, its capacity is 1"
    assert message(lambda: t.write(eos=[1, 2])) == "constraint_tables: the eos table takes 2 words, its capacity is 1"
    # a trie or a forced EOS without an EOS id
    no_eos = tables(suppress_tokens=[1], capacity={"trie": 12})
    want = "`allowed_sequences` needs an `eos_token_id`: behind a complete sequence only EOS is allowed"
    assert message(lambda: ops.constraint_trie(no_eos, 0, [[1]])) == want
    assert message(lambda: ops.constraint_rows(no_eos, 1, trie_root=0)) == want
    assert message(lambda: ops.constraint_rows(no_eos, 1, max_length=9)) == "`forced_eos_token_id` needs an EOS id in the constraint tables"
    setup = lambda con, eos, **kw: generation.constraint_setup(con, V, 4, 8, eos, "cpu", **kw)    # noqa: E731
    assert message(lambda: setup((None, None, None, None, [[1]]), [])) == want
    assert message(lambda: setup((None, None, None, 2, None), [])) == \
        "`forced_eos_token_id` needs an `eos_token_id`: the ids it forces are the generation's EOS ids"
    assert "has to name the `eos_token_id` ids [7]" in message(lambda: setup((None, None, None, 2, None), [EOS]))
    assert "not supported with num_beams > 1" in message(lambda: setup((None, None, None, None, [[1]]), [EOS], beams=True))
    assert "not supported with num_beams > 1" in message(lambda: setup((None, None, None, EOS, None), [EOS], beams=True))
    assert "2 per-row lists for 3 rows" in message(lambda: setup((None, None, None, None, [[[1]], [[2]]]), [EOS], rows=3))
    # what a generation gets: shared and per-row tries, the forced EOS at S + max_new_tokens
    tb, rows = setup(([[3, 4]], [5], [6], [EOS], [[1, 2], [3]]), [EOS], rows=2)
    assert rows.tolist() == [[31, 4, 12, 0]] * 2 and tb.trie_slots == 1
    tb, rows = setup((None, None, None, None, [[[1, 2], [3]], [[4]]]), [EOS], rows=2)
    assert rows.tolist() == [[2, 4, 0, 0], [2, 4, 0, tb.trie_capacity]] and tb.trie_slots == 2
    assert not lib_constrain.loaded()                         # nothing above touched the library


def test_speculation_and_batcher_refusals_name_the_constraints():
    import inspect
    from valley_amd.serving import ContinuousBatcher
    from valley_amd.valley_model import ValleyLlamaForCausalLM
    src = inspect.getsource(ValleyLlamaForCausalLM.generate)
    assert "prompt_lookup_num_tokens is not supported with token constraints" in src
    with pytest.raises(ValueError, match="does not combine with constraints=True"):
        ContinuousBatcher(None, slots=1, prompt_lookup_num_tokens=2, constraints=True)


# ---- the reference loop against transformers' generate ------------------------------------------------------------------------
@pytest.fixture(scope="module")
def model():
    from tests.test_logits_process_cpu import tiny_llama
    return tiny_llama()


CASES = [dict(bad_words_ids=[[20], [21, 22], [EOS]]), dict(suppress_tokens=[30, 31, 32]), dict(begin_suppress_tokens=[40, 41]),
         dict(forced_eos_token_id=EOS), dict(allowed=[[50, 51, 52], [50], [60, 61], [70, 71, 72, 73]]),
         dict(bad_words_ids=[[50]], suppress_tokens=[60], begin_suppress_tokens=[70], forced_eos_token_id=EOS,
              allowed=[[50, 51, 52], [60, 61], [70, 71, 72, 73], [80, 81, 82, 83, 84, 85, 86, 87, 88, 89, 90, 91]],
              repetition_penalty=1.3, no_repeat_ngram_size=2)]


@pytest.mark.parametrize("case", range(len(CASES)))
@pytest.mark.parametrize("B,padded", [(1, False), (2, True)])
def test_reference_loop_matches_hf_generate(model, case, B, padded):
    from tests.test_logits_process_cpu import hf_stepper, make_inputs
    kw = dict(CASES[case])
    ids, mask = make_inputs(B, 8, padded, seed=B * 5 + case)
    S, new = ids.shape[1], 8
    plain = model.generate(input_ids=ids, attention_mask=mask, do_sample=False, max_new_tokens=new, eos_token_id=None, pad_token_id=0)
    if "bad_words_ids" in kw and case == 0:                   # ban what greedy decoding would say: its first token, its second bigram
        kw["bad_words_ids"] = [[int(plain[0, S])], plain[0, S + 1:S + 3].tolist(), [EOS]]
    if "suppress_tokens" in kw and case == 1:
        kw["suppress_tokens"] = sorted(set(plain[:, S + 2].tolist()))
    if "begin_suppress_tokens" in kw and case == 2:
        kw["begin_suppress_tokens"] = sorted(set(plain[:, S].tolist()))
    allowed = kw.pop("allowed", None)
    rp, ng = kw.pop("repetition_penalty", None), kw.pop("no_repeat_ngram_size", None)
    hf_kw = dict(kw, repetition_penalty=rp, no_repeat_ngram_size=ng)
    if allowed is not None:
        hf_kw["prefix_allowed_tokens_fn"] = CR.trie_fn(allowed, S, EOS)
    ref = model.generate(input_ids=ids, attention_mask=mask, do_sample=False, num_beams=1, max_new_tokens=new, eos_token_id=EOS,
                         pad_token_id=0, **hf_kw)
    step, _ = hf_stepper(model, ids, mask)
    front = logits_ref.hf_processors(rp, ng, prompt_len=S, eos=EOS)
    procs = CR.RefConstraints(front, bad_words=kw.get("bad_words_ids"), allowed=allowed, suppress=kw.get("suppress_tokens"),
                              begin_suppress=kw.get("begin_suppress_tokens"), begin=S, eos=EOS,
                              max_length=S + new if "forced_eos_token_id" in kw else 0)
    got = CR.greedy_loop(step, ids, new, procs, eos=EOS, pad=0)
    assert torch.equal(got, ref), (kw, got, ref)
    assert not torch.equal(ref[:, :plain.shape[1]], plain[:, :ref.shape[1]]) or case == 3      # the rule changed the output
    if "forced_eos_token_id" in kw and allowed is None:
        assert bool(((ref[:, S:] == EOS).any(-1)).all())      # every row ends in EOS within max_new_tokens
    if allowed is not None:
        for r in range(B):
            tail = ref[r, S:].tolist()
            said = tail[:tail.index(EOS)]
            if "forced_eos_token_id" in kw:                   # the forced EOS may cut a choice short
                assert any(a[:len(said)] == said for a in allowed)
            else:
                assert said in allowed
