"""Stop strings and the end of a generation on the MI355X: vly_stop_apply against transformers' StopStringCriteria — exact, over
every sequence of one to four of eleven chosen tokens, with guard words around everything it may write — a captured launch
replayed with new rows, state and tables, and generate() / completion() / ContinuousBatcher end to end on the golden model
against the path that runs HF's criterion as a host callback after every token."""
import itertools

import pytest
import torch

from tests import golden_cfg as G
from tests import stop_ref as SR
from tests import stop_tokenizer as ST
from tests.test_logits_process_gpu import inputs

pytestmark = pytest.mark.gpu
GUARD = 0x5A5A5A5A
STRINGS = ["###", "stop"]
CHOSEN = ("#", "##", "###", "####", "a#", "#b", "x###y", "st", "op", "stop", "a")
NEW = 24


def dev():
    return torch.device("cuda:0")


def hf(tokenizer, strings):
    from transformers.generation.stopping_criteria import StopStringCriteria
    return StopStringCriteria(tokenizer, strings)


def guarded(t):
    """``t`` on the device between two rows of guard words -> (the view the launch gets, the whole buffer)"""
    flat = t.reshape(-1).to(torch.int32)
    buf = torch.full((flat.numel() + 32,), GUARD, dtype=torch.int32)
    buf[16:16 + flat.numel()] = flat
    buf = buf.to(dev())
    return buf[16:16 + flat.numel()].view(t.shape), buf


def intact(buf):
    b = buf.cpu()
    return bool((b[:16] == GUARD).all() and (b[-16:] == GUARD).all())


def launch(tables, tok, hist, pos, rows, state=None, eos=None, pos_add=0, shared_pos=False):
    """One launch over host tensors -> (tok, state) afterwards; the history and every guard word must be as they were."""
    from valley_amd import ops
    R = tok.numel()
    state = torch.tensor([[0, -1]] * R, dtype=torch.int32) if state is None else state
    (tk, tkb), (hs, hsb), (stt, stb) = guarded(tok), guarded(hist), guarded(state)
    pos_d = None if pos is None else torch.as_tensor(pos, dtype=torch.int32).view(-1)[:1 if shared_pos else R].contiguous().to(dev())
    ops.stop(tk, rows.to(dev()), stt, tables, hs, pos_d, pos_add, eos=None if eos is None else torch.tensor(eos, dtype=torch.int32, device=dev()))
    torch.cuda.synchronize()
    assert intact(tkb) and intact(hsb) and intact(stb)
    assert torch.equal(hs.cpu(), hist.to(torch.int32))
    return tk.cpu(), stt.cpu()


@pytest.fixture(scope="module")
def small():
    """The small vocabulary, HF's criterion for STRINGS, the device tables, and every sequence of 1..4 of the chosen tokens with
    HF's verdict (computed once, shared)."""
    from valley_amd import ops
    tk = ST.small()
    crit = hf(tk, STRINGS)
    ids = [tk.vocab[p] for p in CHOSEN]
    seqs = [list(s) for n in range(1, 5) for s in itertools.product(ids, repeat=n)]
    want = []
    for n in range(1, 5):
        want += crit(torch.tensor([s for s in seqs if len(s) == n]), None).tolist()
    assert len(seqs) == 11 + 11 ** 2 + 11 ** 3 + 11 ** 4 and any(want) and not all(want)
    return tk, crit, ops.stop_tables(tk, STRINGS, device=dev()), seqs, want


# ---- the kernel ---------------------------------------------------------------------------------------------------------------
def test_every_sequence_of_one_to_four_tokens_equals_hf(small):
    from valley_amd import ops
    tk, crit, tables, seqs, want = small
    R, ld = len(seqs), 8
    assert R <= 65535
    hist = torch.full((R, ld), tk.vocab["#"], dtype=torch.int32)              # what lies behind pos would match: never read
    for r, s in enumerate(seqs):
        hist[r, :len(s) - 1] = torch.tensor(s[:-1], dtype=torch.int32)
    tok = torch.tensor([s[-1] for s in seqs], dtype=torch.int32)
    pos = torch.tensor([len(s) - 2 for s in seqs], dtype=torch.int32)         # -1 for one token: no history at all
    got_tok, state = launch(tables, tok, hist, pos, ops.stop_rows(R))
    assert torch.equal(got_tok, tok)
    assert state[:, 0].tolist() == [int(w) for w in want]
    assert state[:, 1].tolist() == [len(s) - 1 if w else -1 for s, w in zip(seqs, want)]


def test_every_sequence_behind_a_begin_with_poison_in_front(small):
    from valley_amd import ops
    tk, crit, tables, seqs, want = small
    R, ld, b = len(seqs), 8, 3
    hist = torch.full((R, ld), tk.vocab["##"], dtype=torch.int32)             # '##' '##' '##' in front of begin
    for r, s in enumerate(seqs):
        hist[r, b:b + len(s) - 1] = torch.tensor(s[:-1], dtype=torch.int32)
    tok = torch.tensor([s[-1] for s in seqs], dtype=torch.int32)
    pos = torch.tensor([b + len(s) - 2 for s in seqs], dtype=torch.int32)     # b - 1 for one token: begin > pos
    _, state = launch(tables, tok, hist, pos, ops.stop_rows(R, begin=b))
    assert state[:, 0].tolist() == [int(w) for w in want]
    assert state[:, 1].tolist() == [b + len(s) - 1 if w else -1 for s, w in zip(seqs, want)]
    # without the begin the poison counts, as it does for HF on the whole row
    _, state0 = launch(tables, tok, hist, pos, ops.stop_rows(R))
    whole = [hist[r, :int(pos[r]) + 1].tolist() + [int(tok[r])] for r in range(R)]
    want0 = [bool(crit(torch.tensor([w]), None)[0]) for w in whole[:11 + 121]] + \
        crit(torch.tensor(whole[11 + 121:11 + 121 + 1331]), None).tolist() + crit(torch.tensor(whole[11 + 121 + 1331:]), None).tolist()
    assert state0[:, 0].tolist() == [int(w) for w in want0] and want0 != want


def test_out_of_range_and_negative_ids_use_the_last_row(small):
    from valley_amd import ops
    tk, crit, tables, _, _ = small
    T = len(tk.pieces) + 1
    h, s2 = tk.vocab["#"], tk.vocab["##"]
    rows = [[h, h, h], [h, 999, h, h], [h, -5, h, h], [h, h, 999], [h, h, -1], [-7, s2, h], [T - 1, s2, h], [T - 2, h, s2]]
    ld = 6
    hist = torch.zeros((len(rows), ld), dtype=torch.int32)
    for r, s in enumerate(rows):
        hist[r, :len(s) - 1] = torch.tensor(s[:-1], dtype=torch.int32)
    tok = torch.tensor([s[-1] for s in rows], dtype=torch.int32)
    pos = torch.tensor([len(s) - 2 for s in rows], dtype=torch.int32)
    _, state = launch(tables, tok, hist, pos, ops.stop_rows(len(rows)))
    t = SR.tables_of(crit)
    assert state[:, 0].tolist() == [int(SR.fires(t, s)) for s in rows] == [1, 0, 0, 0, 0, 1, 1, 1]
    big = [[i if i >= 0 else 10 ** 6 for i in s] for s in rows]               # HF clamps from above only: a negative id as a huge one
    assert state[:, 0].tolist() == [int(crit(torch.tensor([s]), None)[0]) for s in big]


def test_eos_pad_finished_and_unwatched_rows(small):
    from valley_amd import ops
    tk, crit, tables, _, _ = small
    a, h = tk.vocab["a"], tk.vocab["#"]
    hist = torch.tensor([[a, a, a, a]] * 6, dtype=torch.int32)
    tok = torch.tensor([7, a, a, h, h, 9], dtype=torch.int32)
    rows = ops.stop_rows(6, begin=0, pad=[50, 51, 52, 53, 54, 55], watch=[1, 1, 1, 1, 0, 1], pad_after=[1, 1, 0, 1, 1, 0])
    state = torch.tensor([[0, -1], [1, 2], [1, 1], [0, -1], [1, 0], [0, -1]], dtype=torch.int32)
    got, st = launch(tables, tok, hist, [3], rows, state=state, eos=[7, 9], shared_pos=True)
    # row 0: EOS; row 1: finished, padded; row 2: finished, no pad rule; row 3: goes on; row 4: unwatched; row 5: the second EOS id
    assert got.tolist() == [7, 51, a, h, h, 9]
    assert st.tolist() == [[1, 4], [1, 2], [1, 1], [0, -1], [1, 0], [1, 4]]
    py_tok, py_state = tok.tolist(), state.tolist()
    SR.apply(SR.tables_of(crit), py_tok, hist.tolist(), [3] * 6, rows.tolist(), py_state, eos=[7, 9])
    assert py_tok == got.tolist() and py_state == st.tolist()
    # no EOS list, an empty string table: nothing ever finishes
    empty = ops.stop_tables(None, [], device=dev())
    got, st = launch(empty, tok, hist, [3], ops.stop_rows(6), shared_pos=True)
    assert got.tolist() == tok.tolist() and st.tolist() == [[0, -1]] * 6
    got, st = launch(empty, tok, hist, [3], ops.stop_rows(6), eos=[a], shared_pos=True)
    assert st[:, 0].tolist() == [0, 1, 1, 0, 0, 0]


@pytest.mark.parametrize("R", [1, 3, 8])
@pytest.mark.parametrize("shared", [False, True])
def test_shapes_positions_and_long_strings(R, shared):
    """Strings of 1 and 64 characters among 8, the position at 0 and at ld - 1, shared and per row: HF on the row's valid part."""
    from valley_amd import ops
    tk = ST.small()
    strings = ["#", "#" * 64, "stop", "a#", "#b", "st", "abc", "x###y"]
    crit = hf(tk, strings)
    tables = ops.stop_tables(tk, strings, device=dev())
    assert int(tables.buf[0]) == 8 and tables.maximum_token_len == 64 and int(tables.buf[5]) <= ops.STOP_MAX_WIDTH
    t, ld = SR.tables_of(crit), 70
    g = torch.Generator().manual_seed(R * 2 + shared)
    for strs, lone in ((["#" * 64], True), (strings, False)):
        c1 = hf(tk, strs) if lone else crit
        tb = ops.stop_tables(tk, strs, device=dev()) if lone else tables
        pool = torch.tensor([tk.vocab[p] for p in (("#", "##", "####") if lone else ("#", "a", "st", "op", "b", "c", "x###y", "a#"))])
        for p in (0, ld - 1, 33):
            hist = pool[torch.randint(0, len(pool), (R, ld), generator=g)].to(torch.int32)
            if lone and R > 1:
                hist[R - 1, ld - 20] = tk.vocab["a"]                      # the last row: fewer '#' behind an 'a'
            tok = pool[torch.randint(0, len(pool), (R,), generator=g)].to(torch.int32)
            pos = [p] * R if shared else [max(0, p - r) for r in range(R)]
            _, state = launch(tb, tok, hist, pos, ops.stop_rows(R), shared_pos=shared)
            want = [bool(c1(torch.tensor([hist[r, :pos[r] + 1].tolist() + [int(tok[r])]]), None)[0]) for r in range(R)]
            assert state[:, 0].tolist() == [int(w) for w in want], (strs[0][:4], p)
            assert state[:, 1].tolist() == [pos[r] + 1 if want[r] else -1 for r in range(R)]
            if lone and p == ld - 1:
                assert any(want)                                          # the 64-character string does match
    assert SR.fires(t, [tk.vocab["a"], tk.vocab["#"]])                    # one character


def test_malformed_rows_change_verdicts_only(small):
    from valley_amd import ops
    tk, crit, tables, _, _ = small
    h = tk.vocab["#"]
    hist = torch.full((6, 8), h, dtype=torch.int32)
    tok = torch.tensor([h, h, tk.vocab["##"], h, h, h], dtype=torch.int32)
    rows = torch.tensor([[1, 5, 0, 0], [1, -3, 0, 0], [1 | 4 | 64, 0, 0, 7], [1, 2 ** 31 - 1, 0, 0], [1 | 2 | 1024, -2 ** 31, 9, -1],
                         [8, 0, 0, 0]], dtype=torch.int32)
    pos = torch.tensor([3, 3, 3, 3, 100, 3], dtype=torch.int32)               # row 4: a position outside the history
    got, st = launch(tables, tok, hist, pos, rows)
    # begin > pos: the token alone; a negative begin: 0; unknown bits: ignored; pos >= ld: the token alone; bit 0 clear: unwatched
    assert st.tolist() == [[0, -1], [1, 4], [1, 4], [0, -1], [0, -1], [0, -1]] and got.tolist() == tok.tolist()
    py = [[0, -1] for _ in range(6)]
    SR.apply(SR.tables_of(crit), tok.tolist(), hist.tolist(), pos.tolist(), rows.tolist(), py)
    assert py == st.tolist()
    # a header that does not describe a table inside the buffer: the string test is off, the EOS rule is not
    bad = tables._replace(buf=tables.buf.clone())
    bad.buf[4] = 10 ** 6
    _, st = launch(bad, tok, hist, pos, rows, eos=[tk.vocab["##"]])
    assert st[:, 0].tolist() == [0, 0, 1, 0, 0, 0]


def test_a_row_gives_the_same_result_wherever_it_stands(small):
    from valley_amd import ops
    tk, crit, tables, seqs, want = small
    pick = [i for i in range(0, len(seqs), 97) if len(seqs[i]) == 4][:24]
    ld = 8
    for order in (list(range(len(pick))), list(reversed(range(len(pick)))), [(7 * i + 3) % len(pick) for i in range(len(pick))]):
        rows_ = [seqs[pick[i]] for i in order]
        hist = torch.zeros((len(rows_), ld), dtype=torch.int32)
        hist[:, :3] = torch.tensor([s[:3] for s in rows_], dtype=torch.int32)
        tok = torch.tensor([s[3] for s in rows_], dtype=torch.int32)
        _, st = launch(tables, tok, hist, [2], ops.stop_rows(len(rows_)), shared_pos=True)
        assert st[:, 0].tolist() == [int(want[pick[i]]) for i in order]


def test_captured_launch_follows_new_rows_state_and_tables():
    from valley_amd import ops
    tk = ST.small()
    R, ld, cap = 4, 12, 4096
    tables = ops.StopTables(torch.zeros((cap,), dtype=torch.int32, device=dev()), (), 0)
    tok = torch.zeros((R,), dtype=torch.int32, device=dev())
    hist = torch.zeros((R, ld), dtype=torch.int32, device=dev())
    pos = torch.zeros((R,), dtype=torch.int32, device=dev())
    rows, state = ops.stop_rows(R, device=dev()), ops.stop_state(R, device=dev())
    eos = torch.tensor([tk.vocab["x"]], dtype=torch.int32, device=dev())
    g = torch.Generator().manual_seed(5)
    pool = torch.tensor([tk.vocab[p] for p in ("#", "##", "a#", "st", "op", "a", "x")])

    def fill(k):
        strings = [["###"], ["stop", "a#"], ["#", "op", "st"]][k]
        crit = hf(tk, strings)
        new = ops.stop_tables(tk, strings)
        tables.buf.zero_()
        tables.buf[:new.buf.numel()].copy_(new.buf)
        h = pool[torch.randint(0, len(pool), (R, ld), generator=g)].to(torch.int32)
        t = pool[torch.randint(0, len(pool), (R,), generator=g)].to(torch.int32)
        p = torch.randint(2, ld, (R,), generator=g).to(torch.int32)
        rw = ops.stop_rows(R, begin=[0, 1, 0, 2], pad=40 + k, watch=[1, 1, k != 1, 1], pad_after=True)
        st = torch.tensor([[0, -1], [0, -1], [0, -1], [int(k == 2), 1 if k == 2 else -1]], dtype=torch.int32)
        for dst, src in ((hist, h), (tok, t), (pos, p), (rows, rw), (state, st)):
            dst.copy_(src)
        py_tok, py_state = t.tolist(), st.tolist()
        SR.apply(SR.tables_of(crit), py_tok, h.tolist(), p.tolist(), rw.tolist(), py_state, eos=eos.tolist())
        return py_tok, py_state

    fill(0)
    ops.stop(tok, rows, state, tables, hist, pos, 0, eos=eos)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ops.stop(tok, rows, state, tables, hist, pos, 0, eos=eos)
    seen = set()
    for k in (1, 2, 0, 1):
        want_tok, want_state = fill(k)
        graph.replay()
        assert tok.tolist() == want_tok and state.tolist() == want_state, k
        seen.update(s[0] for s in want_state)
    assert seen == {0, 1}


# ---- generate() on the golden model -------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def model():
    from tests.test_model_gpu import build_golden_model
    return build_golden_model()


@pytest.fixture(scope="module")
def tokenizer():
    return ST.generated(G.GCFG["vocab"])


def three_rows():
    """Three left-padded prompts with their mask and frames: the two of the 'main' case and the 'decode' one."""
    T = G.GCFG["T"]
    (a, am), (b, bm) = G.golden_ids("main"), G.golden_ids("decode")
    prompts = [a[r][am[r] == 1].tolist() for r in range(2)] + [b[0][bm[0] == 1].tolist()]
    S = max(len(p) for p in prompts)
    ids = torch.tensor([[0] * (S - len(p)) + p for p in prompts])
    mask = torch.tensor([[0] * (S - len(p)) + [1] * len(p) for p in prompts])
    px = torch.cat([torch.from_numpy(G.golden_pixels(2 * T, "main")), torch.from_numpy(G.golden_pixels(T, "mixed"))])
    return ids.cuda(), mask.cuda(), px.view(3, T, 3, 224, 224).cuda()


def straddling_strings(tokenizer, plain, S, generated=False, quiet=()):
    """Stop strings from the text of the tokens that came out: one per row, the last character of a token and the whole next
    token, chosen so that every row's FIRST match (of any of the strings, HF's rule over the whole row — over its new tokens
    alone with ``generated``) ends at a step of its own, strictly inside the generation, and begins in the token before.
    ``plain``: the rows (a tensor, or lists with one prompt length each in ``S``); ``quiet``: (row, prompt length) pairs that no
    string may ever stop.  -> (strings, each row's end index).  Fails where no such choice exists."""
    rows = plain.tolist() if isinstance(plain, torch.Tensor) else [list(r) for r in plain]
    lens = [S] * len(rows) if isinstance(S, int) else list(S)
    piece = tokenizer.pieces

    def first_end(row, n0, strings):
        """(the first step at which HF's rule fires — a string ends inside the newest token —, whether every match there
        begins in front of that token)"""
        text = "" if generated else "".join(piece[i] for i in row[:n0])
        for j in range(n0, len(row)):
            text, n = text + piece[row[j]], len(piece[row[j]])
            hits = [(s, k) for s in strings for k in range(n) if text[:len(text) - k].endswith(s)]
            if hits:
                return j, all(len(s) > n - k for s, k in hits)
        return None, False

    options = [[piece[row[j - 1]][-1] + piece[row[j]] for j in range(n0 + 1, len(row) - 1)] for row, n0 in zip(rows, lens)]
    for combo in itertools.islice(itertools.product(*options), 200000):
        strings = sorted(set(combo))
        found = [first_end(row, n0, strings) for row, n0 in zip(rows, lens)]
        steps = [None if e is None else e - n0 for (e, _), n0 in zip(found, lens)]
        if all(e is not None and n0 < e < len(row) - 1 and straddles for (e, straddles), row, n0 in zip(found, rows, lens)) and \
                len(set(steps)) == len(steps) and all(first_end(list(q), n0, strings)[0] is None for q, n0 in quiet):
            return strings, [e for e, _ in found]
    raise AssertionError(f"no stop strings straddle two tokens strictly inside these generations: {[r[n0:] for r, n0 in zip(rows, lens)]}")


def oracle(model, tokenizer, strings, ids, **kw):
    """The existing path: HF's criterion as a host callback after every token."""
    return model.generate(ids, stopping_criteria=[hf(tokenizer, strings)], max_new_tokens=NEW, pad_token_id=0, **kw)


def check_routes(model, tokenizer, ids, kw, syncs=(1, 2, 5, 64), routes=(True, False, None)):
    plain = model.generate(ids, max_new_tokens=NEW, pad_token_id=0, **kw)
    S = ids.shape[1]
    strings, ends = straddling_strings(tokenizer, plain, S)
    want = oracle(model, tokenizer, strings, ids, **kw)
    assert want.shape[1] == max(ends) + 1 < plain.shape[1]
    for r, e in enumerate(ends):                                              # the row as it came out up to its end, then pad
        assert want[r, :e + 1].tolist() == plain[r, :e + 1].tolist() and not want[r, e + 1:].any()
    for ug in routes:
        for n in syncs if ug is not None else (1,):
            got = model.generate(ids, stop_strings=strings, tokenizer=tokenizer, sync_every=n, use_graph=ug, max_new_tokens=NEW,
                                 pad_token_id=0, **kw)
            assert torch.equal(got, want), (ug, n, got[:, S:].tolist(), want[:, S:].tolist())
    return strings, want


def test_generate_one_row_equals_the_host_criterion_in_every_route(model, tokenizer):
    ids, _, img = inputs("one")
    strings, want = check_routes(model, tokenizer, ids, dict(images=img))
    # a single string given as a string; the session is healthy after an early stop, and a plain call is what it was
    plain = model.generate(ids, images=img, max_new_tokens=NEW)
    got = model.generate(ids, images=img, stop_strings=strings[0], tokenizer=tokenizer, sync_every=64, max_new_tokens=NEW)
    assert torch.equal(got, oracle(model, tokenizer, strings[:1], ids, images=img))
    assert torch.equal(model.generate(ids, images=img, max_new_tokens=NEW), plain)


def test_generate_three_padded_rows_end_at_different_steps(model, tokenizer):
    ids, mask, img = three_rows()
    check_routes(model, tokenizer, ids, dict(images=img, attention_mask=mask))


def test_generate_seeded_sampling(model, tokenizer):
    ids, mask, img = three_rows()
    check_routes(model, tokenizer, ids, dict(images=img, attention_mask=mask, do_sample=True, temperature=0.9, top_k=40, seed=7),
                 syncs=(1, 5))


def test_generate_with_a_processor_and_a_constraint(model, tokenizer):
    ids, _, img = inputs("one")
    plain = model.generate(ids, images=img, max_new_tokens=4)
    check_routes(model, tokenizer, ids, dict(images=img, repetition_penalty=1.3, suppress_tokens=[int(plain[0, ids.shape[1] + 1])]),
                 syncs=(1, 5))


def test_generate_with_logprobs_and_eos(model, tokenizer):
    ids, _, img = inputs("one")
    S = ids.shape[1]
    plain = model.generate(ids, images=img, max_new_tokens=NEW, pad_token_id=0)
    strings, ends = straddling_strings(tokenizer, plain, S)
    kw = dict(images=img, max_new_tokens=NEW, pad_token_id=0, output_logprobs=True, top_logprobs=2, return_dict_in_generate=True)
    for ug in (True, None):
        want = model.generate(ids, stopping_criteria=[hf(tokenizer, strings)], use_graph=ug, **kw)
        got = model.generate(ids, stop_strings=strings, tokenizer=tokenizer, use_graph=ug, **kw)
        assert torch.equal(got.sequences, want.sequences) and got.sequences.shape[1] == ends[0] + 1
        assert torch.equal(got.token_logprobs, want.token_logprobs) and torch.equal(got.top_tokens, want.top_tokens)
    # the EOS ids on the device: an EOS in front of the stop string ends the row there, at every sync_every, and without strings
    e = int(plain[0, S + 1])
    want = model.generate(ids, images=img, max_new_tokens=NEW, eos_token_id=e, pad_token_id=0)
    assert S < want.shape[1] < plain.shape[1]
    for n in (1, 3):
        for ss in (strings, None):
            got = model.generate(ids, images=img, max_new_tokens=NEW, eos_token_id=e, pad_token_id=0, sync_every=n,
                                 **({} if ss is None else {"stop_strings": ss, "tokenizer": tokenizer}))
            assert torch.equal(got, want), (n, ss)
    # nothing stops: max_new_tokens ends it, whatever the block size
    never = ["f#f#f#f"]
    full = model.generate(ids, images=img, stop_strings=never, tokenizer=tokenizer, sync_every=5, max_new_tokens=NEW, pad_token_id=0)
    assert torch.equal(full, plain)


def test_host_multinomial_sampling_tests_the_drawn_token(model, tokenizer):
    ids, _, img = inputs("one")
    kw = dict(images=img, do_sample=True, temperature=0.8, max_new_tokens=NEW, pad_token_id=0)
    torch.manual_seed(3)
    plain = model.generate(ids, **kw)
    strings, ends = straddling_strings(tokenizer, plain, ids.shape[1])
    for ug in (True, None):
        torch.manual_seed(3)
        want = model.generate(ids, stopping_criteria=[hf(tokenizer, strings)], use_graph=ug, **kw)
        torch.manual_seed(3)
        got = model.generate(ids, stop_strings=strings, tokenizer=tokenizer, use_graph=ug, **kw)
        assert torch.equal(got, want)
        assert ug is None or got.shape[1] == ends[0] + 1                      # (the generic forward's logits draw their own tokens)


def test_stop_begin_generated_leaves_the_prompt_out(model, tokenizer):
    ids, _, img = inputs("one")
    S = ids.shape[1]
    plain = model.generate(ids, images=img, max_new_tokens=NEW, pad_token_id=0)
    # the prompt ends in the string's first half: its last character, then the whole first new token
    s = [tokenizer.pieces[int(ids[0, -1])][-1] + tokenizer.pieces[int(plain[0, S])]]
    kw = dict(images=img, stop_strings=s, tokenizer=tokenizer, max_new_tokens=NEW, pad_token_id=0)
    seq = model.generate(ids, **kw)
    assert seq.shape[1] == S + 1 and torch.equal(seq, oracle(model, tokenizer, s, ids, images=img))
    want = model.generate(ids, images=img, stopping_criteria=[SR.AsCriterion(hf(tokenizer, s), begin=S)], max_new_tokens=NEW, pad_token_id=0)
    assert want.shape[1] > S + 1
    for n in (1, 5):
        assert torch.equal(model.generate(ids, stop_begin="generated", sync_every=n, **kw), want)
    # where the match lies inside the answer the two are one
    strings, _ = straddling_strings(tokenizer, plain, S)
    kw["stop_strings"] = strings
    assert torch.equal(model.generate(ids, stop_begin="generated", **kw), model.generate(ids, **kw))


def test_a_prefix_session_second_turn(tokenizer):
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
    hand = lambda: HandPrefix(model, copy_rows(model, s, 289), 289)           # noqa: E731
    plain = model.generate(ids2, images=img, prefix=hand(), max_new_tokens=NEW, pad_token_id=0)
    strings, ends = straddling_strings(tokenizer, plain, ids2.shape[1])
    want = model.generate(ids2, images=img, prefix=hand(), stopping_criteria=[hf(tokenizer, strings)], max_new_tokens=NEW, pad_token_id=0)
    got = model.generate(ids2, images=img, prefix=s, stop_strings=strings, tokenizer=tokenizer, sync_every=5, max_new_tokens=NEW,
                         pad_token_id=0)
    assert s.stats["reused"] == 289 and torch.equal(got, want) and got.shape[1] == ends[0] + 1
    assert s.ids == got[0, :len(s.ids)].tolist() and s.cache.seq_len == len(s.ids) >= got.shape[1] - 1


def test_int8_engine(tokenizer):
    from tests.test_model_gpu import build_golden_model
    model = build_golden_model()
    model.quantize_decode_weights("int8")
    ids, _, img = inputs("one")
    check_routes(model, tokenizer, ids, dict(images=img), syncs=(1, 5))


# ---- completion() and the batcher ---------------------------------------------------------------------------------------------
def test_completion_with_stop_strings_returns_what_the_keyword_criterion_returns(model, monkeypatch):
    ids, _, img = inputs("one")
    S, V = ids.shape[1], G.GCFG["vocab"]
    plain = model.generate(ids, images=img, max_new_tokens=NEW)[0].tolist()
    j = next(j for j in range(S + 1, len(plain) - 1) if plain[j] != plain[j - 1] and plain[j] not in plain[S:j] and min(plain[j - 1:j + 1]) > 6)
    # a vocabulary without '#' but in two pieces: 'a#' and '##' meet as "###" where token j follows token j - 1
    pieces = [ST.piece_of(i).replace("#", "x") for i in range(V)]
    pieces[plain[j - 1]], pieces[plain[j]] = "a#", "##"
    tok = ST.ToyTokenizer(pieces)
    calls = []
    real = model.generate
    monkeypatch.setattr(model, "build_inputs", lambda tokenizer, message: type("I", (), {"input_ids": ids.tolist()})(), raising=False)
    monkeypatch.setattr(model, "generate", lambda **kw: calls.append(kw) or real(**kw), raising=False)
    video = img[0].permute(1, 0, 2, 3).float()
    base = dict(do_sample=False, max_new_tokens=NEW)
    want = model.completion(tok, video, [], base)
    got = [model.completion(tok, video, [], dict(base, stop_strings=["###"], **kw)) for kw in ({}, {"sync_every": 4})]
    assert got == [want, want] and "###" not in want[0]
    host, dev1, dev4 = calls
    assert len(host["stopping_criteria"]) == 1 and "stop_strings" not in host and "tokenizer" not in host
    assert dev1["stopping_criteria"] is None and dev1["stop_strings"] == ["###"] and dev1["stop_begin"] == "generated" and dev4["sync_every"] == 4
    out = [real(**c) for c in calls]
    assert torch.equal(out[0], out[1]) and torch.equal(out[0], out[2]) and out[0].shape[1] == j + 1


def test_batcher_reports_the_end_indices_generate_gives(model, tokenizer):
    from valley_amd.serving import ContinuousBatcher
    T = G.GCFG["T"]
    img = torch.from_numpy(G.golden_pixels(T, "mixed")).view(1, T, 3, 224, 224).cuda()
    reqs = [torch.from_numpy(G.golden_ids(c)[0]).cuda() for c in ("decode2", "decode")]
    plain = lambda r: model.generate(r, images=img, max_new_tokens=NEW, pad_token_id=0)[0].tolist()    # noqa: E731
    plains = [plain(r) for r in reqs]
    # two requests that stop at different steps of their answers, and a third that never does: the first prompt that allows it
    for third in (reqs[1][:, :-1], reqs[0][:, :-1], reqs[1][:, :-3], reqs[0][:, :-3], reqs[1][:, 1:], reqs[0][:, 1:]):
        try:
            strings, ends = straddling_strings(tokenizer, plains, [r.shape[1] for r in reqs], generated=True,
                                               quiet=[(plain(third), third.shape[1])])
            break
        except AssertionError as e:
            failure = e
    else:
        raise failure
    three = [reqs[0], reqs[1], third]

    def alone(r):
        out = model.generate(r, images=img, stop_strings=strings, tokenizer=tokenizer, stop_begin="generated", max_new_tokens=NEW,
                             pad_token_id=0)
        return out.shape[1] - 1 if out.shape[1] < r.shape[1] + NEW else None
    assert [alone(r) for r in three] == [ends[0], ends[1], None]
    assert ends[0] - reqs[0].shape[1] != ends[1] - reqs[1].shape[1]
    for order in ((0, 1, 2), (2, 1, 0)):
        cb = ContinuousBatcher(model, slots=4, ctx_max=512, stop_strings=strings, tokenizer=tokenizer)
        slot = {}
        for i in order:
            slot[i] = cb.add(three[i], images=img)
        found, toks = {}, {s: [int(cb.sess.tok[s])] for s in slot.values()}
        for _ in range(NEW - 1):
            out = cb.step()
            for s, t in out.items():
                toks[s].append(t)
            assert not set(cb.stopped) & set(found)                           # reported once
            found.update(cb.stopped)
        assert found == {slot[0]: ends[0], slot[1]: ends[1]}, (found, slot, ends)
        for i in (0, 1):                                                      # what step() returned is what it returns without them
            assert toks[slot[i]] == plains[i][reqs[i].shape[1]:]
        cb.release(slot[0])
        assert cb.sess.stop_rows[slot[0]].tolist() == [0, 0, 0, 0] and cb.sess.stop_state[slot[0]].tolist() == [0, -1]


def test_a_default_generation_never_loads_the_library():
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = ("import sys, torch\n"
            "from tests import golden_cfg as G\n"
            "from tests.test_model_gpu import build_golden_model\n"
            "from valley_amd.serving import ContinuousBatcher\n"
            "model = build_golden_model()\n"
            "T = G.GCFG['T']\n"
            "ids = torch.from_numpy(G.golden_ids('decode')[0]).cuda()\n"
            "img = torch.from_numpy(G.golden_pixels(T, 'mixed')).view(1, T, 3, 224, 224).cuda()\n"
            "for ug in (True, None):\n"
            "    model.generate(ids, images=img, max_new_tokens=3, use_graph=ug, repetition_penalty=1.2, eos_token_id=2)\n"
            "cb = ContinuousBatcher(model, slots=2, ctx_max=512, processors=True)\n"
            "cb.add(ids, images=img); cb.step()\n"
            "assert 'valley_amd.lib_stop' not in sys.modules and 'libvalley_hip_stop' not in open('/proc/self/maps').read()\n"
            "assert cb.sess.stop_state is None and cb.stop is None\n"
            "print('ok')\n")
    p = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, cwd=root, timeout=300)
    assert p.returncode == 0 and p.stdout.strip() == "ok", p.stderr[-2000:]
