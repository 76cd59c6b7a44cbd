"""What ``generate`` and ``ContinuousBatcher.add`` / ``step`` do on the host — which sessions they make and when, which ops.*
functions they call, in which order, on tensors of which dtype and shape and with which scalars, which criteria they evaluate
and where they synchronise — recorded on a toy language model with every launch function and every session replaced: no GPU,
no library.  The expected results and traces in ``EXPECTED`` were recorded from the generation loops as they stood inside
``ValleyLlamaForCausalLM`` and ``ContinuousBatcher.add`` before ``valley_amd/generation.py`` existed; the module is held to them.
The trace sees the ops.* functions, the sessions, the criteria and the stream's synchronise; it does not see torch's own launches
(``torch.zeros``, ``.to``, ``torch.where`` ...), whose order only reading the code, or a run on the device, can compare."""
from types import SimpleNamespace

import pytest
import torch

from valley_amd import decode, ops, serving, spec
from valley_amd import valley_model as vm

# Where the stand-ins go: (module, attribute, name of the stand-in below).  The only part of this file that may follow the code.
PATCHES = [(decode, "DecodeSession", "FakeDecodeSession"), (serving, "DecodeSession", "FakeDecodeSession"),
           (spec, "SpecDecodeSession", "FakeSpecDecodeSession"), (spec, "SpecRowsSession", "FakeSpecRowsSession"),
           (spec, "refuse_engine", "fake_refuse_engine"), (torch.cuda, "current_stream", "fake_current_stream")]
OPS = ("argmax sampling_rows processor_rows token_logprobs score_record logits_process beam_scratch beam_candidates beam_select "
       "logits_beam_candidates kv_beam_table kv_beam_reorder logits_history_gather sk_poll_async sk_check_polled").split()

V = 32
TRACE = []
SCRIPT = []                                                      # tokens per speculative step, consumed from the front (then 1)
DT = {torch.float32: "f32", torch.int32: "i32", torch.int64: "i64", torch.uint8: "u8", torch.bool: "b8"}


def show(v):
    if isinstance(v, torch.Tensor):
        return DT[v.dtype] + str(list(v.shape)).replace(" ", "")
    if isinstance(v, (tuple, list)) and any(isinstance(e, torch.Tensor) for e in v):
        return "(" + ",".join(show(e) for e in v) + ")"
    if isinstance(v, torch.device):
        return str(v)
    return "-" if v is None else repr(v)


def note(name, *a, **kw):
    TRACE.append(name + "(" + ", ".join([show(v) for v in a] + [f"{k}={show(v)}" for k, v in kw.items() if v is not None]) + ")")


# ---- the toy language model: the token behind ``tok`` at position ``pos`` is (3 * tok + pos + 1) % V ------------------------------
def toy_logits(tok, pos):
    """tok [R], pos int or [R] or [1] -> fp32 [R, V]: 0 at the next token, -1, -2, ... behind it (every argmax is unique)"""
    nxt = (tok.long() * 3 + torch.as_tensor(pos).long() + 1) % V
    return -((torch.arange(V)[None, :] - nxt[:, None]) % V).float()


def cpu_argmax(x, out=None, sampling=None, ctr=None, ctr_add=0):
    """the first maximal index; a sampling row with a temperature adds its seed's low word and the draw counter (mod V)"""
    tok = x.argmax(dim=-1).to(torch.int32)
    if sampling is not None:
        c = int(ctr_add) + (0 if ctr is None else ctr.long())
        drawn = ((tok.long() + sampling[:, 3].long() + c) % V).to(torch.int32)
        tok = torch.where(sampling.view(torch.float32)[:, 0] >= ops.GREEDY_T, drawn, tok)
    return tok if out is None else out.copy_(tok)


def cpu_token_logprobs(logits, targets=None, top=0, out_lse=None, copy=None, out_target=None, out_top=None):
    lse = torch.logsumexp(logits, dim=-1)
    if out_lse is not None:
        lse = out_lse.copy_(lse)
    tid = tl = None
    if top:
        v, i = torch.sort(logits, dim=-1, descending=True, stable=True)
        tid, tl = i[:, :top].to(torch.int32), v[:, :top] - lse[:, None]
        if out_top is not None:
            tid, tl = out_top[0].copy_(tid), out_top[1].copy_(tl)
    if copy is not None:
        copy[:, :logits.shape[1]].copy_(logits)
    return None, lse, tid, tl


def cpu_score_record(raw, lse, tok, lp_table, length=None, len_add=0, top=None, top_tables=None):
    for r in range(raw.shape[0]):
        c = int(len_add) + (0 if length is None else int(length[r if length.numel() > 1 else 0]))
        if 0 <= c < lp_table.shape[1]:
            lp_table[r, c] = raw[r, int(tok[r])] - lse[r]
            if top is not None:
                top_tables[0][r, c], top_tables[1][r, c] = top[0][r], top[1][r]


def cpu_beam_candidates(logits, running, B, nb, K, eos, scratch, out=None):
    """per prompt the K best of log_softmax + running, ties to the lower flat index"""
    s = (torch.log_softmax(logits, dim=-1) + running[:, None]).view(B, nb * logits.shape[1])
    v, i = torch.sort(s, dim=1, descending=True, stable=True)
    v, i = v[:, :K], i[:, :K]
    token, beam = (i % logits.shape[1]).to(torch.int32), (i // logits.shape[1] + torch.arange(B)[:, None] * nb).to(torch.int32)
    hit = (torch.isin(token, eos) if eos is not None else torch.zeros_like(token, dtype=torch.bool)).to(torch.uint8)
    res = tuple(t.reshape(-1) for t in (v, token, beam, hit))
    if out is not None:
        for o, t in zip(out, res):
            o.copy_(t)
    return res if out is None else out


def cpu_beam_select(score, token, beam, hit, B, nb, tok=None, parent=None, running=None):
    v = (score + hit.float() * -1e9).view(B, -1)
    keep = torch.sort(v, dim=1, descending=True, stable=True)[1][:, :nb]
    res = (token.view(B, -1).gather(1, keep).reshape(-1), beam.view(B, -1).gather(1, keep).reshape(-1), v.gather(1, keep).reshape(-1))
    for o, t in zip((tok, parent, running), res):
        if o is not None:
            o.copy_(t)
    return tuple(t if o is None else o for o, t in zip((tok, parent, running), res))


CPU = {"argmax": cpu_argmax, "sampling_rows": ops.sampling_rows, "processor_rows": ops.processor_rows, "token_logprobs": cpu_token_logprobs,
       "score_record": cpu_score_record, "logits_process": lambda logits, *a, **kw: logits,
       "beam_scratch": lambda B, nb, K, d: torch.zeros((256,), dtype=torch.uint8), "beam_candidates": cpu_beam_candidates,
       "beam_select": cpu_beam_select, "logits_beam_candidates": cpu_beam_candidates,
       "kv_beam_table": lambda k, v, d: torch.zeros((len(k), 2), dtype=torch.int64), "kv_beam_reorder": lambda *a, **kw: None,
       "logits_history_gather": lambda *a, **kw: None, "sk_poll_async": lambda d: None, "sk_check_polled": lambda d: None}


def traced(name):
    def fn(*a, **kw):
        note(name, *a, **kw)
        return CPU[name](*a, **kw)
    return fn


# ---- the caches and the sessions -------------------------------------------------------------------------------------------------
class Cache:
    growable = False

    def __init__(self, batch, ctx_max):
        self.batch, self.ctx_max, self.seq_len, self.key_valid, self.generation = batch, ctx_max, 0, None, 0
        self.k = self.v = [torch.zeros((batch, 1, ctx_max, 1))]

    @staticmethod
    def rows_of(c, lo, hi):
        note("rows_of", lo, hi)
        return Cache(hi - lo, c.ctx_max)

    def reserve(self, n):
        if n > self.ctx_max:
            raise ValueError("KV cache full")


class FakeDecodeSession:
    """DecodeSession's buffers and the tail of its step over the toy model; its own launches are not traced, its methods are"""

    def __init__(self, ll, cache, use_graph=True, per_row_positions=False, sampling=False, processors=False, processor_eos=None,
                 logprobs=None, beams=None):
        note("DecodeSession", cache.batch, use_graph=use_graph, per_row=per_row_positions or None, sampling=sampling or None,
             processors=processors or None, processor_eos=processor_eos, logprobs=logprobs, beams=beams)
        B = cache.batch
        self.ll, self.cache, self.per_row, self.beams = ll, cache, per_row_positions, beams
        self.tok = torch.zeros((B,), dtype=torch.int32)
        self.pos = torch.zeros((B if per_row_positions else 1,), dtype=torch.int32)
        self.sample = ops.sampling_rows([0.0] * B) if sampling else None
        self.logits = torch.zeros((B, ll.Vpad))
        if beams is not None:
            bB, nb, S, eos = beams[:4]
            K = max(2, 1 + len(eos)) * nb
            self.eos = torch.tensor(list(eos), dtype=torch.int32) if eos else None
            self.cand = (torch.zeros((bB * K,)), torch.zeros((bB * K,), dtype=torch.int32), torch.zeros((bB * K,), dtype=torch.int32),
                         torch.zeros((bB * K,), dtype=torch.uint8))
            self.parent, self.running, self.K = torch.arange(B, dtype=torch.int32), torch.zeros((B,)), K
        self.proc = self.hist = self.proc_eos = None
        if processors:
            self.proc = ops.processor_rows([None] * B)
            self.hist = torch.zeros((B, cache.ctx_max), dtype=torch.int32)
            if processor_eos:
                self.proc_eos = torch.tensor([int(e) for e in processor_eos], dtype=torch.int32)
        self.lp_n = None
        if logprobs is not None:
            self.lp_n = n = int(logprobs)
            self.lp_lse = torch.zeros((B,))
            self.lp_table = torch.zeros((B, cache.ctx_max + 1))
            self.lp_top = self.lp_top_tables = None
            if n:
                self.lp_top = (torch.full((B, n), -1, dtype=torch.int32), torch.zeros((B, n)))
                self.lp_top_tables = (torch.full((B, cache.ctx_max + 1, n), -1, dtype=torch.int32), torch.zeros((B, cache.ctx_max + 1, n)))

    def begin(self, first_token=None, prompt_ids=None):
        note("DecodeSession.begin", first_token, prompt_ids=prompt_ids, seeds=None if self.sample is None else self.sample[:, 3].tolist(),
             proc=None if self.proc is None else self.proc[:, 1:3].tolist())     # what the caller copied into the session's tables
        if prompt_ids is not None:
            self.hist[:, :prompt_ids.shape[1]].copy_(prompt_ids.to(torch.int32))
        if not self.per_row:
            self.pos.fill_(self.cache.seq_len)
            self.tok.copy_(first_token.to(torch.int32).view(-1))

    def _record(self, len_add):
        cpu_score_record(self.logits[:, :V], self.lp_lse, self.tok, self.lp_table, self.pos, len_add, top=self.lp_top,
                         top_tables=self.lp_top_tables)

    def record_token(self):
        note("DecodeSession.record_token", self.tok.tolist())
        self._record(0)

    def beam_tail(self):
        note("DecodeSession.beam_tail")
        cpu_beam_select(*self.cand, self.beams[0], self.beams[1], tok=self.tok, parent=self.parent, running=self.running)
        self.pos += 1

    def step(self):
        note("DecodeSession.step", self.tok.tolist(), self.pos.tolist())
        self.cache.reserve(self.cache.seq_len + 1)
        self.logits[:, :V] = toy_logits(self.tok, self.pos)
        self.cache.seq_len += 1
        if self.beams is not None:
            cpu_beam_candidates(self.logits[:, :V], self.running, self.beams[0], self.beams[1], self.K, self.eos, None, out=self.cand)
            if len(self.beams) < 5 or self.beams[4]:
                self.beam_tail()
            return self.tok
        if self.lp_n is not None:
            cpu_token_logprobs(self.logits[:, :V], top=self.lp_n, out_lse=self.lp_lse, out_top=self.lp_top)
        cpu_argmax(self.logits[:, :V], out=self.tok, sampling=self.sample, ctr=self.pos if self.sample is not None else None, ctr_add=1)
        if self.lp_n is not None:
            self._record(1)
        self.pos += 1
        return self.tok

    def check(self):
        note("DecodeSession.check")


def toy_run(tok, pos, n, sample):
    """the next n tokens of the sequence whose token at position ``pos`` is ``tok``"""
    out = []
    for j in range(n):
        t = cpu_argmax(toy_logits(torch.tensor([tok]), pos + j), sampling=None if sample is None else sample[:1], ctr_add=pos + j + 1)
        tok = int(t[0])
        out.append(tok)
    return out


class FakeSpecDecodeSession:
    def __init__(self, ll, cache, k, max_ngram=2, eos_ids=None, use_graph=True, sampling=False):
        note("SpecDecodeSession", k, max_ngram, eos_ids=eos_ids, use_graph=use_graph, sampling=sampling)
        self.cache, self.k, self.stats = cache, k, {"steps": 0, "drafted": 0, "accepted": 0}
        self.sample = ops.sampling_rows([0.0] * (k + 1)) if sampling else None

    def begin(self, first_token, prompt_ids=None):
        note("SpecDecodeSession.begin", first_token.tolist(), prompt_ids=None if prompt_ids is None else prompt_ids.tolist(),
             seeds=None if self.sample is None else self.sample[:, 3].tolist())
        self.tok = int(first_token[0])

    def step(self):
        n = SCRIPT.pop(0) if SCRIPT else 1
        note("SpecDecodeSession.step", self.tok, self.cache.seq_len, emits=n)
        assert 1 <= n <= self.k + 1 and self.cache.seq_len + self.k + 1 <= self.cache.ctx_max
        out = toy_run(self.tok, self.cache.seq_len, n, self.sample)
        self.cache.seq_len += n
        self.tok = out[-1]
        self.stats = {"steps": self.stats["steps"] + 1, "drafted": self.stats["drafted"] + self.k, "accepted": self.stats["accepted"] + n - 1}
        return out

    def check(self):
        note("SpecDecodeSession.check")

    def speculation(self):
        return dict(self.stats)


class FakeSpecRowsSession:
    def __init__(self, ll, cache, k, max_ngram=2, eos_ids=None, use_graph=True, sampling=False):
        note("SpecRowsSession", cache.batch, k, max_ngram=max_ngram, eos_ids=eos_ids, use_graph=use_graph, sampling=sampling)
        self.k, self.rows = k, {}

    def set_sequence(self, b, position, first_token, prompt_ids=None, sampling_row=None):
        note("SpecRowsSession.set_sequence", b, position, first_token, prompt_ids=prompt_ids.tolist(), sampling_row=sampling_row)
        self.rows[b] = [first_token, position, sampling_row]

    def begin(self):
        note("SpecRowsSession.begin")

    def step(self):
        note("SpecRowsSession.step", sorted(self.rows))
        out = {}
        for b, (tok, pos, sample) in sorted(self.rows.items()):
            n = SCRIPT.pop(0) if SCRIPT else 1
            out[b] = toy_run(tok, pos, n, sample)
            self.rows[b] = [out[b][-1], pos + n, sample]
        return out

    def release(self, b):
        note("SpecRowsSession.release", b)
        del self.rows[b]

    def check(self):
        note("SpecRowsSession.check")

    def speculation(self, b):
        return {"steps": 0, "drafted": 0, "accepted": 0}


def fake_refuse_engine():
    note("spec.refuse_engine")


def fake_current_stream(*a):
    return SimpleNamespace(synchronize=lambda: note("synchronize"))


class FakePrefix:
    """a PrefixSession that holds nothing yet: its forward computes the whole prompt"""

    def __init__(self, model):
        self.model, self.cache = model, Cache(1, 8)

    def refuse(self, input_ids, attention_mask, precision, what):
        note("prefix.refuse", input_ids, attention_mask, precision, what)

    def forward(self, input_ids, images):
        note("prefix.forward", input_ids, images)
        return self.model.run(input_ids, self.cache)

    def reserve(self, n):
        note("prefix.reserve", n)
        self.cache.ctx_max = max(self.cache.ctx_max, n)

    def settle(self, seq):
        note("prefix.settle", seq.tolist())


def make_model(precision="bf16", max_pos=64, pad=None):
    class Stub(vm.ValleyLlamaForCausalLM):
        def __init__(self):
            pass

        def run(self, input_ids, cache):
            S = input_ids.shape[1]
            logits = torch.stack([toy_logits(input_ids[:, i], cache.seq_len + i) for i in range(S)], dim=1)
            cache.seq_len += S
            return SimpleNamespace(logits=logits, past_key_values=cache)

        def forward(self, input_ids=None, images=None, attention_mask=None, past_key_values=None, use_cache=None):
            note("forward", input_ids, images=images, attention_mask=attention_mask, at=past_key_values.seq_len, use_cache=use_cache)
            return self.run(input_ids, past_key_values)

        __call__ = forward

    def new_cache(B, ctx):
        note("new_cache", B, ctx)
        return Cache(B, ctx)

    m = Stub()
    m.device = torch.device("cpu")
    m.config = SimpleNamespace(max_position_embeddings=max_pos, pad_token_id=pad)
    m.model = SimpleNamespace(llama=SimpleNamespace(V=V, Vpad=V, device=m.device, max_positions=max_pos, new_cache=new_cache),
                              precision=precision)
    return m


@pytest.fixture(autouse=True)
def stand_ins(monkeypatch):
    for mod, attr, name in PATCHES:
        monkeypatch.setattr(mod, attr, globals()[name])
    for name in OPS:
        monkeypatch.setattr(ops, name, traced(name))
    del TRACE[:], SCRIPT[:]


# ---- the cases -------------------------------------------------------------------------------------------------------------------
ONE = torch.tensor([[1, 2, 3, 4]])                               # greedy: 16 21 5 22 10 7 31 8
TWO = torch.tensor([[1, 2, 3, 4], [5, 6, 7, 9]])                 # row 1:  31 2 12 11 9 4 22 13
NINE = torch.arange(45).view(9, 5) % 7 + 1
REP = (None, None, None, None)


def crit_bool(n):
    def c(seq, scores):
        note("crit_bool", seq, scores)
        return seq.shape[1] >= n
    return c


def crit_rows(t):
    def c(seq, scores):
        note("crit_rows", seq, scores)
        return seq[:, -1] == t
    return c


def rnd(t):
    return None if t is None else [round(v, 4) for v in t.reshape(-1).tolist()] if t.dtype == torch.float32 else t.tolist()


def gen(ids=TWO, model=None, prefix=False, script=(), manual_seed=None, **kw):
    m = make_model(**(model or {}))
    SCRIPT.extend(script)
    if manual_seed is not None:
        torch.manual_seed(manual_seed)
    if prefix:
        kw["prefix"] = FakePrefix(m)
    out = m.generate(ids, **kw)
    if isinstance(out, torch.Tensor):
        return out.tolist()
    return {k: (rnd(v) if isinstance(v, torch.Tensor) else v) for k, v in vars(out).items()}


def refused(**kw):
    with pytest.raises(ValueError) as e:
        gen(**kw)
    return str(e.value)


def batch(requests, steps=2, script=(), **kw):
    m = make_model()
    SCRIPT.extend(script)
    torch.manual_seed(3)
    b = serving.ContinuousBatcher(m, ctx_max=16, **kw)
    out = [b.add(ONE if i == 0 else TWO[1:], **r) for i, r in enumerate(requests)]
    out.append(rnd(b.last_prefill_logits[:3]))
    out.extend(b.step() for _ in range(steps))
    if b.logprobs is not None:
        out.append({s: (round(lp, 4), ids, [round(v, 4) for v in lps]) for s, (lp, ids, lps) in sorted(b.first_logprobs.items())})
        out.append({s: (round(lp, 4), ids, [round(v, 4) for v in lps]) for s, (lp, ids, lps) in sorted(b.last_logprobs.items())})
    b.release(0)
    return out


LP = dict(output_logprobs=True, return_dict_in_generate=True)
PROC = dict(repetition_penalty=1.3, no_repeat_ngram_size=2, min_new_tokens=3)
CASES = {
    "greedy_eos_list": lambda: gen(max_new_tokens=8, eos_token_id=[5, 9]),
    "greedy_eos_int": lambda: gen(max_new_tokens=6, eos_token_id=5),
    "greedy_eos_int_eager": lambda: gen(max_new_tokens=6, eos_token_id=5, use_graph=False),
    "greedy_eos_int_generic": lambda: gen(max_new_tokens=6, eos_token_id=5, use_graph=None),
    "greedy_masked_generic": lambda: gen(max_new_tokens=3, use_graph=None, attention_mask=torch.ones((2, 4), dtype=torch.long)),
    "pad_keyword": lambda: gen(max_new_tokens=5, eos_token_id=5, pad_token_id=30),
    "pad_config": lambda: gen(max_new_tokens=5, eos_token_id=5, model=dict(pad=29)),
    "pad_zero": lambda: gen(max_new_tokens=5, stopping_criteria=[crit_rows(21)]),
    "criterion_bool": lambda: gen(max_new_tokens=8, stopping_criteria=[crit_bool(7)]),
    "criterion_rows": lambda: gen(max_new_tokens=4, stopping_criteria=[crit_rows(2)], eos_token_id=7),
    "criteria_both": lambda: gen(max_new_tokens=8, stopping_criteria=[crit_rows(21), crit_bool(8)], use_graph=None),
    "nine_rows": lambda: gen(NINE, max_new_tokens=3),
    "fp32": lambda: gen(max_new_tokens=3, model=dict(precision="fp32")),
    "one_token": lambda: gen(max_new_tokens=1, eos_token_id=16),
    "cache_end": lambda: gen(max_new_tokens=8, model=dict(max_pos=7)),
    "cache_end_generic": lambda: gen(max_new_tokens=8, model=dict(max_pos=7), use_graph=None),
    "host_multinomial": lambda: gen(max_new_tokens=4, do_sample=True, temperature=0.7, manual_seed=11, eos_token_id=17),
    "host_multinomial_logprobs": lambda: gen(max_new_tokens=4, do_sample=True, temperature=0.7, manual_seed=11, top_logprobs=2, **LP),
    "host_multinomial_generic": lambda: gen(max_new_tokens=3, do_sample=True, temperature=0.7, manual_seed=11, use_graph=None, **LP),
    "cold_temperature_is_greedy": lambda: gen(max_new_tokens=3, do_sample=True, temperature=1e-5, seed=4),
    "sample_seed_int": lambda: gen(max_new_tokens=4, do_sample=True, temperature=0.8, seed=5, top_k=4),
    "sample_seed_list": lambda: gen(max_new_tokens=4, do_sample=True, seed=[9, 2], top_p=0.9, use_graph=None),
    "sample_seed_wrong_length": lambda: refused(max_new_tokens=4, do_sample=True, seed=[9, 2, 3]),
    "sample_no_seed": lambda: gen(max_new_tokens=3, do_sample=True, top_k=5, manual_seed=7),
    "sample_logprobs": lambda: gen(max_new_tokens=3, do_sample=True, seed=1, **LP),
    "processors_eos": lambda: gen(max_new_tokens=4, eos_token_id=[5, 9], **PROC),
    "processors_no_eos": lambda: gen(max_new_tokens=3, **PROC),
    "processors_generic": lambda: gen(max_new_tokens=3, eos_token_id=5, use_graph=None, top_logprobs=1, **PROC, **LP),
    "processors_that_would_not_act": lambda: gen(max_new_tokens=3, repetition_penalty=1.0, no_repeat_ngram_size=0, min_length=3),
    "logprobs_top0": lambda: gen(max_new_tokens=4, eos_token_id=5, **LP),
    "logprobs_top2": lambda: gen(max_new_tokens=4, eos_token_id=21, top_logprobs=2, **LP),
    "logprobs_top0_generic": lambda: gen(max_new_tokens=3, use_graph=None, **LP),
    "logprobs_top2_generic": lambda: gen(max_new_tokens=3, eos_token_id=21, top_logprobs=2, use_graph=None, **LP),
    "return_dict_plain": lambda: gen(ONE, max_new_tokens=2, return_dict_in_generate=True),
    "spec_stop_inside_a_list": lambda: gen(ONE, max_new_tokens=8, prompt_lookup_num_tokens=3, eos_token_id=5, script=[3],
                                           return_dict_in_generate=True),
    "spec_criterion_inside_a_list": lambda: gen(ONE, max_new_tokens=8, prompt_lookup_num_tokens=3, script=[4, 2],
                                                stopping_criteria=[crit_bool(9), crit_rows(40)], use_graph=False),
    "spec_max_new_tokens_cut": lambda: gen(ONE, max_new_tokens=6, prompt_lookup_num_tokens=3, max_matching_ngram_size=4, script=[2, 4],
                                           eos_token_id=[40, 41], return_dict_in_generate=True),
    "spec_tail_session": lambda: gen(ONE, max_new_tokens=8, prompt_lookup_num_tokens=3, script=[2, 2], model=dict(max_pos=10),
                                     return_dict_in_generate=True),
    "spec_never_made": lambda: gen(ONE, max_new_tokens=3, prompt_lookup_num_tokens=3, return_dict_in_generate=True),
    "spec_seeded": lambda: gen(ONE, max_new_tokens=8, prompt_lookup_num_tokens=3, do_sample=True, temperature=0.8, seed=[6], top_k=3,
                               script=[2, 1], model=dict(max_pos=11), return_dict_in_generate=True),
    "spec_tensor": lambda: gen(ONE, max_new_tokens=3, prompt_lookup_num_tokens=2, script=[3]),
    "beams_one_prompt": lambda: gen(ONE, max_new_tokens=4, num_beams=2),
    "beams_two_prompts": lambda: gen(max_new_tokens=3, num_beams=2, use_graph=False, return_dict_in_generate=True),
    "beams_eos": lambda: gen(max_new_tokens=4, num_beams=2, eos_token_id=[21, 2], num_return_sequences=2, length_penalty=0.5,
                             return_dict_in_generate=True),
    "beams_criterion": lambda: gen(ONE, max_new_tokens=5, num_beams=2, eos_token_id=7, stopping_criteria=[crit_rows(22)],
                                   return_dict_in_generate=True),
    "beams_criterion_bool_generic": lambda: gen(ONE, max_new_tokens=5, num_beams=2, stopping_criteria=[crit_rows(22), crit_bool(7)],
                                                use_graph=None, pad_token_id=3, return_dict_in_generate=True),
    "beams_nine_rows": lambda: gen(NINE[:3], max_new_tokens=3, num_beams=3, eos_token_id=4, early_stopping=True,
                                   return_dict_in_generate=True),
    "beams_processors": lambda: gen(ONE, max_new_tokens=3, num_beams=2, eos_token_id=5, return_dict_in_generate=True, **PROC),
    "beams_processors_generic": lambda: gen(max_new_tokens=3, num_beams=2, use_graph=None, return_dict_in_generate=True, **PROC),
    "beams_fp32": lambda: gen(ONE, max_new_tokens=2, num_beams=2, model=dict(precision="fp32")),
    "beams_cache_end": lambda: gen(ONE, max_new_tokens=8, num_beams=2, model=dict(max_pos=6), use_graph=None, return_dict_in_generate=True),
    "beams_no_room": lambda: gen(max_new_tokens=0, num_beams=2, num_return_sequences=2, return_dict_in_generate=True),
    "prefix_greedy": lambda: gen(ONE, max_new_tokens=4, eos_token_id=22, prefix=True),
    "prefix_spec": lambda: gen(ONE, max_new_tokens=5, prompt_lookup_num_tokens=3, script=[2], prefix=True, return_dict_in_generate=True),
    "batcher_plain": lambda: batch([{}, {}]),
    "batcher_sampling": lambda: batch([dict(temperature=0.8, seed=5, top_k=4), {}, dict(temperature=0.9)], sampling=True),
    "batcher_processors": lambda: batch([dict(repetition_penalty=1.3, min_new_tokens=2), {}], processors=True, eos_token_id=[5, 9]),
    "batcher_logprobs": lambda: batch([{}, {}], logprobs=2),
    "batcher_logprobs_top0_eager": lambda: batch([{}], logprobs=0, use_graph=False),
    "batcher_everything": lambda: batch([dict(temperature=0.8, seed=5, no_repeat_ngram_size=2)], sampling=True, processors=True, logprobs=1,
                                        eos_token_id=5),
    "batcher_first_token": lambda: batch([dict(first_token=7), dict(first_token=9, temperature=0.8, seed=1)], sampling=True, logprobs=0),
    "batcher_speculating": lambda: batch([{}, {}], slots=2, prompt_lookup_num_tokens=1, script=[2, 1, 1, 2]),
    "batcher_speculating_seeded": lambda: batch([dict(temperature=0.8, seed=5)], slots=2, prompt_lookup_num_tokens=2, max_matching_ngram_size=3,
                                                sampling=True, eos_token_id=5, script=[3]),
}

EXPECTED = {
    "batcher_everything": (
        [0, [-16.0, -17.0, -18.0], {0: 26}, {0: 31}, {0: (-9.4587, [16], [-0.4587])}, {0: (-11.4587, [20], [-0.4587])}],
        "new_cache(4, 16); DecodeSession(4, use_graph=True, per_row=True, sampling=True, processors=True, processor_eos=[5], logprobs=1); "
        "sampling_rows([0.0, 0.0, 0.0, 0.0]); processor_rows([None, None, None, None]); sampling_rows(0.8, 0, 1.0, 5, device=cpu); "
        "processor_rows(-, 2, -, -, prompt_len=4, device=cpu); rows_of(0, 1); forward(i64[1,4], at=0, use_cache=True); "
        "token_logprobs(f32[1,32], top=1, copy=f32[1,32]); logits_process(f32[1,32], i32[1,4], i32[1,16], -, 4, -, i32[1]); argmax(f32[1,32], "
        "sampling=i32[1,6], ctr_add=4); score_record(f32[1,32], f32[1], i32[1], f32[1,17], -, 4, top=(i32[1,1],f32[1,1]), "
        "top_tables=(i32[1,17,1],f32[1,17,1])); DecodeSession.begin(-, seeds=[5, 0, 0, 0], proc=[[2, 0], [0, 0], [0, 0], [0, 0]]); "
        "DecodeSession.step([25, 0, 0, 0], [4, 0, 0, 0]); DecodeSession.step([26, 1, 1, 1], [5, 1, 1, 1]); DecodeSession.check()"),
    "batcher_first_token": (
        [0, 1, [-1.0, -2.0, -3.0], {0: 26, 1: 6}, {0: 20, 1: 31}, {0: (-23.4587, [], []), 1: (-10.4587, [], [])},
         {0: (-0.4587, [], []), 1: (-7.4587, [], [])}],
        "new_cache(4, 16); DecodeSession(4, use_graph=True, per_row=True, sampling=True, processor_eos=[], logprobs=0); sampling_rows([0.0, "
        "0.0, 0.0, 0.0]); sampling_rows(0.0, 0, 1.0, 0, device=cpu); rows_of(0, 1); forward(i64[1,4], at=0, use_cache=True); "
        "token_logprobs(f32[1,32], top=0, copy=f32[1,32]); score_record(f32[1,32], f32[1], i32[1], f32[1,17], -, 4); sampling_rows(0.8, 0, 1.0,"
        " 1, device=cpu); rows_of(1, 2); forward(i64[1,4], at=0, use_cache=True); token_logprobs(f32[1,32], top=0, copy=f32[1,32]); "
        "score_record(f32[1,32], f32[1], i32[1], f32[1,17], -, 4); DecodeSession.begin(-, seeds=[0, 1, 0, 0]); DecodeSession.step([7, 9, 0, 0],"
        " [4, 4, 0, 0]); DecodeSession.step([26, 6, 1, 1], [5, 5, 1, 1]); DecodeSession.check()"),
    "batcher_logprobs": (
        [0, 1, [-1.0, -2.0, -3.0], {0: 21, 1: 2}, {0: 5, 1: 12},
         {0: (-0.4587, [16, 17], [-0.4587, -1.4587]), 1: (-0.4587, [31, 0], [-0.4587, -1.4587])},
         {0: (-0.4587, [5, 6], [-0.4587, -1.4587]), 1: (-0.4587, [12, 13], [-0.4587, -1.4587])}],
        "new_cache(4, 16); DecodeSession(4, use_graph=True, per_row=True, processor_eos=[], logprobs=2); rows_of(0, 1); forward(i64[1,4], at=0,"
        " use_cache=True); token_logprobs(f32[1,32], top=2); score_record(f32[1,32], f32[1], i32[1], f32[1,17], -, 4, top=(i32[1,2],f32[1,2]), "
        "top_tables=(i32[1,17,2],f32[1,17,2])); rows_of(1, 2); forward(i64[1,4], at=0, use_cache=True); token_logprobs(f32[1,32], top=2); "
        "score_record(f32[1,32], f32[1], i32[1], f32[1,17], -, 4, top=(i32[1,2],f32[1,2]), top_tables=(i32[1,17,2],f32[1,17,2])); "
        "DecodeSession.begin(-); DecodeSession.step([16, 31, 0, 0], [4, 4, 0, 0]); DecodeSession.step([21, 2, 1, 1], [5, 5, 1, 1]); "
        "DecodeSession.check()"),
    "batcher_logprobs_top0_eager": (
        [0, [-16.0, -17.0, -18.0], {0: 21}, {0: 5}, {0: (-0.4587, [], [])}, {0: (-0.4587, [], [])}],
        "new_cache(4, 16); DecodeSession(4, use_graph=False, per_row=True, processor_eos=[], logprobs=0); rows_of(0, 1); forward(i64[1,4], "
        "at=0, use_cache=True); token_logprobs(f32[1,32], top=0); score_record(f32[1,32], f32[1], i32[1], f32[1,17], -, 4); "
        "DecodeSession.begin(-); DecodeSession.step([16, 0, 0, 0], [4, 0, 0, 0]); DecodeSession.step([21, 1, 1, 1], [5, 1, 1, 1]); "
        "DecodeSession.check()"),
    "batcher_plain": (
        [0, 1, [-1.0, -2.0, -3.0], {0: 21, 1: 2}, {0: 5, 1: 12}],
        "new_cache(4, 16); DecodeSession(4, use_graph=True, per_row=True, processor_eos=[]); rows_of(0, 1); forward(i64[1,4], at=0, "
        "use_cache=True); rows_of(1, 2); forward(i64[1,4], at=0, use_cache=True); DecodeSession.begin(-); DecodeSession.step([16, 31, 0, 0], "
        "[4, 4, 0, 0]); DecodeSession.step([21, 2, 1, 1], [5, 5, 1, 1]); DecodeSession.check()"),
    "batcher_processors": (
        [0, 1, [-1.0, -2.0, -3.0], {0: 21, 1: 2}, {0: 5, 1: 12}],
        "new_cache(4, 16); DecodeSession(4, use_graph=True, per_row=True, processors=True, processor_eos=[5, 9]); processor_rows([None, None, "
        "None, None]); processor_rows(1.3, -, -, 2, prompt_len=4, device=cpu); rows_of(0, 1); forward(i64[1,4], at=0, use_cache=True); "
        "logits_process(f32[1,32], i32[1,4], i32[1,16], -, 4, -, i32[2]); processor_rows(-, -, -, -, prompt_len=4, device=cpu); rows_of(1, 2); "
        "forward(i64[1,4], at=0, use_cache=True); logits_process(f32[1,32], i32[1,4], i32[1,16], -, 4, -, i32[2]); DecodeSession.begin(-, "
        "proc=[[0, 6], [0, 0], [0, 0], [0, 0]]); DecodeSession.step([16, 31, 0, 0], [4, 4, 0, 0]); DecodeSession.step([21, 2, 1, 1], [5, 5, 1, "
        "1]); DecodeSession.check()"),
    "batcher_sampling": (
        [0, 1, 2, [-1.0, -2.0, -3.0], {0: 26, 1: 2, 2: 19}, {0: 31, 1: 12, 2: 29}],
        "new_cache(4, 16); DecodeSession(4, use_graph=True, per_row=True, sampling=True, processor_eos=[]); sampling_rows([0.0, 0.0, 0.0, "
        "0.0]); sampling_rows(0.8, 4, 1.0, 5, device=cpu); rows_of(0, 1); forward(i64[1,4], at=0, use_cache=True); argmax(f32[1,32], "
        "sampling=i32[1,6], ctr_add=4); sampling_rows(0.0, 0, 1.0, 0, device=cpu); rows_of(1, 2); forward(i64[1,4], at=0, use_cache=True); "
        "sampling_rows(0.9, 0, 1.0, 937055941807507096, device=cpu); rows_of(2, 3); forward(i64[1,4], at=0, use_cache=True); argmax(f32[1,32], "
        "sampling=i32[1,6], ctr_add=4); DecodeSession.begin(-, seeds=[5, 0, 303761048, 0]); DecodeSession.step([25, 31, 27, 0], [4, 4, 4, 0]); "
        "DecodeSession.step([26, 2, 19, 1], [5, 5, 5, 1]); DecodeSession.check()"),
    "batcher_speculating": (
        [0, 1, [-1.0, -2.0, -3.0], {0: [21, 5], 1: [2]}, {0: [22], 1: [12, 11]}],
        "spec.refuse_engine(); new_cache(2, 16); SpecRowsSession(2, 1, max_ngram=2, eos_ids=[], use_graph=True, sampling=False); rows_of(0, 1);"
        " forward(i64[1,4], at=0, use_cache=True); SpecRowsSession.set_sequence(0, 4, 16, prompt_ids=[1, 2, 3, 4]); rows_of(1, 2); "
        "forward(i64[1,4], at=0, use_cache=True); SpecRowsSession.set_sequence(1, 4, 31, prompt_ids=[5, 6, 7, 9]); SpecRowsSession.begin(); "
        "SpecRowsSession.step([0, 1]); SpecRowsSession.step([0, 1]); SpecRowsSession.check(); SpecRowsSession.release(0)"),
    "batcher_speculating_seeded": (
        [0, [-16.0, -17.0, -18.0], {0: [26, 31, 16]}, {0: [5]}],
        "spec.refuse_engine(); new_cache(2, 16); SpecRowsSession(2, 2, max_ngram=3, eos_ids=[5], use_graph=True, sampling=True); "
        "sampling_rows(0.8, 0, 1.0, 5, device=cpu); rows_of(0, 1); forward(i64[1,4], at=0, use_cache=True); argmax(f32[1,32], "
        "sampling=i32[1,6], ctr_add=4); SpecRowsSession.set_sequence(0, 4, 25, prompt_ids=[1, 2, 3, 4], sampling_row=i32[1,6]); "
        "SpecRowsSession.begin(); SpecRowsSession.step([0]); SpecRowsSession.step([0]); SpecRowsSession.check(); SpecRowsSession.release(0)"),
    "beams_cache_end": (
        {'sequences': [[1, 2, 3, 4, 16, 21]], 'sequences_scores': [-0.4587]},
        "new_cache(2, 7); rows_of(0, 1); forward(i64[1,4], at=0, use_cache=True); kv_beam_table((f32[2,1,7,1]), (f32[2,1,7,1]), cpu); "
        "kv_beam_reorder(i64[1,2], f32[2,1,7,1], i32[2], 0, 4); beam_scratch(1, 2, 4, cpu); beam_candidates(f32[2,32], f32[2], 1, 2, 4, -, "
        "u8[256]); beam_select(f32[4], i32[4], i32[4], u8[4], 1, 2, running=f32[2]); forward(i64[2,1], at=4, use_cache=True); "
        "beam_candidates(f32[2,32], f32[2], 1, 2, 4, -, u8[256]); synchronize()"),
    "beams_criterion": (
        {'sequences': [[1, 2, 3, 4, 16, 21, 5, 22]], 'sequences_scores': [-0.4587]},
        "new_cache(2, 10); rows_of(0, 1); forward(i64[1,4], at=0, use_cache=True); kv_beam_table((f32[2,1,10,1]), (f32[2,1,10,1]), cpu); "
        "kv_beam_reorder(i64[1,2], f32[2,1,10,1], i32[2], 0, 4); beam_scratch(1, 2, 4, cpu); beam_candidates(f32[2,32], f32[2], 1, 2, 4, "
        "i32[1], u8[256]); DecodeSession(2, use_graph=True, beams=(1, 2, 4, [7], False)); crit_rows(i64[4,5], -); beam_select(f32[4], i32[4], "
        "i32[4], u8[4], 1, 2, tok=i32[2], parent=i32[2], running=f32[2]); DecodeSession.begin(i32[2]); DecodeSession.step([16, 17], [4]); "
        "crit_rows(i64[4,6], -); DecodeSession.beam_tail(); DecodeSession.step([21, 24], [5]); crit_rows(i64[4,7], -); "
        "DecodeSession.beam_tail(); DecodeSession.step([5, 6], [6]); crit_rows(i64[4,8], -); DecodeSession.beam_tail(); DecodeSession.step([23,"
        " 25], [7]); crit_rows(i64[4,9], -); synchronize(); DecodeSession.check()"),
    "beams_criterion_bool_generic": (
        {'sequences': [[1, 2, 3, 4, 16, 21, 5]], 'sequences_scores': [-0.4587]},
        "new_cache(2, 10); rows_of(0, 1); forward(i64[1,4], at=0, use_cache=True); kv_beam_table((f32[2,1,10,1]), (f32[2,1,10,1]), cpu); "
        "kv_beam_reorder(i64[1,2], f32[2,1,10,1], i32[2], 0, 4); beam_scratch(1, 2, 4, cpu); beam_candidates(f32[2,32], f32[2], 1, 2, 4, -, "
        "u8[256]); crit_rows(i64[4,5], -); crit_bool(i64[4,5], -); beam_select(f32[4], i32[4], i32[4], u8[4], 1, 2, running=f32[2]); "
        "forward(i64[2,1], at=4, use_cache=True); beam_candidates(f32[2,32], f32[2], 1, 2, 4, -, u8[256]); crit_rows(i64[4,6], -); "
        "crit_bool(i64[4,6], -); beam_select(f32[4], i32[4], i32[4], u8[4], 1, 2, running=f32[2]); kv_beam_reorder(i64[1,2], f32[2,1,10,1], "
        "i32[2], 4, 5); forward(i64[2,1], at=5, use_cache=True); beam_candidates(f32[2,32], f32[2], 1, 2, 4, -, u8[256]); crit_rows(i64[4,7], "
        "-); crit_bool(i64[4,7], -); synchronize()"),
    "beams_eos": (
        {'sequences': [[1, 2, 3, 4, 16, 21, 21, 21], [1, 2, 3, 4, 16, 22, 8, 31], [5, 6, 7, 9, 31, 2, 21, 21], [5, 6, 7, 9, 0, 5, 21, 21]],
         'sequences_scores': [-0.6487, -1.4174, -0.6487, -1.3718]},
        "new_cache(4, 9); rows_of(0, 2); forward(i64[2,4], at=0, use_cache=True); kv_beam_table((f32[4,1,9,1]), (f32[4,1,9,1]), cpu); "
        "kv_beam_reorder(i64[1,2], f32[4,1,9,1], i32[4], 0, 4); beam_scratch(2, 2, 6, cpu); beam_candidates(f32[4,32], f32[4], 2, 2, 6, i32[2],"
        " u8[256]); DecodeSession(4, use_graph=True, beams=(2, 2, 4, [21, 2], True)); beam_select(f32[12], i32[12], i32[12], u8[12], 2, 2, "
        "tok=i32[4], parent=i32[4], running=f32[4]); DecodeSession.begin(i32[4]); DecodeSession.step([16, 17, 31, 0], [4]); "
        "DecodeSession.beam_tail(); DecodeSession.step([22, 24, 3, 5], [5]); DecodeSession.beam_tail(); DecodeSession.step([8, 14, 15, 16], "
        "[6]); DecodeSession.beam_tail(); synchronize(); DecodeSession.check()"),
    "beams_fp32": (
        [[1, 2, 3, 4, 16, 21]],
        "new_cache(2, 7); rows_of(0, 1); forward(i64[1,4], at=0, use_cache=True); kv_beam_table((f32[2,1,7,1]), (f32[2,1,7,1]), cpu); "
        "kv_beam_reorder(i64[1,2], f32[2,1,7,1], i32[2], 0, 4); beam_scratch(1, 2, 4, cpu); beam_candidates(f32[2,32], f32[2], 1, 2, 4, -, "
        "u8[256]); beam_select(f32[4], i32[4], i32[4], u8[4], 1, 2, running=f32[2]); forward(i64[2,1], at=4, use_cache=True); "
        "beam_candidates(f32[2,32], f32[2], 1, 2, 4, -, u8[256]); synchronize()"),
    "beams_nine_rows": (
        {'sequences': [[1, 2, 3, 4, 5, 20, 2, 13], [6, 7, 1, 2, 3, 14, 16, 23], [4, 5, 6, 7, 1, 8, 30, 1]],
         'sequences_scores': [-0.4587, -0.4587, -0.4587]},
        "new_cache(9, 9); rows_of(0, 3); forward(i64[3,5], at=0, use_cache=True); kv_beam_table((f32[9,1,9,1]), (f32[9,1,9,1]), cpu); "
        "kv_beam_reorder(i64[1,2], f32[9,1,9,1], i32[9], 0, 5); beam_scratch(3, 3, 6, cpu); beam_candidates(f32[9,32], f32[9], 3, 3, 6, i32[1],"
        " u8[256]); beam_select(f32[18], i32[18], i32[18], u8[18], 3, 3, running=f32[9]); forward(i64[9,1], at=5, use_cache=True); "
        "beam_candidates(f32[9,32], f32[9], 3, 3, 6, i32[1], u8[256]); beam_select(f32[18], i32[18], i32[18], u8[18], 3, 3, running=f32[9]); "
        "kv_beam_reorder(i64[1,2], f32[9,1,9,1], i32[9], 5, 6); forward(i64[9,1], at=6, use_cache=True); beam_candidates(f32[9,32], f32[9], 3, "
        "3, 6, i32[1], u8[256]); synchronize()"),
    "beams_no_room": (
        {'sequences': [[1, 2, 3, 4], [5, 6, 7, 9]], 'sequences_scores': [0.0, 0.0, 0.0, 0.0]},
        ""),
    "beams_one_prompt": (
        [[1, 2, 3, 4, 16, 21, 5, 22]],
        "new_cache(2, 9); rows_of(0, 1); forward(i64[1,4], at=0, use_cache=True); kv_beam_table((f32[2,1,9,1]), (f32[2,1,9,1]), cpu); "
        "kv_beam_reorder(i64[1,2], f32[2,1,9,1], i32[2], 0, 4); beam_scratch(1, 2, 4, cpu); beam_candidates(f32[2,32], f32[2], 1, 2, 4, -, "
        "u8[256]); DecodeSession(2, use_graph=True, beams=(1, 2, 4, [], True)); beam_select(f32[4], i32[4], i32[4], u8[4], 1, 2, tok=i32[2], "
        "parent=i32[2], running=f32[2]); DecodeSession.begin(i32[2]); DecodeSession.step([16, 17], [4]); DecodeSession.beam_tail(); "
        "DecodeSession.step([21, 22], [5]); DecodeSession.beam_tail(); DecodeSession.step([5, 6], [6]); DecodeSession.beam_tail(); "
        "synchronize(); DecodeSession.check()"),
    "beams_processors": (
        {'sequences': [[1, 2, 3, 4, 16, 21, 5]], 'sequences_scores': [-0.4587]},
        "new_cache(2, 8); rows_of(0, 1); forward(i64[1,4], at=0, use_cache=True); kv_beam_table((f32[2,1,8,1]), (f32[2,1,8,1]), cpu); "
        "kv_beam_reorder(i64[1,2], f32[2,1,8,1], i32[2], 0, 4); beam_scratch(1, 2, 4, cpu); processor_rows(1.3, 2, -, 3, prompt_len=4); "
        "logits_process(f32[2,32], i32[2,4], i32[2,8], -, 4, -, i32[1], log_softmax=True); logits_beam_candidates(f32[2,32], f32[2], 1, 2, 4, "
        "i32[1], u8[256]); DecodeSession(2, use_graph=True, processors=True, beams=(1, 2, 4, [5], True)); processor_rows([None, None]); "
        "beam_select(f32[4], i32[4], i32[4], u8[4], 1, 2, tok=i32[2], parent=i32[2], running=f32[2]); DecodeSession.begin(i32[2], "
        "prompt_ids=i32[2,4], proc=[[2, 7], [2, 7]]); DecodeSession.step([16, 17], [4]); DecodeSession.beam_tail(); DecodeSession.step([21, "
        "22], [5]); DecodeSession.beam_tail(); synchronize(); DecodeSession.check()"),
    "beams_processors_generic": (
        {'sequences': [[1, 2, 3, 4, 16, 21, 5], [5, 6, 7, 9, 31, 2, 12]], 'sequences_scores': [-0.4587, -0.4587]},
        "new_cache(4, 8); rows_of(0, 2); forward(i64[2,4], at=0, use_cache=True); kv_beam_table((f32[4,1,8,1]), (f32[4,1,8,1]), cpu); "
        "kv_beam_reorder(i64[1,2], f32[4,1,8,1], i32[4], 0, 4); beam_scratch(2, 2, 4, cpu); processor_rows(1.3, 2, -, 3, prompt_len=4); "
        "logits_process(f32[4,32], i32[4,4], i32[4,8], -, 4, -, -, log_softmax=True); logits_beam_candidates(f32[4,32], f32[4], 2, 2, 4, -, "
        "u8[256]); beam_select(f32[8], i32[8], i32[8], u8[8], 2, 2, running=f32[4]); forward(i64[4,1], at=4, use_cache=True); "
        "logits_process(f32[4,32], i32[4,4], i32[4,8], -, 5, i32[4], -, log_softmax=True); logits_beam_candidates(f32[4,32], f32[4], 2, 2, 4, "
        "-, u8[256]); beam_select(f32[8], i32[8], i32[8], u8[8], 2, 2, running=f32[4]); kv_beam_reorder(i64[1,2], f32[4,1,8,1], i32[4], 4, 5); "
        "logits_history_gather(i32[4,8], i32[4], 4, 5); forward(i64[4,1], at=5, use_cache=True); logits_process(f32[4,32], i32[4,4], i32[4,8], "
        "-, 6, i32[4], -, log_softmax=True); logits_beam_candidates(f32[4,32], f32[4], 2, 2, 4, -, u8[256]); synchronize()"),
    "beams_two_prompts": (
        {'sequences': [[1, 2, 3, 4, 16, 21, 5], [5, 6, 7, 9, 31, 2, 12]], 'sequences_scores': [-0.4587, -0.4587]},
        "new_cache(4, 8); rows_of(0, 2); forward(i64[2,4], at=0, use_cache=True); kv_beam_table((f32[4,1,8,1]), (f32[4,1,8,1]), cpu); "
        "kv_beam_reorder(i64[1,2], f32[4,1,8,1], i32[4], 0, 4); beam_scratch(2, 2, 4, cpu); beam_candidates(f32[4,32], f32[4], 2, 2, 4, -, "
        "u8[256]); DecodeSession(4, use_graph=False, beams=(2, 2, 4, [], True)); beam_select(f32[8], i32[8], i32[8], u8[8], 2, 2, tok=i32[4], "
        "parent=i32[4], running=f32[4]); DecodeSession.begin(i32[4]); DecodeSession.step([16, 17, 31, 0], [4]); DecodeSession.beam_tail(); "
        "DecodeSession.step([21, 22, 2, 3], [5]); DecodeSession.beam_tail(); synchronize(); DecodeSession.check()"),
    "cache_end": (
        [[1, 2, 3, 4, 16, 21, 5, 22], [5, 6, 7, 9, 31, 2, 12, 11]],
        "new_cache(2, 7); forward(i64[2,4], at=0, use_cache=True); argmax(f32[2,32]); DecodeSession(2, use_graph=True); "
        "DecodeSession.begin(i64[2]); DecodeSession.step([16, 31], [4]); DecodeSession.step([21, 2], [5]); DecodeSession.step([5, 12], [6]); "
        "sk_poll_async(cpu); synchronize(); sk_check_polled(cpu); DecodeSession.check()"),
    "cache_end_generic": (
        [[1, 2, 3, 4, 16, 21, 5, 22], [5, 6, 7, 9, 31, 2, 12, 11]],
        "new_cache(2, 7); forward(i64[2,4], at=0, use_cache=True); argmax(f32[2,32]); forward(i64[2,1], at=4, use_cache=True); "
        "argmax(f32[2,32]); forward(i64[2,1], at=5, use_cache=True); argmax(f32[2,32]); forward(i64[2,1], at=6, use_cache=True); "
        "argmax(f32[2,32]); sk_poll_async(cpu); synchronize(); sk_check_polled(cpu)"),
    "cold_temperature_is_greedy": (
        [[1, 2, 3, 4, 16, 21, 5], [5, 6, 7, 9, 31, 2, 12]],
        "new_cache(2, 7); forward(i64[2,4], at=0, use_cache=True); argmax(f32[2,32]); DecodeSession(2, use_graph=True); "
        "DecodeSession.begin(i64[2]); DecodeSession.step([16, 31], [4]); DecodeSession.step([21, 2], [5]); sk_poll_async(cpu); synchronize(); "
        "sk_check_polled(cpu); DecodeSession.check()"),
    "criteria_both": (
        [[1, 2, 3, 4, 16, 21, 0, 0], [5, 6, 7, 9, 31, 2, 12, 11]],
        "new_cache(2, 12); forward(i64[2,4], at=0, use_cache=True); argmax(f32[2,32]); crit_rows(i64[2,5], -); crit_bool(i64[2,5], -); "
        "forward(i64[2,1], at=4, use_cache=True); argmax(f32[2,32]); crit_rows(i64[2,6], -); crit_bool(i64[2,6], -); forward(i64[2,1], at=5, "
        "use_cache=True); argmax(f32[2,32]); crit_rows(i64[2,7], -); crit_bool(i64[2,7], -); forward(i64[2,1], at=6, use_cache=True); "
        "argmax(f32[2,32]); crit_rows(i64[2,8], -); crit_bool(i64[2,8], -); sk_poll_async(cpu); synchronize(); sk_check_polled(cpu)"),
    "criterion_bool": (
        [[1, 2, 3, 4, 16, 21, 5], [5, 6, 7, 9, 31, 2, 12]],
        "new_cache(2, 12); forward(i64[2,4], at=0, use_cache=True); argmax(f32[2,32]); DecodeSession(2, use_graph=True); "
        "DecodeSession.begin(i64[2]); crit_bool(i64[2,5], -); DecodeSession.step([16, 31], [4]); crit_bool(i64[2,6], -); "
        "DecodeSession.step([21, 2], [5]); crit_bool(i64[2,7], -); sk_poll_async(cpu); synchronize(); sk_check_polled(cpu); "
        "DecodeSession.check()"),
    "criterion_rows": (
        [[1, 2, 3, 4, 16, 21, 5, 22], [5, 6, 7, 9, 31, 2, 7, 7]],
        "new_cache(2, 8); forward(i64[2,4], at=0, use_cache=True); argmax(f32[2,32]); DecodeSession(2, use_graph=True, processor_eos=[7]); "
        "DecodeSession.begin(i64[2]); crit_rows(i64[2,5], -); DecodeSession.step([16, 31], [4]); crit_rows(i64[2,6], -); "
        "DecodeSession.step([21, 2], [5]); crit_rows(i64[2,7], -); DecodeSession.step([5, 7], [6]); sk_poll_async(cpu); synchronize(); "
        "sk_check_polled(cpu); DecodeSession.check()"),
    "fp32": (
        [[1, 2, 3, 4, 16, 21, 5], [5, 6, 7, 9, 31, 2, 12]],
        "new_cache(2, 7); forward(i64[2,4], at=0, use_cache=True); argmax(f32[2,32]); forward(i64[2,1], at=4, use_cache=True); "
        "argmax(f32[2,32]); forward(i64[2,1], at=5, use_cache=True); argmax(f32[2,32]); sk_poll_async(cpu); synchronize(); sk_check_polled(cpu)"),
    "greedy_eos_int": (
        [[1, 2, 3, 4, 16, 21, 5, 5, 5, 5], [5, 6, 7, 9, 31, 2, 12, 11, 9, 4]],
        "new_cache(2, 10); forward(i64[2,4], at=0, use_cache=True); argmax(f32[2,32]); DecodeSession(2, use_graph=True, processor_eos=[5]); "
        "DecodeSession.begin(i64[2]); DecodeSession.step([16, 31], [4]); DecodeSession.step([21, 2], [5]); DecodeSession.step([5, 12], [6]); "
        "DecodeSession.step([5, 11], [7]); DecodeSession.step([5, 9], [8]); sk_poll_async(cpu); synchronize(); sk_check_polled(cpu); "
        "DecodeSession.check()"),
    "greedy_eos_int_eager": (
        [[1, 2, 3, 4, 16, 21, 5, 5, 5, 5], [5, 6, 7, 9, 31, 2, 12, 11, 9, 4]],
        "new_cache(2, 10); forward(i64[2,4], at=0, use_cache=True); argmax(f32[2,32]); DecodeSession(2, use_graph=False, processor_eos=[5]); "
        "DecodeSession.begin(i64[2]); DecodeSession.step([16, 31], [4]); DecodeSession.step([21, 2], [5]); DecodeSession.step([5, 12], [6]); "
        "DecodeSession.step([5, 11], [7]); DecodeSession.step([5, 9], [8]); sk_poll_async(cpu); synchronize(); sk_check_polled(cpu); "
        "DecodeSession.check()"),
    "greedy_eos_int_generic": (
        [[1, 2, 3, 4, 16, 21, 5, 5, 5, 5], [5, 6, 7, 9, 31, 2, 12, 11, 9, 4]],
        "new_cache(2, 10); forward(i64[2,4], at=0, use_cache=True); argmax(f32[2,32]); forward(i64[2,1], at=4, use_cache=True); "
        "argmax(f32[2,32]); forward(i64[2,1], at=5, use_cache=True); argmax(f32[2,32]); forward(i64[2,1], at=6, use_cache=True); "
        "argmax(f32[2,32]); forward(i64[2,1], at=7, use_cache=True); argmax(f32[2,32]); forward(i64[2,1], at=8, use_cache=True); "
        "argmax(f32[2,32]); sk_poll_async(cpu); synchronize(); sk_check_polled(cpu)"),
    "greedy_eos_list": (
        [[1, 2, 3, 4, 16, 21, 5, 5, 5], [5, 6, 7, 9, 31, 2, 12, 11, 9]],
        "new_cache(2, 12); forward(i64[2,4], at=0, use_cache=True); argmax(f32[2,32]); DecodeSession(2, use_graph=True, processor_eos=[5, 9]); "
        "DecodeSession.begin(i64[2]); DecodeSession.step([16, 31], [4]); DecodeSession.step([21, 2], [5]); DecodeSession.step([5, 12], [6]); "
        "DecodeSession.step([5, 11], [7]); sk_poll_async(cpu); synchronize(); sk_check_polled(cpu); DecodeSession.check()"),
    "greedy_masked_generic": (
        [[1, 2, 3, 4, 16, 21, 5], [5, 6, 7, 9, 31, 2, 12]],
        "new_cache(2, 7); forward(i64[2,4], attention_mask=i64[2,4], at=0, use_cache=True); argmax(f32[2,32]); forward(i64[2,1], "
        "attention_mask=i64[2,5], at=4, use_cache=True); argmax(f32[2,32]); forward(i64[2,1], attention_mask=i64[2,6], at=5, use_cache=True); "
        "argmax(f32[2,32]); sk_poll_async(cpu); synchronize(); sk_check_polled(cpu)"),
    "host_multinomial": (
        [[1, 2, 3, 4, 17, 17, 17, 17], [5, 6, 7, 9, 31, 2, 13, 16]],
        "new_cache(2, 8); forward(i64[2,4], at=0, use_cache=True); DecodeSession(2, use_graph=True, processor_eos=[17]); "
        "DecodeSession.begin(i64[2]); DecodeSession.step([17, 31], [4]); DecodeSession.step([17, 2], [5]); DecodeSession.step([17, 13], [6]); "
        "sk_poll_async(cpu); synchronize(); sk_check_polled(cpu); DecodeSession.check()"),
    "host_multinomial_generic": (
        {'sequences': [[1, 2, 3, 4, 17, 24, 15], [5, 6, 7, 9, 31, 2, 13]],
         'sequences_scores': None,
         'token_logprobs': [-1.4587, -0.4587, -1.4587, -0.4587, -0.4587, -1.4587]},
        "new_cache(2, 7); forward(i64[2,4], at=0, use_cache=True); token_logprobs(f32[2,32], top=0); score_record(f32[2,32], f32[2], i32[2], "
        "f32[2,1], -, 0); forward(i64[2,1], at=4, use_cache=True); token_logprobs(f32[2,32], top=0); score_record(f32[2,32], f32[2], i32[2], "
        "f32[2,1], -, 0); forward(i64[2,1], at=5, use_cache=True); token_logprobs(f32[2,32], top=0); score_record(f32[2,32], f32[2], i32[2], "
        "f32[2,1], -, 0); sk_poll_async(cpu); synchronize(); sk_check_polled(cpu)"),
    "host_multinomial_logprobs": (
        {'sequences': [[1, 2, 3, 4, 17, 24, 15, 23], [5, 6, 7, 9, 31, 2, 13, 16]],
         'sequences_scores': None,
         'token_logprobs': [-1.4587, -0.4587, -1.4587, -3.4587, -0.4587, -0.4587, -1.4587, -2.4587],
         'top_tokens': [[[16, 17], [24, 25], [14, 15], [20, 21]], [[31, 0], [2, 3], [12, 13], [14, 15]]],
         'top_logprobs': [-0.4587, -1.4587, -0.4587, -1.4587, -0.4587, -1.4587, -0.4587, -1.4587, -0.4587, -1.4587, -0.4587, -1.4587, -0.4587,
                          -1.4587, -0.4587, -1.4587]},
        "new_cache(2, 8); forward(i64[2,4], at=0, use_cache=True); token_logprobs(f32[2,32], top=2); score_record(f32[2,32], f32[2], i32[2], "
        "f32[2,1], -, 0, top=(i32[2,2],f32[2,2]), top_tables=(i32[2,1,2],f32[2,1,2])); DecodeSession(2, use_graph=True, logprobs=2); "
        "DecodeSession.begin(i64[2]); DecodeSession.step([17, 31], [4]); DecodeSession.record_token([24, 2]); DecodeSession.step([24, 2], [5]);"
        " DecodeSession.record_token([15, 13]); DecodeSession.step([15, 13], [6]); DecodeSession.record_token([23, 16]); sk_poll_async(cpu); "
        "synchronize(); sk_check_polled(cpu); DecodeSession.check()"),
    "logprobs_top0": (
        {'sequences': [[1, 2, 3, 4, 16, 21, 5, 5], [5, 6, 7, 9, 31, 2, 12, 11]],
         'sequences_scores': None,
         'token_logprobs': [-0.4587, -0.4587, -0.4587, 0.0, -0.4587, -0.4587, -0.4587, -0.4587]},
        "new_cache(2, 8); forward(i64[2,4], at=0, use_cache=True); token_logprobs(f32[2,32], top=0); argmax(f32[2,32]); score_record(f32[2,32],"
        " f32[2], i32[2], f32[2,1], -, 0); DecodeSession(2, use_graph=True, processor_eos=[5], logprobs=0); DecodeSession.begin(i64[2]); "
        "DecodeSession.step([16, 31], [4]); DecodeSession.step([21, 2], [5]); DecodeSession.step([5, 12], [6]); sk_poll_async(cpu); "
        "synchronize(); sk_check_polled(cpu); DecodeSession.check()"),
    "logprobs_top0_generic": (
        {'sequences': [[1, 2, 3, 4, 16, 21, 5], [5, 6, 7, 9, 31, 2, 12]],
         'sequences_scores': None,
         'token_logprobs': [-0.4587, -0.4587, -0.4587, -0.4587, -0.4587, -0.4587]},
        "new_cache(2, 7); forward(i64[2,4], at=0, use_cache=True); token_logprobs(f32[2,32], top=0); argmax(f32[2,32]); score_record(f32[2,32],"
        " f32[2], i32[2], f32[2,1], -, 0); forward(i64[2,1], at=4, use_cache=True); token_logprobs(f32[2,32], top=0); argmax(f32[2,32]); "
        "score_record(f32[2,32], f32[2], i32[2], f32[2,1], -, 0); forward(i64[2,1], at=5, use_cache=True); token_logprobs(f32[2,32], top=0); "
        "argmax(f32[2,32]); score_record(f32[2,32], f32[2], i32[2], f32[2,1], -, 0); sk_poll_async(cpu); synchronize(); sk_check_polled(cpu)"),
    "logprobs_top2": (
        {'sequences': [[1, 2, 3, 4, 16, 21, 21, 21], [5, 6, 7, 9, 31, 2, 12, 11]],
         'sequences_scores': None,
         'token_logprobs': [-0.4587, -0.4587, 0.0, 0.0, -0.4587, -0.4587, -0.4587, -0.4587],
         'top_tokens': [[[16, 17], [21, 22], [-1, -1], [-1, -1]], [[31, 0], [2, 3], [12, 13], [11, 12]]],
         'top_logprobs': [-0.4587, -1.4587, -0.4587, -1.4587, 0.0, 0.0, 0.0, 0.0, -0.4587, -1.4587, -0.4587, -1.4587, -0.4587, -1.4587, -0.4587,
                          -1.4587]},
        "new_cache(2, 8); forward(i64[2,4], at=0, use_cache=True); token_logprobs(f32[2,32], top=2); argmax(f32[2,32]); score_record(f32[2,32],"
        " f32[2], i32[2], f32[2,1], -, 0, top=(i32[2,2],f32[2,2]), top_tables=(i32[2,1,2],f32[2,1,2])); DecodeSession(2, use_graph=True, "
        "processor_eos=[21], logprobs=2); DecodeSession.begin(i64[2]); DecodeSession.step([16, 31], [4]); DecodeSession.step([21, 2], [5]); "
        "DecodeSession.step([21, 12], [6]); sk_poll_async(cpu); synchronize(); sk_check_polled(cpu); DecodeSession.check()"),
    "logprobs_top2_generic": (
        {'sequences': [[1, 2, 3, 4, 16, 21, 21], [5, 6, 7, 9, 31, 2, 12]],
         'sequences_scores': None,
         'token_logprobs': [-0.4587, -0.4587, 0.0, -0.4587, -0.4587, -0.4587],
         'top_tokens': [[[16, 17], [21, 22], [-1, -1]], [[31, 0], [2, 3], [12, 13]]],
         'top_logprobs': [-0.4587, -1.4587, -0.4587, -1.4587, 0.0, 0.0, -0.4587, -1.4587, -0.4587, -1.4587, -0.4587, -1.4587]},
        "new_cache(2, 7); forward(i64[2,4], at=0, use_cache=True); token_logprobs(f32[2,32], top=2); argmax(f32[2,32]); score_record(f32[2,32],"
        " f32[2], i32[2], f32[2,1], -, 0, top=(i32[2,2],f32[2,2]), top_tables=(i32[2,1,2],f32[2,1,2])); forward(i64[2,1], at=4, "
        "use_cache=True); token_logprobs(f32[2,32], top=2); argmax(f32[2,32]); score_record(f32[2,32], f32[2], i32[2], f32[2,1], -, 0, "
        "top=(i32[2,2],f32[2,2]), top_tables=(i32[2,1,2],f32[2,1,2])); forward(i64[2,1], at=5, use_cache=True); token_logprobs(f32[2,32], "
        "top=2); argmax(f32[2,32]); score_record(f32[2,32], f32[2], i32[2], f32[2,1], -, 0, top=(i32[2,2],f32[2,2]), "
        "top_tables=(i32[2,1,2],f32[2,1,2])); sk_poll_async(cpu); synchronize(); sk_check_polled(cpu)"),
    "nine_rows": (
        [[1, 2, 3, 4, 5, 20, 2, 13], [6, 7, 1, 2, 3, 14, 16, 23], [4, 5, 6, 7, 1, 8, 30, 1], [2, 3, 4, 5, 6, 23, 11, 8],
         [7, 1, 2, 3, 4, 17, 25, 18], [5, 6, 7, 1, 2, 11, 7, 28], [3, 4, 5, 6, 7, 26, 20, 3], [1, 2, 3, 4, 5, 20, 2, 13],
         [6, 7, 1, 2, 3, 14, 16, 23]],
        "new_cache(9, 8); forward(i64[9,5], at=0, use_cache=True); argmax(f32[9,32]); forward(i64[9,1], at=5, use_cache=True); "
        "argmax(f32[9,32]); forward(i64[9,1], at=6, use_cache=True); argmax(f32[9,32]); sk_poll_async(cpu); synchronize(); sk_check_polled(cpu)"),
    "one_token": (
        [[1, 2, 3, 4, 16], [5, 6, 7, 9, 31]],
        "new_cache(2, 5); forward(i64[2,4], at=0, use_cache=True); argmax(f32[2,32]); DecodeSession(2, use_graph=True, processor_eos=[16]); "
        "DecodeSession.begin(i64[2]); sk_poll_async(cpu); synchronize(); sk_check_polled(cpu); DecodeSession.check()"),
    "pad_config": (
        [[1, 2, 3, 4, 16, 21, 5, 29, 29], [5, 6, 7, 9, 31, 2, 12, 11, 9]],
        "new_cache(2, 9); forward(i64[2,4], at=0, use_cache=True); argmax(f32[2,32]); DecodeSession(2, use_graph=True, processor_eos=[5]); "
        "DecodeSession.begin(i64[2]); DecodeSession.step([16, 31], [4]); DecodeSession.step([21, 2], [5]); DecodeSession.step([5, 12], [6]); "
        "DecodeSession.step([29, 11], [7]); sk_poll_async(cpu); synchronize(); sk_check_polled(cpu); DecodeSession.check()"),
    "pad_keyword": (
        [[1, 2, 3, 4, 16, 21, 5, 30, 30], [5, 6, 7, 9, 31, 2, 12, 11, 9]],
        "new_cache(2, 9); forward(i64[2,4], at=0, use_cache=True); argmax(f32[2,32]); DecodeSession(2, use_graph=True, processor_eos=[5]); "
        "DecodeSession.begin(i64[2]); DecodeSession.step([16, 31], [4]); DecodeSession.step([21, 2], [5]); DecodeSession.step([5, 12], [6]); "
        "DecodeSession.step([30, 11], [7]); sk_poll_async(cpu); synchronize(); sk_check_polled(cpu); DecodeSession.check()"),
    "pad_zero": (
        [[1, 2, 3, 4, 16, 21, 0, 0, 0], [5, 6, 7, 9, 31, 2, 12, 11, 9]],
        "new_cache(2, 9); forward(i64[2,4], at=0, use_cache=True); argmax(f32[2,32]); DecodeSession(2, use_graph=True); "
        "DecodeSession.begin(i64[2]); crit_rows(i64[2,5], -); DecodeSession.step([16, 31], [4]); crit_rows(i64[2,6], -); "
        "DecodeSession.step([21, 2], [5]); crit_rows(i64[2,7], -); DecodeSession.step([0, 12], [6]); crit_rows(i64[2,8], -); "
        "DecodeSession.step([0, 11], [7]); sk_poll_async(cpu); synchronize(); sk_check_polled(cpu); DecodeSession.check()"),
    "prefix_greedy": (
        [[1, 2, 3, 4, 16, 21, 5, 22]],
        "prefix.refuse(i64[1,4], -, 'bf16', 'generate(prefix=)'); prefix.forward(i64[1,4], -); prefix.reserve(8); argmax(f32[1,32]); "
        "DecodeSession(1, use_graph=True, processor_eos=[22]); DecodeSession.begin(i64[1]); DecodeSession.step([16], [4]); "
        "DecodeSession.step([21], [5]); DecodeSession.step([5], [6]); sk_poll_async(cpu); synchronize(); sk_check_polled(cpu); "
        "DecodeSession.check(); prefix.settle([[1, 2, 3, 4, 16, 21, 5, 22]])"),
    "prefix_spec": (
        {'sequences': [[1, 2, 3, 4, 16, 21, 5, 22, 10]], 'sequences_scores': None, 'speculation': {'steps': 3, 'drafted': 3, 'accepted': 1}},
        "prefix.refuse(i64[1,4], -, 'bf16', 'generate(prefix=)'); spec.refuse_engine(); prefix.forward(i64[1,4], -); prefix.reserve(9); "
        "argmax(f32[1,32]); SpecDecodeSession(3, 2, use_graph=True, sampling=False); SpecDecodeSession.begin([16], prompt_ids=[1, 2, 3, 4]); "
        "SpecDecodeSession.step(16, 4, emits=2); DecodeSession(1, use_graph=True); DecodeSession.begin(i64[1]); DecodeSession.step([5], [6]); "
        "DecodeSession.step([22], [7]); sk_poll_async(cpu); synchronize(); sk_check_polled(cpu); SpecDecodeSession.check(); "
        "DecodeSession.check(); prefix.settle([[1, 2, 3, 4, 16, 21, 5, 22, 10]])"),
    "processors_eos": (
        [[1, 2, 3, 4, 16, 21, 5, 5], [5, 6, 7, 9, 31, 2, 12, 11]],
        "new_cache(2, 8); forward(i64[2,4], at=0, use_cache=True); processor_rows(1.3, 2, -, 3, prompt_len=4); logits_process(f32[2,32], "
        "i32[2,4], i32[2,8], -, 4, -, i32[2]); argmax(f32[2,32]); DecodeSession(2, use_graph=True, processors=True, processor_eos=[5, 9]); "
        "processor_rows([None, None]); DecodeSession.begin(i64[2], prompt_ids=i64[2,4], proc=[[2, 7], [2, 7]]); DecodeSession.step([16, 31], "
        "[4]); DecodeSession.step([21, 2], [5]); DecodeSession.step([5, 12], [6]); sk_poll_async(cpu); synchronize(); sk_check_polled(cpu); "
        "DecodeSession.check()"),
    "processors_generic": (
        {'sequences': [[1, 2, 3, 4, 16, 21, 5], [5, 6, 7, 9, 31, 2, 12]],
         'sequences_scores': None,
         'token_logprobs': [-0.4587, -0.4587, -0.4587, -0.4587, -0.4587, -0.4587],
         'top_tokens': [[[16], [21], [5]], [[31], [2], [12]]],
         'top_logprobs': [-0.4587, -0.4587, -0.4587, -0.4587, -0.4587, -0.4587]},
        "new_cache(2, 7); forward(i64[2,4], at=0, use_cache=True); processor_rows(1.3, 2, -, 3, prompt_len=4); token_logprobs(f32[2,32], top=1,"
        " copy=f32[2,32]); logits_process(f32[2,32], i32[2,4], i32[2,7], -, 4, -, i32[1]); argmax(f32[2,32]); score_record(f32[2,32], f32[2], "
        "i32[2], f32[2,1], -, 0, top=(i32[2,1],f32[2,1]), top_tables=(i32[2,1,1],f32[2,1,1])); forward(i64[2,1], at=4, use_cache=True); "
        "token_logprobs(f32[2,32], top=1, copy=f32[2,32]); logits_process(f32[2,32], i32[2,4], i32[2,7], -, 5, i32[2], i32[1]); "
        "argmax(f32[2,32]); score_record(f32[2,32], f32[2], i32[2], f32[2,1], -, 0, top=(i32[2,1],f32[2,1]), "
        "top_tables=(i32[2,1,1],f32[2,1,1])); forward(i64[2,1], at=5, use_cache=True); token_logprobs(f32[2,32], top=1, copy=f32[2,32]); "
        "logits_process(f32[2,32], i32[2,4], i32[2,7], -, 6, i32[2], i32[1]); argmax(f32[2,32]); score_record(f32[2,32], f32[2], i32[2], "
        "f32[2,1], -, 0, top=(i32[2,1],f32[2,1]), top_tables=(i32[2,1,1],f32[2,1,1])); sk_poll_async(cpu); synchronize(); sk_check_polled(cpu)"),
    "processors_no_eos": (
        [[1, 2, 3, 4, 16, 21, 5], [5, 6, 7, 9, 31, 2, 12]],
        "new_cache(2, 7); forward(i64[2,4], at=0, use_cache=True); processor_rows(1.3, 2, -, 3, prompt_len=4); logits_process(f32[2,32], "
        "i32[2,4], i32[2,7], -, 4, -, -); argmax(f32[2,32]); DecodeSession(2, use_graph=True, processors=True); processor_rows([None, None]); "
        "DecodeSession.begin(i64[2], prompt_ids=i64[2,4], proc=[[2, 0], [2, 0]]); DecodeSession.step([16, 31], [4]); DecodeSession.step([21, "
        "2], [5]); sk_poll_async(cpu); synchronize(); sk_check_polled(cpu); DecodeSession.check()"),
    "processors_that_would_not_act": (
        [[1, 2, 3, 4, 16, 21, 5], [5, 6, 7, 9, 31, 2, 12]],
        "new_cache(2, 7); forward(i64[2,4], at=0, use_cache=True); processor_rows(1.0, 0, 3, -, prompt_len=4); argmax(f32[2,32]); "
        "DecodeSession(2, use_graph=True); DecodeSession.begin(i64[2]); DecodeSession.step([16, 31], [4]); DecodeSession.step([21, 2], [5]); "
        "sk_poll_async(cpu); synchronize(); sk_check_polled(cpu); DecodeSession.check()"),
    "return_dict_plain": (
        {'sequences': [[1, 2, 3, 4, 16, 21]], 'sequences_scores': None},
        "new_cache(1, 6); forward(i64[1,4], at=0, use_cache=True); argmax(f32[1,32]); DecodeSession(1, use_graph=True); "
        "DecodeSession.begin(i64[1]); DecodeSession.step([16], [4]); sk_poll_async(cpu); synchronize(); sk_check_polled(cpu); "
        "DecodeSession.check()"),
    "sample_logprobs": (
        {'sequences': [[1, 2, 3, 4, 21, 10, 11], [5, 6, 7, 9, 5, 27, 31]],
         'sequences_scores': None,
         'token_logprobs': [-5.4587, -6.4587, -7.4587, -6.4587, -7.4587, -8.4587]},
        "new_cache(2, 7); forward(i64[2,4], at=0, use_cache=True); sampling_rows(1.0, 0, 1.0, [1, 2], device=cpu); token_logprobs(f32[2,32], "
        "top=0, copy=f32[2,32]); argmax(f32[2,32], sampling=i32[2,6], ctr_add=4); score_record(f32[2,32], f32[2], i32[2], f32[2,1], -, 0); "
        "DecodeSession(2, use_graph=True, sampling=True, logprobs=0); sampling_rows([0.0, 0.0]); DecodeSession.begin(i64[2], seeds=[1, 2]); "
        "DecodeSession.step([21, 5], [4]); DecodeSession.step([10, 27], [5]); sk_poll_async(cpu); synchronize(); sk_check_polled(cpu); "
        "DecodeSession.check()"),
    "sample_no_seed": (
        [[1, 2, 3, 4, 24, 22, 18], [5, 6, 7, 9, 8, 7, 6]],
        "new_cache(2, 7); forward(i64[2,4], at=0, use_cache=True); sampling_rows(1.0, 5, 1.0, [1407639518939636932, 1407639518939636933], "
        "device=cpu); argmax(f32[2,32], sampling=i32[2,6], ctr_add=4); DecodeSession(2, use_graph=True, sampling=True); sampling_rows([0.0, "
        "0.0]); DecodeSession.begin(i64[2], seeds=[976413892, 976413893]); DecodeSession.step([24, 8], [4]); DecodeSession.step([22, 7], [5]); "
        "sk_poll_async(cpu); synchronize(); sk_check_polled(cpu); DecodeSession.check()"),
    "sample_seed_int": (
        [[1, 2, 3, 4, 25, 26, 31, 16], [5, 6, 7, 9, 9, 11, 19, 13]],
        "new_cache(2, 8); forward(i64[2,4], at=0, use_cache=True); sampling_rows(0.8, 4, 1.0, [5, 6], device=cpu); argmax(f32[2,32], "
        "sampling=i32[2,6], ctr_add=4); DecodeSession(2, use_graph=True, sampling=True); sampling_rows([0.0, 0.0]); DecodeSession.begin(i64[2],"
        " seeds=[5, 6]); DecodeSession.step([25, 9], [4]); DecodeSession.step([26, 11], [5]); DecodeSession.step([31, 19], [6]); "
        "sk_poll_async(cpu); synchronize(); sk_check_polled(cpu); DecodeSession.check()"),
    "sample_seed_list": (
        [[1, 2, 3, 4, 29, 10, 19, 16], [5, 6, 7, 9, 5, 27, 31, 13]],
        "new_cache(2, 8); forward(i64[2,4], at=0, use_cache=True); sampling_rows(1.0, 0, 0.9, [9, 2], device=cpu); argmax(f32[2,32], "
        "sampling=i32[2,6], ctr_add=4); forward(i64[2,1], at=4, use_cache=True); argmax(f32[2,32], sampling=i32[2,6], ctr_add=5); "
        "forward(i64[2,1], at=5, use_cache=True); argmax(f32[2,32], sampling=i32[2,6], ctr_add=6); forward(i64[2,1], at=6, use_cache=True); "
        "argmax(f32[2,32], sampling=i32[2,6], ctr_add=7); sk_poll_async(cpu); synchronize(); sk_check_polled(cpu)"),
    "sample_seed_wrong_length": (
        'generate: 3 seeds for 2 rows',
        "new_cache(2, 8); forward(i64[2,4], at=0, use_cache=True)"),
    "spec_criterion_inside_a_list": (
        [[1, 2, 3, 4, 16, 21, 5, 22, 10]],
        "spec.refuse_engine(); new_cache(1, 12); forward(i64[1,4], at=0, use_cache=True); argmax(f32[1,32]); crit_bool(i64[1,5], -); "
        "crit_rows(i64[1,5], -); SpecDecodeSession(3, 2, use_graph=False, sampling=False); SpecDecodeSession.begin([16], prompt_ids=[1, 2, 3, "
        "4]); SpecDecodeSession.step(16, 4, emits=4); crit_bool(i64[1,6], -); crit_rows(i64[1,6], -); crit_bool(i64[1,7], -); "
        "crit_rows(i64[1,7], -); crit_bool(i64[1,8], -); crit_rows(i64[1,8], -); crit_bool(i64[1,9], -); sk_poll_async(cpu); synchronize(); "
        "sk_check_polled(cpu); SpecDecodeSession.check()"),
    "spec_max_new_tokens_cut": (
        {'sequences': [[1, 2, 3, 4, 16, 21, 5, 22, 10, 7]], 'sequences_scores': None, 'speculation': {'steps': 2, 'drafted': 6, 'accepted': 4}},
        "spec.refuse_engine(); new_cache(1, 10); forward(i64[1,4], at=0, use_cache=True); argmax(f32[1,32]); SpecDecodeSession(3, 4, "
        "eos_ids=[40, 41], use_graph=True, sampling=False); SpecDecodeSession.begin([16], prompt_ids=[1, 2, 3, 4]); SpecDecodeSession.step(16, "
        "4, emits=2); SpecDecodeSession.step(5, 6, emits=4); sk_poll_async(cpu); synchronize(); sk_check_polled(cpu); SpecDecodeSession.check()"),
    "spec_never_made": (
        {'sequences': [[1, 2, 3, 4, 16, 21, 5]], 'sequences_scores': None, 'speculation': {'steps': 2, 'drafted': 0, 'accepted': 0}},
        "spec.refuse_engine(); new_cache(1, 7); forward(i64[1,4], at=0, use_cache=True); argmax(f32[1,32]); DecodeSession(1, use_graph=True); "
        "DecodeSession.begin(i64[1]); DecodeSession.step([16], [4]); DecodeSession.step([21], [5]); sk_poll_async(cpu); synchronize(); "
        "sk_check_polled(cpu); DecodeSession.check()"),
    "spec_seeded": (
        {'sequences': [[1, 2, 3, 4, 26, 30, 12, 24, 30, 18, 16, 12]],
         'sequences_scores': None,
         'speculation': {'steps': 6, 'drafted': 9, 'accepted': 1}},
        "spec.refuse_engine(); sampling_rows(0.8, 3, 1.0, [6]); new_cache(1, 11); forward(i64[1,4], at=0, use_cache=True); argmax(f32[1,32], "
        "sampling=i32[1,6], ctr_add=4); SpecDecodeSession(3, 2, use_graph=True, sampling=True); sampling_rows([0.0, 0.0, 0.0, 0.0]); "
        "SpecDecodeSession.begin([26], prompt_ids=[1, 2, 3, 4], seeds=[6, 6, 6, 6]); SpecDecodeSession.step(26, 4, emits=2); "
        "SpecDecodeSession.step(12, 6, emits=1); SpecDecodeSession.step(24, 7, emits=1); DecodeSession(1, use_graph=True, sampling=True); "
        "sampling_rows([0.0]); DecodeSession.begin(i64[1], seeds=[6]); DecodeSession.step([30], [8]); DecodeSession.step([18], [9]); "
        "DecodeSession.step([16], [10]); sk_poll_async(cpu); synchronize(); sk_check_polled(cpu); SpecDecodeSession.check(); "
        "DecodeSession.check()"),
    "spec_stop_inside_a_list": (
        {'sequences': [[1, 2, 3, 4, 16, 21, 5]], 'sequences_scores': None, 'speculation': {'steps': 1, 'drafted': 3, 'accepted': 2}},
        "spec.refuse_engine(); new_cache(1, 12); forward(i64[1,4], at=0, use_cache=True); argmax(f32[1,32]); SpecDecodeSession(3, 2, "
        "eos_ids=[5], use_graph=True, sampling=False); SpecDecodeSession.begin([16], prompt_ids=[1, 2, 3, 4]); SpecDecodeSession.step(16, 4, "
        "emits=3); sk_poll_async(cpu); synchronize(); sk_check_polled(cpu); SpecDecodeSession.check()"),
    "spec_tail_session": (
        {'sequences': [[1, 2, 3, 4, 16, 21, 5, 22, 10, 7, 31]], 'sequences_scores': None, 'speculation': {'steps': 4, 'drafted': 6, 'accepted': 2}},
        "spec.refuse_engine(); new_cache(1, 10); forward(i64[1,4], at=0, use_cache=True); argmax(f32[1,32]); SpecDecodeSession(3, 2, "
        "use_graph=True, sampling=False); SpecDecodeSession.begin([16], prompt_ids=[1, 2, 3, 4]); SpecDecodeSession.step(16, 4, emits=2); "
        "SpecDecodeSession.step(5, 6, emits=2); DecodeSession(1, use_graph=True); DecodeSession.begin(i64[1]); DecodeSession.step([10], [8]); "
        "DecodeSession.step([7], [9]); sk_poll_async(cpu); synchronize(); sk_check_polled(cpu); SpecDecodeSession.check(); "
        "DecodeSession.check()"),
    "spec_tensor": (
        [[1, 2, 3, 4, 16, 21, 5]],
        "spec.refuse_engine(); new_cache(1, 7); forward(i64[1,4], at=0, use_cache=True); argmax(f32[1,32]); SpecDecodeSession(2, 2, "
        "use_graph=True, sampling=False); SpecDecodeSession.begin([16], prompt_ids=[1, 2, 3, 4]); SpecDecodeSession.step(16, 4, emits=3); "
        "sk_poll_async(cpu); synchronize(); sk_check_polled(cpu); SpecDecodeSession.check()"),
}


@pytest.mark.parametrize("name", sorted(CASES))
def test_generation_is_the_recorded_one(name):
    result = CASES[name]()
    want = EXPECTED[name]
    assert result == want[0]
    assert TRACE == [e for e in want[1].split("; ") if e]


def test_lookup_argument_messages_are_shared():
    """generate and the batcher refuse the two lookup arguments with the same words"""
    m = make_model()
    for kw, msg in ((dict(prompt_lookup_num_tokens=8), r"prompt_lookup_num_tokens must be an int in \[1, 7\], got 8"),
                    (dict(prompt_lookup_num_tokens=True), r"prompt_lookup_num_tokens must be an int in \[1, 7\], got True"),
                    (dict(prompt_lookup_num_tokens=2, max_matching_ngram_size=9), r"max_matching_ngram_size must be an int in \[1, 8\], got 9"),
                    (dict(max_matching_ngram_size=2), "max_matching_ngram_size needs prompt_lookup_num_tokens")):
        with pytest.raises(ValueError, match=msg):
            m.generate(ONE, **kw)
        with pytest.raises(ValueError, match=msg):
            serving.ContinuousBatcher(m, **kw)
    assert TRACE == []                                           # before the model, a cache or a session is touched
