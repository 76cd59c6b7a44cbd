"""Prompt-lookup speculative decoding: one hipGraph-captured verify step for k drafted tokens of one sequence.

HF's ``generate(prompt_lookup_num_tokens=k)`` proposes, as the next k tokens, the continuation of the EARLIEST earlier
occurrence of the sequence's last n-gram, and checks them in ONE forward of k + 1 rows: row i holds the logits behind the
i-th drafted token, so the leading drafts that equal the argmax of the row before them are tokens greedy decoding would
have produced, and the argmax behind the last accepted draft is one more.  A step therefore emits 1 .. k + 1 tokens of
exactly the greedy sequence for one pass over the weights (the weight-streaming GEMVs take up to 8 rows at almost the cost
of one: DESIGN.md "speculative decoding").

Everything that changes between steps lives on the device — the position, the token history the lookup reads, the draft —
so the step (draft -> embedding -> L x [norm + q|k|v GEMV, RoPE + KV of the rows, split attention, o GEMV, norm + gate|up GEMV
with SwiGLU, down GEMV] -> norm + lm_head -> argmax -> acceptance) is captured once and replayed; the host reads one small
buffer per step (how many tokens, and which).

Under seeded sampling (``sampling=True``) "argmax" reads "draw": row i draws, with the counter of the position it would occupy,
the token plain seeded decoding draws there (a draw is a function of the logits, the seed and that counter), so the leading
drafts that equal the draws of the rows before them are tokens of exactly the seed's sequence (counters -> ops.argmax with
per-row counters in place of the plain argmax; DESIGN.md "seeded sampling").

``_VerifyStep`` is that step, written once: the buffers, the launch order, the capture and the check.  Its two subclasses say
where a row's position comes from.  ``SpecDecodeSession``: ONE sequence of k + 1 rows at one position (ops.spec_*,
libvalley_hip_spec.so), with the cache bookkeeping of ``generate()``.  ``SpecRowsSession``: B sequences x (k + 1) rows <= 8, one
position, history, draft and acceptance per sequence (ops.spec_rows_*, libvalley_hip_spec_rows.so) — the captured step of a
speculating ``ContinuousBatcher``.  The norm -> projection dispatch is DecodeSession's (decode._norm_gemv)."""
from __future__ import annotations

import os
from typing import List, Optional, Sequence

import torch

from . import decode as _decode
from . import ops
from . import runtime
from .decode import _gemv_residual, _norm_gemv
from .llama import HipKVCache, HipLlama


def refuse_engine() -> None:
    """The configurations a SpecDecodeSession does not run on, with the reason."""
    if runtime.PRECISION == "fp32":
        raise ValueError("speculative decoding needs a 16-bit engine: the fp32 engine (VALLEY_PRECISION=fp32) has no multi-row "
                         "weight-streaming step to verify a draft with")
    if _decode.PERSISTENT:
        raise ValueError("speculative decoding runs the per-layer launches: unset VALLEY_DECODE_PERSISTENT (the persistent step "
                         "is built for one query per sequence)")
    if _decode.MERGE_IN == "oproj":
        raise ValueError("speculative decoding merges the attention's splits inside the attention launch: unset "
                         "VALLEY_DECODE_MERGE=oproj")


def _refuse_draft(k, max_ngram) -> None:
    if not 1 <= int(k) <= ops.SPEC_MAX_DRAFT:
        raise ValueError(f"k (prompt_lookup_num_tokens) must be in [1, {ops.SPEC_MAX_DRAFT}], got {k!r}")
    if not 1 <= int(max_ngram) <= ops.SPEC_MAX_NGRAM:
        raise ValueError(f"max_ngram (max_matching_ngram_size) must be in [1, {ops.SPEC_MAX_NGRAM}], got {max_ngram!r}")


def _stats_dict(stats: torch.Tensor) -> dict:
    s = stats.tolist()
    return {"steps": s[0], "drafted": s[1], "accepted": s[2]}


class _VerifyStep:
    """The verify step of ``cache.batch`` = B sequences x S = k + 1 rows: every buffer, the one launch order, its capture and its
    check.  A subclass names its attention entry point (``ATTENTION``, for ``check``), refuses the geometries it does not take
    (``_refuse``) and issues the four launches that know where a row's position comes from: ``_draft``, ``_attention(li)`` (RoPE +
    KV append + attention of layer li), ``_counters`` and ``_accept``."""
    ATTENTION = None

    def __init__(self, llama: HipLlama, cache: HipKVCache, k: int, max_ngram: int, eos_ids: Optional[Sequence[int]], use_graph: bool,
                 lookup: bool, sampling: bool):
        refuse_engine()
        self._refuse(cache, k, max_ngram)
        if llama.heads * 128 != llama.H:
            raise ValueError("speculative decoding needs head_dim 128")
        self.ll, self.cache = llama, cache
        self.B, self.k, self.S, self.M = cache.batch, int(k), int(k) + 1, cache.batch * (int(k) + 1)
        self.max_ngram, self.lookup = int(max_ngram), bool(lookup)
        mode = getattr(llama, "weight_quant", None)
        self.wq = bool(mode)
        self.q_gemv, self.q_gemv_rmsnorm, self.q_gemv_rmsnorm_ok = ops.quant_ops(mode)[1:] if mode else (None, None, None)
        d, B, M, bf = llama.device, self.B, self.M, runtime.HALF
        self.pos = torch.zeros((B,), dtype=torch.int32, device=d)          # position of each sequence's tok row 0 = tokens in its cache
        self.hist = torch.full((B, cache.ctx_max), -1, dtype=torch.int32, device=d)  # hist[b, j]: the token at cache position j
        self.tok = torch.zeros((M,), dtype=torch.int32, device=d)          # per sequence: the last token, then the draft
        self.draft = torch.zeros((B, self.k), dtype=torch.int32, device=d)
        self.draft_len = torch.zeros((B,), dtype=torch.int32, device=d)
        self.emit = torch.zeros((B, self.k + 2), dtype=torch.int32, device=d)
        self.stats = torch.zeros((B, 3), dtype=torch.int32, device=d)      # per sequence: steps, drafted, accepted
        self.am = torch.zeros((M,), dtype=torch.int32, device=d)
        self.sample = ops.sampling_rows([0.0] * M, device=d) if sampling else None
        self.ctr = torch.zeros((M,), dtype=torch.int32, device=d) if sampling else None
        self.eos = torch.tensor([int(e) for e in eos_ids], dtype=torch.int32, device=d) if eos_ids else None
        self.h = torch.empty((M, llama.H), dtype=torch.float32, device=d)
        self.x = torch.empty((M, llama.H), dtype=bf, device=d)
        self.qkv = torch.empty((M, 3 * llama.H), dtype=bf, device=d)
        self.att = torch.empty((M, llama.H), dtype=bf, device=d)
        self.mlp = torch.empty((M, llama.I), dtype=bf, device=d)
        self.logits = torch.empty((M, llama.Vpad), dtype=torch.float32, device=d)
        self.scratch = ops.spec_scratch(B, self.S, llama.heads, d)
        self.use_graph = use_graph
        self.graph: Optional[torch.cuda.CUDAGraph] = None
        self._gen = cache.generation

    def _enqueue_step(self):
        ll = self.ll
        self._draft()
        ops.embed_splice(self.tok, ll.embed, None, out=self.h)
        for li in range(ll.L):
            L = ll.layers[li]
            _norm_gemv(self, L["ln1"], L.get("w_qkv"), L.get("wq_qkv"), self.qkv)
            # K / V of all k + 1 rows of a sequence go into the cache at positions pos .. pos + k before anything is accepted.  The
            # rows of rejected drafts then lie AT or BEHIND the new position: no later query sees them (a query at P reads keys <= P,
            # and every position <= P has been rewritten by the step that fed its accepted token), and the next step's RoPE + KV
            # launch overwrites them, starting at the new pos.
            self._attention(li)
            _gemv_residual(self, self.att, L, "o")
            _norm_gemv(self, L["ln2"], L.get("w_gu"), L.get("wq_gu"), self.mlp, epilogue=ops.EPI_SWIGLU)
            _gemv_residual(self, self.mlp, L, "down")
        _norm_gemv(self, ll.norm, ll.lm_head, None, self.logits)
        if self.sample is None:
            ops.argmax(self.logits[:, :ll.V], out=self.am)
        else:                                                # row j of a sequence: the draw of sequence index pos + j + 1
            self._counters()
            ops.argmax(self.logits[:, :ll.V], sampling=self.sample, ctr=self.ctr, ctr_add=1, out=self.am)
        self._accept()

    def _capture(self):
        """DecodeSession._capture's scheme: a warm-up step on a side stream, the device-side state restored, ONE step
        captured.  (The warm-up's K / V rows lie at and behind each sequence's position: the first real step overwrites them.)"""
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        state = [self.pos, self.tok, self.hist, self.stats, self.draft, self.draft_len, self.emit] + \
            ([self.ctr] if self.ctr is not None else [])
        saved = [t.clone() for t in state]
        with torch.cuda.stream(s):
            self._enqueue_step()
        torch.cuda.current_stream().wait_stream(s)
        torch.cuda.synchronize()
        for t, t0 in zip(state, saved):
            t.copy_(t0)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            self._enqueue_step()
        self.graph = g
        self._gen = self.cache.generation

    def check(self) -> None:
        """Raise if the split attention's ticket counters are not back at zero (a launch that did not complete)."""
        if int(self.scratch[1].abs().sum().item()) != 0:
            self.scratch[1].zero_()
            raise RuntimeError(f"{self.ATTENTION}: ticket counters not at zero after a step (an attention launch did not "
                               "complete); the step's output is invalid")


class SpecDecodeSession(_VerifyStep):
    ATTENTION = "vly_spec_attention"

    def __init__(self, llama: HipLlama, cache: HipKVCache, k: int, max_ngram: int = 2, eos_ids: Optional[Sequence[int]] = None,
                 use_graph: bool = True, lookup: bool = True, sampling: bool = False):
        """``k`` in [1, 7]: drafted tokens per step (HF's ``prompt_lookup_num_tokens``); ``max_ngram`` in [1, 8]: HF's
        ``max_matching_ngram_size``; ``eos_ids``: a draft stops in front of the first of them.  ``lookup=False``: the step
        does not search — the caller writes ``self.draft`` / ``self.draft_len`` before each ``step()`` (tests, and the
        cost measurement of a step that accepts nothing).  ``VALLEY_SPEC_ATTN=prefill`` (read here) routes the attention
        through ops.llama_attention(S = k + 1) instead of ops.spec_attention: the A/B arm and a second opinion.
        ``sampling``: the step DRAWS its k + 1 tokens instead of taking the argmax, with the parameters in ``self.sample`` (int32
        [k + 1, 6]: the sequence's ops.sampling_rows row, replicated by the caller; all rows greedy until written).  Row j draws
        with the counter of the token it would emit, ``pos + j + 1`` (``self.ctr``, written by ops.spec_counters inside the step),
        which is what DecodeSession(sampling=True) draws with at that position: the same seed gives the same sequence."""
        super().__init__(llama, cache, k, max_ngram, eos_ids, use_graph, lookup, sampling)
        self.attn = os.environ.get("VALLEY_SPEC_ATTN", "split")
        if self.attn not in ("split", "prefill"):
            raise ValueError(f"VALLEY_SPEC_ATTN must be 'split' or 'prefill', got {self.attn!r}")
        # one sequence: its tables are flat (hist [ctx_max], draft [k], emit [k + 2], stats [3])
        self.hist, self.draft, self.stats, self.emit = self.hist[0], self.draft[0], self.stats[0], self.emit[0].fill_(-1)

    def _refuse(self, cache, k, max_ngram):
        if cache.batch != 1:
            raise ValueError(f"a SpecDecodeSession decodes one sequence: cache.batch == 1 expected, got {cache.batch}")
        _refuse_draft(k, max_ngram)

    def _draft(self):
        ops.spec_draft(self.hist, self.pos, 1, self.k, self.max_ngram, self.draft, self.draft_len, self.tok, eos=self.eos,
                       vocab=self.ll.V, lookup=self.lookup)

    def _attention(self, li):
        ll, c, M = self.ll, self.cache, self.M
        ops.rope_kv(self.qkv, c.k[li], c.v[li], ll.cos, ll.sin, 1, M, ll.heads, 0, past_dev=self.pos)
        if self.attn == "prefill":
            ops.llama_attention(self.qkv, c.k[li], c.v[li], c.key_valid, 1, M, ll.heads, 0, out=self.att, past_dev=self.pos)
        else:
            ops.spec_attention(self.qkv, c.k[li], c.v[li], c.key_valid, 1, M, ll.heads, 0, self.scratch, out=self.att,
                               past_dev=self.pos)

    def _counters(self):
        ops.spec_counters(self.pos, self.k, self.cache.ctx_max, self.ctr)

    def _accept(self):
        ops.spec_accept(self.am, self.draft, self.draft_len, self.k, self.hist, self.pos, self.emit, self.tok, self.stats)

    def _ensure_hist(self):
        """The history spans the cache's positions (it grows with a model-sized cache)."""
        if self.hist.numel() < self.cache.ctx_max:
            h = torch.full((self.cache.ctx_max,), -1, dtype=torch.int32, device=self.hist.device)
            h[:self.hist.numel()].copy_(self.hist)
            self.hist = h
            self._gen = None                                 # a graph holds the old history's pointer: capture again

    def begin(self, first_token: torch.Tensor, prompt_ids: Optional[torch.Tensor] = None):
        """Call after the prefill filled ``cache``: the history is the prompt's ids (``prompt_ids`` [S] or [1, S]; right-aligned
        in front of the cache's position when the prefill spliced more positions than ids, the rest never matches) followed
        by ``first_token``, the position is the cache's, the counters are zero."""
        c = self.cache
        if self.room():
            c.reserve(c.seq_len + self.M)                    # a model-sized cache grows BEFORE the warm-up step writes its rows
        self._ensure_hist()
        self.hist.fill_(-1)
        if prompt_ids is not None:
            ids = prompt_ids.reshape(-1).to(torch.int32)[-c.seq_len:] if c.seq_len else prompt_ids.reshape(-1)[:0].to(torch.int32)
            self.hist[c.seq_len - ids.numel():c.seq_len].copy_(ids)
        self.hist[c.seq_len:c.seq_len + 1].copy_(first_token.reshape(-1)[:1].to(torch.int32))
        self.pos.fill_(c.seq_len)
        self.tok.fill_(0)
        self.tok[:1].copy_(first_token.reshape(-1)[:1].to(torch.int32))
        self.stats.zero_()
        if c.key_valid is not None:
            c.key_valid[:, c.seq_len:] = 1                   # generated positions are always attended
        # capturing runs a warm-up step, whose rope_kv writes k + 1 rows from the position on — and the kernels clamp the position
        # to ctx_max - (k + 1), so on a cache without that room the rows of REAL positions would be overwritten: no room, no
        # warm-up (step() captures once there is room, and raises before anything is launched when there never is)
        if self.use_graph and self.room() and (self.graph is None or self._gen != c.generation):
            self._capture()

    def room(self) -> bool:
        """Whether the cache has (or can grow to) the k + 1 positions a step writes."""
        c = self.cache
        return c.seq_len + self.M <= (c.limit if c.growable else c.ctx_max)

    def step(self) -> List[int]:
        """One verify step: returns the 1 .. k + 1 tokens it emitted (python ints, from one small device-to-host copy) and
        advances ``cache.seq_len`` by as many."""
        c = self.cache
        try:
            c.reserve(c.seq_len + self.M)                    # grows a model-sized cache (new storage -> new graph)
        except ValueError:
            raise ValueError(f"KV cache: fewer than k + 1 = {self.M} positions left ({c.ctx_max - c.seq_len}); decode the rest one "
                             "token at a time") from None
        if c.key_valid is not None and c.key_valid.shape[1] != c.ctx_max:
            raise RuntimeError("key_valid out of step with the cache")
        self._ensure_hist()
        if self.use_graph and (self.graph is None or self._gen != c.generation):
            self._capture()
        if self.use_graph:
            self.graph.replay()
        else:
            self._enqueue_step()
        emit = self.emit.tolist()                            # the step's one read: (n + 1, tokens, -1 ...)
        n1 = emit[0]
        if not 1 <= n1 <= self.M:
            raise RuntimeError(f"vly_spec_accept reported {n1} tokens for a step of {self.M} rows")
        c.seq_len += n1
        return emit[1:1 + n1]

    def speculation(self) -> dict:
        return _stats_dict(self.stats)


class SpecRowsSession(_VerifyStep):
    """The verify step for SEVERAL sequences: ``cache.batch`` = B sequences x (k + 1) rows <= 8 rows in one captured step, every
    sequence with its own position, history, draft and acceptance count (include/valley_hip_spec_rows.h) — the step of a
    speculating ``ContinuousBatcher``.

    A row whose position lies behind its sequence's cache is dead (it stores nothing), and a draft never sits on one, so the
    step runs at ANY position: a sequence near the end of its cache decodes its last tokens one per step inside the same graph.
    A sequence that is not live (``self.live[b] == 0``) rides along: its rows are computed and ignored, and its position,
    history and counters stay where they are."""
    ATTENTION = "vly_spec_rows_attention"

    def __init__(self, llama: HipLlama, cache: HipKVCache, k: int, max_ngram: int = 2, eos_ids: Optional[Sequence[int]] = None,
                 use_graph: bool = True, lookup: bool = True, sampling: bool = False):
        """Arguments as SpecDecodeSession's.  ``lookup=False``: the caller writes ``self.draft`` [B, k] / ``self.draft_len`` [B]
        before each ``step()``.  ``sampling``: row j of sequence b draws with ``self.sample[b * (k + 1) + j]`` (the sequence's
        ops.sampling_rows row, replicated over its k + 1 rows by ``set_sequence``) and the counter pos[b] + j + 1."""
        super().__init__(llama, cache, k, max_ngram, eos_ids, use_graph, lookup, sampling)
        self.live = torch.zeros((self.B,), dtype=torch.uint8, device=llama.device)

    def _refuse(self, cache, k, max_ngram):
        _refuse_draft(k, max_ngram)
        B = cache.batch
        if B * (int(k) + 1) > ops.SPEC_MAX_QUERIES:
            raise ValueError(f"a SpecRowsSession verifies sequences x (k + 1) <= {ops.SPEC_MAX_QUERIES} rows per step: "
                             f"{B} sequences x (k + 1 = {int(k) + 1}) = {B * (int(k) + 1)} rows")

    def _draft(self):
        ops.spec_rows_draft(self.hist, self.pos, 1, self.k, self.max_ngram, self.draft, self.draft_len, self.tok, live=self.live,
                            eos=self.eos, vocab=self.ll.V, lookup=self.lookup)

    def _attention(self, li):                                # dead rows (behind the cache's end) are not written at all
        ll, c, B, S = self.ll, self.cache, self.B, self.S
        ops.spec_rows_rope_kv(self.qkv, c.k[li], c.v[li], ll.cos, ll.sin, B, S, ll.heads, self.pos)
        ops.spec_rows_attention(self.qkv, c.k[li], c.v[li], c.key_valid, B, S, ll.heads, self.pos, self.scratch, out=self.att)

    def _counters(self):
        ops.spec_rows_counters(self.pos, self.k, self.cache.ctx_max, self.ctr)

    def _accept(self):
        ops.spec_rows_accept(self.am, self.draft, self.draft_len, self.k, self.hist, self.pos, self.emit, self.tok, self.stats,
                             live=self.live)

    def set_sequence(self, b: int, position: int, first_token: int, prompt_ids: Optional[torch.Tensor] = None, sampling_row=None):
        """Sequence ``b`` starts (after its prefill filled ``position`` rows of its cache): its history is ``prompt_ids`` —
        right-aligned in front of the position, as SpecDecodeSession.begin — followed by ``first_token``; its counters are zero,
        it is live.  ``sampling_row``: its ops.sampling_rows row (a sampling session), replicated over its k + 1 rows."""
        c, S = self.cache, self.S
        if not 0 <= b < self.B:
            raise ValueError(f"sequence {b} of {self.B}")
        if not 0 <= position < c.ctx_max:
            raise ValueError(f"position {position}: the first token's row must lie inside the cache's {c.ctx_max} positions")
        self.hist[b].fill_(-1)
        if prompt_ids is not None and position:
            ids = prompt_ids.reshape(-1).to(torch.int32)[-position:]
            self.hist[b, position - ids.numel():position].copy_(ids)
        self.hist[b, position] = int(first_token)
        self.pos[b] = position
        self.tok[b * S:(b + 1) * S] = 0
        self.tok[b * S] = int(first_token)
        self.stats[b].zero_()
        self.emit[b].zero_()
        if sampling_row is not None:
            if self.sample is None:
                raise ValueError("set_sequence(sampling_row=...) needs SpecRowsSession(..., sampling=True)")
            self.sample[b * S:(b + 1) * S].copy_(sampling_row.reshape(1, -1).expand(S, -1))
        self.live[b] = 1

    def release(self, b: int) -> None:
        """Sequence ``b`` leaves: its rows ride along unread, from position 0 (an idle sequence reads one key block per step)."""
        self.live[b] = 0
        self.pos[b] = 0

    def begin(self):
        """Capture the step (once, or again when the cache's storage moved).  Any position will do: dead rows store nothing."""
        if self.use_graph and (self.graph is None or self._gen != self.cache.generation):
            self._capture()

    def step(self) -> dict:
        """One verify step for every live sequence: ``{b: [tokens]}``, 1 .. k + 1 tokens each, from ONE device-to-host copy."""
        c = self.cache
        if c.key_valid is not None and c.key_valid.shape[1] != c.ctx_max:
            raise RuntimeError("key_valid out of step with the cache")
        if self.hist.shape[1] != c.ctx_max:
            raise RuntimeError("the cache's depth changed under a SpecRowsSession: make a new session")
        self.begin()
        if self.use_graph:
            self.graph.replay()
        else:
            self._enqueue_step()
        out = {}
        for b, row in enumerate(self.emit.tolist()):         # the step's one read: per sequence (n + 1, tokens, -1 ...)
            n1 = row[0]
            if n1 == 0:
                continue
            if not 1 <= n1 <= self.S:
                raise RuntimeError(f"vly_spec_rows_accept reported {n1} tokens for a sequence of {self.S} rows")
            out[b] = row[1:1 + n1]
        return out

    def speculation(self, b: int) -> dict:
        return _stats_dict(self.stats[b])
