"""hipGraph-captured autoregressive decode step (BASELINE.json configs[4]; the loop of
valley/serve/model_worker.py:380-394 and of HF ``generate`` behind valley_model.py:432).

One decode step = embedding gather of the current token -> L x [RMSNorm + q|k|v GEMV, RoPE + KV append +
decode attention (every head split over four workgroups at batch <= 2), (merge +) o GEMV(+res), RMSNorm + gate/up GEMV with SwiGLU, down GEMV(+res)] -> RMSNorm +
lm_head GEMV -> argmax (or a seeded draw) -> position += 1.  Every kernel is HBM-bound weight/KV streaming, 5 launches
per layer (the norms ride inside the GEMV that consumes them at batch <= 2; 7 otherwise): launched eagerly from Python the step would be host-bound (>300 launches x ~15 us), so the
step is captured ONCE into a hipGraph and replayed.  Static shapes are what capture needs: the KV
cache is pre-allocated to ctx_max, and the only thing that changes between replays — the position —
lives on the device (``pos``) and is read by vly_rope_kv / vly_llama_attention through their
``past_len_dev`` argument."""
from __future__ import annotations

import os
from typing import Optional, Sequence

import torch

from . import ops
from . import runtime
from .llama import HipKVCache, HipLlama


FUSE_NORM = os.environ.get("VALLEY_DECODE_FUSE_NORM", "1") != "0"
SPLIT_ATTN = os.environ.get("VALLEY_DECODE_SPLIT_ATTN", "1") != "0"       # flash-decoding split + merge inside the o GEMV (B <= 2)
# round 4: every decoder layer of the step in ONE persistent launch (vly_decode_layers: grid barriers between the five phases of a
# layer, the next phase's first weight units requested before the barrier; BIT-identical to the five launches per layer,
# tests/test_decode_persistent_gpu.py).  Measured (13B, 256 tokens, same box, profiles/r04): 198.7 tokens/s against the launches'
# 208-209 — its weight loops stream at 6.9-7 TB/s, but a phase boundary inside the launch (arrival skew 3.5-8 us + barrier 1.5-2 us +
# activation hand-off and norm 1.4-2.8 us) costs no less than a kernel boundary (1.3 us + ramp), and requests issued before the
# barrier land before it ends (DESIGN.md "decode: the persistent step").  Kept as an option: VALLEY_DECODE_PERSISTENT=1.
PERSISTENT = os.environ.get("VALLEY_DECODE_PERSISTENT", "0") != "0"
# round 4: where the split attention's partials are merged — "attn": by the last workgroup of a head inside the attention launch
# (vly_decode_attention_merged; the o projection is then a plain GEMV), "oproj": in the o GEMV's prologue (round 3).  Same bits.
# ("oproj" and the persistent step need the experimental library: VALLEY_EXPERIMENTAL=1, include/valley_hip.h's EXPERIMENTAL prototypes)
MERGE_IN = os.environ.get("VALLEY_DECODE_MERGE", "attn")
SPLIT_ROWS = os.environ.get("VALLEY_DECODE_SPLIT_ROWS", "1") != "0"       # round 5: the merged split attention for 3 .. 8 rows as well


def _norm_gemv(sess, gamma, w16, wq, out, epilogue=ops.EPI_NONE):
    """RMSNorm + projection of a step's ``sess.M`` rows of ``sess.h`` — THE norm -> projection dispatch of DecodeSession and of the
    verify steps (spec.py): one launch where the fused kernel takes the shape (bit-identical either way; VALLEY_DECODE_FUSE_NORM=0
    keeps the pairs, for A/B runs), the int8 / int4 forms where the engine is quantized and the seam has a quantized weight ``wq``
    (the lm_head has none)."""
    ll, M = sess.ll, sess.M
    fused = FUSE_NORM and ops.gemv_rmsnorm_ok(M, ll.H)
    if sess.wq and wq is not None:
        if fused and sess.q_gemv_rmsnorm_ok(M, ll.H):
            sess.q_gemv_rmsnorm(sess.h, gamma, ll.eps, *wq, epilogue=epilogue, out=out)
        else:
            ops.rmsnorm(sess.h, gamma, ll.eps, out=sess.x)
            sess.q_gemv(sess.x, *wq, epilogue=epilogue, out=out)
    elif fused:
        ops.gemv_rmsnorm(sess.h, gamma, ll.eps, w16, epilogue=epilogue, out=out)
    else:
        ops.rmsnorm(sess.h, gamma, ll.eps, out=sess.x)
        ops.gemv(sess.x, w16, epilogue=epilogue, out=out)


def _gemv_residual(sess, a, L, name):
    """h += a @ W^T for the layer's ``o`` or ``down`` projection, over the engine's weight format."""
    if sess.wq:
        sess.q_gemv(a, *L["wq_" + name], residual=sess.h, out=sess.h)
    else:
        ops.gemv(a, L["w_" + name], residual=sess.h, out=sess.h)


class DecodeSession:
    def __init__(self, llama: HipLlama, cache: HipKVCache, use_graph: bool = True, per_row_positions: bool = False,
                 sampling: bool = False, beams: Optional[tuple] = None, processors: bool = False,
                 processor_eos: Optional[Sequence[int]] = None, logprobs: Optional[int] = None, constraints=None,
                 guidance: bool = False, stop=None, stop_eos: Optional[Sequence[int]] = None):
        """``per_row_positions``: every batch row is an independent sequence at its own position (``pos`` is int32 [B]
        and advances by one per step for every row) — the captured step of valley_amd.serving.ContinuousBatcher.
        ``sampling``: the step draws each row's next token with that row's parameters in ``self.sample`` (int32 [B, 6],
        ops.sampling_rows; all rows greedy until written) instead of taking the argmax.  The draw counter is the index of
        the drawn token in the row's sequence (``pos + 1``), and ``self.sample`` is read at every replay: writing it
        between steps changes the parameters without a re-capture.
        ``beams = (B, nb, S, eos_ids[, tail])``: beam search over the cache's B * nb rows (prompt b in rows b * nb ..), whose
        shared prompt positions are [0, S).  Where the argmax ran, the step runs ops.beam_candidates over the running
        scores in ``self.running`` (into ``self.cand``: score, token, parent row, hit — K per prompt) and then, with
        ``tail`` (default True: the hits are the EOS ids), the rest of the step: ops.beam_select into ``self.tok`` /
        ``self.parent`` / ``self.running``, ops.kv_beam_reorder of the generated positions [S, pos + 1) and pos += 1.
        Without ``tail`` the caller writes its own hit mask into ``self.cand[3]`` and calls ``beam_tail()`` after each step.
        ``processors``: HF's repetition penalty, no-repeat n-grams and minimum length run on the step's logits before the
        argmax / draw (ops.logits_process), with each row's parameters in ``self.proc`` (int32 [B, 4], ops.processor_rows;
        all rows neutral until written) over the token history ``self.hist`` (int32 [B, ctx_max]: the prompt ids, written by
        ``begin(prompt_ids=...)`` or by the caller per slot, then every token fed to a step, appended on the device).  The
        EOS ids of the minimum length are ``processor_eos`` (default: a beam session's EOS ids).  With beams the step runs
        the history gather (rows follow their parents over [S, pos)), the processors on log_softmax(logits) and the
        candidates over those scores (ops.logits_beam_candidates) instead of ops.beam_candidates.
        ``logprobs = n`` (0 <= n <= 20): the step records log_softmax(raw logits)[chosen token] of every row in
        ``self.lp_table`` (fp32 [B, ctx_max + 1], column = the token's index in the row's sequence, ``pos + 1``: the step
        at the cache's last position chooses the token of index ctx_max) and, for n > 0, the n most probable ids and their
        log-probabilities in ``self.lp_top_tables`` (int32 / fp32 [B, ctx_max + 1, n]):
        ops.token_logprobs right behind the lm_head, ops.score_record behind the argmax / draw.  The processors and the
        sampler rewrite the logits in place before the token is known, so with either the raw row is copied aside
        (``self.lp_raw``).  A token the caller picks itself (host sampling) is recorded by ``record_token()``.
        ``constraints`` (an ops.ConstraintTables): the token constraints — bad words, suppressed and begin-suppressed ids, the
        forced EOS, allowed-sequence tries — run right behind the processors' launch (ops.constrain), before the argmax /
        draw / beam candidates, with each row's parameters in ``self.con`` (int32 [B, 4], ops.constraint_rows; all rows
        neutral until written).  It implies ``processors`` (that launch appends the fed token to the history the constraints
        read; its rows stay neutral unless written).  Rows, table contents and counts are read at every replay.
        ``guidance`` (per-row sessions only; not with beams or logprobs): classifier-free guidance over pairs of rows, each
        pair's roles, scale and plausibility cut-off in ``self.guide`` (int32 [B, 4], ops.guidance_rows; all rows neutral until
        written, read at every replay).  Right behind the lm_head a conditional row's logits are combined with its
        unconditional partner's (ops.guide: HF puts this processor first), then the processors, the constraints and the
        argmax / draw run as ever, and the unconditional row takes its conditional row's token (ops.guide_follow) before
        pos += 1: both rows of a pair are fed the same token at the next step.
        ``stop`` (an ops.StopTables; not with beams or guidance): the end of a row's generation is decided inside the step, right
        behind the argmax / draw (ops.stop): a watched row finishes when the chosen token is one of ``stop_eos`` or HF's
        stop-string test fires on the row's last tokens in ``self.hist`` followed by it, and a finished row's tokens become its
        pad id.  Each row's flags, first matchable index and pad id are in ``self.stop_rows`` (int32 [B, 4], ops.stop_rows; no row
        is watched until written), the verdicts in ``self.stop_state`` (int32 [B, 2] = {finished, index of the finishing token};
        the caller clears a row with ops.stop_state's values).  It implies ``processors`` (that launch appends the fed token to the
        history; its rows stay neutral unless written).  Rows, state, tables and EOS ids are read at every replay, so the host
        may replay several steps and read ``self.stop_state`` once."""
        if stop is not None and (beams is not None or guidance):
            raise ValueError("DecodeSession(stop=) takes no beams and no guidance")
        self.ll, self.cache = llama, cache
        B, d = cache.batch, llama.device
        if B > 8:
            raise ValueError("decode sessions stream weights with the GEMV kernel: batch <= 8")
        self.B = self.M = B                                      # M: the step's rows (_norm_gemv)
        if logprobs is not None:
            if beams is not None:
                raise ValueError("beam sessions take no logprobs: beam search reports sequences_scores")
            if PERSISTENT:
                raise ValueError("the persistent decode step (VALLEY_DECODE_PERSISTENT=1) takes no logprobs: unset it")
            if not 0 <= int(logprobs) <= ops.SCORE_MAX_TOP:
                raise ValueError(f"logprobs must be in [0, {ops.SCORE_MAX_TOP}] (the number of alternatives per token), got {logprobs!r}")
        mode = getattr(llama, "weight_quant", None)
        self.wq = bool(mode)                                     # the four projections of every layer stream int8 / int4 weights
        # the mode's GEMVs (int8: ops.wq_*, int4: ops.w4_*), with one signature
        self.q_gemv, self.q_gemv_rmsnorm, self.q_gemv_rmsnorm_ok = ops.quant_ops(mode)[1:] if mode else (None, None, None)
        if self.wq and (PERSISTENT or MERGE_IN == "oproj"):
            raise ValueError(f"an {mode}-quantized engine decodes with the per-layer launches only: unset VALLEY_DECODE_PERSISTENT and "
                             "VALLEY_DECODE_MERGE=oproj (those forms read 16-bit weights)")
        self.per_row = per_row_positions
        self.tok = torch.zeros((B,), dtype=torch.int32, device=d)          # token fed to the next step
        self.pos = torch.zeros((B if per_row_positions else 1,), dtype=torch.int32, device=d)   # on the device: replays need no patching
        self.sample = ops.sampling_rows([0.0] * B, device=d) if sampling else None
        self.h = torch.empty((B, llama.H), dtype=torch.float32, device=d)
        bf = runtime.HALF
        self.x = torch.empty((B, llama.H), dtype=bf, device=d)
        self.qkv = torch.empty((B, 3 * llama.H), dtype=bf, device=d)
        self.att = torch.empty((B, llama.H), dtype=bf, device=d)
        self.partials = ops.decode_partials(B, llama.heads, d)
        self.arrivals = torch.zeros((B * llama.heads,), dtype=torch.int32, device=d)     # tickets of vly_decode_attention_merged
        self.mlp = torch.empty((B, llama.I), dtype=bf, device=d)
        self.logits = torch.empty((B, llama.Vpad), dtype=torch.float32, device=d)
        # the persistent form takes the whole GPU (one workgroup per CU, all resident): shapes it supports, and only with the
        # fused norm / split attention arithmetic it reproduces
        self.persistent = (PERSISTENT and FUSE_NORM and SPLIT_ATTN and llama.heads * 128 == llama.H
                           and ops.decode_layers_ok(B, llama.H, llama.heads, llama.I))
        if self.persistent:
            self.mlp32 = torch.empty((B, llama.I), dtype=torch.float32, device=d)
            self.sync = torch.zeros((ops.DECODE_SYNC_WORDS,), dtype=torch.int32, device=d)
            self.table = None
            self._table_gen = None
        self.beams = None
        if beams is not None:
            if per_row_positions or sampling:
                raise ValueError("beam sessions share one position and select deterministically")
            bB, nb, S, eos = beams[:4]
            if bB * nb != B:
                raise ValueError(f"beam session: {bB} prompts x {nb} beams != {B} cache rows")
            self.beams = (bB, nb, int(S), ops.beam_k(nb, len(eos or ())), len(beams) < 5 or bool(beams[4]))
            K = self.beams[3]
            self.eos = torch.tensor(list(eos), dtype=torch.int32, device=d) if eos else None
            self.bscratch = ops.beam_scratch(bB, nb, K, d)
            self.cand = (torch.zeros((bB * K,), dtype=torch.float32, device=d), torch.zeros((bB * K,), dtype=torch.int32, device=d),
                         torch.zeros((bB * K,), dtype=torch.int32, device=d), torch.zeros((bB * K,), dtype=torch.uint8, device=d))
            self.parent = torch.arange(B, dtype=torch.int32, device=d)
            self.running = torch.zeros((B,), dtype=torch.float32, device=d)
            self.kv_table = None
            self._kv_table_gen = None
        self.guide = None
        if guidance:
            if not per_row_positions:
                raise ValueError("DecodeSession(guidance=True) needs per_row_positions=True (the two rows of a pair are sequences "
                                 "of their own lengths)")
            if beams is not None or logprobs is not None:
                raise ValueError("DecodeSession(guidance=True) takes no beams and no logprobs")
            self.guide = ops.guidance_rows(B, device=d)
        self.stop_tables, self.stop_rows, self.stop_state, self.stop_eos = stop, None, None, None
        if stop is not None:
            processors = True
            self.stop_rows = ops.stop_rows(B, watch=False, device=d)
            self.stop_state = ops.stop_state(B, device=d)
            if stop_eos:
                self.stop_eos = torch.tensor([int(e) for e in stop_eos], dtype=torch.int32, device=d)
        self.proc = self.hist = self.proc_eos = None
        self.con, self.con_tables = None, constraints
        if constraints is not None:
            processors = True
            self.con = ops.constraint_rows(constraints, B, flags=0, device=d)
        if processors:
            self.proc = ops.processor_rows([None] * B, device=d)
            self.hist = torch.zeros((B, cache.ctx_max), dtype=torch.int32, device=d)
            if processor_eos is None and beams is not None:
                processor_eos = beams[3]
            if processor_eos:
                self.proc_eos = torch.tensor([int(e) for e in processor_eos], dtype=torch.int32, device=d)
        self.lp_n = None
        if logprobs is not None:
            self.lp_n = n = int(logprobs)
            self.lp_lse = torch.zeros((B,), dtype=torch.float32, device=d)
            self.lp_table = torch.zeros((B, cache.ctx_max + 1), dtype=torch.float32, device=d)
            self.lp_top = self.lp_top_tables = None
            if n:
                self.lp_top = (torch.full((B, n), -1, dtype=torch.int32, device=d), torch.zeros((B, n), dtype=torch.float32, device=d))
                self.lp_top_tables = (torch.full((B, cache.ctx_max + 1, n), -1, dtype=torch.int32, device=d),
                                      torch.zeros((B, cache.ctx_max + 1, n), dtype=torch.float32, device=d))
            # in place before the token is picked: the processors' rescaling and bans, the sampler's temperature and filters
            self.lp_raw = torch.empty((B, llama.V), dtype=torch.float32, device=d) if (processors or sampling) else None
        self.use_graph = use_graph
        self.graph: Optional[torch.cuda.CUDAGraph] = None
        self._gen = cache.generation

    def _enqueue_step(self):
        ll, c = self.ll, self.cache
        B = self.B
        # every head over four workgroups.  Merged inside the attention launch (the default) it does not depend on the o GEMV's form, so
        # three to eight rows take it too: at eight requests decode_fused_kernel's 320 workgroups of 512 threads are 1.25 rounds of one
        # workgroup per CU (23 us per layer, 15 % of the step); 1280 quarter-head workgroups stream the same K / V evenly
        # (VALLEY_DECODE_SPLIT_ROWS=0: the one-workgroup-per-head kernel for more than two rows, A/B runs)
        split = SPLIT_ATTN and ll.heads * 128 == ll.H and (ops.gemv_rmsnorm_ok(B, ll.H) or (SPLIT_ROWS and MERGE_IN == "attn"))
        ops.embed_splice(self.tok, ll.embed, None, out=self.h)
        if self.persistent:
            if self.table is None or self._table_gen != c.generation:      # raw pointers: the cache's storage may have moved
                self.table = ops.decode_layer_table(ll.layers, c.k, c.v, ll.device)
                self._table_gen = c.generation
            ops.decode_layers(self.table, self.h, self.qkv, self.partials, self.mlp32, ll.cos, ll.sin, c.key_valid, self.pos,
                              self.per_row, ll.heads, ll.I, ll.eps, c.ctx_max, self.sync)
        for li in range(0 if self.persistent else ll.L):
            L = ll.layers[li]
            _norm_gemv(self, L["ln1"], L.get("w_qkv"), L.get("wq_qkv"), self.qkv)      # input_layernorm (inside) the q|k|v GEMV
            if split:                                            # every head over four workgroups; the o GEMV merges
                if MERGE_IN == "attn":
                    ops.decode_attention_split(self.qkv, c.k[li], c.v[li], ll.cos, ll.sin, c.key_valid, B, ll.heads, 0, self.partials,
                                               past_dev=self.pos, per_row=self.per_row, out=self.att, arrivals=self.arrivals)
                    _gemv_residual(self, self.att, L, "o")
                else:
                    ops.decode_attention_split(self.qkv, c.k[li], c.v[li], ll.cos, ll.sin, c.key_valid, B, ll.heads, 0,
                                               self.partials, past_dev=self.pos, per_row=self.per_row)
                    ops.gemv_attnmerge(self.partials, L["w_o"], residual=self.h, out=self.h)
            elif self.per_row:
                ops.decode_attention_rows(self.qkv, c.k[li], c.v[li], ll.cos, ll.sin, c.key_valid, B, ll.heads, self.pos, out=self.att)
            else:
                ops.decode_attention(self.qkv, c.k[li], c.v[li], ll.cos, ll.sin, c.key_valid, B, ll.heads, 0, out=self.att,
                                     past_dev=self.pos)          # RoPE + KV append + attention in one launch
            if not split:
                _gemv_residual(self, self.att, L, "o")
            _norm_gemv(self, L["ln2"], L.get("w_gu"), L.get("wq_gu"), self.mlp, epilogue=ops.EPI_SWIGLU)
            _gemv_residual(self, self.mlp, L, "down")
        _norm_gemv(self, ll.norm, ll.lm_head, None, self.logits)
        # greedy (or sampled) next token straight into the input slot of the next step (the V-padding columns of the
        # lm_head buffer are excluded through the row stride)
        if self.beams is not None:
            bB, nb, S, K, tail = self.beams
            if self.proc is None:
                ops.beam_candidates(self.logits[:, :ll.V], self.running, bB, nb, K, self.eos, self.bscratch, out=self.cand)
            else:                                    # the history follows the last selection, then HF's processors on log-probs
                ops.logits_history_gather(self.hist, self.parent, S, 0, len_dev=self.pos)
                ops.logits_process(self.logits[:, :ll.V], self.proc, self.hist, self.pos, 1, tok=self.tok, eos=self.proc_eos,
                                   log_softmax=True)
                if self.con is not None:
                    ops.constrain(self.logits[:, :ll.V], self.con, self.con_tables, self.hist, self.pos, 1)
                ops.logits_beam_candidates(self.logits[:, :ll.V], self.running, bB, nb, K, self.eos, self.bscratch,
                                           out=self.cand)
            if tail:
                self.beam_tail()
            return
        if self.guide is not None:                   # first, as in HF: every processor behind sees the guided scores
            ops.guide(self.logits[:, :ll.V], self.guide)
        if self.lp_n is not None:                    # lse (and the top-n) of the raw logits, before anything rewrites them
            ops.token_logprobs(self.logits[:, :ll.V], top=self.lp_n, out_lse=self.lp_lse, copy=self.lp_raw, out_top=self.lp_top)
        if self.proc is not None:                    # the token fed to this step joins the history at index pos
            ops.logits_process(self.logits[:, :ll.V], self.proc, self.hist, self.pos, 1, tok=self.tok, eos=self.proc_eos)
        if self.con is not None:                     # behind the append: the constraints read the history up to the fed token
            ops.constrain(self.logits[:, :ll.V], self.con, self.con_tables, self.hist, self.pos, 1)
        if self.sample is None:
            ops.argmax(self.logits[:, :ll.V], out=self.tok)
        else:
            ops.argmax(self.logits[:, :ll.V], sampling=self.sample, ctr=self.pos, ctr_add=1, out=self.tok)
        if self.lp_n is not None:                    # the token just chosen has index pos + 1 in its row's sequence
            self._record(1)
        if self.stop_tables is not None:             # the history holds the row up to the fed token, index pos; tok is index pos + 1
            ops.stop(self.tok, self.stop_rows, self.stop_state, self.stop_tables, self.hist, self.pos, 0, eos=self.stop_eos)
        if self.guide is not None:                   # the unconditional row is fed its conditional row's token
            ops.guide_follow(self.tok, self.guide)
        ops.incr_i32(self.pos, 1)

    def _record(self, len_add: int):
        ops.score_record(self.lp_raw if self.lp_raw is not None else self.logits[:, :self.ll.V], self.lp_lse, self.tok, self.lp_table,
                         self.pos, len_add, top=self.lp_top, top_tables=self.lp_top_tables)

    def record_token(self):
        """After ``step()``, for a caller that picked the token itself and wrote it into ``self.tok`` (host sampling): the
        step's column of ``self.lp_table`` is rewritten for that token (``pos`` has advanced: the column is ``pos``)."""
        if self.lp_n is None:
            raise ValueError("record_token() needs DecodeSession(..., logprobs=n)")
        self._record(0)

    def _ensure_kv_table(self):
        """The per-layer K / V pointer table of the reorder (raw pointers: rebuilt when the cache's storage moved)."""
        if self.kv_table is None or self._kv_table_gen != self.cache.generation:
            self.kv_table = ops.kv_beam_table(self.cache.k, self.cache.v, self.ll.device)
            self._kv_table_gen = self.cache.generation

    def beam_tail(self):
        """The rest of a beam step behind the candidates: running beams from ``self.cand`` (its hit mask included), the KV
        rows of the generated positions [S, pos + 1) follow their parents, pos += 1."""
        bB, nb, S, _K, _tail = self.beams
        ops.beam_select(*self.cand, bB, nb, tok=self.tok, parent=self.parent, running=self.running)
        ops.kv_beam_reorder(self.kv_table, self.cache.k[0], self.parent, S, 1, pos_dev=self.pos)
        ops.incr_i32(self.pos, 1)

    def _ensure_hist(self):
        """A processor session's history spans the cache's positions (it grows with a model-sized cache)."""
        if self.hist is not None and self.hist.shape[1] < self.cache.ctx_max:
            h = torch.zeros((self.B, self.cache.ctx_max), dtype=torch.int32, device=self.hist.device)
            h[:, :self.hist.shape[1]].copy_(self.hist)
            self.hist = h
            self._gen = None                                 # a graph holds the old history's pointer: capture again
        if self.lp_n is not None and self.lp_table.shape[1] < self.cache.ctx_max + 1:    # the log-probability tables likewise
            old = [self.lp_table] + list(self.lp_top_tables or ())
            new = [torch.full((self.B, self.cache.ctx_max + 1) + tuple(t.shape[2:]), -1 if t.dtype == torch.int32 else 0, dtype=t.dtype,
                              device=t.device) for t in old]
            for t, u in zip(old, new):
                u[:, :t.shape[1]].copy_(t)
            self.lp_table = new[0]
            if self.lp_top_tables is not None:
                self.lp_top_tables = (new[1], new[2])
            self._gen = None

    def begin(self, first_token: Optional[torch.Tensor] = None, prompt_ids: Optional[torch.Tensor] = None):
        """Call after the prefill filled ``cache``: sets the device position and the first input token (per-row sessions
        manage ``pos`` / ``tok`` per slot themselves and call this once, to capture).  ``prompt_ids`` [B, S]: the history
        of a processor session (per-row sessions write ``self.hist`` per slot)."""
        self._ensure_hist()
        if prompt_ids is not None:
            if self.hist is None:
                raise ValueError("begin(prompt_ids=...) needs DecodeSession(..., processors=True)")
            self.hist[:, :prompt_ids.shape[1]].copy_(prompt_ids.to(torch.int32))
        if not self.per_row:
            self.pos.fill_(self.cache.seq_len)
            self.tok.copy_(first_token.to(torch.int32).view(-1))
            if self.cache.key_valid is not None:
                self.cache.key_valid[:, self.cache.seq_len:] = 1       # generated positions are always attended
        if self.beams is not None:
            self._ensure_kv_table()
        if self.use_graph and (self.graph is None or self._gen != self.cache.generation):
            self._capture()

    def _capture(self):
        """Warm-up outside capture on a side stream (module loading, lazy init), then capture ONE step; the device-side
        position / token are restored, so capturing is invisible to the sequence.  Re-run whenever the cache's storage
        moved (HipKVCache.reserve grew it): the graph holds raw pointers."""
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        pos0, tok0 = self.pos.clone(), self.tok.clone()
        beam0 = None
        hist0 = None if self.hist is None else self.hist.clone()   # the warm-up step appends / gathers: restored
        stop0 = None if self.stop_state is None else self.stop_state.clone()   # ... and may finish a row: restored
        lp0 = None
        if self.lp_n is not None:                            # the warm-up step records a column: restored
            lp0 = [(t, t.clone()) for t in [self.lp_table] + list(self.lp_top_tables or ())]
        if self.beams is not None:                           # the warm-up step also moves the beams: restored with the rest
            beam0 = [self.parent.clone(), self.running.clone()] + [t.clone() for t in self.cand]
            S, hi = self.beams[2], self.cache.seq_len + 1
            kv0 = [(t[:, :, S:hi].clone(), u[:, :, S:hi].clone()) for t, u in zip(self.cache.k, self.cache.v)]
        with torch.cuda.stream(s):
            self._enqueue_step()
        torch.cuda.current_stream().wait_stream(s)
        torch.cuda.synchronize()
        self.pos.copy_(pos0)
        self.tok.copy_(tok0)
        if hist0 is not None:
            self.hist.copy_(hist0)
        if stop0 is not None:
            self.stop_state.copy_(stop0)
        for t, t0 in lp0 or ():
            t.copy_(t0)
        if beam0 is not None:
            for t, t0 in zip([self.parent, self.running] + list(self.cand), beam0):
                t.copy_(t0)
            for (t, u), (t0, u0) in zip(zip(self.cache.k, self.cache.v), kv0):
                t[:, :, S:hi].copy_(t0)
                u[:, :, S:hi].copy_(u0)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            self._enqueue_step()
        self.graph = g
        self._gen = self.cache.generation

    def check(self) -> None:
        """Raise if a workgroup of the persistent launch gave up at a grid barrier in the last step (it needs every CU: a kernel
        of another stream was holding some), or if the merged attention's ticket counters are not back at zero (a launch that
        did not complete).  Costs a device-to-host copy: callers check once per generation, tests per step."""
        if int(self.arrivals.abs().sum().item()) != 0:
            self.arrivals.zero_()
            raise RuntimeError("vly_decode_attention_merged: ticket counters not at zero after a step (an attention launch did "
                               "not complete); the step's output is invalid")
        if self.persistent and int(self.sync[ops.DECODE_SYNC_ABORT].item()) != 0:
            self.sync.zero_()                                    # the barrier counters are inconsistent after an abort
            raise RuntimeError("vly_decode_layers: a grid barrier timed out (not every workgroup was resident); the step's "
                               "output is invalid — rerun with VALLEY_DECODE_PERSISTENT=0 or keep the GPU to this stream")

    def step(self) -> torch.Tensor:
        """Run one decode step; returns the (device) int32 [B] buffer holding the newly chosen token.
        ``self.logits[:, :V]`` holds that step's logits (for temperature sampling on the host side)."""
        if not self.per_row:
            try:
                self.cache.reserve(self.cache.seq_len + 1)           # grows a model-sized cache (new storage -> new graph)
            except ValueError:
                raise ValueError("KV cache full") from None
            if self.cache.key_valid is not None and self.cache.key_valid.shape[1] != self.cache.ctx_max:
                raise RuntimeError("key_valid out of step with the cache")
            if self.beams is not None:
                self._ensure_kv_table()
            self._ensure_hist()
            if self.graph is not None and self._gen != self.cache.generation:
                self._capture()
        if self.graph is not None:
            self.graph.replay()
        else:
            self._enqueue_step()
        self.cache.seq_len += 1
        return self.tok
