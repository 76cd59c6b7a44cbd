"""The decode service loop of the reference worker (valley/serve/model_worker.py:321-426) on the HIP
path: prompt expansion with the clip's real frame count, prefill, per-token KV decode
with greedy / temperature sampling, stop-token and stop-string handling, and ``json\\0`` chunks every
``stream_interval`` tokens.  The HTTP fabric around it (FastAPI worker, controller, gradio) is out of
scope; this generator is what those routes would wrap.

Decode steps run through the hipGraph-captured ``DecodeSession``: the greedy token never leaves the
device between steps; with temperature sampling ``generate_video_stream`` samples the step's logits by
torch.multinomial (as in the reference) and writes the chosen token back into the session's input slot,
while a sampling ``ContinuousBatcher`` draws seeded tokens inside the captured step."""
from __future__ import annotations

import json
from typing import Iterator, Optional

import torch

from . import ops
from .decode import DecodeSession
from .generation import NO_TOKENIZER, eos_ids, guidance_scalars, lookup_args, negative_prompt, score_raw
from .valley_model import (DEFAULT_IM_END_TOKEN, DEFAULT_IM_START_TOKEN, DEFAULT_IMAGE_PATCH_TOKEN, DEFAULT_VI_END_TOKEN,
                           DEFAULT_VI_START_TOKEN, DEFAULT_VIDEO_FRAME_TOKEN, DEFAULT_VIDEO_TOKEN)


def expand_video_prompt(prompt: str, n_frames: int, use_im_start_end: bool = False) -> str:
    """model_worker.py:338-341."""
    replace_token = DEFAULT_IMAGE_PATCH_TOKEN * 256
    if use_im_start_end:
        replace_token = DEFAULT_IM_START_TOKEN + replace_token + DEFAULT_IM_END_TOKEN + DEFAULT_VI_START_TOKEN + \
            DEFAULT_VIDEO_FRAME_TOKEN * n_frames + DEFAULT_VI_END_TOKEN
    return prompt.replace(DEFAULT_VIDEO_TOKEN, replace_token)


def generate_video_stream(model, tokenizer, params: dict, video: Optional[torch.Tensor] = None, stream_interval: int = 2,
                          context_len: int = 2048, use_graph: bool = True, sampler=None) -> Iterator[bytes]:
    """``params``: prompt, temperature, max_new_tokens, stop (model_worker.py:323-358).  ``video``: preprocessed
    frames [3,T,224,224] (what ``load_video`` returns) or None.  ``sampler(probs) -> token`` replaces the default
    ``torch.multinomial(probs, 1)`` of the temperature branch (:393-394), e.g. to seed it."""
    prompt = params["prompt"]
    ori_prompt = prompt
    images = None
    if video is not None:
        assert prompt.count(DEFAULT_VIDEO_TOKEN) == 1, "Number of video does not match number of <video> tokens in prompt"
        frames = video.permute(1, 0, 2, 3)
        prompt = expand_video_prompt(prompt, frames.shape[0], getattr(model.config, "mm_use_im_start_end", False))
        images = frames.unsqueeze(0)
    temperature = float(params.get("temperature", 1.0))
    max_new_tokens = min(int(params.get("max_new_tokens", 256)), 1024)
    stop_str = params.get("stop", None)
    stop_idx = None
    if stop_str is not None:
        stop_idx = tokenizer(stop_str).input_ids
        stop_idx = stop_idx[0] if len(stop_idx) == 1 else None
    input_ids = tokenizer(prompt).input_ids
    max_src_len = context_len - max_new_tokens - 8
    input_ids = input_ids[-max_src_len:]
    pred_ids = []
    dev = model.device
    ll = model.get_model().llama
    cache = ll.new_cache(1, min(context_len, len(input_ids) + max_new_tokens + 1))
    sess = None
    ret = None
    for i in range(max_new_tokens):
        if i == 0:
            out = model(input_ids=torch.as_tensor([input_ids], device=dev), use_cache=True, images=images, past_key_values=cache)
            last = out.logits[0, -1]
        else:
            if sess is None:
                sess = DecodeSession(ll, cache, use_graph=use_graph)
                sess.begin(torch.as_tensor([token], device=dev))
            else:
                sess.tok.copy_(torch.as_tensor([token], device=dev, dtype=torch.int32))
            sess.step()
            last = sess.logits[0, :ll.V]
        if temperature < 1e-4:
            token = int(torch.argmax(last))
        else:
            probs = torch.softmax(last / temperature, dim=-1)
            token = int(torch.multinomial(probs, num_samples=1)) if sampler is None else int(sampler(probs))
        pred_ids.append(token)
        if stop_idx is not None and token == stop_idx:
            stopped = True
        elif token == getattr(tokenizer, "eos_token_id", None):
            stopped = True
        else:
            stopped = False
        if i % stream_interval == 0 or i == max_new_tokens - 1 or stopped:
            cur_out = tokenizer.decode(pred_ids, skip_special_tokens=True)
            pos = cur_out.rfind(stop_str) if stop_str is not None else -1
            if pos != -1:
                cur_out = cur_out[:pos]
                stopped = True
            ret = {"text": ori_prompt + cur_out, "error_code": 0}
            yield json.dumps(ret).encode() + b"\0"
        if stopped or cache.seq_len + 1 > cache.ctx_max:
            break
    if sess is not None:
        sess.check()                                         # the decode launches' ticket counters / abort word, once per request


class ContinuousBatcher:
    """Continuous batching over ONE hipGraph-captured decode step: up to ``slots`` (<= 8) requests
    share a KV cache [slots, heads, ctx_max, 128] and a captured step of batch ``slots``; a request joins at any step
    (its prompt is prefilled into its slot's cache rows by the ordinary MFMA prefill), leaves at any step, and the
    weight stream of every decode step — the whole cost of a step at these batch sizes (HBM-bound GEMV) — is shared by
    all live requests.  The reference's worker serialises requests behind a semaphore and runs the loop of
    model_worker.py:371-394 once per request; the per-request token sequence here is the same as that loop's.

    Every slot has its own position (device int32, advanced by the captured step) and its own key-validity row, so the
    slots are fully independent sequences: ``vly_decode_attention_rows``.  Idle slots run along (their rows are computed
    and ignored: the GEMV cost does not depend on the row count), clamped inside their cache rows."""

    def __init__(self, model, slots: int = 4, ctx_max: int = 1024, use_graph: bool = True, sampling: bool = False,
                 processors: bool = False, eos_token_id=None, logprobs: Optional[int] = None,
                 prompt_lookup_num_tokens: Optional[int] = None, max_matching_ngram_size: Optional[int] = None,
                 constraints: bool = False, bad_words_ids=None, suppress_tokens=None, begin_suppress_tokens=None,
                 trie_capacity: int = 4096, guidance: bool = False, stop_strings=None, tokenizer=None):
        """``sampling``: the captured step draws every slot's token with the parameters ``add`` gave its request
        (temperature, top-k, top-p, seed; DecodeSession ``sampling``) — a seeded request's tokens then depend on its seed
        alone, not on its slot or its neighbours.  Greedy requests take the argmax in either kind of batcher.
        ``processors``: the captured step runs HF's repetition penalty, no-repeat n-grams and minimum new tokens with the
        parameters ``add`` gave each request (DecodeSession ``processors``), over the slot's history (its prompt, then its
        tokens); ``eos_token_id`` (an int or a list) is what ``min_new_tokens`` keeps out.
        ``logprobs = n`` (0 <= n <= 20): every token's log_softmax(raw logits)[token] and the n most probable alternatives
        (DecodeSession ``logprobs``).  ``add`` leaves the first token's in ``self.first_logprobs[slot]``, ``step`` the step's
        in ``self.last_logprobs`` — ``{slot: (lp, top ids, top lps)}`` — and the slot's row of ``self.sess.lp_table``
        (column = the token's index in the request's sequence) keeps them all.  A request's values do not depend on its slot
        or its neighbours.
        ``prompt_lookup_num_tokens = k`` (1 <= k <= 7, slots x (k + 1) <= 8): prompt-lookup speculation for every slot in the one
        captured step (valley_amd.spec.SpecRowsSession) — each slot drafts up to k tokens from its own history (its prompt, then
        its tokens; ``max_matching_ngram_size``, default 2, in [1, 8]; a draft stops in front of ``eos_token_id``) and the step
        verifies all slots' k + 1 rows at once.  ``step()`` then returns ``{slot: [t0, ...]}``, 1 .. k + 1 tokens per live slot:
        exactly the tokens the plain batcher would have returned over as many steps (greedy, or the request's seed's under
        ``sampling=True``, where a sampling request must bring its ``seed``).  EOS, stop criteria and max_new_tokens stay the
        caller's business: the caller truncates a step's list at its own stop and releases the slot.  Not with ``processors``
        or ``logprobs``.  ``speculation(slot)`` reports the slot's {"steps", "drafted", "accepted"}.
        ``constraints``: the captured step runs the token constraints (DecodeSession ``constraints``; ops.constrain).
        ``bad_words_ids`` / ``suppress_tokens`` / ``begin_suppress_tokens`` are shared by all requests; ``add`` gives a request
        its own ``allowed_sequences`` — written into the slot's region of ``trie_capacity`` int32 words (2 per trie node + 2 per
        edge) between steps, without a re-capture — and its forced EOS.  ``eos_token_id`` is what ends an allowed sequence and
        what the forced EOS leaves.  A request's tokens do not depend on its slot or its neighbours.  Not with
        ``prompt_lookup_num_tokens``.
        ``guidance``: the captured step runs classifier-free guidance (DecodeSession ``guidance``; ops.guide / ops.guide_follow).
        A request ``add``ed with a ``guidance_scale`` takes TWO slots — its own and an unconditional one behind its negative
        prompt — written into the step's table between steps, without a re-capture; every other request takes one, as ever.
        Not with ``prompt_lookup_num_tokens`` or ``logprobs``.
        ``stop_strings`` (with ``tokenizer``; HF's names): the captured step decides for every slot whether its request is over
        (DecodeSession ``stop``; ops.stop) — one of the strings at the end of its generated text, or one of ``eos_token_id``.
        ``step()`` returns what it returns without them and leaves ``self.stopped`` = {slot: index of the finishing token in the
        request's sequence} for the slots that finished since the last step (``add``'s first token included), read in the
        step's one device-to-host copy; releasing the slot stays the caller's business.  Not with
        ``prompt_lookup_num_tokens`` or ``guidance``."""
        if stop_strings is not None:
            if prompt_lookup_num_tokens is not None or guidance:
                raise ValueError("stop_strings does not combine with prompt_lookup_num_tokens or guidance=True")
            if tokenizer is None:
                raise ValueError(NO_TOKENIZER)
        if not 1 <= slots <= 8:
            raise ValueError("1 <= slots <= 8 (the decode step streams weights with the GEMV kernels)")
        if guidance and (prompt_lookup_num_tokens is not None or logprobs is not None):
            raise ValueError("guidance=True does not combine with prompt_lookup_num_tokens or logprobs")
        self.spec_k = None
        k, n = lookup_args(prompt_lookup_num_tokens, max_matching_ngram_size)
        if k is not None:
            if slots * (k + 1) > ops.SPEC_MAX_QUERIES:
                raise ValueError(f"speculation verifies slots x (k + 1) <= {ops.SPEC_MAX_QUERIES} rows per step: {slots} slots x "
                                 f"(k + 1 = {k + 1}) = {slots * (k + 1)} rows")
            if processors:
                raise ValueError("prompt_lookup_num_tokens does not combine with processors=True (the logits processors run on "
                                 "one row per sequence)")
            if logprobs is not None:
                raise ValueError("prompt_lookup_num_tokens does not combine with logprobs")
            if constraints:
                raise ValueError("prompt_lookup_num_tokens does not combine with constraints=True (the token constraints rewrite "
                                 "the logits a draft is checked against)")
            from . import spec as _spec
            _spec.refuse_engine()
            self.spec_k, self.spec_ngram = k, n
        self.model, self.ll = model, model.get_model().llama
        if ctx_max > self.ll.max_positions:
            # positions index the RoPE tables, which hold max_position_embeddings rows
            raise ValueError(f"ctx_max {ctx_max} exceeds the model's {self.ll.max_positions} positions")
        self.slots, self.ctx_max = slots, ctx_max
        self.full = []                                           # slots released by step() because their cache rows filled up
        self.cache = self.ll.new_cache(slots, ctx_max)
        self.cache.key_valid = torch.ones((slots, ctx_max), dtype=torch.uint8, device=self.ll.device)
        self.sampling = sampling
        self.processors = processors
        eos = eos_ids(eos_token_id)
        if not constraints and any(a is not None for a in (bad_words_ids, suppress_tokens, begin_suppress_tokens)):
            raise ValueError("bad_words_ids / suppress_tokens / begin_suppress_tokens need ContinuousBatcher(..., constraints=True)")
        self.constraints = None                                  # the shared tables: one trie region per slot
        if constraints:
            self.constraints = ops.constraint_tables(bad_words_ids, suppress_tokens, begin_suppress_tokens, eos=eos or None, V=self.ll.V,
                                                     capacity={"trie": int(trie_capacity), "trie_slots": slots}, device=self.ll.device)
        self.stop = None if stop_strings is None else ops.stop_tables(tokenizer, stop_strings, device=self.ll.device)
        self.stopped, self._told = {}, [False] * slots           # what the last step found; the slots already reported
        if self.spec_k is not None:
            self.sess = _spec.SpecRowsSession(self.ll, self.cache, self.spec_k, max_ngram=self.spec_ngram, eos_ids=eos,
                                              use_graph=use_graph, sampling=sampling)
        else:
            self.sess = DecodeSession(self.ll, self.cache, use_graph=use_graph, per_row_positions=True, sampling=sampling,
                                      processors=processors, processor_eos=eos, **({} if logprobs is None else {"logprobs": logprobs}),
                                      **({} if self.constraints is None else {"constraints": self.constraints}),
                                      **({"guidance": True} if guidance else {}),
                                      **({} if self.stop is None else {"stop": self.stop, "stop_eos": eos}))
        self.guidance = bool(guidance)
        self.partner = [None] * slots                            # a guided request's other slot, in both directions
        self.uncond = [False] * slots                            # the slot is the unconditional one of its pair
        self.logprobs = None if logprobs is None else int(logprobs)
        self.first_logprobs, self.last_logprobs = {}, {}
        self.live = [False] * slots
        self.length = [0] * slots                                # tokens in each slot's cache (host mirror of sess.pos)
        self._captured = False

    def free_slots(self):
        return [i for i, v in enumerate(self.live) if not v]

    def add(self, input_ids, images=None, attention_mask=None, first_token: Optional[int] = None, temperature: float = 0.0,
            top_k: int = 0, top_p: float = 1.0, seed: Optional[int] = None, repetition_penalty=None, no_repeat_ngram_size=None,
            min_new_tokens=None, allowed_sequences=None, forced_eos_at: Optional[int] = None, guidance_scale=None,
            negative_prompt_ids=None, negative_prompt_attention_mask=None, negative_images=None, guidance_plausibility=0.0) -> int:
        """Prefill one request (input_ids [1, S]) into a free slot; returns the slot.  The first generated token is the
        prefill's argmax unless ``first_token`` is given.  ``temperature`` >= 1e-4 (a sampling batcher only) makes the
        request sample: its first token is drawn on the device from the prefill's logits (draw counter S), the following
        ones inside the captured step; without a ``seed`` one is drawn from torch's generator.
        ``repetition_penalty`` / ``no_repeat_ngram_size`` / ``min_new_tokens`` (a processor batcher only) are HF's
        processors for this request, applied to the prefill's logits (its first token) and inside every step.
        ``allowed_sequences`` (token-id lists: the request answers with exactly one of them, then EOS) and ``forced_eos_at = n``
        (its n-th new token can only be an EOS id: HF's forced EOS at max_new_tokens = n) need a constraints batcher, whose
        shared lists apply to every request.
        ``guidance_scale`` (a guidance batcher only; None or 1: off) with ``negative_prompt_ids`` [1, S_neg] (None: the prompt's
        last token), its mask, ``negative_images`` (the unconditional row's frames; None: text only) and
        ``guidance_plausibility`` are ``generate``'s: the request takes two free slots and the conditional one is returned."""
        guide = guidance_scalars(guidance_scale, guidance_plausibility)
        if guidance_scale is None and any(a is not None for a in (negative_prompt_ids, negative_prompt_attention_mask, negative_images)):
            raise ValueError("negative_prompt_ids / negative_prompt_attention_mask / negative_images need a guidance_scale")
        if guidance_scale is not None and not self.guidance:
            raise ValueError("add(guidance_scale=) needs ContinuousBatcher(..., guidance=True)")
        if temperature > 0 and not self.sampling:
            raise ValueError("add(temperature > 0) needs ContinuousBatcher(..., sampling=True)")
        params = None
        if self.sampling:
            if seed is None and self.spec_k is not None and temperature >= ops.GREEDY_T:
                raise ValueError("a sampling request of a speculating batcher needs its seed (add(..., seed=)): the drafts are "
                                 "verified against the seed's own sequence")
            if seed is None:
                seed = int(torch.randint(0, 1 << 62, (1,)).item()) if temperature >= ops.GREEDY_T else 0
            params = ops.sampling_rows(float(temperature), top_k, top_p, seed, device=self.ll.device)   # validates
        proc = None
        wants = any(a is not None for a in (repetition_penalty, no_repeat_ngram_size, min_new_tokens))
        if wants and not self.processors:
            raise ValueError("add(repetition_penalty= / no_repeat_ngram_size= / min_new_tokens=) needs "
                             "ContinuousBatcher(..., processors=True)")
        ids = torch.as_tensor(input_ids, device=self.ll.device).view(1, -1)
        S = ids.shape[1]
        if self.processors:                                      # validates; a request without them gets a neutral row
            proc = ops.processor_rows(repetition_penalty, no_repeat_ngram_size, None, min_new_tokens, prompt_len=S,
                                      device=self.ll.device)
        if (allowed_sequences is not None or forced_eos_at is not None) and self.constraints is None:
            raise ValueError("add(allowed_sequences= / forced_eos_at=) needs ContinuousBatcher(..., constraints=True)")
        if forced_eos_at is not None and (isinstance(forced_eos_at, bool) or not isinstance(forced_eos_at, int) or forced_eos_at < 1):
            raise ValueError(f"forced_eos_at must be an int >= 1 (the new token that is forced to EOS), got {forced_eos_at!r}")
        free = self.free_slots()
        if not free:
            raise RuntimeError("no free slot")
        slot = free[0]
        if S + 1 > self.ctx_max:
            raise ValueError("prompt does not fit the slot")
        if guide is not None:                                    # validates; the second slot and the negative prompt
            neg_ids, neg_mask = negative_prompt(ids, negative_prompt_ids, negative_prompt_attention_mask, self.ll.device)
            if len(free) < 2:
                raise RuntimeError("no two free slots for a guided request")
            if neg_ids.shape[1] + 1 > self.ctx_max:
                raise ValueError("negative prompt does not fit the slot")
        con = None
        if self.constraints is not None:                         # validates; the trie goes into the slot's own region
            root = -1 if allowed_sequences is None else ops.constraint_trie(self.constraints, slot, allowed_sequences)
            con = ops.constraint_rows(self.constraints, 1, begin=S, max_length=0 if forced_eos_at is None else S + forced_eos_at,
                                      trie_root=root, device=self.ll.device)
        self.cache.key_valid[slot] = 1
        row = type(self.cache).rows_of(self.cache, slot, slot + 1)
        out = self.model(input_ids=ids, images=images, attention_mask=attention_mask, past_key_values=row, use_cache=True)
        last = out.logits[0, -1:]
        if guide is not None:                                    # the pair's first token: the same launch on the two prefills' logits
            other, Sn = free[1], neg_ids.shape[1]
            self.cache.key_valid[other] = 1
            out_u = self.model(input_ids=neg_ids, images=negative_images, attention_mask=neg_mask,
                               past_key_values=type(self.cache).rows_of(self.cache, other, other + 1), use_cache=True)
            both = torch.cat([last, out_u.logits[0, -1:]]).float().contiguous()
            ops.guide(both, ops.guidance_rows(2, [(0, 1, *guide)], device=self.ll.device))
            last = both[:1]
        scored = None
        if self.logprobs is not None:                            # the raw logits: before the processors and the draw rewrite them
            last = last.float().contiguous()
            scored = score_raw(last, self.logprobs, proc is not None or params is not None or con is not None)
        if proc is not None:                                     # the slot's history: the prompt; the first token is processed
            self.sess.proc[slot:slot + 1].copy_(proc)
            self.sess.hist[slot, :S] = ids[0].to(torch.int32)
            last = last.float().contiguous()
            ops.logits_process(last, proc, self.sess.hist[slot:slot + 1], None, S, None, self.sess.proc_eos)
        if con is not None:                                      # behind the processors, on the same history
            self.sess.con[slot:slot + 1].copy_(con)
            self.sess.hist[slot, :S] = ids[0].to(torch.int32)
            last = last.float().contiguous()
            ops.constrain(last, con, self.constraints, self.sess.hist[slot:slot + 1], None, S)
        if first_token is not None:
            tok = int(first_token)
        elif params is not None and temperature >= ops.GREEDY_T:
            tok = int(ops.argmax(last, sampling=params, ctr_add=S)[0])
        else:                                                    # (a greedy request: torch's argmax of the row as the forward left it)
            tok = int(last[0].argmax())
        if self.spec_k is not None:                              # the slot's history: the prompt, then the first token
            self.sess.set_sequence(slot, S, tok, prompt_ids=ids[0], sampling_row=params)
        else:
            if params is not None:
                self.sess.sample[slot:slot + 1].copy_(params)
            self.sess.pos[slot:slot + 1].fill_(S)
            self.sess.tok[slot:slot + 1].fill_(tok)
        if self.stop is not None:                                # the slot's row: only generated text matches, no pad rule
            one = slice(slot, slot + 1)
            self.sess.hist[slot, :S] = ids[0].to(torch.int32)
            self.sess.stop_rows[one].copy_(ops.stop_rows(1, begin=S))
            self.sess.stop_state[one].copy_(ops.stop_state(1))
            self._told[slot] = False                             # the first token goes through the same launch
            ops.stop(self.sess.tok[one], self.sess.stop_rows[one], self.sess.stop_state[one], self.stop, self.sess.hist[one], None,
                     S - 1, eos=self.sess.stop_eos)
        if guide is not None:                                    # the pair's rows of the step's table, read at the next replay
            self.sess.pos[other:other + 1].fill_(Sn)
            self.sess.tok[other:other + 1].fill_(tok)
            if self.sess.sample is not None:                     # the unconditional slot: a greedy, neutral row that follows
                self.sess.sample[other:other + 1].copy_(ops.sampling_rows(0.0, device=self.ll.device))
            if self.sess.proc is not None:
                self.sess.proc[other:other + 1].copy_(ops.processor_rows([None], device=self.ll.device))
            pair = ops.guidance_rows(self.slots, [(slot, other, *guide)], device=self.ll.device)
            self.sess.guide[slot:slot + 1].copy_(pair[slot:slot + 1])
            self.sess.guide[other:other + 1].copy_(pair[other:other + 1])
            self.partner[slot], self.partner[other], self.uncond[other] = other, slot, True
            self.live[other], self.length[other] = True, Sn
        if scored is not None:                                   # the first token sits at index S of the request's sequence
            tabs = None if not self.logprobs else tuple(t[slot:slot + 1] for t in self.sess.lp_top_tables)
            ops.score_record(*scored[:2], self.sess.tok[slot:slot + 1], self.sess.lp_table[slot:slot + 1], None, S,
                             top=scored[2:] if self.logprobs else None, top_tables=tabs)
            self.first_logprobs[slot] = self._read_logprobs(self.sess.lp_table[slot:slot + 1, S:S + 1], scored[2:])[0]
        self.live[slot], self.length[slot] = True, S
        self.last_prefill_logits = last[0]
        return slot

    def step(self) -> dict:
        """One decode step for every live slot: feeds each slot's current token, returns {slot: next token} (greedy, or
        drawn with the slot's parameters in a sampling batcher).  ``self.sess.logits[slot, :V]`` holds that slot's logits.
        A speculating batcher returns {slot: [tokens]}, 1 .. k + 1 per live slot (the logits are then the verify step's rows)."""
        if not self._captured:
            self.sess.begin()
            self._captured = True
        # a slot whose cache rows are full leaves the batch here (reported in self.full) instead of failing the shared
        # step of every other live request
        self.full = [i for i in range(self.slots) if self.live[i] and self.length[i] + 1 > self.ctx_max]
        if self.guidance:                                        # a pair leaves when either slot is full, reported by its conditional slot
            self.full = sorted({self.partner[i] if self.uncond[i] else i for i in self.full})
        for i in self.full:
            self.release(i)
        if not any(self.live):
            return {}
        if self.spec_k is not None:                              # one D2H read per step for all requests, here too
            out = self.sess.step()
            for i, toks in out.items():
                self.length[i] += len(toks)
            return out
        self.sess.step()
        if self.stop is None:
            toks = self.sess.tok.tolist()                        # one D2H read per step for all requests
        else:                                                    # ... the slots' verdicts in the same copy
            toks = torch.cat([self.sess.tok, self.sess.stop_state.view(-1)]).tolist()
            state = toks[self.slots:]
            self.stopped = {i: state[2 * i + 1] for i in range(self.slots) if self.live[i] and state[2 * i] and not self._told[i]}
            for i in self.stopped:
                self._told[i] = True
        rows = None
        if self.logprobs is not None:                            # ... and one more for their log-probabilities: the step's column
            # pos has advanced to the chosen token's index, at most ctx_max for a live slot: the tables' last column.  (An idle
            # slot's counter runs on; the bound only keeps its ignored read inside the table.)
            col = self.sess.pos.long().clamp(0, self.ctx_max)[:, None]
            rows = self._read_logprobs(self.sess.lp_table.gather(1, col), self.sess.lp_top)
            self.last_logprobs = {}
        out = {}
        for i in range(self.slots):
            if self.live[i]:
                self.length[i] += 1
                if self.uncond[i]:                               # advances with its pair, reported by the conditional slot alone
                    continue
                out[i] = toks[i]
                if rows is not None:
                    self.last_logprobs[i] = rows[i]
        return out

    def _read_logprobs(self, lp, top):
        """lp fp32 [R, 1] and the step's top-n rows -> [(lp, ids, lps)] per row, through ONE device-to-host copy"""
        n = self.logprobs
        packed = lp if not n else torch.cat([lp, top[1], top[0].view(torch.float32)], dim=1)
        host = packed.cpu()
        return [(float(host[r, 0]), host[r, 1 + n:].contiguous().view(torch.int32).tolist() if n else [],
                 host[r, 1:1 + n].tolist() if n else []) for r in range(host.shape[0])]

    def release(self, slot: int) -> None:
        if self._captured and self.live[slot]:
            self.sess.check()                                    # once per leaving request (the step's D2H read has synchronised already)
        if self.spec_k is not None and self.live[slot]:
            self.sess.release(slot)
        if self.constraints is not None:                         # the slot's row back to neutral: nothing carries over
            self.sess.con[slot:slot + 1].copy_(ops.constraint_rows(self.constraints, 1, flags=0))
        if self.stop is not None:                                # unwatched again, nothing carries over
            self.sess.stop_rows[slot:slot + 1].copy_(ops.stop_rows(1, watch=False))
            self.sess.stop_state[slot:slot + 1].copy_(ops.stop_state(1))
        self.live[slot] = False
        if self.guidance and self.partner[slot] is not None:     # both slots of a pair leave, their rows back to neutral
            other = self.partner[slot]
            neutral = ops.guidance_rows(1, device=self.ll.device)
            for i in (slot, other):
                self.sess.guide[i:i + 1].copy_(neutral)
                self.partner[i], self.uncond[i], self.live[i] = None, False, False

    def speculation(self, slot: int) -> dict:
        """{"steps", "drafted", "accepted"} of the request in ``slot`` (a speculating batcher; kept until the slot is reused)."""
        if self.spec_k is None:
            raise ValueError("speculation() needs ContinuousBatcher(..., prompt_lookup_num_tokens=k)")
        return self.sess.speculation(slot)
