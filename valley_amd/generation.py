"""What ``ValleyLlamaForCausalLM.generate`` does behind its argument checks: the host loops over the decode sessions — greedy / sampling,
prompt-lookup speculation, beam search — on the pieces they and ``serving.ContinuousBatcher`` share.  decode, spec and beam are
imported where a loop needs them (a generation loads only the companion libraries it uses); a ``prefix`` session is only handed in."""
import torch

from . import ops


def eos_ids(eos_token_id) -> list:
    """``eos_token_id`` (None, an int or a sequence of ints) as a list of ints, [] for None."""
    return [] if eos_token_id is None else [int(eos_token_id)] if isinstance(eos_token_id, int) else [int(e) for e in eos_token_id]


def context_limit(config, S: int, max_new_tokens: int) -> int:
    """Positions a generation may fill: the prompt and its new tokens, within the model's position tables."""
    return min(getattr(config, "max_position_embeddings", 2048), S + max_new_tokens)


def criterion_answers(criteria, seqs, seq_device, device):
    """HF's StoppingCriteriaList, lazily: each criterion is called as ``c(seqs on seq_device, None)`` and answers per row with a tensor
    (yielded as bool [rows] on ``device``) or for the whole batch with a python bool (yielded as it is).  ANY one firing counts: the
    caller ORs the answers into its mask, or stops at the first that fires (then no criterion behind it is called)."""
    for c in criteria or ():
        r = c(seqs.to(seq_device), None)
        yield r.to(device, torch.bool).view(-1) if isinstance(r, torch.Tensor) else bool(r)


def finish(device, *sessions, poll: bool = True) -> None:
    """The end of a generation: synchronise; a stream-K hand-off failure (``poll``) and every session's abort word surface here at the latest."""
    if poll:
        ops.sk_poll_async(device)
    torch.cuda.current_stream().synchronize()
    if poll:
        ops.sk_check_polled(device)
    for s in sessions:
        if s is not None:
            s.check()


def lookup_args(k, max_ngram):
    """``(prompt_lookup_num_tokens, max_matching_ngram_size)`` checked, with HF's default 2; (None, None) when no speculation was asked for."""
    if k is None:
        if max_ngram is not None:
            raise ValueError("max_matching_ngram_size needs prompt_lookup_num_tokens")
        return None, None
    max_ngram = 2 if max_ngram is None else max_ngram
    if isinstance(k, bool) or not isinstance(k, int) or not 1 <= k <= ops.SPEC_MAX_DRAFT:
        raise ValueError(f"prompt_lookup_num_tokens must be an int in [1, {ops.SPEC_MAX_DRAFT}], got {k!r}")
    if isinstance(max_ngram, bool) or not isinstance(max_ngram, int) or not 1 <= max_ngram <= ops.SPEC_MAX_NGRAM:
        raise ValueError(f"max_matching_ngram_size must be an int in [1, {ops.SPEC_MAX_NGRAM}], got {max_ngram!r}")
    return k, max_ngram


def processor_table(proc, S: int, eos, device, rows: int = 1):
    """HF's processors of ``generate`` as ``rows`` equal rows of ops.processor_rows (checked with HF's messages), or None when
    none of them would act (HF adds no processor: the decode is exactly the one without them)."""
    if proc is None or all(a is None for a in proc):
        return None
    rp, nr, ml, mn = proc
    table = ops.processor_rows(rp, nr, ml, mn, prompt_len=S)
    if not eos:
        table[:, 2] = 0                                      # HF's minimum lengths need an EOS id
    if bool((table.view(torch.float32)[:, 0] == 1.0).all() and (table[:, 1] == 0).all() and (table[:, 2] <= S).all()):
        return None
    return table.to(device).expand(rows, 4).contiguous()


def constraint_setup(con, V: int, S: int, max_new_tokens: int, eos, device, rows: int = 1, beams: bool = False):
    """``generate``'s token constraints — ``con`` = (bad_words_ids, suppress_tokens, begin_suppress_tokens, forced_eos_token_id,
    allowed_sequences) — as (ops.ConstraintTables, int32 [rows, 4] rows of ops.constraint_rows) on ``device``, or None when none
    was given.  Checked before anything is launched, with HF's messages where HF has one.  ``forced_eos_token_id`` (an int or a
    list) is HF's: at length S + max_new_tokens - 1 only those ids remain; it has to name the ``eos`` ids, the one EOS table of
    every rule.  ``allowed_sequences``: token-id lists shared by all rows, or one such list of lists per row."""
    if con is None or all(a is None for a in con):
        return None
    bad, sup, beg, forced, allowed = con
    if beams and (allowed is not None or forced is not None):
        raise ValueError("allowed_sequences and forced_eos_token_id are not supported with num_beams > 1 (a row that is all "
                         "-inf but a few ids changes which ties the beams' top-K picks); bad_words_ids, suppress_tokens and "
                         "begin_suppress_tokens are")
    if forced is not None:
        if not eos:
            raise ValueError("`forced_eos_token_id` needs an `eos_token_id`: the ids it forces are the generation's EOS ids")
        if isinstance(forced, bool) or not isinstance(forced, (int, list, tuple)) or sorted(set(eos_ids(forced))) != sorted(set(eos)):
            raise ValueError(f"`forced_eos_token_id` has to name the `eos_token_id` ids {sorted(set(eos))} (one EOS table serves "
                             f"every rule), but is {forced}")
    if allowed is not None and not eos:
        raise ValueError("`allowed_sequences` needs an `eos_token_id`: behind a complete sequence only EOS is allowed")
    per_row, tries = False, []
    if allowed is not None:
        if not isinstance(allowed, (list, tuple)) or len(allowed) == 0:
            raise ValueError(f"`allowed_sequences` has to be a non-empty list of lists, but is {allowed}.")
        first = allowed[0]
        per_row = isinstance(first, (list, tuple)) and len(first) > 0 and isinstance(first[0], (list, tuple))
        if per_row and len(allowed) != rows:
            raise ValueError(f"allowed_sequences: {len(allowed)} per-row lists for {rows} rows")
        tries = list(allowed) if per_row else [allowed]
        words = [len(ops.pack_trie(t, V)) for t in tries]    # validates every sequence
    cap = {"trie": max(words), "trie_slots": len(tries)} if tries else None
    tables = ops.constraint_tables(bad, sup, beg, eos=eos or None, V=V, capacity=cap, device=device)
    roots = [ops.constraint_trie(tables, i, t) for i, t in enumerate(tries)]
    root = -1 if not roots else (roots if per_row else roots[0])
    return tables, ops.constraint_rows(tables, rows, begin=S, max_length=S + max_new_tokens if forced is not None else 0,
                                       trie_root=root, device=device)


def score_raw(x, n: int, rewritten: bool):
    """(raw logits, lse, top-n ids, top-n values) of ``x``; the raw logits are a copy when processors or a sampler will rewrite ``x``.
    The first token is, in every caller: score_raw -> ops.logits_process -> ops.argmax (counter S) -> ops.score_record of the token."""
    raw = torch.empty_like(x) if rewritten else None
    _, lse, tid, tl = ops.token_logprobs(x, top=n, copy=raw)
    return (x if raw is None else raw), lse, tid, tl


def _prefill(model, prefix, input_ids, images, attention_mask, B, S, max_new_tokens):
    """The cache of a generation and the forward that fills it: a new cache and the whole prompt, or — with a
    PrefixSession — the session's cache, the tokens behind its common prefix, and room for the new tokens."""
    if prefix is None:
        cache = model.model.llama.new_cache(B, max(context_limit(model.config, S, max_new_tokens), S + 1))
        return cache, model.forward(input_ids=input_ids, images=images, attention_mask=attention_mask, past_key_values=cache, use_cache=True)
    out = prefix.forward(input_ids, images)
    prefix.reserve(S + max_new_tokens)
    return prefix.cache, out


def _generate_spec(model, input_ids, images, attention_mask, max_new_tokens, stopping_criteria, eos_token_id, use_graph, spec,
                   do_sample=False, temperature=1.0, top_k=None, top_p=None, prefix=None):
    """Generation of one row through SpecDecodeSession: the tokens a step emits are appended ONE at a time, the EOS test and every
    stopping criterion see the sequence up to that token as in ``_generate``'s loop, and whatever a step emitted behind the stop or
    behind ``max_new_tokens`` is dropped.  With fewer than k + 1 cache positions left, the remaining tokens come from the one-token
    DecodeSession; the speculative session is made (warmed up and captured, which writes k + 1 cache rows) only once a step of it
    can run, so ``max_new_tokens <= k`` never makes one.  Greedy, or seeded sampling (``generate`` admits ``do_sample`` with a seed
    only): both sessions hold the row's parameters and every draw is keyed by (seed, index of the drawn token)."""
    from .decode import DecodeSession
    from .spec import SpecDecodeSession
    k, max_ngram, seed = spec
    sample = None                                            # the row's parameters of the on-device draw (checked before the prefill)
    if do_sample and temperature >= ops.GREEDY_T:
        sample = ops.sampling_rows(float(temperature), 0 if top_k is None else top_k, 1.0 if top_p is None else top_p, [seed])
    d = model.device
    input_ids = input_ids.to(d)
    S = input_ids.shape[1]
    cache, out = _prefill(model, prefix, input_ids, images, attention_mask, 1, S, max_new_tokens)
    eos = eos_ids(eos_token_id) or None
    if sample is not None:
        sample = sample.to(d)
    last = out.logits[:, -1, :].contiguous()                 # ``_generate``'s first token: the draw's counter is the prompt's length
    new = [int((ops.argmax(last) if sample is None else ops.argmax(last, sampling=sample, ctr_add=S))[0])]
    sess, plain, plain_steps = None, None, 0

    def stopped() -> bool:
        """EOS, or a stopping criterion on the sequence so far: a python bool stays on the host, none is called behind the first hit"""
        if eos is not None and new[-1] in eos:
            return True
        if stopping_criteria is None:
            return False
        seq = torch.cat([input_ids, torch.tensor([new], dtype=input_ids.dtype, device=d)], dim=1)
        return any(bool(a.all()) if isinstance(a, torch.Tensor) else a for a in criterion_answers(stopping_criteria, seq, d, d))

    done = False
    while len(new) < max_new_tokens and not done:
        if stopped() or cache.seq_len + 1 > cache.ctx_max:
            break
        if plain is None and cache.seq_len + k + 1 <= cache.ctx_max:
            if sess is None:
                sess = SpecDecodeSession(model.model.llama, cache, k, max_ngram, eos_ids=eos, use_graph=use_graph, sampling=sample is not None)
                if sample is not None:
                    sess.sample.copy_(sample.expand(k + 1, 6))
                known = torch.cat([input_ids[0], torch.tensor(new[:-1], dtype=input_ids.dtype, device=d)])
                sess.begin(torch.tensor(new[-1:], device=d), prompt_ids=known)
            emitted = sess.step()
        else:                                                # the cache's last positions: one token per step
            if plain is None:
                plain = DecodeSession(model.model.llama, cache, use_graph=use_graph, sampling=sample is not None)
                if sample is not None:                       # its counters go on from the cache's position: the seed's sequence
                    plain.sample.copy_(sample)
                plain.begin(torch.tensor([new[-1]], device=d))
            emitted = [int(plain.step()[0])]
            plain_steps += 1
        for j, t in enumerate(emitted):
            if j and stopped():                              # (before the step's first token the loop has tested already)
                done = True
                break
            new.append(t)
            if len(new) == max_new_tokens:
                break
    finish(d, sess, plain)
    seq = torch.cat([input_ids, torch.tensor([new], dtype=input_ids.dtype, device=d)], dim=1)
    speculation = sess.speculation() if sess is not None else {"steps": 0, "drafted": 0, "accepted": 0}
    speculation["steps"] += plain_steps                      # decode steps of either kind: steps + accepted = tokens they emitted
    if prefix is not None:
        prefix.settle(seq)
    return seq, speculation


def token_loop(step, token, seq, finished, eos, stopping_criteria, max_new_tokens, cache, d):
    """The loop of ``_generate`` and ``_generate_guided`` behind the first token: a row has finished once it emitted an EOS id or a
    stopping criterion fired on the sequences so far (``finished`` is updated in place; ``step`` pads a finished row's tokens); the
    loop ends when every row has, at ``max_new_tokens`` or with the cache full.  -> the sequences."""
    for _ in range(max_new_tokens - 1):
        if eos is not None:
            finished |= torch.isin(token, eos)
        for a in criterion_answers(stopping_criteria, seq, d, d):
            finished |= a if isinstance(a, torch.Tensor) else torch.full_like(finished, a)
        if bool(finished.all()) or cache.seq_len + 1 > cache.ctx_max:
            break
        token = step(token)
        seq = torch.cat([seq, token[:, None]], dim=1)
    return seq


STOP_KEYS = ("stop_strings", "stop_begin", "sync_every")
NO_TOKENIZER = ("There are one or more stop strings, either in the arguments to `generate` or in the model's generation config, but "
                "we could not locate a tokenizer. When generating with stop strings, you must pass the model's tokenizer to the "
                "`tokenizer` argument of `generate`.")                       # HF's message


def stop_args(model, input_ids, stop_strings, tokenizer, stop_begin, sync_every, num_beams, prompt_lookup_num_tokens, guided,
              stopping_criteria, do_sample, temperature, top_k, top_p, seed, output_logprobs, use_graph, eos_token_id):
    """``generate``'s stop arguments checked -> (ops.StopTables on the host, stop_begin, sync_every), or None where the end of the
    generation stays with the host (no ``stop_strings``, ``sync_every`` 1): that call launches what it launched before.  Every
    combination the loops do not cover is refused here, before the model is touched; the tables are built on the host."""
    if isinstance(sync_every, bool) or not isinstance(sync_every, int) or sync_every < 1:
        raise ValueError(f"sync_every must be an int >= 1, got {sync_every!r}")
    if stop_strings is None and sync_every == 1:
        return None
    if stop_begin not in ("sequence", "generated"):
        raise ValueError(f'stop_begin must be "sequence" or "generated", got {stop_begin!r}')
    what = "stop_strings" if stop_strings is not None else "sync_every > 1"
    if num_beams is not None and not isinstance(num_beams, bool) and int(num_beams) > 1:
        raise ValueError(f"{what} is not supported with num_beams > 1")
    if prompt_lookup_num_tokens is not None:
        raise ValueError(f"{what} is not supported with prompt_lookup_num_tokens")
    if guided:
        raise ValueError(f"{what} is not supported with guidance_scale")
    if sync_every > 1:
        if stopping_criteria:
            raise ValueError("sync_every > 1 is not supported with stopping_criteria (a host callback looks at every token)")
        if do_sample and temperature >= ops.GREEDY_T and top_k is None and top_p is None and seed is None:
            raise ValueError("sync_every > 1 is not supported with do_sample without top_k / top_p / seed (the host draws every token)")
        if output_logprobs:
            raise ValueError("sync_every > 1 is not supported with output_logprobs")
        if use_graph is None or input_ids.shape[0] > 8 or model.model.precision == "fp32":
            raise ValueError("sync_every > 1 needs the decode session: use_graph True (captured) or False (eager), not None, at "
                             "most 8 rows, not the fp32 engine")
        if stop_strings is None and not eos_ids(eos_token_id):
            raise ValueError("sync_every > 1 needs stop_strings or an eos_token_id (nothing on the device would end the generation)")
    if stop_strings is not None and tokenizer is None:
        raise ValueError(NO_TOKENIZER)
    return ops.stop_tables(tokenizer, () if stop_strings is None else stop_strings), stop_begin, sync_every


def block_loop(sess, S, max_new_tokens, sync_every, cache):
    """The loop of ``_generate`` behind the first token where the device decides the end (DecodeSession ``stop``): up to
    ``sync_every`` steps are enqueued, then ``sess.stop_state`` is read — the block's only device-to-host traffic — until every
    row has finished, at ``max_new_tokens`` or with the cache full.  -> the new tokens [B, n] (one read of the history and the
    last chosen token), cut at the step where the last row finished: steps replayed behind the end are dropped."""
    steps = 0
    while True:
        state = sess.stop_state.cpu()
        left = min(max_new_tokens - 1 - steps, cache.ctx_max - cache.seq_len)
        if bool(state[:, 0].all()) or left <= 0:
            break
        for _ in range(min(sync_every, left)):
            sess.step()
        steps += min(sync_every, left)
    new = torch.cat([sess.hist[:, S:S + steps], sess.tok[:, None]], dim=1).to(torch.long)
    return new[:, :int(state[:, 1].max()) + 1 - S] if bool(state[:, 0].all()) else new


def sampling_setup(do_sample, temperature, top_k, top_p, seed, B, device):
    """(greedy, per-row parameters of the on-device draw or None): sampling with any of top_k / top_p / seed draws on the device,
    row r with seed + r (or its own seed of a list); without a seed one is drawn from torch's generator."""
    greedy = not (do_sample and temperature >= ops.GREEDY_T)
    sample = None
    if not greedy and (top_k is not None or top_p is not None or seed is not None):
        if seed is None:
            seed = int(torch.randint(0, 1 << 62, (1,)).item())           # reproducible under torch.manual_seed
        seeds = [(int(seed) + r) % (1 << 64) for r in range(B)] if not isinstance(seed, (list, tuple)) else list(seed)
        if len(seeds) != B:
            raise ValueError(f"generate: {len(seeds)} seeds for {B} rows")
        sample = ops.sampling_rows(float(temperature), 0 if top_k is None else top_k, 1.0 if top_p is None else top_p, seeds, device=device)
    return greedy, sample


def _generate(model, input_ids, images, attention_mask, max_new_tokens, do_sample, temperature, stopping_criteria, eos_token_id,
              use_graph, top_k, top_p, seed, pad, proc=None, logprobs=None, prefix=None, con=None, stop=None):
    """Greedy decoding and sampling: the first token from the prefill's logits, then one ``step`` per token (the decode session's, or
    the generic forward's) until every row has finished; a finished row emits ``pad`` (HF).  -> sequences, log-probability fields.
    ``stop`` (stop_args'): EOS and HF's stop strings are tested on the device behind every chosen token (ops.stop: inside the
    session's step, eagerly behind the first token, the generic forward's and a host draw), and with ``sync_every`` > 1 the
    session's steps run in blocks (``block_loop``)."""
    d = model.device
    input_ids = input_ids.to(d)
    B, S = input_ids.shape
    con = constraint_setup(con, model.model.llama.V, S, max_new_tokens, eos_ids(eos_token_id), d, B)
    cache, out = _prefill(model, prefix, input_ids, images, attention_mask, B, S, max_new_tokens)
    greedy, sample = sampling_setup(do_sample, temperature, top_k, top_p, seed, B, d)
    on_device = greedy or sample is not None                 # else the host draws: torch.multinomial over the step's logits

    def pick(last, ctr):                                     # ctr: index of the drawn token in the sequence
        if on_device:
            return (ops.argmax(last) if sample is None else ops.argmax(last, sampling=sample, ctr_add=ctr)).to(torch.long)
        return torch.multinomial(torch.softmax(last / temperature, dim=-1), num_samples=1).view(B)

    eos_list = eos_ids(eos_token_id) or None
    eos = None if eos_list is None else torch.as_tensor(eos_list, device=d)
    if pad is None:
        pad = int(eos[0]) if eos is not None else 0
    finished = torch.zeros((B,), dtype=torch.bool, device=d)
    table = processor_table(proc, S, eos_list, d, B)
    if con is not None and table is None:                    # the constraints read the history the processors' launch appends to
        table = ops.processor_rows([None] * B, device=d)
    rewritten = table is not None or sample is not None      # the logits are rewritten in place before the token is picked
    if stop is not None and table is None:                   # the stop test reads that history too (neutral rows rewrite nothing)
        table = ops.processor_rows([None] * B, device=d)
    eos32 = None if eos is None or table is None else eos.to(torch.int32)
    st_rows = st_state = st_tables = None
    sync_every = 1
    if stop is not None:                                     # every row watched; a finished row's tokens become pad
        st_tables, sync_every = stop[0]._replace(buf=stop[0].buf.to(d)), stop[2]
        st_rows = ops.stop_rows(B, begin=S if stop[1] == "generated" else 0, pad=pad, pad_after=True, device=d)
        st_state = ops.stop_state(B, device=d)
    lp_cols, lp_done = [], []                                # per new token: its [B, 1(, n)] record; the rows already finished

    def record(scored, tok):
        col = torch.zeros((B, 1), dtype=torch.float32, device=d)
        tabs = (torch.full((B, 1, logprobs), -1, dtype=torch.int32, device=d),
                torch.zeros((B, 1, logprobs), dtype=torch.float32, device=d)) if logprobs else None
        ops.score_record(*scored[:2], tok.to(torch.int32), col, None, 0, top=scored[2:] if logprobs else None, top_tables=tabs)
        lp_cols.append((col,) + (tabs or ()))
        lp_done.append(finished.clone())

    last = out.logits[:, -1, :].contiguous()
    scored = score_raw(last, logprobs, rewritten) if logprobs is not None else None
    hist = None
    if table is not None:                                    # HF's processors over each row's whole input_ids, on the device
        hist = torch.zeros((B, cache.ctx_max), dtype=torch.int32, device=d)
        hist[:, :S] = input_ids.to(torch.int32)
        ops.logits_process(last, table, hist, None, S, None, eos32)
        if con is not None:
            ops.constrain(last, con[1], con[0], hist, None, S)
    token = pick(last, S)
    if logprobs is not None:                                 # the first token: from the prefill's last logits
        record(scored, token)
    if stop is not None:                                     # the same launch over the prompt's history: the token has index S
        ops.stop(token.to(torch.int32), st_rows, st_state, st_tables, hist, None, S - 1, eos=eos32)
    seq = torch.cat([input_ids, token[:, None]], dim=1)
    if B > 8 or model.model.precision == "fp32":
        use_graph = None                                     # the GEMV decode session is bf16, for <= 8 sequences
    sess, mask = None, attention_mask
    if use_graph is not None:
        from .decode import DecodeSession
        sess = DecodeSession(model.model.llama, cache, use_graph=bool(use_graph), sampling=sample is not None, processors=table is not None,
                             processor_eos=eos_list, **({} if logprobs is None else {"logprobs": logprobs}),
                             **({} if con is None else {"constraints": con[0]}),
                             **({} if stop is None or not on_device else {"stop": st_tables, "stop_eos": eos_list}))
        if sample is not None:
            sess.sample.copy_(sample)
        if table is not None:
            sess.proc.copy_(table)
        if con is not None:
            sess.con.copy_(con[1])
        if stop is not None and on_device:                   # the step tests the token it chose; the state goes on from the first
            sess.stop_rows.copy_(st_rows)
            sess.stop_state.copy_(st_state)
            st_state = sess.stop_state
        sess.begin(token, prompt_ids=input_ids if table is not None else None)

    def session_step(token):
        nxt = sess.step()
        token = nxt.to(torch.long).clone() if on_device else pick(sess.logits[:, :model.model.llama.V], None)
        if bool(finished.any()) or not on_device:
            token = torch.where(finished, torch.full_like(token, pad), token)
            sess.tok.copy_(token.to(torch.int32))
            if logprobs is not None and not on_device:
                sess.record_token()                          # the step recorded its own argmax: the host's draw replaces it
        if stop is not None and not on_device:               # the host's draw is tested (pos has advanced: the history ends at pos - 1)
            ops.stop(sess.tok, st_rows, st_state, st_tables, sess.hist, sess.pos, -1, eos=eos32)
        if logprobs is not None:
            lp_done.append(finished.clone())
        return token

    def forward_step(token):
        nonlocal mask
        if mask is not None:
            mask = torch.cat([mask.to(d), torch.ones((B, 1), dtype=mask.dtype, device=d)], dim=1)
        last = model.forward(input_ids=token[:, None], attention_mask=mask, past_key_values=cache, use_cache=True).logits[:, -1, :].contiguous()
        scored = score_raw(last, logprobs, rewritten) if logprobs is not None else None
        if table is not None:                                # the fed token joins the history at index seq_len - 1
            ops.logits_process(last, table, hist, None, cache.seq_len, token.to(torch.int32), eos32)
            if con is not None:
                ops.constrain(last, con[1], con[0], hist, None, cache.seq_len)
        token = torch.where(finished, torch.full_like(token, pad), pick(last, cache.seq_len))
        if logprobs is not None:
            record(scored, token)
        if stop is not None:                                 # the history ends at the fed token, index seq_len - 1
            ops.stop(token.to(torch.int32), st_rows, st_state, st_tables, hist, None, cache.seq_len - 1, eos=eos32)
        return token

    if sync_every > 1:                                       # the device decides the end and pads; the host looks once per block
        seq = torch.cat([input_ids, block_loop(sess, S, max_new_tokens, sync_every, cache).to(input_ids.dtype)], dim=1)
    else:
        if stop is not None:                                 # the device's verdict joins the criteria: no token leaves the device for it
            stopping_criteria = [*(stopping_criteria or ()), lambda seqs, scores: st_state[:, 0] != 0]
        step = forward_step if sess is None else session_step
        seq = token_loop(step, token, seq, finished, eos, stopping_criteria, max_new_tokens, cache, d)
    finish(d, sess)
    lp_out = {}
    if logprobs is not None:                                 # one read of the session's tables, after the loop
        parts = [torch.cat([c[k] for c in lp_cols], dim=1) for k in range(3 if logprobs else 1)]
        if sess is not None:                                 # columns S + 1 ..: the tokens the steps chose
            tabs = [sess.lp_table] + list(sess.lp_top_tables or ())
            parts = [torch.cat([p, t[:, S + 1:seq.shape[1]]], dim=1) for p, t in zip(parts, tabs)]
        done = torch.stack(lp_done, dim=1)                   # [B, new]: the row had finished before this token (a pad)
        lp_out["token_logprobs"] = torch.where(done, torch.zeros_like(parts[0]), parts[0])
        if logprobs:
            lp_out["top_tokens"] = torch.where(done[:, :, None], torch.full_like(parts[1], -1), parts[1])
            lp_out["top_logprobs"] = torch.where(done[:, :, None], torch.zeros_like(parts[2]), parts[2])
    if prefix is not None:
        prefix.settle(seq)
    return seq, lp_out


GUIDANCE_KEYS = ("guidance_scale", "negative_prompt_ids", "negative_prompt_attention_mask", "negative_images", "guidance_plausibility")
GUIDANCE_MAX_ROWS = 4                                        # prompts of a guided generation: 2 rows each in the 8-row decode step


def guidance_scalars(scale, beta):
    """A request's ``guidance_scale`` and ``guidance_plausibility``, checked -> (float scale, float beta), or None where guidance
    is off (a scale of None or 1, as in HF)."""
    import math
    if scale is None:
        if beta not in (None, 0, 0.0):
            raise ValueError("guidance_plausibility needs a guidance_scale")
        return None
    if isinstance(scale, bool) or not isinstance(scale, (int, float)) or not math.isfinite(scale):
        raise ValueError(f"guidance_scale must be a finite float, got {scale!r}")
    beta = 0.0 if beta is None else beta
    if isinstance(beta, bool) or not isinstance(beta, (int, float)) or not 0.0 <= beta <= 1.0:
        raise ValueError(f"guidance_plausibility must lie in [0, 1], got {beta!r}")
    return None if scale == 1 else (float(scale), float(beta))


def negative_prompt(input_ids, neg_ids, neg_mask, device):
    """HF's unconditional context: the negative prompt [B, S_neg] and its mask, or — without one — each row's last prompt token."""
    B = input_ids.shape[0]
    if neg_ids is None:
        if neg_mask is not None:
            raise ValueError("negative_prompt_attention_mask needs negative_prompt_ids")
        return input_ids[:, -1:].to(device), None
    neg_ids = torch.as_tensor(neg_ids)
    if neg_ids.dim() != 2 or neg_ids.shape[0] != B or neg_ids.shape[1] < 1:
        raise ValueError(f"negative_prompt_ids must be [{B}, S_neg] (one negative prompt per prompt row), got {tuple(neg_ids.shape)}")
    if neg_mask is not None:
        neg_mask = torch.as_tensor(neg_mask)
        if tuple(neg_mask.shape) != tuple(neg_ids.shape):
            raise ValueError(f"negative_prompt_attention_mask must have negative_prompt_ids' shape {tuple(neg_ids.shape)}, got "
                             f"{tuple(neg_mask.shape)}")
    return neg_ids.to(device), neg_mask


def guidance_args(model, input_ids, guidance_scale, negative_prompt_ids, negative_prompt_attention_mask, negative_images,
                  guidance_plausibility, num_beams, prompt_lookup_num_tokens, prefix, output_logprobs, use_graph):
    """``generate``'s guidance arguments checked -> (scale, beta, negative ids, negative mask, negative images), or None where
    guidance is off; every combination the guided loop does not cover is refused here, before the model is touched."""
    if guidance_scale is None and any(a is not None for a in (negative_prompt_ids, negative_prompt_attention_mask, negative_images)):
        raise ValueError("negative_prompt_ids / negative_prompt_attention_mask / negative_images need a guidance_scale")
    g = guidance_scalars(guidance_scale, guidance_plausibility)
    if g is None:
        return None
    if input_ids.dim() != 2 or input_ids.shape[0] > GUIDANCE_MAX_ROWS:
        raise ValueError(f"guidance_scale decodes two rows per prompt in the 8-row decode step: at most {GUIDANCE_MAX_ROWS} prompt "
                         f"rows, got input_ids {tuple(input_ids.shape)}")
    if num_beams is not None and not isinstance(num_beams, bool) and int(num_beams) > 1:
        raise ValueError("guidance_scale is not supported with num_beams > 1")
    if prompt_lookup_num_tokens is not None:
        raise ValueError("guidance_scale is not supported with prompt_lookup_num_tokens (guidance rewrites the logits a draft is "
                         "checked against)")
    if prefix is not None:
        raise ValueError("guidance_scale is not supported with prefix= (a session holds one row)")
    if output_logprobs:
        raise ValueError("guidance_scale is not supported with output_logprobs")
    if use_graph is None:
        raise ValueError("guidance_scale needs the decode session: use_graph True (captured) or False (eager), not None")
    if model.model.precision == "fp32":
        raise ValueError("guidance_scale needs a 16-bit or weight-quantized engine (the decode session's), not fp32")
    neg_ids, neg_mask = negative_prompt(input_ids, negative_prompt_ids, negative_prompt_attention_mask, model.device)
    return g[0], g[1], neg_ids, neg_mask, negative_images


def _generate_guided(model, input_ids, images, attention_mask, max_new_tokens, do_sample, temperature, stopping_criteria, eos_token_id,
                     use_graph, top_k, top_p, seed, pad, guide, proc=None, con=None):
    """Classifier-free guidance (HF's ``guidance_scale`` / ``negative_prompt_ids``; ``guide`` = guidance_args'): the B prompts and
    their B negative prompts are prefilled into rows [0, B) and [B, 2B) of one cache and decoded by one per-row session of 2B rows
    (DecodeSession ``guidance``).  Row b's logits become scale * (lc - lu) + lu of its own and row B + b's log-softmax
    (ops.guide) in front of the processors, the constraints and the draw, which act on the conditional rows as in ``_generate``;
    row B + b is then fed row b's token (ops.guide_follow).  Stop rule, padding and the end are ``_generate``'s."""
    from .decode import DecodeSession
    scale, beta, neg_ids, neg_mask, neg_images = guide
    d, ll = model.device, model.model.llama
    input_ids = input_ids.to(d)
    B, S = input_ids.shape
    Sn, R = neg_ids.shape[1], 2 * B
    eos_list = eos_ids(eos_token_id) or None
    con = constraint_setup(con, ll.V, S, max_new_tokens, eos_list or [], d, B)
    table = processor_table(proc, S, eos_list, d, B)
    rows = ops.guidance_rows(R, [(b, B + b, scale, beta) for b in range(B)], device=d)
    top = max(S, Sn)
    cache = ll.new_cache(R, max(context_limit(model.config, top, max_new_tokens), top + 1))
    cache.key_valid = torch.ones((R, cache.ctx_max), dtype=torch.uint8, device=d)
    half = type(cache).rows_of
    out_c = model.forward(input_ids=input_ids, images=images, attention_mask=attention_mask, past_key_values=half(cache, 0, B), use_cache=True)
    out_u = model.forward(input_ids=neg_ids, images=neg_images, attention_mask=neg_mask, past_key_values=half(cache, B, R), use_cache=True)
    cache.seq_len = top                                      # the deeper half: what the loop's room test counts
    greedy, sample = sampling_setup(do_sample, temperature, top_k, top_p, seed, B, d)
    if sample is not None:                                   # the unconditional rows take the argmax of their own logits, then follow
        sample = torch.cat([sample, ops.sampling_rows([0.0] * B, device=d)])
    on_device = greedy or sample is not None

    eos = None if eos_list is None else torch.as_tensor(eos_list, device=d)
    if pad is None:
        pad = int(eos[0]) if eos is not None else 0
    finished = torch.zeros((B,), dtype=torch.bool, device=d)
    if con is not None and table is None:                    # the constraints read the history the processors' launch appends to
        table = ops.processor_rows([None] * B, device=d)
    eos32 = hist = None
    if table is not None:                                    # the conditional rows' whole input_ids, as in HF; the others stay neutral
        table = torch.cat([table, ops.processor_rows([None] * B, device=d)])
        eos32 = None if eos is None else eos.to(torch.int32)
        hist = torch.zeros((R, cache.ctx_max), dtype=torch.int32, device=d)
        hist[:B, :S] = input_ids.to(torch.int32)
        hist[B:, :Sn] = neg_ids.to(torch.int32)
    con_rows = None if con is None else torch.cat([con[1], ops.constraint_rows(con[0], B, flags=0, device=d)])
    pos = torch.tensor([S] * B + [Sn] * B, dtype=torch.int32, device=d)

    last = torch.cat([out_c.logits[:, -1, :], out_u.logits[:, -1, :]]).float().contiguous()
    ops.guide(last, rows)                                    # the first token: the same launch on the two prefills' last logits
    if table is not None:
        ops.logits_process(last, table, hist, pos, 0, None, eos32)
        if con is not None:
            ops.constrain(last, con_rows, con[0], hist, pos, 0)

    def pick(x, ctr_add):                                    # x [2B, V] -> the conditional rows' tokens [B]
        if on_device:
            tok = ops.argmax(x) if sample is None else ops.argmax(x, sampling=sample, ctr=pos, ctr_add=ctr_add)
            return tok[:B].to(torch.long)
        return torch.multinomial(torch.softmax(x[:B] / temperature, dim=-1), num_samples=1).view(B)

    token = pick(last, 0)
    seq = torch.cat([input_ids, token[:, None]], dim=1)
    sess = DecodeSession(ll, cache, use_graph=bool(use_graph), per_row_positions=True, sampling=sample is not None,
                         processors=table is not None, processor_eos=eos_list, guidance=True,
                         **({} if con is None else {"constraints": con[0]}))
    sess.guide.copy_(rows)
    if sample is not None:
        sess.sample.copy_(sample)
    if table is not None:
        sess.proc.copy_(table)
        sess.hist.copy_(hist)
    if con is not None:
        sess.con.copy_(con_rows)
    sess.pos.copy_(pos)
    sess.tok.copy_(token.to(torch.int32).repeat(2))
    sess.begin()

    def step(token):
        nxt = sess.step()
        token = nxt[:B].to(torch.long).clone() if on_device else pick(sess.logits[:, :ll.V], None)
        if bool(finished.any()) or not on_device:
            token = torch.where(finished, torch.full_like(token, pad), token)
            sess.tok.copy_(token.to(torch.int32).repeat(2))
        return token

    seq = token_loop(step, token, seq, finished, eos, stopping_criteria, max_new_tokens, cache, d)
    finish(d, sess)
    return seq


def _generate_beams(model, input_ids, images, attention_mask, max_new_tokens, nb, length_penalty, early_stopping, nrs,
                    stopping_criteria, eos_token_id, use_graph, pad, proc=None, con=None):
    """Beam search (HF ``_beam_search``): the B prompts are prefilled once (images, padding mask) into rows [0, B) of a B * nb-row
    cache, whose prompt positions the reorder kernel then copies into every beam row (key_valid likewise).  Every step picks the K
    best continuations per prompt on the device (ops.beam_candidates), selects the running beams (ops.beam_select) and makes the KV
    rows of the generated positions follow their parents (ops.kv_beam_reorder); the host keeps the hypotheses (valley_amd.beam) from
    one small copy of the candidates.  Up to 8 rows the step is the decode session's (captured or eager); otherwise, or with
    ``use_graph=None``, the generic forward followed by the same three kernels.  Stopping criteria are evaluated on the host over the
    [B * K, cur_len + 1] candidate sequences, as HF does, and hand the hit mask to the select kernel.  With processors every beam row
    keeps its token history on the device (following its parent, as its KV rows do); candidates: over the processed log_softmax."""
    from .beam import BeamSearch
    from .decode import DecodeSession
    d = model.device
    input_ids = input_ids.to(d)
    B, S = input_ids.shape
    R, ll = B * nb, model.model.llama
    eos = eos_ids(eos_token_id)
    max_len = context_limit(model.config, S, max_new_tokens)
    con = constraint_setup(con, ll.V, S, max_new_tokens, eos, d, R, beams=True)
    if max_len <= S:
        return input_ids.clone(), torch.zeros((B * nrs,), dtype=torch.float32)
    state = BeamSearch(input_ids, nb, max_len, eos_ids=eos, pad_token_id=pad, length_penalty=length_penalty,
                       early_stopping=early_stopping, num_return_sequences=nrs)
    K = state.K
    if state.K > ops.BEAM_MAX_K or nb > ops.BEAM_MAX_NB:
        raise ValueError(f"beam search takes num_beams <= {ops.BEAM_MAX_NB} and max(2, 1 + n_eos) * num_beams <= "
                         f"{ops.BEAM_MAX_K} (got {nb} beams, {len(eos)} EOS ids)")
    cache = ll.new_cache(R, max_len + 1)
    prompt = type(cache).rows_of(cache, 0, B)                # (HipKVCache, or the fp32 engine's F32KVCache)
    out = model.forward(input_ids=input_ids, images=images, attention_mask=attention_mask, past_key_values=prompt, use_cache=True)
    expand = torch.arange(R, dtype=torch.int32, device=d) // nb          # row b * nb + j <- prompt row b
    kv_table = ops.kv_beam_table(cache.k, cache.v, d)
    ops.kv_beam_reorder(kv_table, cache.k[0], expand, 0, S)
    cache.seq_len = S
    if prompt.key_valid is not None:
        cache.key_valid = prompt.key_valid.index_select(0, expand.long()).contiguous()
    eos_dev = torch.tensor(eos, dtype=torch.int32, device=d) if eos else None
    scratch = ops.beam_scratch(B, nb, K, d)
    running = state.initial_running().to(d)
    first = out.logits[:, -1, :].float().repeat_interleave(nb, dim=0).contiguous()
    table = processor_table(proc, S, eos, d, R)
    if con is not None and table is None:                    # the constraints run behind the processors' launch, on its scores
        table = ops.processor_rows([None] * R, device=d)
    hist = None
    if table is not None:                                    # every beam row's history: its prompt's whole input_ids
        hist = torch.zeros((R, cache.ctx_max), dtype=torch.int32, device=d)
        hist[:, :S] = input_ids.to(torch.int32).repeat_interleave(nb, dim=0)

    def candidates(x, length, tok):
        """the K best continuations per prompt of the logits ``x``; with processors, HF's: over log_softmax(x), then + running"""
        if table is None:
            return ops.beam_candidates(x, running, B, nb, K, eos_dev, scratch)
        ops.logits_process(x, table, hist, None, length, tok, eos_dev, log_softmax=True)
        if con is not None:
            ops.constrain(x, con[1], con[0], hist, None, length)
        return ops.logits_beam_candidates(x, running, B, nb, K, eos_dev, scratch)

    def finish_step(c):
        """the host half of a step: hits (EOS, the caller's criteria), the host state; the mask goes back when a criterion added hits"""
        seqs = state.candidates(c[0], c[1], c[2])
        hits = eos_hits = c[3].to("cpu", torch.bool).view(-1)
        for a in criterion_answers(stopping_criteria if host_crit else (), seqs, d, "cpu"):
            hits = hits | (a if isinstance(a, torch.Tensor) else torch.full_like(hits, a))
        state.advance(hits)
        if host_crit and bool((hits & ~eos_hits).any()):
            c[3].copy_(hits.to(torch.uint8).to(d))

    cand = candidates(first, S, None)
    host_crit = stopping_criteria is not None and len(stopping_criteria) > 0
    if model.model.precision == "fp32" or R > 8:
        use_graph = None                                     # the GEMV decode session: 16-bit storage, <= 8 rows
    sess = None
    if use_graph is not None:
        sess = DecodeSession(ll, cache, use_graph=bool(use_graph), beams=(B, nb, S, eos, not host_crit), processors=table is not None,
                             **({} if con is None else {"constraints": con[0]}))
        if table is not None:
            sess.proc.copy_(table)
        if con is not None:
            sess.con.copy_(con[1])
    finish_step(cand)
    if sess is not None and not state.done:
        ops.beam_select(*cand, B, nb, tok=sess.tok, parent=sess.parent, running=sess.running)
        sess.begin(sess.tok.clone(), prompt_ids=hist[:, :S] if hist is not None else None)   # (nothing to reorder yet)
    while not state.done:
        if sess is not None:
            sess.step()                                      # forward + candidates (+ select, reorder, pos += 1 without criteria)
            finish_step(sess.cand)
            if host_crit and not state.done:
                sess.beam_tail()
        else:
            tok, parent, running = ops.beam_select(*cand, B, nb, running=running)
            if cache.seq_len > S:                            # the generated positions follow their parents
                ops.kv_beam_reorder(kv_table, cache.k[0], parent, S, cache.seq_len)
                if hist is not None:
                    ops.logits_history_gather(hist, parent, S, cache.seq_len)
            if cache.seq_len + 1 > cache.ctx_max:
                break
            cand = candidates(model.forward(input_ids=tok.to(torch.long)[:, None], past_key_values=cache, use_cache=True).logits[:, -1, :],
                              cache.seq_len, tok)
            finish_step(cand)
    finish(d, sess, poll=False)                              # (beam search has never polled the stream-K hand-off at its end: kept so)
    seq, scores = state.result()
    return seq.to(d), scores
