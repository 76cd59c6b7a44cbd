"""Reference decoding loops with transformers' own logits processors, shared by tests/test_logits_process_cpu.py (where they
are pinned to ``LlamaForCausalLM.generate`` on a tiny CPU Llama) and tests/test_logits_process_gpu.py (where they run on the
device tensors of the HIP forward).  ``step(tokens)`` returns the fp32 logits [R, V] of the last position: ``step(None)`` is
the prefill, ``step(tok)`` feeds one token per row."""
import torch


def hf_processors(repetition_penalty=None, no_repeat_ngram_size=None, min_length=None, min_new_tokens=None, prompt_len=0,
                  eos=None):
    """transformers' LogitsProcessorList in _get_logits_processor's order and under its conditions."""
    from transformers.generation.logits_process import (LogitsProcessorList, MinLengthLogitsProcessor,
                                                        MinNewTokensLengthLogitsProcessor, NoRepeatNGramLogitsProcessor,
                                                        RepetitionPenaltyLogitsProcessor)
    procs = LogitsProcessorList()
    if repetition_penalty is not None and repetition_penalty != 1.0:
        procs.append(RepetitionPenaltyLogitsProcessor(penalty=repetition_penalty))
    if no_repeat_ngram_size is not None and no_repeat_ngram_size > 0:
        procs.append(NoRepeatNGramLogitsProcessor(no_repeat_ngram_size))
    if eos is not None:
        eos_t = torch.tensor([eos] if isinstance(eos, int) else list(eos))
        if min_length is not None and min_length > 0:
            procs.append(MinLengthLogitsProcessor(min_length, eos_t))
        if min_new_tokens is not None and min_new_tokens > 0:
            procs.append(MinNewTokensLengthLogitsProcessor(prompt_len, min_new_tokens, eos_t))
    return procs


def _to(procs, device):
    """The EOS masks of the min-length processors on the scores' device, and the penalty as a 0-dim tensor there: torch
    divides a device tensor by a Python scalar as a multiplication by its reciprocal, by a device tensor it divides (the
    IEEE division HF's penalty specifies, which a host run does either way)."""
    for p in procs:
        if hasattr(p, "eos_token_id") and isinstance(p.eos_token_id, torch.Tensor):
            p.eos_token_id = p.eos_token_id.to(device)
        if hasattr(p, "penalty") and torch.device(device).type != "cpu":
            p.penalty = torch.tensor(float(p.penalty), dtype=torch.float32, device=device)
    return procs


def greedy_loop(step, ids, max_new, procs, eos=None, pad=0):
    """HF's greedy decoding (``_sample`` without sampling): processors over the whole sequence, argmax, finished rows emit
    ``pad``, stop when every row finished or after ``max_new`` tokens."""
    seq = ids.clone()
    logits = step(None)
    _to(procs, logits.device)
    finished = torch.zeros(ids.shape[0], dtype=torch.bool, device=ids.device)
    eos_t = None if eos is None else torch.tensor([eos] if isinstance(eos, int) else list(eos), device=ids.device)
    for i in range(max_new):
        scores = procs(seq, logits.float().clone())
        tok = scores.argmax(-1)
        tok = torch.where(finished, torch.full_like(tok, pad), tok)
        seq = torch.cat([seq, tok[:, None]], dim=1)
        if eos_t is not None:
            finished |= torch.isin(tok, eos_t)
        if bool(finished.all()) or i == max_new - 1:
            break
        logits = step(tok)
    return seq


def beam_loop(step, reorder, ids, nb, max_new, procs, eos=None, pad=0):
    """HF's ``_beam_search``: processors over the running sequences and log_softmax(logits), then + running scores; the top
    K per prompt; valley_amd.beam keeps the hypotheses.  ``step`` runs B * nb rows (the prompts repeated nb times),
    ``reorder(parent)`` makes the model state follow the running beams (absolute parent rows, int64 [R])."""
    from valley_amd.beam import BeamSearch
    B, S = ids.shape
    R = B * nb
    st = BeamSearch(ids, nb, S + max_new, eos_ids=None if eos is None else [eos], pad_token_id=pad)
    logits = step(None)
    dev = logits.device
    _to(procs, dev)
    running = st.initial_running().to(dev)
    while True:
        run_seq = st.run_seq[:, :, :st.cur_len].reshape(R, -1).to(dev)
        lp = procs(run_seq, torch.log_softmax(logits.float(), -1))
        V = lp.shape[-1]
        acc = (lp + running[:, None]).view(B, nb * V)
        score, idx = torch.topk(acc, st.K)
        parent = idx // V + torch.arange(B, device=dev)[:, None] * nb
        st.candidates(score.reshape(-1), (idx % V).reshape(-1), parent.reshape(-1))
        st.advance(st.eos_hits())
        if st.done:
            break
        reorder(st.run_ptr[:, :, st.cur_len - 1 - S].reshape(-1).long().to(dev))
        running = st.run_score.reshape(-1).to(dev)
        logits = step(st.run_seq[:, :, st.cur_len - 1].reshape(R).to(dev))
    seq, sc = st.result()
    return seq, sc
