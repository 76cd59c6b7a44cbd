"""A plain-torch reference of vly_constrain_apply's contract (include/valley_hip_constrain.h), stated on python lists — no
packed tables, so the packers of valley_amd.ops are checked through it too — plus transformers' own processors for the same
arguments, in _get_logits_processor's order, and the python trie function that drives PrefixConstrainedLogitsProcessor.
tests/test_constrain_cpu.py pins the reference to transformers (per call, and end to end through ``LlamaForCausalLM.generate``);
tests/test_constrain_gpu.py holds the kernel and generate() to it."""
import torch

from tests import logits_ref

NEG = float("-inf")
MAX_DEPTH = 64
MAX_WORD = 64


def eos_list(eos):
    return [] if eos is None else [int(eos)] if isinstance(eos, int) else [int(e) for e in eos]


def trie_allowed(sequences, generated, eos):
    """The ids allowed behind ``generated`` (the ids since ``begin``): the next ids of every sequence that starts with them,
    plus the EOS ids where a sequence equals them; only the EOS ids for a leaf, a history that left the trie, or more than
    64 generated ids.  Brute force over the sequences: no trie is built."""
    g = [int(t) for t in generated]
    eos = eos_list(eos)
    if len(g) > MAX_DEPTH:
        return sorted(set(eos))
    out, ends = set(), False
    for s in sequences:
        s = [int(t) for t in s]
        if s[:len(g)] == g:
            if len(s) == len(g):
                ends = True
            else:
                out.add(s[len(g)])
    if ends or not out:
        out |= set(eos)
    return sorted(out)


def trie_fn(sequences, begin, eos):
    """HF's ``prefix_allowed_tokens_fn(batch_id, input_ids)`` with the semantics above; ``sequences`` shared by all rows, or
    one list of sequences per row; ``begin`` an int or one per row."""
    per_row = isinstance(sequences[0][0], (list, tuple))

    def fn(batch_id, sent):
        b = begin[batch_id] if isinstance(begin, (list, tuple)) else begin
        return trie_allowed(sequences[batch_id] if per_row else sequences, sent[b:].tolist(), eos)
    return fn


def constrain_row(x, ids, bad_words=None, allowed=None, max_length=0, suppress=None, begin_suppress=None, begin=0, eos=None):
    """One row of the kernel's contract: ``x`` fp32 [V] (returned as a new tensor), ``ids`` the row's history (a list of
    ``len`` ids), each rule None / 0 when off.  A logit no rule bans keeps its bits."""
    x = x.clone()
    V, ids, eos, n = x.shape[0], [int(t) for t in ids], eos_list(eos), len(ids)
    if bad_words is not None:
        for w in dict.fromkeys(tuple(w) for w in bad_words):
            if any(list(w) == [e] for e in eos) or not 0 <= w[-1] < V:
                continue
            L = len(w)
            if L == 1 or (L <= n and ids[n - L + 1:] == list(w[:-1])):
                x[w[-1]] = x[w[-1]] + NEG
    if allowed is not None:
        b = min(max(begin, 0), n)
        keep = torch.zeros(V, dtype=torch.bool)
        ok = [t for t in trie_allowed(allowed, ids[b:], eos) if 0 <= t < V]
        keep[ok] = True
        x = torch.where(keep, x, x + NEG)
    if max_length > 0 and n == max_length - 1:
        x = torch.full_like(x, NEG)
        x[[e for e in eos if 0 <= e < V]] = 0.0
    if suppress is not None:
        x[[t for t in suppress if 0 <= t < V]] = NEG
    if begin_suppress is not None and n == begin:
        x[[t for t in begin_suppress if 0 <= t < V]] = NEG
    return x


def hf_constraint_processors(bad_words_ids=None, allowed=None, max_length=0, suppress_tokens=None, begin_suppress_tokens=None,
                             begin=0, eos=None, front=(), middle=()):
    """transformers' processors for the five rules in _get_logits_processor's order; ``front`` (repetition penalty, n-grams)
    goes before them and ``middle`` (the minimum lengths) between the bad words and the trie, where HF has them."""
    from transformers.generation.logits_process import (ForcedEOSTokenLogitsProcessor, LogitsProcessorList, NoBadWordsLogitsProcessor,
                                                        PrefixConstrainedLogitsProcessor, SuppressTokensAtBeginLogitsProcessor,
                                                        SuppressTokensLogitsProcessor)
    procs = LogitsProcessorList(list(front))
    eos_l = eos_list(eos)
    if bad_words_ids is not None:
        procs.append(NoBadWordsLogitsProcessor(bad_words_ids, eos_l or None))
    procs.extend(middle)
    if allowed is not None:
        procs.append(PrefixConstrainedLogitsProcessor(trie_fn(allowed, begin, eos_l), 1))
    if max_length:
        procs.append(ForcedEOSTokenLogitsProcessor(max_length, eos_l))
    if suppress_tokens is not None:
        procs.append(SuppressTokensLogitsProcessor(suppress_tokens))
    if begin_suppress_tokens is not None:
        procs.append(SuppressTokensAtBeginLogitsProcessor(begin_suppress_tokens, begin))
    return procs


class RefConstraints(list):
    """The reference as a processor: ``self(input_ids, scores)`` applies ``front`` (transformers' repetition penalty / n-gram /
    minimum-length objects) and then ``constrain_row`` to every row — the order of the device step.  ``allowed`` shared or
    per row."""

    def __init__(self, front=(), **rules):
        super().__init__(front)
        self.rules = rules

    def __call__(self, input_ids, scores):
        for p in self:
            scores = p(input_ids, scores)
        rules = dict(self.rules)
        allowed = rules.pop("allowed", None)
        per_row = allowed is not None and isinstance(allowed[0][0], (list, tuple))
        rows = [constrain_row(scores[r].cpu(), input_ids[r].tolist(), allowed=(allowed[r] if per_row else allowed), **rules)
                for r in range(scores.shape[0])]
        return torch.stack(rows).to(scores.device)


def same_values(a, b):
    """Equal values, NaN where NaN (-0.0 == +0.0: HF's ``scores + 0`` loses the sign of a zero)."""
    return torch.equal(a.isnan(), b.isnan()) and torch.equal(torch.where(a.isnan(), 0.0, a), torch.where(b.isnan(), 0.0, b))


def same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


greedy_loop = logits_ref.greedy_loop
