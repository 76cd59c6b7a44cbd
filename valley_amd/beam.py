"""Host bookkeeping of beam search: the state HF ``generate(num_beams > 1)`` keeps between steps (transformers
generation/utils.py ``_beam_search`` is the specification), fed with the K candidates per prompt that the device selects
(ops.beam_candidates).  The device keeps the running beams themselves (tokens, parent rows, running scores, the reordered
KV cache); the host keeps what only the final answer needs: the back-pointers and running sequences, the finished
hypotheses with their length-penalised scores, and the stopping rules.  Per step it costs one small device-to-host copy
of the candidates ([B, K] scores, tokens, parents, hits).

Every step, in HF's order:
  1. candidates: per prompt the K best continuations, best first (score = running score + log-probability);
  2. hits: EOS (from the device), the caller's stopping criteria over the candidate sequences, and — at the last
     position — every candidate (HF's max-length criterion);
  3. running beams: the nb best of score + hit * (-1e9), stable in candidate order;
  4. finished hypotheses: a candidate in the top nb positions that hits may replace a worse finished one, scored
     score / (generated length) ** length_penalty, unless the prompt is done;
  5. the early-stop heuristic and the loop condition (``early_stopping`` True, False or "never")."""
from __future__ import annotations

from typing import Optional, Sequence

import torch

NEG = -1.0e9                    # HF's score of a beam that must not be chosen


def _take(t: torch.Tensor, idx: torch.Tensor) -> torch.Tensor:
    """t [B, n, ...] -> t[b, idx[b, k], ...] as [B, k, ...]."""
    while idx.dim() < t.dim():
        idx = idx.unsqueeze(-1)
    return torch.take_along_dim(t, idx, dim=1)


def _top(v: torch.Tensor, k: int) -> torch.Tensor:
    """Indices of the k largest values per row, ties to the lower index (a stable descending sort)."""
    return torch.sort(v, dim=1, descending=True, stable=True)[1][:, :k]


class BeamSearch:
    """``input_ids`` int64 [B, S] (the prompts, left padding included); ``max_length`` = S + max_new_tokens."""

    def __init__(self, input_ids: torch.Tensor, num_beams: int, max_length: int, eos_ids: Optional[Sequence[int]] = None,
                 pad_token_id: Optional[int] = None, length_penalty: float = 1.0, early_stopping=False,
                 num_return_sequences: int = 1):
        if early_stopping not in (True, False, "never"):
            raise ValueError(f"early_stopping must be True, False or 'never', got {early_stopping!r}")
        if not 1 <= num_return_sequences <= num_beams:
            raise ValueError(f"num_return_sequences ({num_return_sequences}) must be in [1, num_beams = {num_beams}]")
        ids = input_ids.detach().to("cpu", torch.int64)
        self.B, self.S = ids.shape
        self.nb, self.max_length = int(num_beams), int(max_length)
        if self.max_length <= self.S:
            raise ValueError("beam search needs at least one new token")
        self.eos = [int(e) for e in (eos_ids or [])]
        self.K = max(2, 1 + len(self.eos)) * self.nb
        self.length_penalty, self.early_stopping, self.nrs = float(length_penalty), early_stopping, int(num_return_sequences)
        # HF's fill value of unused positions: the pad token, else the first EOS (a pad id of 0 counts as absent); -1
        # without EOS
        self.fill = (pad_token_id or self.eos[0]) if self.eos else -1
        B, nb, S, T = self.B, self.nb, self.S, self.max_length
        self.run_seq = torch.full((B, nb, T), self.fill, dtype=torch.int64)
        self.run_seq[:, :, :S] = ids[:, None, :]
        self.fin_seq = self.run_seq.clone()
        self.run_score = torch.zeros((B, nb), dtype=torch.float32)
        self.run_score[:, 1:] = NEG
        self.fin_score = torch.full((B, nb), NEG, dtype=torch.float32)
        self.fin = torch.zeros((B, nb), dtype=torch.bool)
        self.improvable = torch.ones((B, 1), dtype=torch.bool)
        self.run_ptr = torch.full((B, nb, T - S), -1, dtype=torch.int32)     # the parent row chosen at every generated step
        self.fin_ptr = self.run_ptr.clone()
        self.cur_len = S
        self.done = False
        self.cand = None                # the current step's candidates (see candidates())

    def initial_running(self) -> torch.Tensor:
        """fp32 [B * nb]: (0, -1e9, ...) per prompt, so that the first step only extends beam 0."""
        return self.run_score.reshape(-1).clone()

    def candidates(self, score: torch.Tensor, token: torch.Tensor, beam: torch.Tensor) -> torch.Tensor:
        """Take this step's candidates, [B * K] each (``beam`` = absolute parent row), and return the candidate sequences
        [B * K, cur_len + 1] over which the caller evaluates its stopping criteria."""
        B, K, nb = self.B, self.K, self.nb
        score = score.detach().to("cpu", torch.float32).view(B, K)
        token = token.detach().to("cpu", torch.int64).view(B, K)
        parent = beam.detach().to("cpu", torch.int64).view(B, K)
        local = parent - torch.arange(B)[:, None] * nb
        if bool(((local < 0) | (local >= nb)).any()):
            raise RuntimeError("beam search: a candidate's parent row lies outside its prompt")
        seq = _take(self.run_seq, local)
        seq[:, :, self.cur_len] = token
        ptr = _take(self.run_ptr, local)
        ptr[:, :, self.cur_len - self.S] = parent.to(torch.int32)
        self.cand = (score, token, seq, ptr)
        return seq[:, :, :self.cur_len + 1].reshape(B * K, -1)

    def eos_hits(self) -> torch.Tensor:
        """bool [B * K]: candidates whose token is an EOS id."""
        tok = self.cand[1]
        return torch.isin(tok, torch.tensor(self.eos, dtype=torch.int64)).reshape(-1) if self.eos else \
            torch.zeros(tok.numel(), dtype=torch.bool)

    def advance(self, hits: torch.Tensor) -> None:
        """Close the step with the final hit mask (bool [B * K]): running beams, finished hypotheses, stop condition."""
        B, K, nb, S = self.B, self.K, self.nb, self.S
        score, _, seq, ptr = self.cand
        hits = hits.detach().to("cpu", torch.bool).view(B, K)
        if self.cur_len + 1 >= self.max_length:
            hits = torch.ones_like(hits)                         # the max-length criterion fires for every candidate
        # running beams of the next step
        v = score + hits.to(torch.float32) * NEG
        keep = _top(v, nb)
        self.run_seq, self.run_score, self.run_ptr = _take(seq, keep), _take(v, keep), _take(ptr, keep)
        # finished hypotheses: only the top nb candidates may finish; a prompt whose hypotheses are full (early_stopping
        # True) or that cannot improve takes no more
        top_nb = torch.zeros(K, dtype=torch.bool)
        top_nb[:nb] = True
        new_fin = hits & top_nb[None, :]
        cand_score = score / ((self.cur_len + 1 - S) ** self.length_penalty)
        full = torch.all(self.fin, dim=1, keepdim=True) & (self.early_stopping is True)
        cand_score = cand_score + full.to(torch.float32) * NEG
        cand_score = cand_score + (~self.improvable).to(torch.float32) * NEG
        cand_score = cand_score + (~new_fin) * NEG
        all_seq = torch.cat((self.fin_seq, seq), dim=1)
        all_score = torch.cat((self.fin_score, cand_score), dim=1)
        all_ptr = torch.cat((self.fin_ptr, ptr), dim=1)
        all_fin = torch.cat((self.fin, new_fin), dim=1)
        best = torch.topk(all_score, k=nb)[1]
        self.fin_seq, self.fin_score = _take(all_seq, best), _take(all_score, best)
        self.fin_ptr, self.fin = _take(all_ptr, best), _take(all_fin, best)
        # next step: can a running beam still beat the worst finished hypothesis?
        self.cur_len += 1
        if self.early_stopping == "never" and self.length_penalty > 0.0:
            best_len = self.max_length - S
        else:
            best_len = self.cur_len - S
        best_running = self.run_score[:, :1] / (best_len ** self.length_penalty)
        worst_fin = torch.where(self.fin, torch.min(self.fin_score, dim=1, keepdim=True)[0], NEG)
        self.improvable = self.improvable & torch.any(best_running > worst_fin, dim=-1, keepdim=True)
        go_on = bool(torch.any(self.improvable))
        go_on &= not (bool(torch.all(self.fin)) and self.early_stopping is True)
        go_on &= not bool(torch.all(hits))
        self.done = not go_on
        self.cand = None

    def result(self):
        """-> (sequences int64 [B * num_return_sequences, L], scores fp32 [B * num_return_sequences]): the best finished
        hypotheses per prompt, cropped to the longest of them and padded with the fill value."""
        n = self.nrs
        seq = self.fin_seq[:, :n].reshape(self.B * n, -1)
        sc = self.fin_score[:, :n].reshape(-1)
        ptr = self.fin_ptr[:, :n].reshape(self.B * n, -1)
        gen = int((ptr + 1).bool().sum(dim=1).max())
        return seq[:, :self.S + gen], sc
