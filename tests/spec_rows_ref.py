"""Plain-Python statement of the per-sequence draft, acceptance and counter rules of include/valley_hip_spec_rows.h: the rules of
tests/spec_ref.py looped over the sequences, plus what a sequence that is not live gets.  tests/test_spec_rows_cpu.py holds it to
spec_ref; tests/test_spec_rows_gpu.py holds the kernels to it."""
from typing import List, Optional, Sequence

import numpy as np

from tests import spec_ref as SR


def draft_rows(hist: np.ndarray, lengths: Sequence[int], k: int, max_ngram: int, eos: Sequence[int] = (), vocab: int = 0,
               live: Optional[Sequence[int]] = None, lookup: bool = True, draft: Optional[np.ndarray] = None,
               draft_len: Optional[Sequence[int]] = None):
    """What vly_spec_rows_draft leaves -> (draft [B, k], draft_len [B], tok [B, k + 1]).  hist [B, ctx_max]; ``lengths[b]`` known
    tokens (pos + len_add, clamped to [1, ctx_max]).  ``draft`` / ``draft_len``: what the tables held before (kept where the
    kernel does not write: a sequence that is not live keeps its draft row; everything of ``lookup=False``)."""
    B, ctx_max = hist.shape
    d = np.array(draft, dtype=np.int64, copy=True).reshape(B, k) if draft is not None else np.zeros((B, k), dtype=np.int64)
    dl = [int(x) for x in draft_len] if draft_len is not None else [0] * B
    tok = np.zeros((B, k + 1), dtype=np.int64)
    for b in range(B):
        if live is not None and not live[b]:
            dl[b] = 0
            continue
        length = max(1, min(int(lengths[b]), ctx_max))
        if lookup:
            full, n, t = SR.draft_outputs(hist[b], length, k, max_ngram, eos, ctx_max=ctx_max, vocab=vocab)
            d[b], dl[b], tok[b] = full, n, t
        else:
            last = int(hist[b, length - 1])
            n = max(0, min(dl[b], k, ctx_max - length))
            tok[b] = [last] + [int(d[b, i]) if i < n else last for i in range(k)]
    return d.tolist(), dl, tok.tolist()


def accept_rows(am: Sequence[int], draft: np.ndarray, draft_len: Sequence[int], k: int, hist: np.ndarray, pos: Sequence[int],
                stats: np.ndarray, live: Optional[Sequence[int]] = None, emit: Optional[np.ndarray] = None,
                tok: Optional[Sequence[int]] = None):
    """What vly_spec_rows_accept leaves -> (n [B] (None: not live), hist', emit [B, k + 2], tok [B * (k + 1)], stats', pos').
    ``emit`` / ``tok``: the tables' contents before (a sequence that is not live keeps all of its emit row but column 0; only
    tok[b * (k + 1)] of a live sequence is written)."""
    B = hist.shape[0]
    am = np.asarray(am).reshape(B, k + 1)
    h = np.array(hist, copy=True)
    e = np.array(emit, copy=True).reshape(B, k + 2) if emit is not None else np.zeros((B, k + 2), dtype=np.int64)
    t = [int(x) for x in tok] if tok is not None else [0] * (B * (k + 1))
    st = np.array(stats, copy=True).reshape(B, 3)
    p = [int(x) for x in pos]
    ns: List[Optional[int]] = []
    for b in range(B):
        if live is not None and not live[b]:
            e[b, 0] = 0
            ns.append(None)
            continue
        n, hb, eb, tok0, sb, pb = SR.accept(am[b].tolist(), np.asarray(draft).reshape(B, k)[b].tolist(), int(draft_len[b]), k, h[b],
                                            p[b], st[b].tolist())
        h[b], e[b], st[b], p[b] = hb, eb, sb, pb
        t[b * (k + 1)] = tok0
        ns.append(n)
    return ns, h, e.tolist(), t, st.tolist(), p


def counters(pos: Sequence[int], k: int, ctx_max: int) -> List[int]:
    """What vly_spec_rows_counters writes: ctr[b * (k + 1) + j] = clamp(pos[b], 0, ctx_max - 1) + j."""
    return [max(0, min(int(p), ctx_max - 1)) + j for p in pos for j in range(k + 1)]


def dead(pos: int, j: int, ctx_max: int) -> bool:
    """Whether row j of a sequence at ``pos`` lies behind its cache."""
    return max(0, min(int(pos), ctx_max - 1)) + j >= ctx_max
