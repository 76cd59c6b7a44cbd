"""Plain-Python statements of the two rules of prompt-lookup speculative decoding (include/valley_hip_spec.h): the draft lookup
(HF's PromptLookupCandidateGenerator.get_candidates) and the acceptance of a verified draft.  tests/test_spec_cpu.py holds
``draft`` to transformers' generator; tests/test_spec_gpu.py holds the kernels to both."""
from typing import List, Optional, Sequence, Tuple

import numpy as np


def draft(hist: Sequence[int], length: int, k: int, max_ngram: int, eos: Sequence[int] = (), ctx_max: Optional[int] = None,
          vocab: int = 0) -> List[int]:
    """The draft for the ``length`` known tokens hist[:length]: for n = min(max_ngram, length - 1) .. 1 the SMALLEST window
    start i in [0, length - n) whose n tokens equal the last n; the first n with a match decides.  The continuation
    hist[i + n : min(i + n + k, length)] is cropped in front of the first EOS (or id outside [0, vocab), vocab > 0; negative
    ids always); an empty crop ends the search.  With ``ctx_max`` the draft is capped at ctx_max - length tokens."""
    h = [int(t) for t in hist[:length]]
    out: List[int] = []
    for n in range(min(max_ngram, length - 1), 0, -1):
        tail = h[length - n:]
        hit = next((i for i in range(length - n) if h[i:i + n] == tail), None)
        if hit is None:
            continue
        out = h[hit + n:min(hit + n + k, length)]
        for j, t in enumerate(out):
            if t in eos or t < 0 or (vocab > 0 and t >= vocab):
                out = out[:j]
                break
        break
    if ctx_max is not None:
        out = out[:max(0, ctx_max - length)]
    return out


def draft_outputs(hist: Sequence[int], length: int, k: int, max_ngram: int, eos: Sequence[int] = (), ctx_max: Optional[int] = None,
                  vocab: int = 0) -> Tuple[List[int], int, List[int]]:
    """What vly_spec_draft writes: (draft [k] padded with the last token, draft_len, tok [k + 1])."""
    d = draft(hist, length, k, max_ngram, eos, ctx_max, vocab)
    last = int(hist[length - 1])
    full = d + [last] * (k - len(d))
    return full, len(d), [last] + full


def accept(am: Sequence[int], drafted: Sequence[int], draft_len: int, k: int, hist: np.ndarray, pos: int, stats: Sequence[int]):
    """What vly_spec_accept writes -> (n, hist', emit [k + 2], tok0, stats', pos')."""
    dl = max(0, min(int(draft_len), k, len(hist) - (pos + 1)))          # the draft kernel's clamp: rows that were fed a draft
    n = 0
    while n < dl and int(drafted[n]) == int(am[n]):
        n += 1
    h = np.array(hist, copy=True)
    for j in range(n + 1):
        c = pos + 1 + j
        if 0 <= c < h.shape[0]:
            h[c] = am[j]
    emit = [n + 1] + [int(t) for t in am[:n + 1]] + [-1] * (k - n)
    return n, h, emit, int(am[n]), [stats[0] + 1, stats[1] + dl, stats[2] + n], pos + n + 1


def random_case(g: np.random.Generator):
    """One case of the ranges the generator was compared on: vocabulary 2 .. 6, length 1 .. 39, k 1 .. 7, max_ngram 1 .. 4,
    0 .. 2 EOS ids."""
    V = int(g.integers(2, 7))
    L = int(g.integers(1, 40))
    hist = g.integers(0, V, size=L).tolist()
    k = int(g.integers(1, 8))
    n = int(g.integers(1, 5))
    eos = g.choice(V, size=int(g.integers(0, 3)), replace=False).tolist()
    return hist, k, n, eos
