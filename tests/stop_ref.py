"""The scalar walk of include/valley_hip_stop.h in plain Python: what vly_stop_apply computes for one row, from the tables of
a transformers StopStringCriteria (``tables_of``), and the launch's whole effect on tok / state (``apply``)."""
from types import SimpleNamespace

WATCH, PAD_AFTER = 1, 2


def tables_of(crit):
    """A StopStringCriteria's tables as python lists."""
    return SimpleNamespace(emb=crit.embedding_vec.tolist(), ns=len(crit.stop_strings), mvp=int(crit.max_valid_positions),
                           mvel=int(crit.max_valid_end_lens), mtl=int(crit.maximum_token_len), target=crit.target_lens.tolist())


def fires(t, ids, begin: int = 0) -> bool:
    """HF's stop-string test on the token ids ``ids`` (the newest last), never walking in front of index ``begin``."""
    T = len(t.emb)
    row = lambda i: t.emb[T - 1 if i < 0 or i >= T - 1 else i]    # noqa: E731  (HF's clamp to the last, all -1 row)
    new = row(ids[-1])
    prev = [row(i) for i in ids[max(begin, 0):-1][::-1][:t.mtl - 1]]     # newest first, at most maximum_token_len tokens in all
    for s in range(t.ns):
        for e in range(t.mvel):
            cum = new[t.ns * t.mvp + s * t.mvel + e]
            if cum <= 0:
                continue
            if cum >= t.target[s]:
                return True
            for r in prev:
                if cum not in r[s * t.mvp:(s + 1) * t.mvp]:
                    break
                cum += r[-1]
                if cum >= t.target[s]:
                    return True
    return False


def apply(t, tok, hist, pos, rows, state, eos=()):
    """vly_stop_apply over python lists, in place: tok [R], hist [R][ld], pos [R] (the index of each row's last valid history
    entry), rows [R][4], state [R][2]; ``t`` None: no string table."""
    for r in range(len(tok)):
        flags, begin, pad = rows[r][:3]
        if not flags & WATCH:
            continue
        if state[r][0]:
            if flags & PAD_AFTER:
                tok[r] = pad
            continue
        p = pos[r]
        lo = max(begin, 0)
        seen = hist[r][lo:p + 1] if 0 <= p < len(hist[r]) and lo <= p else []     # a position outside the history: the token alone
        if tok[r] in eos or (t is not None and fires(t, seen + [tok[r]])):
            state[r] = [1, p + 1]


class AsCriterion:
    """The reference as a ``stopping_criteria`` callback of HF's ``generate`` (per-row bool tensor)."""

    def __init__(self, crit, begin: int = 0):
        self.t, self.begin = tables_of(crit), begin

    def __call__(self, input_ids, scores, **kw):
        import torch
        return torch.tensor([fires(self.t, row, self.begin) for row in input_ids.tolist()], dtype=torch.bool, device=input_ids.device)
