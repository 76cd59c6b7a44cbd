"""Classifier-free guidance in plain torch: the contract of include/valley_hip_guide.h, shared by tests/test_guide_cpu.py (where
it is pinned to transformers' UnbatchedClassifierFreeGuidanceLogitsProcessor, per call and through ``LlamaForCausalLM.generate``)
and tests/test_guide_gpu.py (where the kernel is held to it exactly and ``generate`` to its loop over the HIP forward's logits)."""
import math

import torch

NEUTRAL, COND, UNCOND = 0, 1, 2
NEG_INF = float("-inf")


def log_softmax_row(x):
    """x - lse of one fp32 row as the header defines it: lse = m + log(sum exp(x - m)) over the non-NaN values, 0 when the maximum
    m is not finite (a row of -inf, a row that holds +inf)."""
    x = x.float()
    real = x[~x.isnan()]
    m = real.max() if real.numel() else torch.tensor(NEG_INF)
    if not torch.isfinite(m):
        return x - 0.0
    return x - (m + torch.log(torch.exp(real - m).sum()))


def combine(lc, lu, scale, log_beta=NEG_INF):
    """Row c's new values from the two rows' log-softmaxes lc and lu (fp32 [V]): scale * (lc - lu) + lu, three fp32 roundings in
    HF's order (a scale of exactly 1: lc itself, as HF returns).  lc NaN or -inf -> -inf; else lu NaN or -inf -> lc; whatever is
    still NaN -> lc.  With log_beta > -inf a column
    with lc < max(lc) + log_beta becomes -inf (max over the non-NaN values: the row maximum minus the lse)."""
    lc, lu = lc.float(), lu.float()
    s = torch.tensor(scale, dtype=torch.float32)
    out = s * (lc - lu) + lu if scale != 1 else lc.clone()
    no_u = lu.isnan() | (lu == NEG_INF)
    out = torch.where(no_u | out.isnan(), lc, out)
    dead = lc.isnan() | (lc == NEG_INF)
    out = torch.where(dead, torch.full_like(out, NEG_INF), out)
    if log_beta > NEG_INF:
        real = lc[~lc.isnan()]
        floor = (real.max() if real.numel() else torch.tensor(NEG_INF)) + torch.tensor(log_beta, dtype=torch.float32)
        out = torch.where(lc < floor, torch.full_like(out, NEG_INF), out)
    return out


def valid_partner(table, r, mine, theirs):
    """Row r's partner where (r, partner) is a valid pair of the int32 [R, 4] table, else None."""
    R = table.shape[0]
    if int(table[r, 0]) != mine:
        return None
    p = int(table[r, 1])
    if p < 0 or p >= R or p == r or int(table[p, 0]) != theirs:
        return None
    return p


def log_softmax_rows(x):
    return torch.stack([log_softmax_row(r) for r in x])


def apply(x, table, lsm=log_softmax_rows):
    """vly_guide_apply on the host: x fp32 [R, V], table int32 [R, 4] = {role, partner, scale bits, log_beta bits} -> a new
    tensor; every row but the valid conditional rows keeps its bits.  ``lsm``: the log-softmax of all rows, [R, V] -> [R, V] (the
    device's bits in the exact GPU tests, torch's in the per-call comparison with transformers)."""
    x = x.detach().float().cpu()
    table = table.cpu()
    f = table.contiguous().view(torch.float32)
    out, ls = x.clone(), lsm(x).float().cpu()
    for c in range(x.shape[0]):
        u = valid_partner(table, c, COND, UNCOND)
        if u is not None:
            out[c] = combine(ls[c], ls[u], float(f[c, 2]), float(f[c, 3]))
    return out


def follow(tok, table):
    """vly_guide_follow on the host: every valid unconditional row takes its conditional row's token."""
    out = tok.clone()
    for u in range(tok.shape[0]):
        c = valid_partner(table.cpu(), u, UNCOND, COND)
        if c is not None:
            out[u] = tok[c]
    return out


def table_of(R, pairs):
    """The int32 [R, 4] table of (cond, uncond, scale, beta) pairs, packed here independently of ops.guidance_rows."""
    t = torch.zeros((R, 4), dtype=torch.int32)
    t[:, 1] = -1
    f = t.view(torch.float32)
    f[:, 2], f[:, 3] = 1.0, NEG_INF
    for c, u, scale, beta in pairs:
        t[c, 0], t[c, 1], t[u, 0], t[u, 1] = COND, u, UNCOND, c
        f[c, 2] = scale
        f[c, 3] = math.log(beta) if beta > 0 else NEG_INF
    return t


def guided_scores(lc_logits, lu_logits, scale, beta=0.0):
    """[B, V] guided scores of B conditional rows and their B unconditional rows."""
    lb = math.log(beta) if beta > 0 else NEG_INF
    lb = float(torch.tensor(lb, dtype=torch.float32))
    rows = [combine(log_softmax_row(lc_logits[b].cpu()), log_softmax_row(lu_logits[b].cpu()), scale, lb) for b in range(lc_logits.shape[0])]
    return torch.stack(rows).to(lc_logits.device)


def guided_loop(cstep, ustep, ids, max_new, scale, beta=0.0, back=(), eos=None, pad=0):
    """HF's greedy decoding with the guidance processor in front of ``back`` (transformers' processors behind it, which see the
    conditional sequence): ``cstep`` / ``ustep`` are the steppers of tests/logits_ref.py over the prompt and over the negative
    prompt; both are fed the chosen token.  -> (sequences [B, S + n], margins [B, n]: the gap between the two best final scores
    at every step)."""
    from tests.logits_ref import _to
    seq = ids.clone()
    lc, lu = cstep(None), ustep(None)
    _to(back, lc.device)
    finished = torch.zeros(ids.shape[0], dtype=torch.bool, device=ids.device)
    eos_t = None if eos is None else torch.tensor([eos] if isinstance(eos, int) else list(eos), device=ids.device)
    margins = []
    for i in range(max_new):
        scores = guided_scores(lc.float(), lu.float(), scale, beta)
        for p in back:
            scores = p(seq, scores)
        top = scores.float().topk(2, dim=-1).values
        margins.append((top[:, 0] - top[:, 1]).cpu())
        tok = scores.argmax(-1)
        tok = torch.where(finished, torch.full_like(tok, pad), tok)
        seq = torch.cat([seq, tok[:, None]], dim=1)
        if eos_t is not None:
            finished |= torch.isin(tok, eos_t)
        if bool(finished.all()) or i == max_new - 1:
            break
        lc, lu = cstep(tok), ustep(tok)
    return seq, torch.stack(margins, dim=1)


def same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))
