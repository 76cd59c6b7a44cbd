"""The attention oracle: constructed inputs whose correct attention output is known exactly, the plain fp64 softmax they are
measured against, and the three checks built on them (tests/test_attention_exact_gpu.py drives the HIP kernels through them,
tests/test_attention_exact_cpu.py proves on mutated references that they catch a one-key mistake).

  (a) pointer      K rows are +-1 codes, pairwise distinct inside a (batch, head); query i is GAMMA * code(t(i)).  The target's score
                   exceeds every other visible key's by a gap G (log2 units, after the kernel's scale).  With G >= 160 every other
                   probability underflows to exactly 0 in fp32 (2^-160 is below the smallest subnormal), the target's is
                   exp2(0) = 1 and l = 1: the output row IS V[t(i)], bit for bit, whatever 16-bit data V holds.  G and the
                   distinctness are conditions, computed per case from the operands and asserted.
  (b) invisibility every key / V row a set of queries may NOT see (the future, key_valid == 0, cache rows from kv_len to ctx_max) is
                   replaced; the queries' output rows are bit-identical between the two launches.  A masked key contributes
                   exp2(NEG_BIG - m) * V = 0 exactly and wholly future tiles are skipped, so this holds on any finite data.
  (c) count        q = 0: all visible scores are equal, p = 1, l = n (the number of visible keys); V[j][c] = 1 iff j mod d == c,
                   so the channel sums are exact small integers and the output is count_c / n after one fp32 reciprocal, one
                   multiply and one rounding: within one ulp of the storage type (4 ulps on fp32 outputs).  One key too many or
                   too few moves a channel from k / n to (k +- 1) / (n +- 1), k ~ n / d: tens of percent at any context length.

Everything is a pure function of the case (seeded tables, index arithmetic), on any device: the CPU module asserts the gap and the
distinctness of every GPU case before a GPU ever sees it."""
import functools
import math
from dataclasses import dataclass, field
from typing import Callable, List, Optional

import torch

LOG2E = 1.4426950408889634
SCALE128 = 0.08838834764831845          # 128^-0.5, the constant of attention.hip
G_MIN = 160.0                           # log2 units: exp2(-160) = 0 in fp32 (smallest subnormal 2^-149), expf(-110.9) = 0 as well
G_ROPE_SLACK = 8.0                      # fused decode: the kernel's fp32 rotation may round an element of q one 16-bit ulp away from the
                                        # fp64 one: <= 128 elements x ulp(45) = 0.25 (bf16) x |k| = 1 x 0.1275 = 4.1 log2 units
GAMMA = 32.0
GAMMA_VIT = 64.0
TABLE_ROWS = 8448                       # >= the longest cache (8192 keys) + the per-(batch, head) offsets' wrap
D = 128


# ---------------------------------------------------------------------------------------------------------------------------------
# seeded tables: K[b, h, j] = codes[(j + 131 h + 977 b) % rows], V likewise: a head or batch mix-up points at another row
# ---------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def code_table(d: int, rows: int = TABLE_ROWS) -> torch.Tensor:
    g = torch.Generator(device="cpu").manual_seed(97 + d)
    t = torch.randint(0, 2, (rows, d), generator=g, dtype=torch.int8) * 2 - 1
    # pairwise distinct rows (the condition of check (a)); the per-case gap assertion then bounds every cross-correlation that matters
    assert torch.unique(t, dim=0).shape[0] == rows
    return t


@functools.lru_cache(maxsize=None)
def value_table(d: int, seed: int, rows: int = TABLE_ROWS) -> torch.Tensor:
    """Arbitrary finite data, no zeros (a signed zero would not survive 0 + (-0) * 1), distinct rows."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    t = torch.randn((rows, d), generator=g)
    t[t.abs() < 2.0 ** -6] = 0.75
    return t


def _rows(table: torch.Tensor, B: int, heads: int, n: int, device, shift: int = 0) -> torch.Tensor:
    assert n <= table.shape[0], "cache longer than the code table: rows of a (batch, head) would repeat"
    j = torch.arange(n, device=device)[None, None, :]
    h = torch.arange(heads, device=device)[None, :, None]
    b = torch.arange(B, device=device)[:, None, None]
    return table.to(device)[(j + 131 * h + 977 * b + shift) % table.shape[0]]


def rope_tables(n: int, theta: float = 10000.0):
    inv = 1.0 / (theta ** (torch.arange(0, 128, 2, dtype=torch.float32) / 128))
    ang = torch.arange(n, dtype=torch.float32)[:, None] * inv[None]
    return ang.cos().contiguous(), ang.sin().contiguous()


def rope64(x: torch.Tensor, cos: torch.Tensor, sin: torch.Tensor, inverse: bool = False) -> torch.Tensor:
    """x [..., 128] fp64, cos / sin [..., 64] (the fp32 table rows, as fp64): out[d] = x[d] c - x[d + 64] s, out[d + 64] = x[d + 64] c + x[d] s."""
    c, s = cos.double(), sin.double()
    if inverse:
        s = -s
    lo, hi = x[..., :64], x[..., 64:]
    return torch.cat([lo * c - hi * s, hi * c + lo * s], -1)


# ---------------------------------------------------------------------------------------------------------------------------------
# causal + validity attention over a KV cache (prefill, decode, the fp32 twin, attention_probs)
# ---------------------------------------------------------------------------------------------------------------------------------
@dataclass
class Case:
    """One launch shape.  pasts: one cache length per batch row (prefill: all equal).  pads: left padding per row (keys 0 .. pad - 1
    invalid).  holes: interior keys j > pad with j % 37 == 5 invalid too.  stride_extra: key_valid rows are that much longer than kv_len.
    fused: the entry point rotates / appends the new token itself (S = 1; q | k | v raw)."""
    name: str
    B: int
    S: int
    pasts: List[int]
    heads: int
    ctx_max: int
    pads: List[int] = field(default_factory=list)
    holes: bool = False
    stride_extra: int = 0
    fused: bool = False
    full_valid: bool = False            # key_valid spans ctx_max (the per-row decode entry points require it)

    def __post_init__(self):
        self.pads = list(self.pads) + [0] * (self.B - len(self.pads))
        assert len(self.pasts) == self.B and all(p + self.S <= self.ctx_max for p in self.pasts)
        assert not self.fused or self.S == 1

    @property
    def past(self) -> int:
        assert len(set(self.pasts)) == 1
        return self.pasts[0]

    @property
    def has_valid(self) -> bool:
        return any(self.pads) or self.holes or self.stride_extra > 0 or self.full_valid

    def kv_lens(self):
        return [p + self.S for p in self.pasts]

    def valid_width(self) -> int:
        return self.ctx_max if self.full_valid else max(self.kv_lens()) + self.stride_extra

    def valid_buffer(self, device) -> Optional[torch.Tensor]:
        """uint8 [B, width]: 1 everywhere (the slack beyond kv_len too: a wrong stride then reads ones where zeros belong, and the
        other way round) except the padding and the holes."""
        if not self.has_valid:
            return None
        v = torch.ones((self.B, self.valid_width()), dtype=torch.uint8)
        for b in range(self.B):
            v[b, :self.pads[b]] = 0
            if self.holes:
                j = torch.arange(self.pads[b] + 1, self.kv_lens()[b] - 1)
                v[b, j[j % 37 == 5]] = 0
        return v.to(device)

    def vis(self, valid: Optional[torch.Tensor] = None) -> torch.Tensor:
        """bool [B, S, ctx_max] on the CPU: key j visible to query i of row b."""
        j = torch.arange(self.ctx_max)[None, None, :]
        i = torch.arange(self.S)[None, :, None]
        past = torch.tensor(self.pasts)[:, None, None]
        v = (j <= past + i) & (j < past + self.S)
        vb = self.valid_buffer("cpu") if valid is None else valid.cpu()
        if vb is not None:
            w = min(vb.shape[1], self.ctx_max)
            ok = torch.ones((self.B, self.ctx_max), dtype=torch.bool)
            ok[:, :w] = vb[:, :w].bool()
            v = v & ok[:, None, :]
        return v

    def live_rows(self) -> torch.Tensor:
        """bool [B, S]: query rows with at least one visible key; the others are don't-care.  Only a padded query can be dead."""
        vis = self.vis()
        live = vis.any(-1)
        vb = self.valid_buffer("cpu")
        for b in range(self.B):
            for i in (~live[b]).nonzero().flatten().tolist():
                assert vb is not None and vb[b, self.pasts[b] + i] == 0, "a query that is not padding has no visible key"
        assert bool((live == vis.any(-1)).all())            # (nothing else is excluded)
        return live


@dataclass
class Inputs:
    case: Case
    q: torch.Tensor                       # [B, S, heads, 128]: the ROTATED query the scores are made of (the oracle's view)
    k: torch.Tensor                       # [B, heads, ctx_max, 128] (fused: the new key already in its row, as the oracle rotates it)
    v: torch.Tensor
    valid: Optional[torch.Tensor]
    qkv_raw: Optional[torch.Tensor] = None   # fused entry points: [B, 3 * heads * 128] unrotated q | k | v of the new token
    targets: Optional[torch.Tensor] = None   # (a): int64 [B, S, heads]


def candidates(case: Case, vis_b: torch.Tensor, b: int, i: int) -> List[int]:
    """Where a key can be wrongly excluded, for query i of row b: its own position, the first valid key, key 0, the last and the first key
    of every 64-key tile (these are also the 512-key chunk and every 64-aligned split boundary of the decode kernels)."""
    p = case.pasts[b] + i
    row = vis_b[i]
    nz = row.nonzero().flatten()
    if nz.numel() == 0:
        return []
    c = [p, int(nz[0]), 0, int(nz[-1])]
    for m in range(64, p + 1, 64):
        c += [m - 1, m]
    seen, out, row = set(), [], row.tolist()
    for j in c:
        if 0 <= j <= p and row[j] and j not in seen:
            seen.add(j)
            out.append(j)
    return out


def pick_targets(case: Case, rnd: int = 0) -> torch.Tensor:
    vis = case.vis()
    t = torch.zeros((case.B, case.S, case.heads), dtype=torch.int64)
    for b in range(case.B):
        for i in range(case.S):
            c = candidates(case, vis[b], b, i)
            if c:
                for h in range(case.heads):
                    t[b, i, h] = c[(i + h + b + rnd * case.heads) % len(c)]
    return t


def pointer_rounds(case: Case) -> int:
    """Launches needed for every candidate of every row's last query to be some head's target (not capped: the longest walk is the
    125 candidates of a 4001-key row on one head, 125 launches of an S = 1 kernel)."""
    vis = case.vis()
    longest = max(len(candidates(case, vis[b], b, case.S - 1)) for b in range(case.B))
    return max(1, math.ceil(longest / case.heads))


def _fused_finish(case: Case, q_want: torch.Tensor, k: torch.Tensor, v: torch.Tensor, k_raw: torch.Tensor, v_new: torch.Tensor,
                  self_rows: Optional[torch.Tensor], dtype, device):
    """Fused decode: from the wanted rotated query (fp64 [B, 1, heads, 128]) to the raw q | k | v the kernel is given, and back to the
    rotated 16-bit operands it then forms (rounded as it rounds them).  self_rows [B, heads]: q_raw = GAMMA * k_raw (rotation keeps the
    dot product) where the target is the new key."""
    B, heads = case.B, case.heads
    cos, sin = rope_tables(case.ctx_max)
    pos = torch.tensor(case.pasts)
    c, s = cos[pos][:, None, :].to(device), sin[pos][:, None, :].to(device)           # [B, 1, 64]
    q_raw = rope64(q_want[:, 0].double(), c, s, inverse=True)
    if self_rows is not None:
        q_raw = torch.where(self_rows[:, :, None].to(device), GAMMA * k_raw.double(), q_raw)
    q_raw = q_raw.to(dtype)
    q_rot = rope64(q_raw.double(), c, s).to(dtype)
    k_rot = rope64(k_raw.double(), c, s).to(dtype)
    bi = torch.arange(B, device=device)
    k, v = k.clone(), v.clone()
    k[bi, :, pos.to(device)] = k_rot
    v[bi, :, pos.to(device)] = v_new
    raw = torch.cat([q_raw.reshape(B, -1), k_raw.to(dtype).reshape(B, -1), v_new.reshape(B, -1)], 1).contiguous()
    return q_rot[:, None].contiguous(), k, v, raw


def _new_token(case: Case, dtype, device, count: bool):
    k_raw = _rows(code_table(D), case.B, case.heads, 1, device, shift=4099)[:, :, 0].to(dtype)
    if count:
        pos = torch.tensor(case.pasts, device=device)
        v_new = (torch.arange(D, device=device)[None, None, :] == (pos % D)[:, None, None]).expand(case.B, case.heads, D).to(dtype)
    else:
        v_new = _rows(value_table(D, 11), case.B, case.heads, 1, device, shift=5003)[:, :, 0].to(dtype)
    return k_raw, v_new.contiguous()


def build_pointer(case: Case, dtype, device="cpu", rnd: int = 0) -> Inputs:
    k = _rows(code_table(D), case.B, case.heads, case.ctx_max, device).to(dtype)
    v = _rows(value_table(D, 7), case.B, case.heads, case.ctx_max, device, shift=17).to(dtype)
    t = pick_targets(case, rnd).to(device)
    live = case.live_rows().to(device)
    bi = torch.arange(case.B, device=device)[:, None, None]
    hi = torch.arange(case.heads, device=device)[None, None, :]
    q = GAMMA * k[bi, hi, t].double() * live[:, :, None, None]                          # dead rows: q = 0
    raw = None
    if case.fused:
        k_raw, v_new = _new_token(case, dtype, device, False)
        self_rows = t[:, 0, :] == torch.tensor(case.pasts, device=device)[:, None]
        q, k, v, raw = _fused_finish(case, q, k, v, k_raw, v_new, self_rows, dtype, device)
    inp = Inputs(case, q.to(dtype), k, v, case.valid_buffer(device), raw, t)
    assert_gap(inp)
    return inp


def assert_gap(inp: Inputs) -> float:
    """The condition of check (a), from the operands themselves: for every live (row, query, head) the target's score exceeds every other
    VISIBLE key's by G_MIN log2 units after the kernel's scale (fp64; the prefill operands are integers below 2^24, whose fp32
    products and sums are exact, so the matrix product may run in fp32)."""
    case = inp.case
    kvm = max(case.kv_lens())
    q, k = inp.q.cpu(), inp.k[:, :, :kvm].cpu()
    exact32 = not case.fused
    s = torch.einsum("bihd,bhjd->bihj", q.float(), k.float()).double() if exact32 else torch.einsum("bihd,bhjd->bihj", q.double(), k.double())
    s = s * (SCALE128 * LOG2E)
    vis = case.vis()[:, :, None, :kvm].expand(-1, -1, case.heads, -1)
    t = inp.targets.cpu()
    ts = s.gather(-1, t[..., None])[..., 0]
    other = s.masked_fill(~vis, -math.inf).scatter(-1, t[..., None], -math.inf).amax(-1)
    gap = (ts - other)[case.live_rows()]
    assert bool(vis.gather(-1, t[..., None])[..., 0][case.live_rows()].all()), "a target is not visible"
    g = float(gap.min()) if gap.numel() else math.inf
    need = G_MIN + (G_ROPE_SLACK if case.fused else 0.0)
    assert g >= need, f"{case.name}: gap {g:.1f} < {need}"
    return g


def build_count(case: Case, dtype, device="cpu") -> Inputs:
    k = _rows(code_table(D), case.B, case.heads, case.ctx_max, device).to(dtype)
    j = torch.arange(case.ctx_max, device=device)
    v = (j[:, None] % D == torch.arange(D, device=device)[None, :]).to(dtype).expand(case.B, case.heads, -1, -1).contiguous()
    q = torch.zeros((case.B, case.S, case.heads, D), dtype=dtype, device=device)
    raw = None
    if case.fused:
        k_raw, v_new = _new_token(case, dtype, device, True)
        q, k, v, raw = _fused_finish(case, q.double(), k, v, k_raw, v_new, None, dtype, device)
    return Inputs(case, q, k, v, case.valid_buffer(device), raw)


def build_dense(case: Case, dtype, device="cpu") -> Inputs:
    """(b)'s base launch: ordinary data, a dense softmax row."""
    k = _rows(code_table(D), case.B, case.heads, case.ctx_max, device).to(dtype)
    v = _rows(value_table(D, 7), case.B, case.heads, case.ctx_max, device, shift=17).to(dtype)
    q = (0.5 * _rows(value_table(D, 9), case.B, case.heads, case.S, device, shift=29)).transpose(1, 2).to(dtype).contiguous()
    raw = None
    if case.fused:
        k_raw, v_new = _new_token(case, dtype, device, False)
        q, k, v, raw = _fused_finish(case, q.double(), k, v, k_raw, v_new, None, dtype, device)
    return Inputs(case, q, k, v, case.valid_buffer(device), raw)


def replace_invisible(inp: Inputs, cut: int) -> Inputs:
    """Every K / V row that queries 0 .. cut of a batch row may not see — beyond past + cut, key_valid == 0, kv_len .. ctx_max — replaced:
    K by 8 x the sign pattern of one of those queries (the code that would win outright), V by other finite data."""
    case = inp.case
    dev = inp.k.device
    seen = case.vis()[:, :cut + 1].any(1).to(dev)                                           # [B, ctx_max]
    if case.fused:                                                                         # (the kernel writes the new row itself)
        seen[torch.arange(case.B), torch.tensor(case.pasts)] = True
    sgn = torch.where(inp.q >= 0, 1.0, -1.0).to(inp.k.dtype)                                # [B, S, heads, 128]
    idx = torch.arange(case.ctx_max, device=dev) % (cut + 1)
    k_rep = 8.0 * sgn[:, idx].transpose(1, 2)
    v_rep = _rows(value_table(D, 13), case.B, case.heads, case.ctx_max, dev, shift=41).to(inp.v.dtype)
    m = seen[:, None, :, None]
    return Inputs(case, inp.q, torch.where(m, inp.k, k_rep).contiguous(), torch.where(m, inp.v, v_rep).contiguous(), inp.valid, inp.qkv_raw)


def cut_points(S: int) -> List[int]:
    """Query rows on and around every 16-, 64- and 128-boundary, and the last row."""
    c = {S - 1}
    for m in range(16, S + 16, 16):
        c.update(x for x in (m - 2, m - 1, m) if 0 <= x < S)
    return sorted(c)


def thin_cuts(S: int) -> List[int]:
    """The CPU module's subset (every launch there is an fp64 reference): around the first 16-, 64- and every 128-boundary."""
    c = {S - 1}
    for m in [16, 64] + list(range(128, S + 128, 128)):
        c.update(x for x in (m - 1, m) if 0 <= x < S)
    return sorted(c)


def reference(inp: Inputs, vis: Optional[torch.Tensor] = None, probs: bool = False) -> torch.Tensor:
    """Plain fp64 softmax(q k^T / sqrt(128)) v over the keys of ``vis`` (default: the case's own mask) -> [B, S, heads, 128] fp64 on the
    CPU; rows with no visible key are zeros."""
    case = inp.case
    vis = case.vis(inp.valid) if vis is None else vis
    n = int(vis.any(0).any(0).nonzero().max()) + 1 if bool(vis.any()) else 1
    q, k, v = inp.q.cpu().double(), inp.k[:, :, :n].cpu().double(), inp.v[:, :, :n].cpu().double()
    s = torch.einsum("bihd,bhjd->bhij", q, k) * SCALE128
    m = vis[:, None, :, :n]
    s = s.masked_fill(~m, -math.inf)
    p = torch.softmax(s, -1).masked_fill(~m, 0.0)
    p = torch.nan_to_num(p, nan=0.0)
    if probs:
        return p
    return torch.einsum("bhij,bhjd->bihd", p, v)


# ---- the checks: ``run(inputs) -> [B, S, heads, 128]`` is the kernel under test (or a reference standing in for it) ---------------
def ulp(x: torch.Tensor, dtype) -> torch.Tensor:
    """Spacing of ``dtype`` at the fp64 value x (the normal range; below it, the smallest normal's)."""
    fi = torch.finfo(dtype)
    mant = {torch.bfloat16: 7, torch.float16: 10, torch.float32: 23}[dtype]
    e = torch.floor(torch.log2(x.abs().clamp_min(fi.tiny)))
    return torch.exp2(e - mant)


def bits(x: torch.Tensor) -> torch.Tensor:
    """The integer view of a 16- or 32-bit float tensor: comparisons through it are bit for bit (-0.0 differs from 0.0, NaN from nothing)."""
    return x.contiguous().view({2: torch.int16, 4: torch.int32}[x.element_size()])


def name_key(row: torch.Tensor, vhead: torch.Tensor) -> str:
    hit = (vhead == row[None]).all(-1).nonzero().flatten().tolist()
    return f"V row of key {hit}" if hit else "no single V row"


def check_pointer(case: Case, run: Callable, dtype, device="cpu", rounds: Optional[int] = None) -> None:
    live = case.live_rows()
    for rnd in range(pointer_rounds(case) if rounds is None else rounds):
        inp = build_pointer(case, dtype, device, rnd)
        out = run(inp).cpu()
        bi = torch.arange(case.B)[:, None, None]
        hi = torch.arange(case.heads)[None, None, :]
        want = inp.v.cpu()[bi, hi, inp.targets.cpu()]                                   # [B, S, heads, 128]
        assert out.dtype == want.dtype and out.shape == want.shape, (out.dtype, out.shape)
        bad = (bits(out) != bits(want)).any(-1) & live[:, :, None]
        if bool(bad.any()):
            b, i, h = bad.nonzero()[0].tolist()
            raise AssertionError(f"pointer {case.name} round {rnd}: row b={b} i={i} (position {case.pasts[b] + i}) head {h} should be V of "
                                 f"key {int(inp.targets[b, i, h])}, is {name_key(out[b, i, h], inp.v[b, h].cpu())}; {int(bad.sum())} rows differ")


def check_count(case: Case, run: Callable, dtype, device="cpu", ulps: float = 1.0) -> None:
    inp = build_count(case, dtype, device)
    out = run(inp).cpu().double()
    vis = case.vis().double()                                                             # [B, S, ctx]
    onehot = (torch.arange(case.ctx_max)[:, None] % D == torch.arange(D)[None, :]).double()
    n = vis.sum(-1, keepdim=True)
    want = (vis @ onehot / n.clamp_min(1.0))[:, :, None, :].expand(-1, -1, case.heads, -1)
    live = case.live_rows()[:, :, None, None]
    tol = torch.where(want == 0, torch.zeros_like(want), ulps * ulp(want, dtype))
    bad = ((out - want).abs() > tol) & live
    if bool(bad.any()):
        b, i, h, c = bad.nonzero()[0].tolist()
        raise AssertionError(f"count {case.name}: row b={b} i={i} (position {case.pasts[b] + i}) head {h} channel {c} (keys = {c} mod 128): "
                             f"{float(out[b, i, h, c]):.6g}, want {float(want[b, i, h, c]):.6g} = count / n with n = {int(n[b, i, 0])}; "
                             f"{int(bad.sum())} elements off")


def check_invisible(case: Case, run: Callable, dtype, device="cpu", cuts: Optional[List[int]] = None) -> None:
    base = build_dense(case, dtype, device)
    ref = run(base)
    live = case.live_rows().to(ref.device)
    for cut in (cut_points(case.S) if cuts is None else cuts):
        got = run(replace_invisible(base, cut))
        same = (bits(got[:, :cut + 1]) == bits(ref[:, :cut + 1])).flatten(2).all(-1) | ~live[:, :cut + 1]
        if not bool(same.all()):
            b, i = (~same).nonzero()[0].tolist()
            raise AssertionError(f"invisible {case.name}: row b={b} i={i} (position {case.pasts[b] + i}) changed when the keys beyond "
                                 f"position {case.pasts[b] + cut}, the invalid keys and the cache rows past kv_len were replaced")


# ---- mask mutations: what a subtly wrong kernel would compute ---------------------------------------------------------------------
def _pos(case: Case):
    j = torch.arange(case.ctx_max)[None, None, :]
    i = torch.arange(case.S)[None, :, None]
    past = torch.tensor(case.pasts)[:, None, None]
    return j, past + i, past + case.S


def _ok(case: Case) -> torch.Tensor:
    vb = case.valid_buffer("cpu")
    ok = torch.ones((case.B, case.ctx_max), dtype=torch.bool)
    if vb is not None:
        w = min(vb.shape[1], case.ctx_max)
        ok[:, :w] = vb[:, :w].bool()
    return ok


def mutations(case: Case):
    """name -> mutated visibility, only those the shape can express (the mutated mask differs from the true one on a live row)."""
    vis = case.vis()
    j, p, kv = _pos(case)
    ok = _ok(case)[:, None, :]
    out = {}
    out["causal_plus_one"] = (j <= p + 1) & ok & (j < kv + 1)
    out["causal_minus_one"] = vis & (j <= p - 1)
    out["newest_key_dropped"] = vis & (j != kv - 1)
    pad_last = torch.tensor([max(case.pads[b] - 1, -1) for b in range(case.B)])[:, None, None]
    out["padded_key_let_in"] = vis | ((j == pad_last) & (j <= p))
    kvmax = max(case.kv_lens())
    for step in (64, 512):
        m = (kvmax - 1) // step * step
        if m > 0:
            out[f"key_{m}_at_a_{step}_boundary_dropped"] = vis & (j != m)
    c0 = (kvmax - 1) // 512 * 512 if kvmax > 512 else ((kvmax - 1) // 64 * 64)
    out["sixteen_keys_of_a_chunk_start_dropped"] = vis & ~((j >= c0) & (j < c0 + 16))
    out["key_at_kv_len_counted"] = vis | ((j == kv) & (torch.arange(case.S)[None, :, None] == case.S - 1))
    live = case.live_rows()
    return {k: v for k, v in out.items() if bool(((v != vis).any(-1) & live).any())}


# ---------------------------------------------------------------------------------------------------------------------------------
# ViT attention: F frames x 16 heads x 257 tokens x 64, no mask; qkv [F * 257, 3072] = q | k | v
# ---------------------------------------------------------------------------------------------------------------------------------
VN, VH, VD = 257, 16, 64
VIT_CANDS = [None, 0, 256, 255, 15, 16, 31, 32, 63, 64, 127, 128, 191, 192, 223, 224, 239, 240, 241]     # None: the query's own key


def vit_targets(F: int) -> torch.Tensor:
    i = torch.arange(VN)[None, :, None]
    n = (i + torch.arange(VH)[None, None, :] + 5 * torch.arange(F)[:, None, None]) % len(VIT_CANDS)
    c = torch.tensor([-1 if x is None else x for x in VIT_CANDS])[n]
    return torch.where(c < 0, i.expand_as(c), c)                                           # [F, 257, 16]


def vit_pack(q, k, v) -> torch.Tensor:
    """[F, 257, 16, 64] x 3 -> [F * 257, 3072]."""
    F = q.shape[0]
    return torch.cat([q.reshape(F * VN, 1024), k.reshape(F * VN, 1024), v.reshape(F * VN, 1024)], 1).contiguous()


def vit_unpack(qkv: torch.Tensor):
    F = qkv.shape[0] // VN
    return tuple(qkv[:, 1024 * i:1024 * (i + 1)].reshape(F, VN, VH, VD) for i in range(3))


def vit_codes(F: int, device) -> torch.Tensor:
    return _rows(code_table(VD), F, VH, VN, device).transpose(1, 2)                         # [F, 257, 16, 64] int8


def vit_build_pointer(F: int, dtype, device="cpu"):
    k = vit_codes(F, device).to(dtype)
    v = _rows(value_table(VD, 21), F, VH, VN, device, shift=19).transpose(1, 2).to(dtype)
    t = vit_targets(F).to(device)
    fi = torch.arange(F, device=device)[:, None, None]
    hi = torch.arange(VH, device=device)[None, None, :]
    q = (GAMMA_VIT * k[fi, t, hi].float()).to(dtype)
    # the gap, from the operands (integers below 2^24: exact in fp32), per (frame, head), sixteen frames at a time
    gap = math.inf
    for f0 in range(0, F, 16):
        s = torch.einsum("fihd,fjhd->fhij", q[f0:f0 + 16].float().cpu(), k[f0:f0 + 16].float().cpu())
        tt = t[f0:f0 + 16].cpu().permute(0, 2, 1)[..., None]                                # [f, 16, 257, 1]
        gap = min(gap, float((s.gather(-1, tt)[..., 0] - s.scatter(-1, tt, -math.inf).amax(-1)).min()) * 0.125 * LOG2E)
    assert gap >= G_MIN, f"ViT F={F}: gap {gap:.1f}"
    return vit_pack(q, k, v), v[fi, t, hi], t


def vit_build_count(F: int, dtype, device="cpu"):
    k = vit_codes(F, device).to(dtype)
    v = (torch.arange(VN, device=device)[:, None] % VD == torch.arange(VD, device=device)[None, :]).to(dtype)
    v = v[None, :, None, :].expand(F, VN, VH, VD)
    cnt = torch.full((VD,), 4.0, dtype=torch.float64)
    cnt[0] = 5.0                                                                          # keys 0, 64, 128, 192 and 256
    return vit_pack(torch.zeros_like(k), k, v), cnt / VN


def vit_build_dense(F: int, dtype, device="cpu") -> torch.Tensor:
    q = 0.5 * _rows(value_table(VD, 23), F, VH, VN, device, shift=3).transpose(1, 2)
    v = _rows(value_table(VD, 21), F, VH, VN, device, shift=19).transpose(1, 2)
    return vit_pack(q.to(dtype), vit_codes(F, device).to(dtype), v.to(dtype))


def vit_replace_others(qkv: torch.Tensor, keep: torch.Tensor) -> torch.Tensor:
    """Every (frame, head) NOT in ``keep`` (bool [F, 16]) gets other q | k | v."""
    F = qkv.shape[0] // VN
    dev = qkv.device
    q, k, v = vit_unpack(qkv)
    m = keep.to(dev)[:, None, :, None]
    q2 = 2.0 * _rows(value_table(VD, 25), F, VH, VN, dev, shift=7).transpose(1, 2).to(qkv.dtype)
    k2 = 8.0 * vit_codes(F, dev).flip(1).to(qkv.dtype)
    v2 = _rows(value_table(VD, 27), F, VH, VN, dev, shift=9).transpose(1, 2).to(qkv.dtype)
    return vit_pack(torch.where(m, q, q2), torch.where(m, k, k2), torch.where(m, v, v2))


def vit_keep(F: int) -> torch.Tensor:
    f = torch.arange(F)[:, None]
    h = torch.arange(VH)[None, :]
    return (f * 7 + h * 3) % 5 < 2


def vit_reference(qkv: torch.Tensor, extra_zero_keys: int = 0) -> torch.Tensor:
    """fp64 softmax(q k^T / 8) v per (frame, head) -> [F, 257, 16, 64]; extra_zero_keys: the mutation "the padding (zero K, zero V rows,
    as the kernels' LDS holds them) is counted"."""
    q, k, v = (x.cpu().double() for x in vit_unpack(qkv))
    if extra_zero_keys:
        z = torch.zeros((q.shape[0], extra_zero_keys, VH, VD), dtype=torch.float64)
        k, v = torch.cat([k, z], 1), torch.cat([v, z], 1)
    p = torch.softmax(torch.einsum("fihd,fjhd->fhij", q, k) * 0.125, -1)
    return torch.einsum("fhij,fjhd->fihd", p, v)


def vit_check_pointer(F: int, run: Callable, dtype, device="cpu") -> None:
    qkv, want, t = vit_build_pointer(F, dtype, device)
    out = run(qkv).reshape(F, VN, VH, VD)
    assert out.dtype == want.dtype
    bad = (bits(out) != bits(want)).any(-1)
    if bool(bad.any()):
        f, i, h = bad.nonzero()[0].tolist()
        raise AssertionError(f"ViT pointer F={F}: frame {f} query {i} head {h} should be V of key {int(t[f, i, h])}; {int(bad.sum())} rows differ")


def vit_check_count(F: int, run: Callable, dtype, device="cpu", ulps: float = 1.0) -> None:
    qkv, want = vit_build_count(F, dtype, device)
    out = run(qkv).reshape(F, VN, VH, VD).cpu().double()
    bad = (out - want).abs() > ulps * ulp(want, dtype)
    if bool(bad.any()):
        f, i, h, c = bad.nonzero()[0].tolist()
        raise AssertionError(f"ViT count F={F}: frame {f} query {i} head {h} channel {c}: {float(out[f, i, h, c]):.6g}, want {float(want[c]):.6g} "
                             f"(n = 257; 272 or 288 if the padding is counted); {int(bad.sum())} elements off")


def vit_check_invisible(F: int, run: Callable, dtype, device="cpu") -> None:
    base = vit_build_dense(F, dtype, device)
    keep = vit_keep(F)
    a = run(base).reshape(F, VN, VH, VD)
    b = run(vit_replace_others(base, keep)).reshape(F, VN, VH, VD)
    same = (bits(a) == bits(b)).all(-1).all(1) | ~keep.to(a.device)
    assert bool(same.all()), f"ViT invisible F={F}: (frame, head) {(~same).nonzero()[0].tolist()} changed with the OTHER frames' / heads' q | k | v"


# ---------------------------------------------------------------------------------------------------------------------------------
# delta attention (temporal_delta.hip): nseq x nhead units, one query against T keys, no mask.  q [nseq, H], kv [nseq * T, 2 H] = k | v
# ---------------------------------------------------------------------------------------------------------------------------------
def delta_build_pointer(nseq: int, T: int, H: int, nhead: int, dtype, device="cpu"):
    hd = H // nhead
    g = torch.Generator(device="cpu").manual_seed(1000 + 7 * T + hd)
    k = (torch.randint(0, 2, (nseq, T, nhead, hd), generator=g) * 2 - 1).double()
    v = torch.randn((nseq, T, nhead, hd), generator=g)
    v[v.abs() < 2.0 ** -6] = 0.75
    v = v.to(dtype)
    t = (torch.arange(nseq)[:, None] + 3 * torch.arange(nhead)[None, :]) % T               # [nseq, nhead]
    q = GAMMA * k[torch.arange(nseq)[:, None], t, torch.arange(nhead)[None, :]]            # [nseq, nhead, hd]
    s = torch.einsum("shd,sthd->sht", q, k) * (hd ** -0.5 * LOG2E)
    ts = s.gather(-1, t[..., None])
    gap = float((ts[..., 0] - s.scatter(-1, t[..., None], -math.inf).amax(-1)).min()) if T > 1 else math.inf
    assert gap >= G_MIN, f"delta T={T} hd={hd}: gap {gap:.1f}"
    assert all(torch.unique(k[s0, :, h0], dim=0).shape[0] == T for s0 in range(0, nseq, 7) for h0 in range(nhead))
    want = v[torch.arange(nseq)[:, None], t, torch.arange(nhead)[None, :]].reshape(nseq, H)
    kv = torch.cat([k.to(dtype).reshape(nseq * T, H), v.reshape(nseq * T, H)], 1).contiguous()
    return q.to(dtype).reshape(nseq, H).to(device), kv.to(device), want


def delta_build_count(nseq: int, T: int, H: int, nhead: int, dtype, device="cpu"):
    hd = H // nhead
    k = delta_build_pointer(nseq, T, H, nhead, dtype, "cpu")[1][:, :H]
    v = (torch.arange(T)[:, None] % hd == torch.arange(hd)[None, :]).to(dtype)[None, :, None, :].expand(nseq, T, nhead, hd)
    kv = torch.cat([k, v.reshape(nseq * T, H)], 1).contiguous()
    cnt = torch.zeros(hd, dtype=torch.float64)
    for t in range(T):
        cnt[t % hd] += 1
    want = (cnt / T)[None, None, :].expand(nseq, nhead, hd).reshape(nseq, H)
    return torch.zeros((nseq, H), dtype=dtype, device=device), kv.to(device), want


def delta_reference(q: torch.Tensor, kv: torch.Tensor, T: int, nhead: int, drop_last: bool = False) -> torch.Tensor:
    nseq, H = q.shape
    hd = H // nhead
    k = kv[:, :H].cpu().double().reshape(nseq, T, nhead, hd)
    v = kv[:, H:].cpu().double().reshape(nseq, T, nhead, hd)
    if drop_last:
        k, v = k[:, :-1], v[:, :-1]
    p = torch.softmax(torch.einsum("shd,sthd->sht", q.cpu().double().reshape(nseq, nhead, hd), k) * hd ** -0.5, -1)
    return torch.einsum("sht,sthd->shd", p, v).reshape(nseq, H)


# ---------------------------------------------------------------------------------------------------------------------------------
# the cases (one list for the GPU module and for the CPU module's proofs)
# ---------------------------------------------------------------------------------------------------------------------------------
S_ALL = [1, 15, 16, 17, 63, 64, 65, 127, 128, 129, 200, 256, 257, 336, 520]
PASTS = [0, 1, 63, 64, 100, 1000]
PAD_SETS = [[0], [9, 0], [0, 64, 9], [70, 0, 128], [200, 9, 0], [128, 0]]
DEC_PASTS = [0, 1, 63, 64, 255, 256, 511, 512, 513, 1023, 1024, 1025, 1300, 4000]


def prefill_cases() -> List[Case]:
    """Every S at past = 0, every past at S = 17, 128, 129, and a pruned rest (kv_len = 64, 128, 1001 on the S = 1 kernel ...)."""
    pairs = [(S, 0) for S in S_ALL] + [(S, p) for S in (17, 128, 129) for p in PASTS[1:]]
    pairs += [(64, 64), (1, 63), (1, 1000), (65, 63), (256, 100), (15, 1), (1, 4000), (1, 512), (200, 1000)]
    out = []
    for n, (S, past) in enumerate(pairs):
        kv = past + S
        heads = [1, 3, 3, 40, 3, 1][n % 6]
        if heads == 40 and S > 129:
            heads = 3
        pads = [p for p in PAD_SETS[(n + n // 6) % 6] if p < kv] or [0]
        ctx_max = kv if n % 4 == 1 else kv + [37, 64, 200][n % 3]
        out.append(Case(f"prefill-S{S}-past{past}-h{heads}-B{len(pads)}-ctx{ctx_max}", len(pads), S, [past] * len(pads), heads, ctx_max, pads,
                        holes=(n % 5 == 2 and kv > 80), stride_extra=24 if n % 3 == 0 else 0))
    assert any(c.kv_lens()[0] % 64 == 0 for c in out) and any(c.kv_lens()[0] == c.ctx_max for c in out)
    return out


def decode_uniform_cases() -> List[Case]:
    """One position for the whole launch (host or device side): two rows, the second left-padded up to 600 keys."""
    return [Case(f"decode-past{p}", 2, 1, [p, p], 3, p + 1 if k % 2 else p + 40, [0, min(600, p * 3 // 4)], holes=(k % 3 == 0 and p > 80),
                 fused=True, full_valid=True) for k, p in enumerate(DEC_PASTS)]


def decode_rows_cases() -> List[Case]:
    """Per-row positions, short rows next to long ones: the shapes of the merged launch (8 x 40 and 5 x 32: serving's; 1 x 16)."""
    return [Case("rows-8x40", 8, 1, [1300, 0, 63, 512, 1, 1025, 255, 64], 40, 1408, [600, 0, 9, 200, 0, 70, 128, 0], fused=True, full_valid=True),
            Case("rows-5x32", 5, 1, [4000, 511, 1023, 256, 513], 32, 4096, [0, 200, 600, 0, 64], holes=True, fused=True, full_valid=True),
            Case("rows-1x16", 1, 1, [4000], 16, 4001, [0], fused=True, full_valid=True),
            Case("rows-1x16-short", 1, 1, [1024], 16, 1100, [70], fused=True, full_valid=True)]


F32_PREFILL = [(1, 0), (15, 1), (16, 0), (17, 100), (65, 63), (129, 64), (200, 0)]      # (S, past): the scalar kernel below 16 queries, the MFMA one from 16


def f32_cases() -> List[Case]:
    by = {(c.S, c.pasts[0]): c for c in prefill_cases()}
    return [by[k] for k in F32_PREFILL]


VIT_FRAMES = [1, 17, 129]
DELTA_SHAPES = [(64, 8, 4096, 8), (40, 32, 5120, 8), (33, 1, 1024, 8), (17, 5, 512, 8)]     # (nseq, T, H, nhead): head_dim 512, 640, 128, 64
