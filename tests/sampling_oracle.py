"""The sampling oracle: rows, margins and probes for the token-selection kernels (sampling.hip: argmax_kernel, sample_kernel<REG>).
Host only: nothing here needs a GPU; tests/test_sampling_exact_gpu.py runs the cases through vly_argmax, tests/test_sampling_exact_cpu.py
through a numpy emulation of the kernel and through mutated emulations that must fail.

The kernel returns one token per row, so a kept set is observed through probes.  A row's builder writes fp32 logits from chosen uint32
bit patterns (the four radix digits of a key are set directly) and names the lowest kept token b: the intended kept set is
K = {s >= s_b}, re-derived with ``host_kept`` and asserted equal.  X is the near-miss set, the highest-scoring excluded tokens (at
most 8).  For a probe token t of K u X a draw counter c is searched, by host Philox, at which
  * t's float64 perturbed score s + g beats every other token of K u X by >= 1e-3, and
  * for t in X, the best token of K leads the rest of K by >= 1e-3.
The expected token is t if t is kept, else that best token of K: a wrongly kept token, a wrongly dropped one, a wrong Philox word,
counter or tie rule changes a probe's answer, and every comparison on the GPU side is exact equality of token ids.

Margins, asserted here before anything reaches a kernel:
  * top-p: every cumulative mass that decides membership is >= 1e-4 from p in float64 (the kernel's own error is the 2^-40 truncation
    times N, <= 3e-8 at N = 32768, plus expf's few ulp, about 2.4e-7 relative: 1e-4 is more than 100 times that).  Two masses are
    exact in the kernel's integer arithmetic and exempt: 0 (the maximum's tie group: 0 < p Z always) and, on the ``exact_tail`` row,
    the tail more than 27.8 below the maximum, whose fixed-point mass floor(exp(s - m) 2^40) is 0, so the mass above it is the
    whole of Z and Z < p Z is false for every p < 1;
  * draws: |s| <= 64 on every probed token, so the fp32 evaluation of s + g is within about 1e-5 of float64 (half an ulp at 81 plus
    a few ulp of two logf): the 1e-3 lead is 100 times that.

T = 1 and T = 2 (logits = 2 s, an exact scaling) put the chosen bit patterns into the scores; at T = 0.7 the patterns are the logits
and the scores are whatever the fp32 division gives (the host divides in np.float32, as the kernel does): keys one ulp apart may then
collapse into a tie, which K = {s >= s_b} follows."""
import functools
import zlib
from dataclasses import dataclass, field
from typing import List, Optional

import numpy as np

from tests.test_sampling_cpu import MASK, host_kept, mass_above, philox4x32_10, scores

P_MARGIN = 1e-4
Z_MARGIN = 1e-3
S_MAX = 64.0
HOT = 12.0                      # tokens of K u X within this of the best one are searched; the others are verified per chosen counter
TEMPS = (1.0, 2.0, 0.7)
SENTINEL = -77
CTR_ADD = 3
BUDGET = 200000                 # counters searched per row before the builder is declared unsatisfiable
TINY = 0x00800000               # the smallest normal fp32

_POISON = np.array([np.inf, 3e38, np.nan], dtype=np.float32)


def poison(n: int, start: int = 0) -> np.ndarray:
    """+inf, 3e38, NaN, ... : what every padding column (column N first: +inf) and the guard row hold."""
    return _POISON[(np.arange(n) + start) % 3]


def f32(bits) -> np.ndarray:
    return np.asarray(bits, dtype=np.uint32).view(np.float32)


def key_value(key) -> np.ndarray:
    """The fp32 value of an order-preserving key (sampling.hip okey_value)."""
    key = np.asarray(key, dtype=np.uint32)
    return np.where(key & np.uint32(0x80000000), key & np.uint32(0x7fffffff), ~key).astype(np.uint32).view(np.float32)


@dataclass(eq=False)
class Row:
    name: str
    logits: np.ndarray
    T: float
    k: int = 0
    p: float = 1.0
    b: Optional[int] = None             # the lowest kept token (sampled rows)
    fixed: Optional[int] = None         # fallback and greedy rows: the answer at every seed and counter
    nK: int = 8
    nX: int = 8
    exact_tail: bool = False
    K: Optional[np.ndarray] = None
    X: Optional[np.ndarray] = None
    entries: Optional[list] = None

    @property
    def N(self):
        return len(self.logits)

    @property
    def seed(self):
        raw = self.name.encode()
        return (zlib.crc32(raw) << 32) | zlib.crc32(raw[::-1])


@dataclass(eq=False)
class Entry:
    row: Row
    c: int
    expect: int
    what: str


@dataclass(eq=False)
class Case:
    """One launch: rows of one width and stride; ``null`` is the rows == NULL entry (argmax_kernel)."""
    name: str
    N: int
    ld: int
    offset: int
    entries: List[Entry] = field(default_factory=list)
    null: bool = False


# ---- margins, kept set and near misses ------------------------------------------------------------------------------------------------
def mid_p(logits, T, k, b) -> float:
    """The fp32 p halfway between the mass strictly above token b's tie group and the mass above the next group (over the top-k
    survivors): the cut falls right after b."""
    surv, s = host_kept(logits, T, k, 1.0)
    assert surv[b]
    e = np.where(surv, np.exp(s - s[surv].max()), 0.0)
    q = e / e.sum()
    return float(np.float32(mass_above(s, surv)[b] + q[surv & (s == s[b])].sum() / 2))


def finish(row: Row) -> Row:
    """Derive K and X, assert the builder's kept set against host_kept and both margins."""
    if row.fixed is not None:
        return row
    s = scores(row.logits, row.T)
    row.p = float(np.float32(row.p))
    K = ~np.isnan(s) & (s >= s[row.b])
    keep, _ = host_kept(row.logits, row.T, row.k, row.p)
    assert np.array_equal(keep, K), f"{row.name}: the builder's kept set ({K.sum()}) is not host_kept's ({keep.sum()})"
    row.K = K
    if 0 < row.p < 1:
        surv, _ = host_kept(row.logits, row.T, row.k, 1.0)
        sel = surv & np.isfinite(s)
        ma = mass_above(s, surv)[sel]
        exempt = ma == 0.0
        if row.exact_tail:
            tail = s[sel] - s[sel].max() < -27.8
            assert tail.any() and not K[sel][tail].any() and (np.exp(s[sel][tail] - s[sel].max() + 1e-5) * 2.0 ** 40 < 1).all(), row.name
            exempt |= tail
        d = np.abs(ma - row.p)
        assert (exempt | (d >= P_MARGIN)).all(), f"{row.name}: a top-p mass is {d[~exempt].min():.2e} from p"
    out = np.flatnonzero(~K & np.isfinite(s) & (s >= s[K].max() - HOT))       # a token further down cannot win a draw: no probe sees it
    row.X = out[np.argsort(-s[out], kind="stable")][:row.nX]
    return row


def probe_tokens(row: Row, s) -> np.ndarray:
    """All of X plus the kept tokens next to the boundary (the lowest scores; of a larger tie group, members spread over the row)."""
    kept = np.flatnonzero(row.K & np.isfinite(s))
    near = kept[np.argsort(s[kept], kind="stable")]
    if len(near) > row.nK:
        pool = np.sort(near[s[near] <= s[near[row.nK - 1]]])
        if len(pool) > row.nK:
            pool = pool[np.unique(np.linspace(0, len(pool) - 1, row.nK).round().astype(int))]
        near = pool
    return np.concatenate([row.X, near]).astype(np.int64)


def noise(idx, seed: int, ctrs) -> np.ndarray:
    """float64 Gumbel noise [len(ctrs), len(idx)] of tokens idx: word i & 3 of Philox at counter (i >> 2, c, 0, 0)."""
    idx = np.asarray(idx, dtype=np.uint64)
    ctrs = (np.asarray(ctrs, dtype=np.int64) & MASK).astype(np.uint64)
    words = philox4x32_10((idx[None, :] >> np.uint64(2), ctrs[:, None], 0, 0), (seed & MASK, seed >> 32))
    w = np.stack(np.broadcast_arrays(*words))
    x = w[(idx & np.uint64(3)).astype(np.int64), :, np.arange(len(idx))].T
    u = (2.0 * (x >> np.uint64(9)).astype(np.float64) + 1.0) * 2.0 ** -24
    return -np.log(-np.log(u))


def probes(row: Row) -> List[Entry]:
    if row.entries is not None:
        return row.entries
    finish(row)
    if row.fixed is not None:
        row.entries = [Entry(row, 7, row.fixed, f"{row.name}: fixed answer {row.fixed}")]
        return row.entries
    s = scores(row.logits, row.T)
    cand = np.flatnonzero(row.K | np.isin(np.arange(row.N), row.X))
    cand = cand[np.isfinite(s[cand])]
    top = s[cand].max()
    hot, cold = cand[s[cand] >= top - HOT], cand[s[cand] < top - HOT]
    targets = probe_tokens(row, s)
    assert len(targets) and np.isin(targets, hot).all() and (np.abs(s[targets]) <= S_MAX).all(), row.name
    isK = row.K[hot]
    assert isK.any()
    want, found = set(int(t) for t in targets), {}
    B = int(np.clip(400000 // len(hot), 64, 4096))
    c = CTR_ADD
    while len(found) < len(want):
        assert c < BUDGET, f"{row.name}: no counter for tokens {sorted(want - set(found))}"
        ctrs = np.arange(c, c + B)
        z = s[hot][None, :] + noise(hot, row.seed, ctrs)
        zk = np.where(isK[None, :], z, -np.inf)
        w, wk = z.argmax(1), zk.argmax(1)
        ar = np.arange(B)
        best, bestk = z[ar, w], zk[ar, wk]
        z[ar, w] = -np.inf
        zk[ar, wk] = -np.inf
        ok = (best - z.max(1) >= Z_MARGIN) & (isK[w] | (bestk - zk.max(1) >= Z_MARGIN))
        for j in np.flatnonzero(ok):
            t = int(hot[w[j]])
            if t in want and t not in found:
                if len(cold) and (s[cold] + noise(cold, row.seed, ctrs[j:j + 1])[0]).max() > bestk[j] - Z_MARGIN:
                    continue
                found[t] = (int(ctrs[j]), int(hot[wk[j]]))
        c += B
    row.entries = [Entry(row, found[t][0], found[t][1],
                         f"{row.name}: token {t} ({'kept' if row.K[t] else 'near miss'}) at c = {found[t][0]}") for t in sorted(found)]
    return row.entries


def make_case(name, rows, ld=None, offset=0, null=False) -> Case:
    N = rows[0].N
    assert all(r.N == N for r in rows)
    case = Case(name, N, N if ld is None else ld, offset, null=null)
    for r in rows:
        case.entries += probes(r)
    return case


def layout(case: Case):
    """What a launch needs: the distinct rows [U, N], each entry's row index and its parameters."""
    uniq, where, index = [], {}, []
    for e in case.entries:
        if id(e.row) not in where:
            where[id(e.row)] = len(uniq)
            uniq.append(e.row.logits)
        index.append(where[id(e.row)])
    rows = [e.row for e in case.entries]
    return dict(uniq=np.stack(uniq), index=np.array(index), T=[float(r.T) for r in rows], k=[int(r.k) for r in rows],
                p=[float(np.float32(r.p)) for r in rows], seed=[r.seed for r in rows],
                ctr=np.array([e.c - CTR_ADD for e in case.entries], dtype=np.int32), expect=np.array([e.expect for e in case.entries]))


def successor(case: Case, L, i: int) -> np.ndarray:
    """The four floats that follow entry i's row in memory: padding, the next row, or the guard row."""
    if case.ld > case.N:
        return poison(4)
    if i + 1 < len(case.entries):
        return np.concatenate([L["uniq"][L["index"][i + 1]], poison(4)])[:4]
    return poison(4, start=-case.N)


def check(case: Case, got) -> None:
    got = np.asarray(got).astype(np.int64)
    assert got.shape == (len(case.entries),)
    bad = [i for i, e in enumerate(case.entries) if got[i] != e.expect]
    assert not bad, (f"{case.name} (N = {case.N}, ld = {case.ld}, offset {case.offset}): {len(bad)} of {len(case.entries)} probes fail; "
                     + "; ".join(f"[{case.entries[i].what}] got {got[i]}, want {case.entries[i].expect}" for i in bad[:4]))


# ---- row builders ---------------------------------------------------------------------------------------------------------------------
def filler(N, rng) -> np.ndarray:
    """Scores far below every planted one: never a candidate of a probe, and 2e-9 of the mass apiece at most."""
    return rng.uniform(-30.0, -20.0, N).astype(np.float32)


def as_logits(vals, T) -> np.ndarray:
    """T = 1 and T = 2: the planted patterns are the scores (2 s is exact); T = 0.7: they are the logits."""
    vals = np.asarray(vals, dtype=np.float32)
    with np.errstate(over="ignore"):
        return vals * np.float32(2.0) if T == 2.0 else vals.copy()


def spread(N, n, rng, taken=()) -> np.ndarray:
    free = np.setdiff1d(np.arange(N), np.asarray(list(taken), dtype=np.int64))
    return rng.choice(free, size=n, replace=False)


# the k-th and (k+1)-th key first differ in digit d (positive scores near 2; minus 2^31: negative scores near -2)
BOUNDARY = {0: (0xC0000008, 0xBFFFFFF8), 1: (0xC0400008, 0xC03FFFF8), 2: (0xC0408008, 0xC0407FF8), 3: (0xC0408009, 0xC0408008)}
ABOVE = (1, 2, 3, 0x100, 0x200, 0x300, 0x10000, 0x20000, 0x30000, 0x40000, 0x50000)
BELOW = (1, 2, 0x100, 0x200, 0x10000, 0x20000, 0x30000)


def digit_row(name, N, d, negative, pair, T, top_p, rng) -> Row:
    hi, lo = (v - (0x80000000 if negative else 0) for v in BOUNDARY[d])
    vals = filler(N, rng)
    pos = spread(N, len(ABOVE) + len(BELOW), rng, taken=pair)
    vals[pair[0]], vals[pair[1]] = key_value(hi), key_value(lo)
    vals[pos[:len(ABOVE)]] = key_value([hi + a for a in ABOVE])
    vals[pos[len(ABOVE):]] = key_value([lo - a for a in BELOW])
    logits = as_logits(vals, T)
    if top_p:
        return Row(name, logits, T, 0, mid_p(logits, T, 0, pair[0]), b=pair[0])
    return Row(name, logits, T, len(ABOVE) + 1, 1.0, b=pair[0])


N_A = 32767


def pairs_a():
    N = N_A
    return {"element 0": (0, 1), "element N-1": (N - 1, 4096), "last partial group": (4 * (N // 4), 4 * (N // 4) + 1),
            "thread 1023": (4 * 1023 + 1, 4 * (3 * 1024 + 1023) + 2), "register group 7": (4 * (7 * 1024 + 5), 4 * (7 * 1024 + 5) + 3)}


@functools.lru_cache(maxsize=None)
def family_a():
    """top-k boundary at each digit, both signs, the boundary pair at every place the row is split at."""
    rng = np.random.default_rng(101)
    rows = [digit_row(f"A digit {d} {'-' if neg else '+'} pair at {where} T={T}", N_A, d, neg, pair, T, False, rng)
            for d in range(4) for neg in (False, True) for where, pair in pairs_a().items() for T in TEMPS]
    return [make_case("A top-k boundary at each digit", rows)]


def tiny_row(name, N, kind, T, rng) -> Row:
    """Scores around zero in steps of the smallest normal number (kind 'denormal': of 8 denormal steps)."""
    unit = 8 if kind.startswith("denormal") else TINY
    vals = filler(N, rng)
    pos = spread(N, 16, rng)
    up = [unit * j for j in (6, 5, 4, 3, 2, 1)]                               # +6 u ... +1 u
    down = [0x80000000 | unit * j for j in (1, 2, 3, 4, 5, 6)]              # -1 u ... -6 u
    bits = up + [0x00000000, 0x80000000, 0x00000000, 0x80000000] + down    # +0, -0, +0, -0 in the middle
    vals[pos] = f32(bits)
    logits = as_logits(vals, T)
    last_pos, first_zero, last_zero = pos[5], pos[6], pos[9]
    if kind in ("above zero", "denormal"):
        return Row(name, logits, T, 6, 1.0, b=last_pos)
    if kind == "below zero":
        return Row(name, logits, T, 10, 1.0, b=last_zero)
    if kind == "zeros tie":                                                  # the k-th is a zero: all four zeros are one tie group
        return Row(name, logits, T, 7, 1.0, b=first_zero)
    if kind == "top-p above zero":
        return Row(name, logits, T, 0, mid_p(logits, T, 0, last_pos), b=last_pos)
    assert kind == "top-p below zero"
    return Row(name, logits, T, 0, mid_p(logits, T, 0, last_zero), b=last_zero)


B_KINDS = ("above zero", "below zero", "zeros tie", "top-p above zero", "top-p below zero")


@functools.lru_cache(maxsize=None)
def family_b():
    """The key's sign fold: the kept set ends between +tiny and the zeros, between the zeros and -tiny; -0 and +0 are one group."""
    rng = np.random.default_rng(102)
    rows = [tiny_row(f"B {kind} T={T}", 4097, kind, T, rng) for kind in B_KINDS for T in TEMPS]
    return [make_case("B sign fold", rows)]


@functools.lru_cache(maxsize=None)
def family_b_denormal():
    rng = np.random.default_rng(103)
    return [make_case("B denormal scores", [tiny_row(f"B denormal T={T}", 4097, "denormal", T, rng) for T in TEMPS])]


def tie_row(name, N, g, T, rng) -> Row:
    """g equal scores straddle the k-th place: all are kept, |K| = 4 + g > k.  Members lie in every wave's groups."""
    tie = np.unique(np.linspace(0, N - 1, g).round().astype(np.int64))
    assert len(tie) == g
    vals = filler(N, rng)
    other = spread(N, 12, rng, taken=tie)
    key = 0xC0408008
    vals[tie] = key_value(key)
    vals[other[:4]] = key_value([key + a for a in (1, 0x100, 0x10000, 0x20000)])
    vals[other[4:]] = key_value([key - a for a in (1, 2, 0x100, 0x200, 0x10000, 0x20000, 0x30000, 0x40000)])
    few = 4 if g > 100 else 8
    return Row(name, as_logits(vals, T), T, 4 + (g + 1) // 2, 1.0, b=int(tie[0]), nK=few, nX=few)


@functools.lru_cache(maxsize=None)
def family_c():
    """Boundary ties of 2, 65 and 1025 equal scores across the k-th place."""
    rng = np.random.default_rng(104)
    return [make_case("C boundary ties", [tie_row(f"C tie group of {g} T={T}", 4097, g, T, rng) for g in (2, 65, 1025) for T in TEMPS])]


N_D = 261


def edge_row(name, kind, T, rng) -> Row:
    """Every token within 0.5 of the others, so each can win a draw: the lowest kept and the dropped ones are probed."""
    N = N_D
    vals = (2.0 + rng.permutation(N) * (0.5 / N)).astype(np.float32)
    order = np.argsort(vals)
    lowest, second = int(order[0]), int(order[1])
    if kind == "k = 1":
        k, b = 1, int(order[-1])
    elif kind == "k = 1, two maxima":
        vals[order[-2]] = vals[order[-1]]
        k, b = 1, int(order[-1])
    elif kind == "k = N-1":
        k, b = N - 1, second
    elif kind == "k = N":
        k, b = N, lowest
    elif kind == "k = N+5":
        k, b = N + 5, lowest
    elif kind in ("k = candidates", "k = candidates + 1"):
        vals[order[2::3]] = np.nan                                          # a third of the row, never the two lowest
        k = int((~np.isnan(vals)).sum()) + (kind == "k = candidates + 1")
        b = lowest
    elif kind == "k-th is -inf":
        vals[order[:20]] = -np.inf
        k, b = N - 10, int(order[0])                                        # the tie group of -inf is kept whole, and never drawn
    else:
        assert kind == "-inf below the k-th"
        vals[order[:20]] = -np.inf
        k, b = N - 28, int(order[28])                                       # ascending place i is the (N - i)-th largest
    return Row(name, as_logits(vals, T), T, k, 1.0, b=b)


D_KINDS = ("k = 1", "k = 1, two maxima", "k = N-1", "k = N", "k = N+5", "k = candidates", "k = candidates + 1", "k-th is -inf",
           "-inf below the k-th")


@functools.lru_cache(maxsize=None)
def family_d():
    """Edge values of k; k against the number of non-NaN candidates (the status branch); -inf among the candidates."""
    rng = np.random.default_rng(105)
    rows = [edge_row(f"D {kind} T={T}", kind, T, rng) for kind in D_KINDS for T in TEMPS]
    wide = []
    for T in TEMPS:                                                          # k = 1 and top-k off at a re-reading width too
        vals = filler(40001, rng)
        pos = spread(40001, 12, rng)
        vals[pos] = (2.0 + np.arange(12) * 0.04).astype(np.float32)
        wide.append(Row(f"D wide k = 1 T={T}", as_logits(vals, T), T, 1, 1.0, b=int(pos[-1])))
    return [make_case("D edge values of k", rows), make_case("D k = 1 on a wide row", wide)]


def top_p_edge_row(name, N, kind, T, rng) -> Row:
    vals = filler(N, rng)
    pos = spread(N, 12, rng)
    key = 0xC0408008
    vals[pos] = key_value([key - 3 * j for j in range(12)])
    if kind == "p = 1e-6":
        return Row(name, as_logits(vals, T), T, 0, 1e-6, b=int(pos[0]))
    if kind == "p = 1e-6, three maxima":
        vals[pos[1]] = vals[pos[2]] = vals[pos[0]]
        return Row(name, as_logits(vals, T), T, 0, 1e-6, b=int(pos[0]))
    assert kind == "p = 1 - 2^-20"
    vals[np.setdiff1d(np.arange(N), pos)] -= np.float32(12.0)               # the tail: 30 to 40 below the maximum
    return Row(name, as_logits(vals, T), T, 0, 1.0 - 2.0 ** -20, b=int(pos[-1]), nX=0, exact_tail=True)


@functools.lru_cache(maxsize=None)
def family_e():
    """top-p cut at each digit, both signs; p = 1e-6 keeps the maximum's tie group; p = 1 - 2^-20 over a tail of zero fixed-point mass."""
    rng = np.random.default_rng(106)
    N = 4097
    rows = [digit_row(f"E digit {d} {'-' if neg else '+'} T={T}", N, d, neg, tuple(spread(N, 2, rng)), T, True, rng)
            for d in range(4) for neg in (False, True) for T in TEMPS]
    rows += [top_p_edge_row(f"E {kind} T={T}", N, kind, T, rng) for kind in ("p = 1e-6", "p = 1e-6, three maxima", "p = 1 - 2^-20")
             for T in TEMPS]
    return [make_case("E top-p cut at each digit", rows)]


@functools.lru_cache(maxsize=None)
def family_f():
    """top-k then top-p: eight survivors hold 1 % of the row's mass.  Over the survivors the cut keeps five of them; with Z over
    the whole row every survivor's mass above would be < 1 % and all eight would stay."""
    rng = np.random.default_rng(107)
    rows = []
    for N in (4097, 40001):
        for T in TEMPS:
            vals = filler(N, rng)
            pos = spread(N, 2008, rng)
            vals[pos[:8]] = (2.0 + 0.01 * np.arange(8, 0, -1)).astype(np.float32)
            vals[pos[8:]] = (1.0 - rng.permutation(2000) * 1e-4).astype(np.float32)
            logits = as_logits(vals, T)
            b = int(pos[4])
            rows.append(Row(f"F N={N} T={T}", logits, T, 8, mid_p(logits, T, 8, b), b=b))
            whole = mass_above(scores(logits, T), ~np.isnan(logits))[pos[:8]]
            assert (whole < rows[-1].p - P_MARGIN).all()                      # the other reading keeps all eight
    return [make_case("F Z over the top-k survivors", rows[:3]), make_case("F Z over the top-k survivors, wide", rows[3:])]


WIDTHS = (1, 2, 3, 4, 5, 4093, 4096, 4097, 32765, 32767, 32768, 32769, 32772, 65541)


def width_rows(N) -> List[Row]:
    rng = np.random.default_rng(1000 + N)
    edge = [v for j in range(4) for v in (N - 1 - j, j)]
    inner = list(np.linspace(0, N - 1, 8).round().astype(int)[1:-1])
    pos = list(dict.fromkeys(int(v) for v in edge + inner if 0 <= v < N))[:14]
    kept, miss = pos[0::2], pos[1::2]                                        # N-1, N-2, ... kept; 0, 1, ... near misses
    rows = []
    for T in TEMPS:
        vals = filler(N, rng)
        vals[kept] = (2.0 + 0.03 * (1 + np.arange(len(kept)))).astype(np.float32)
        vals[miss] = (2.0 - 0.03 * (1 + np.arange(len(miss)))).astype(np.float32)
        logits = as_logits(vals, T)
        rows.append(Row(f"G N={N} top-k T={T}", logits, T, len(kept), 1.0, b=kept[0]))
        rows.append(Row(f"G N={N} top-p T={T}", logits, T, 0, mid_p(logits, T, 0, kept[0]), b=kept[0]))
    return rows


@functools.lru_cache(maxsize=None)
def family_g(N):
    """One width: contiguous rows, then rows of stride N + 3 that start one float past the allocation (unaligned)."""
    rows = width_rows(N)
    return [make_case(f"G width {N}", rows), make_case(f"G width {N}, ld = N + 3, unaligned base", rows, ld=N + 3, offset=1)]


def fallback_rows(N) -> List[Row]:
    rng = np.random.default_rng(108)
    rows = []
    a, b = N // 4, (3 * N) // 4
    for T in TEMPS:
        v = filler(N, rng)
        v[a] = v[b] = np.inf
        rows.append(Row(f"H maximum +inf T={T}", v, T, 50, 0.9, fixed=a))
    for T in (0.7, 0.5):
        v = filler(N, rng)
        v[a], v[b] = 3.0e38, 3.2e38                                          # both quotients are +inf: the argmax is over the logits
        rows.append(Row(f"H l/T overflows T={T}", v, T, 50, 0.9, fixed=b))
    for T in TEMPS:
        rows.append(Row(f"H all -inf T={T}", np.full(N, -np.inf, dtype=np.float32), T, 50, 0.9, fixed=0))
    return rows


def all_nan_rows(N) -> List[Row]:
    nan = np.full(N, np.nan, dtype=np.float32)
    return [Row(f"H all NaN T={T}", nan, T, 50, 0.9, fixed=0) for T in (0.0,) + TEMPS]


@functools.lru_cache(maxsize=None)
def family_h(N):
    return [make_case(f"H fallbacks N={N}", fallback_rows(N), ld=N + 3)]


@functools.lru_cache(maxsize=None)
def family_h_nan(N):
    rows = all_nan_rows(N)
    return [make_case(f"H all NaN, rows == NULL, N={N}", rows[:1], ld=N + 3, null=True), make_case(f"H all NaN N={N}", rows, ld=N + 3)]


N_GREEDY = 20483                # nv = 5120 float4: the last chunk of 4096 has absent slots, which must never be taken


def greedy_rows() -> List[Row]:
    """argmax_row: the unique maximum in each unrolled slot, at the 4096-float4 chunk seam, in the scalar tail; tied maxima whose
    first occurrence belongs to a later wave; NaNs in front."""
    N = N_GREEDY
    rng = np.random.default_rng(109)
    places = {f"slot {u}": 4 * (u * 1024 + 3) + u for u in range(4)}
    places.update({"16383": 16383, "16384": 16384, "scalar tail": N - 1, "scalar tail start": 4 * (N // 4), "element 0": 0})
    rows = []
    for what, i in places.items():
        v = rng.standard_normal(N).astype(np.float32)
        v[i] = 9.0
        rows.append(Row(f"greedy maximum at {what}", v, 0.0, fixed=i))
    v = rng.standard_normal(N).astype(np.float32)
    first, second = 4 * 1000, 4 * (1024 + 5)                                 # thread 1000 (wave 15) owns the first, thread 5 (wave 0) the second
    v[first] = v[second] = 9.0
    rows.append(Row("greedy tied maxima, first in a later wave", v, 0.0, fixed=first))
    v = rng.standard_normal(N).astype(np.float32)
    v[: N // 3] = np.nan
    v[N // 3 + 7] = 9.0
    rows.append(Row("greedy NaNs in front", v, 0.0, fixed=N // 3 + 7))
    v = np.full(N, -np.inf, dtype=np.float32)
    v[:5] = np.nan
    rows.append(Row("greedy NaN then -inf", v, 0.0, fixed=5))
    v = np.full(N, np.nan, dtype=np.float32)
    v[N - 1] = -np.inf                                                        # the only element: an absent float4 slot claims no index
    rows.append(Row("greedy NaN but a -inf in the scalar tail", v, 0.0, fixed=N - 1))
    return rows


@functools.lru_cache(maxsize=None)
def family_greedy(offset):
    """ld a multiple of four: with offset 0 every row is 16-byte aligned (the float4 path), with offset 1 none is (the scalar loop)."""
    rows = greedy_rows()
    ld = N_GREEDY + 5
    assert ld % 4 == 0
    tag = "unaligned" if offset else "aligned"
    return [make_case(f"greedy rows == NULL, {tag}", rows, ld=ld, offset=offset, null=True),
            make_case(f"greedy T = 0, {tag}", rows, ld=ld, offset=offset)]


FAMILIES = {"A": family_a, "B": family_b, "B denormal": family_b_denormal, "C": family_c, "D": family_d, "E": family_e, "F": family_f,
            **{f"G {N}": functools.partial(family_g, N) for N in WIDTHS},
            "H 4097": functools.partial(family_h, 4097), "H 32769": functools.partial(family_h, 32769),
            "H NaN 4096": functools.partial(family_h_nan, 4096), "H NaN 4097": functools.partial(family_h_nan, 4097), "H NaN 32769": functools.partial(family_h_nan, 32769),
            "greedy aligned": functools.partial(family_greedy, 0), "greedy unaligned": functools.partial(family_greedy, 1)}


def probe_counts():
    """Entries per family (the GPU module prints it)."""
    out = {}
    for name, fam in FAMILIES.items():
        key = name.split()[0]
        out[key] = out.get(key, 0) + sum(len(c.entries) for c in fam())
    return out


# ---- the draw replica of the counter contract ------------------------------------------------------------------------------------------
def replay(logits, T, k, p, seed, c):
    """(token, checkable) of one draw on the host: checkable when the winner leads by >= 1e-3 and no top-p mass is within 1e-4 of p."""
    from tests.test_sampling_cpu import gumbel_noise
    p = float(np.float32(p))
    keep, s = host_kept(logits, T, k, p)
    z = np.where(keep, s + gumbel_noise(len(s), seed, c), -np.inf)
    order = np.argsort(-z, kind="stable")
    ok = len(order) < 2 or z[order[0]] - z[order[1]] >= Z_MARGIN
    if 0 < p < 1:
        surv, _ = host_kept(logits, T, k, 1.0)
        ma = mass_above(s, surv)[surv]
        ok = ok and bool((np.abs(ma - p)[ma > 0] >= P_MARGIN).all())
    return int(order[0]), bool(ok)
