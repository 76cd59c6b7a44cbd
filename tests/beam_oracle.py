"""The beam and processor oracle: exact expectations and constructed cases for the kernels that decide which beams live and which
tokens are banned (beam_rows.inc: beam_rows_kernel<REG, LSE>; beam.hip: beam_select_kernel, kv_reorder_kernel; logits.hip:
logits_process_kernel).  Host only, numpy: tests/test_beam_exact_gpu.py runs the cases through valley_amd.ops and the C ABI,
tests/test_beam_exact_cpu.py through a numpy emulation of the kernels and through mutated emulations that must fail.

Everything the kernels select on is one fp32 operation away from their input, so the host reproduces it to the bit:
  * scored candidates (LSE = false): key = okey(v + running), one fp32 add;
  * candidates over logits (LSE = true) on rows with one maximum m and every other finite value <= m - 120: exp(x - m) is 0 in fp32,
    the sum is 1 and lse = m + logf(1) = m, so key = okey((x - m) + running) (the GPU test asserts lse == m from the device first);
  * the running beams: okey(score + hit * -1e9f) (an FMA of a product with 0 or 1 rounds as the add does);
  * the processors: one IEEE fp32 multiplication or division per distinct in-range id, -inf stores, integer comparisons.
A case builder writes fp32 values from chosen uint32 keys (the four radix digits of a key are set directly) and does not trust its
own construction: every case carries an ``edge`` check that asserts, through ``radix_trace``, that the kernel's two descents reach
the edge the case is named after."""
import os
import re
import zlib
from dataclasses import dataclass, field
from typing import Callable, List, Optional

import numpy as np

from tests.sampling_oracle import f32, key_value, poison

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "valley_amd", "csrc")
SENTINEL = -77
NEG_RUN = np.float32(-1.0e9)            # HF's initial running score of beams 1 and up, and the hit penalty of the selection
ICUT_OFF = 0x7fffffff
WIDTHS = (64, 97, 1024, 1025, 32768, 32769, 66000)


# ---- the constants and the dispatch, read from the source text ------------------------------------------------------------------
def source_constants() -> dict:
    """Every ``constexpr int NAME = expr;`` of beam_rows.inc, beam.hip and logits.hip, evaluated in order."""
    out = {}
    for name in ("beam_rows.inc", "beam.hip", "logits.hip"):
        src = open(os.path.join(CSRC, name)).read()
        for m in re.finditer(r"^constexpr int (\w+) = ([^;]+);", src, re.M):
            out[m.group(1)] = int(eval(m.group(2), {"__builtins__": {}}, dict(out)))
    return out


_C = source_constants()
MAX_K, MAX_NB, ROW_THREADS, REG_J = _C["MAX_K"], _C["MAX_NB"], _C["ROW_THREADS"], _C["REG_J"]
PROC_MAX_V, RO_VECS, RO_MAX_R, G_STAGE, G_POS = _C["PROC_MAX_V"], _C["RO_VECS"], _C["RO_MAX_R"], _C["G_STAGE"], _C["G_POS"]
DISPATCH_TEXT = "if (V <= REG_J * ROW_THREADS)"        # launch_beam_rows: the register form up to and including this width


def kernel_of(V: int) -> str:
    """Which instantiation launch_beam_rows picks: beam_rows_kernel<true, *> ("reg") or <false, *> ("stream")."""
    return "reg" if V <= REG_J * ROW_THREADS else "stream"


def reorder_run(n: int, elem_bytes: int) -> int:
    """kv_reorder_kernel's positions per run for n changed rows."""
    return RO_VECS // (n * (128 * elem_bytes // 16))


# ---- key arithmetic (beam_rows.inc) ---------------------------------------------------------------------------------------------
def okey(s, zero_apart: bool = False, nan_high: bool = False) -> np.ndarray:
    """The order-preserving uint32 key of fp32 values: NaN is 0, below every real value; s + 0.0f makes -0 and +0 share a key.
    ``zero_apart`` / ``nan_high`` are the two mis-keyings the CPU module's mutated emulations use."""
    s = np.asarray(s, dtype=np.float32)
    with np.errstate(invalid="ignore"):
        u = (s if zero_apart else s + np.float32(0.0)).view(np.uint32)
    k = np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000)).astype(np.uint32)
    return np.where(np.isnan(s), np.uint32(0xffffffff if nan_high else 0), k).astype(np.uint32)


okey_value = key_value                    # the fp32 value of a key; key 0 (NaN) gives the bits 0xffffffff


def float_of_key(bits) -> np.ndarray:
    """The fp32 value whose key is ``bits`` (valid for 0x007fffff <= bits <= 0xff800000, bits != 0x7fffffff)."""
    return key_value(bits)


def acc_of(v, run) -> np.ndarray:
    """acc = v + running[r] per row, in fp32."""
    with np.errstate(invalid="ignore", over="ignore"):
        return (np.asarray(v, dtype=np.float32) + np.asarray(run, dtype=np.float32)[:, None]).astype(np.float32)


def lse_scores(x, m) -> np.ndarray:
    """x - lse in fp32 for rows whose lse is exactly m (one maximum, everything else at most m - 120)."""
    with np.errstate(invalid="ignore"):
        return (np.asarray(x, dtype=np.float32) - np.asarray(m, dtype=np.float32)[:, None]).astype(np.float32)


# ---- expectations -------------------------------------------------------------------------------------------------------------------
def expected_candidates(scores, running, B, nb, K, eos, key_fn=okey):
    """Per prompt the K best of okey(scores + running) over its nb * V values, key descending, flat index j * V + t ascending.
    Returns (score as uint32 bits of okey_value(key), token int32, absolute beam int32, hit uint8), each [B * K]."""
    keys = key_fn(acc_of(scores, running))
    R, V = keys.shape
    assert R == B * nb
    flat = keys.reshape(B, nb * V)
    order = np.argsort(~flat, axis=1, kind="stable")[:, :K]             # ~key ascending = key descending; stable = lower index first
    k = np.take_along_axis(flat, order, 1)
    token = (order % V).astype(np.int32)
    beam = (order // V + np.arange(B)[:, None] * nb).astype(np.int32)
    hit = np.isin(token, np.asarray(list(eos), dtype=np.int64)).astype(np.uint8) if len(eos) else np.zeros_like(token, dtype=np.uint8)
    return okey_value(k).view(np.uint32).reshape(-1), token.reshape(-1), beam.reshape(-1), hit.reshape(-1)


def expected_select(score, token, beam, hit, B, nb):
    """Per prompt the nb best of v = score + hit * -1e9f (fp32), by okey(v), stable in candidate order.
    ``score`` as fp32 or uint32 bits.  Returns (tok int32, parent int32, running as uint32 bits), each [B * nb]."""
    score = np.asarray(score)
    s = score.view(np.float32) if score.dtype == np.uint32 else score.astype(np.float32)
    K = s.size // B
    with np.errstate(invalid="ignore", over="ignore"):
        v = (s + np.asarray(hit).astype(np.float32) * NEG_RUN).astype(np.float32).reshape(B, K)
    order = np.argsort(~okey(v), axis=1, kind="stable")[:, :nb]
    pick = lambda a: np.take_along_axis(np.asarray(a).reshape(B, K), order, 1).reshape(-1)      # noqa: E731
    return pick(token).astype(np.int32), pick(beam).astype(np.int32), np.take_along_axis(v, order, 1).reshape(-1).view(np.uint32)


def expected_process(x, hist, length, tok, params, eos, V, lse=None):
    """include/valley_hip_logits.h restated.  x fp32 [R, >= V], hist int32 [R, hist_ld], length[r] the row's length before the
    clamp to hist_ld, tok int32 [R] or None, params rows (penalty, n, min_len), eos ids.  Per row, in order: the append
    (hist[len - 1] = tok when len >= 1), x - lse when ``lse`` is given (log-softmax mode on an exact-lse row), one fp32 s * p
    (s < 0) or s / p per DISTINCT id in [0, V), the n-gram windows, the EOS mask; ids outside [0, V) are skipped everywhere.
    Returns (rows [R, V], history after the append)."""
    x = np.array(x, dtype=np.float32)[:, :V].copy()
    hist = np.array(hist, dtype=np.int32).copy()
    R, hist_ld = hist.shape
    for r in range(R):
        pen, n, m = np.float32(params[r][0]), int(params[r][1]), int(params[r][2])
        ln = min(int(length[r]), hist_ld)
        if tok is not None and ln >= 1:
            hist[r, ln - 1] = tok[r]
        ids = hist[r, :max(ln, 0)].astype(np.int64)
        row = x[r]
        if lse is not None:
            with np.errstate(invalid="ignore"):
                row[:] = row - np.float32(lse[r])
        if pen != np.float32(1.0) and ln > 0:
            inr = ids[(ids >= 0) & (ids < V)]
            for t in np.unique(inr):
                s = row[t]
                with np.errstate(all="ignore"):
                    row[t] = s * pen if s < 0 else s / pen
        if n > 0 and ln >= n:
            last = ids[ln - n + 1:]
            for i in range(ln - n + 1):
                if np.array_equal(ids[i:i + n - 1], last):
                    t = ids[i + n - 1]
                    if 0 <= t < V:
                        row[t] = -np.inf
        if ln < m:
            for t in eos:
                if 0 <= t < V:
                    row[t] = -np.inf
    return x, hist


def expected_reorder(cache, parent, lo, hi):
    """vly_kv_beam_reorder on one [R, heads, ctx_max, 128] cache: index_select semantics over positions [lo, min(hi, ctx_max)); rows
    whose parent is themselves or lies outside [0, R) are left alone."""
    R, _, ctx_max, _ = cache.shape
    out = cache.copy()
    hi = min(hi, ctx_max)
    if hi <= lo:
        return out
    for r, p in enumerate(parent):
        if p != r and 0 <= p < R:
            out[r, :, lo:hi] = cache[p, :, lo:hi]
    return out


# ---- the two descents -----------------------------------------------------------------------------------------------------------------
def level(values, sel, shift, rem, desc):
    """One level of the kernel's ``level``: the 256-bin histogram of digit(v) over the selected values, and the digit (searched from
    255 down if desc) at which the running count reaches rem.  Returns (digit or None, rem inside that digit, histogram)."""
    h = np.bincount((values[sel] >> np.uint32(shift)) & np.uint32(255), minlength=256).astype(np.int64)
    o = h[::-1] if desc else h
    before = np.cumsum(o) - o
    pos = np.flatnonzero((o > 0) & (before < rem) & (rem <= before + o))
    if not len(pos):
        return None, rem, h
    p = int(pos[0])
    return (255 - p if desc else p), int(rem - before[p]), h


@dataclass
class Trace:
    key_digits: list
    thr: int
    rem: int
    n_eq: int
    idx_digits: Optional[list]
    icut: int


def radix_trace(keys, K, index_levels=3, reduce_rem=True) -> Trace:
    """Walk one row's keys as beam_rows_kernel does: four 8-bit levels over the key from the top (the K-th largest key thr, rem of
    its tie group to take, n_eq its size), then, when n_eq > rem, three 8-bit levels over the index bits of the tied elements
    (icut: the rem-th lowest tied index).  ``index_levels`` / ``reduce_rem`` are the CPU module's planted errors."""
    keys = np.asarray(keys, dtype=np.uint32)
    prefix, mask, rem, digits, h = 0, 0, int(K), [], None
    for lev in range(4):
        shift = 24 - 8 * lev
        d, r, h = level(keys, (keys & np.uint32(mask)) == np.uint32(prefix), shift, rem, True)
        d = digits[-1] if d is None else d                                # (a level that finds nothing leaves L.digit as it was)
        digits.append(d)
        prefix |= d << shift
        mask |= 0xff << shift
        rem = r if reduce_rem else rem
    thr, n_eq = prefix, int(h[prefix & 255])
    idx_digits, icut = None, ICUT_OFF
    if n_eq > rem:
        idx = np.flatnonzero(keys == np.uint32(thr)).astype(np.uint32)
        ip, im, irem, idx_digits = 0, 0, rem, []
        for lev in range(index_levels):
            shift = 16 - 8 * lev
            d, r, _ = level(idx, (idx & np.uint32(im | 0xff000000)) == np.uint32(ip), shift, irem, False)
            d = (idx_digits[-1] if idx_digits else 0) if d is None else d
            idx_digits.append(d)
            ip |= d << shift
            im |= 0xff << shift
            irem = r if reduce_rem else irem
        icut = ip
    return Trace(digits, thr, rem, n_eq, idx_digits, icut)


# ---- inputs as the kernels see them ---------------------------------------------------------------------------------------------------
def padded(a, ld) -> np.ndarray:
    """[R + 1, ld] fp32: the rows of ``a`` in columns [0, V), poison (+inf, 3e38, NaN in turn) in the padding columns and in the
    guard row that follows the input."""
    R, V = a.shape
    buf = np.stack([poison(ld, start=r) for r in range(R + 1)])
    buf[:R, :V] = a
    return buf


def _rng(name):
    return np.random.default_rng(zlib.crc32(name.encode()))


@dataclass(eq=False)
class Cand:
    """One launch of the candidates kernels: scores fp32 [B * nb, V] (acc = scores + running), K, the EOS ids."""
    name: str
    scores: np.ndarray
    running: np.ndarray
    B: int
    nb: int
    K: int
    eos: list = field(default_factory=list)
    edge: Optional[Callable] = None          # edge(case, traces): asserts the named edge from the per-row radix traces
    m: Optional[np.ndarray] = None           # exact-lse cases: the logits are ``logits`` and scores = logits - m

    logits: Optional[np.ndarray] = None

    @property
    def V(self):
        return self.scores.shape[1]

    @property
    def R(self):
        return self.B * self.nb

    @property
    def ld(self):
        return self.V + (0 if self.V % 2 == 0 and self.V != 1024 else 3)   # some rows are dense, some are windows of wider rows

    def keys(self):
        return okey(acc_of(self.scores, self.running))

    def traces(self):
        return [radix_trace(k, self.K) for k in self.keys()]

    def check_edge(self):
        tr = self.traces()
        for t in tr:                                                   # what every trace must satisfy
            assert 1 <= t.rem <= t.n_eq, self.name
            assert (t.idx_digits is None) == (t.n_eq == t.rem), self.name
        assert self.edge is not None, self.name
        self.edge(self, tr)
        return tr


def _acc(c):
    return acc_of(c.scores, c.running)


def plant(V, rng, thr, above, tied, span=0x30000):
    """A row of V keys: ``above`` (keys > thr) at random places, thr at the indices ``tied``, everything else below thr within
    ``span`` keys (never the key of -0, which no value produces)."""
    tied = np.asarray(sorted(tied), dtype=np.int64)
    above = np.asarray(above, dtype=np.int64)
    assert (above > thr).all() and len(above) + len(tied) <= V
    lo_floor = 0x80000001 if thr > 0x80000001 else 0x00800000
    span = int(min(span, thr - 1 - lo_floor))
    assert span >= 1, hex(thr)
    keys = (thr - 1 - rng.integers(0, span, size=V)).astype(np.int64)
    keys[keys == 0x7fffffff] -= 1
    free = np.setdiff1d(np.arange(V), tied)
    keys[rng.choice(free, size=len(above), replace=False)] = above
    keys[tied] = thr
    assert ((keys >= 0x007fffff) & (keys <= 0xff800000) & (keys != 0x7fffffff)).all()
    row = float_of_key(keys.astype(np.uint32))
    assert np.array_equal(okey(row), keys.astype(np.uint32))
    return row


DIGIT_THR = {(0, 0x00): 0x00c08080, (0, 0xff): 0xff408080, (1, 0x00): 0xc0008080, (1, 0xff): 0xc0ff8080,
             (2, 0x00): 0xc0800080, (2, 0xff): 0xc080ff80, (3, 0x00): 0xc0808000, (3, 0xff): 0xc08080ff}


def digit_cases(V) -> List[Cand]:
    """Two rows, each a prompt of its own (nb = 1): the whole of every row's list is in the output."""
    out = []
    nb, K = 2, 4
    zeros = np.zeros(nb, dtype=np.float32)
    for (lev, dig), thr in DIGIT_THR.items():
        name = f"digit{lev}_{dig:02x}@{V}"
        rng = _rng(name)
        rows = [plant(V, rng, thr, [thr + (i + 1) * 0x1003 + r for i in range(K - 1)], [int(rng.integers(0, V))]) for r in range(nb)]

        def edge(c, tr, lev=lev, dig=dig, thr=thr):
            for t in tr:
                assert t.thr == thr and t.key_digits[lev] == dig and t.n_eq == 1 and t.rem == 1 and t.idx_digits is None, c.name
        out.append(Cand(name, np.stack(rows), zeros, nb, 1, K, edge=edge))

    name = f"low_digit_only@{V}"
    rng = _rng(name)
    thr = 0xc0808081
    rows = []
    for r in range(nb):
        row = plant(V, rng, thr, [thr + (i + 1) * 0x1003 for i in range(K - 1)], [5 + r])
        row[V - 2 - r] = float_of_key(np.uint32(thr - 1))
        rows.append(row)

    def edge_low(c, tr):
        for k, t in zip(c.keys(), tr):
            s = np.sort(k)[::-1].astype(np.int64)
            assert t.thr == s[c.K - 1] and s[c.K - 1] != s[c.K] and (s[c.K - 1] ^ s[c.K]) < 256, c.name
    out.append(Cand(name, np.stack(rows), zeros, nb, 1, K, edge=edge_low))

    name = f"signed_zero_thr@{V}"
    rng = _rng(name)
    rows = []
    for r in range(nb):
        tied = sorted(rng.choice(V, size=5, replace=False).tolist())
        row = plant(V, rng, 0x80000000, [0xc0000000 + i for i in range(2)], tied)
        row[tied] = np.where(np.arange(5) % 2 == r % 2, np.float32(-0.0), np.float32(0.0))
        rows.append(row)

    def edge_zero(c, tr):
        for row, t in zip(_acc(c), tr):                                  # running = -0.0: v + running keeps the sign of a zero
            z = row[row == 0]
            assert t.thr == 0x80000000 and t.n_eq == 5 and t.rem == 2 and np.signbit(z).any() and not np.signbit(z).all(), c.name
    out.append(Cand(name, np.stack(rows), np.full(nb, -0.0, dtype=np.float32), nb, 1, K, edge=edge_zero))

    name = f"negative_kth@{V}"
    rng = _rng(name)
    thr = int(okey(np.float32(-1.5)))
    rows = [plant(V, rng, thr, [0xbf800000 + i + r for i in range(K - 1)], [int(rng.integers(0, V))]) for r in range(nb)]

    def edge_neg(c, tr):
        for k, t in zip(c.keys(), tr):
            s = np.sort(k)[::-1]
            assert t.thr < 0x80000000 and s[c.K - 2] > 0x80000000 and t.n_eq == 1, c.name
    out.append(Cand(name, np.stack(rows), zeros, nb, 1, K, edge=edge_neg))
    return out


def tie_case(name, V, K, specs, one_prompt=False) -> Cand:
    """One row per (tied indices, rem): K - rem keys above thr, thr at the tied indices, the rest below.  Every row is a prompt of
    its own (nb = 1: the whole of its list is in the output) unless ``one_prompt``."""
    rng = _rng(name)
    thr = 0xc1200000
    rows = [plant(V, rng, thr, [thr + 7 * (i + 1) for i in range(K - rem)], tied) for tied, rem in specs]

    def edge(c, tr):
        for (tied, rem), t in zip(specs, tr):
            tied = sorted(tied)
            assert t.thr == thr and t.n_eq == len(tied) and t.rem == rem, c.name
            if rem < len(tied):
                icut = tied[rem - 1]
                assert t.icut == icut and t.idx_digits == [icut >> 16, (icut >> 8) & 255, icut & 255], c.name
            else:
                assert t.idx_digits is None and t.icut == ICUT_OFF, c.name             # the descent is skipped
    B, nb = (1, len(specs)) if one_prompt else (len(specs), 1)
    return Cand(name, np.stack(rows), np.zeros(len(specs), dtype=np.float32), B, nb, K, edge=edge)


def tie_cases(V) -> List[Cand]:
    K = 8
    blk = [300, 301, 305, 310, 400, 511]
    strad = list(range(250, 262))
    out = [tie_case(f"ties_in_one_block@{V}", V, K, [(blk, 2), (blk, 4)]),
           tie_case(f"ties_straddle_255@{V}", V, K, [(strad, 6), (strad, 7), ([255, 256], 1), ([0, 255, 256, V - 1], 3)]),
           tie_case(f"ties_rem_1@{V}", V, K, [(blk, 1), ([0, V - 1], 1)]),
           tie_case(f"ties_rem_n_eq_minus_1@{V}", V, K, [(blk, 5), ([V - 2, V - 1], 1)]),
           tie_case(f"ties_rem_n_eq@{V}", V, K, [(blk, 6), ([V - 1], 1)])]
    if V > 65536:
        s = list(range(65530, 65542))
        out.append(tie_case(f"ties_straddle_65535@{V}", V, K, [(s, 6), (s, 7), ([65535, 65536], 1), ([255, 65535, 65536, V - 1], 2)]))
    return out


def whole_row_cases(V) -> List[Cand]:
    out = []
    nb, K = 2, 4
    for what, val in (("constant", np.float32(-3.25)), ("all_minus_inf", np.float32(-np.inf)), ("all_nan", np.float32(np.nan))):
        def edge(c, tr):
            for t in tr:
                assert t.n_eq == c.V and t.rem == c.K and t.icut == c.K - 1, c.name
        out.append(Cand(f"whole_row_{what}@{V}", np.full((nb, V), val, dtype=np.float32), np.zeros(nb, dtype=np.float32), nb, 1, K,
                        edge=edge))
    return out


def nan_cases(V) -> List[Cand]:
    nb, K = 2, 4
    out = []
    name = f"nan_row_short_of_k@{V}"
    rng = _rng(name)
    s = (rng.standard_normal((nb, V)) * 3).astype(np.float32)
    s[0] = np.nan
    s[0, [V - 1, 7]] = [1.0, 50.0]                                       # row 0: two real values; row 1 supplies the rest

    def edge_a(c, tr):
        assert tr[0].thr == 0 and tr[0].n_eq == c.V - 2 and tr[0].rem == 2 and tr[0].icut == 1 and tr[1].n_eq == 1, c.name
        assert not np.isnan(f32(expected_candidates(c.scores, c.running, c.B, c.nb, c.K, c.eos)[0])).any(), c.name
    out.append(Cand(name, s, np.zeros(nb, dtype=np.float32), 1, nb, K, edge=edge_a))

    name = f"nan_prompt_short_of_k@{V}"
    s = np.full((nb, V), np.nan, dtype=np.float32)
    s[0, 3], s[1, 0] = -2.0, -1.0

    def edge_b(c, tr):
        sc, tok, beam, _ = expected_candidates(c.scores, c.running, c.B, c.nb, c.K, c.eos)
        assert [t.thr for t in tr] == [0, 0] and sc.tolist()[2:] == [0xffffffff] * 2, c.name       # NaN entries with a NaN score ...
        assert tok.tolist() == [0, 3, 0, 1] and beam.tolist() == [1, 0, 0, 0], c.name               # ... in flat-index order
    out.append(Cand(name, s, np.zeros(nb, dtype=np.float32), 1, nb, K, edge=edge_b))

    name = f"few_finite@{V}"
    rng = _rng(name)
    s = np.full((nb, V), -np.inf, dtype=np.float32)
    s[0, rng.choice(V, 2, replace=False)] = [-1.0, -7.0]
    s[1, rng.choice(V, 3, replace=False)] = [-2.0, -3.0, np.inf]

    def edge_c(c, tr):
        assert [t.thr for t in tr] == [0x007fffff] * 2 and tr[0].n_eq == c.V - 2 and tr[1].n_eq == c.V - 3, c.name
    out.append(Cand(name, s, np.zeros(nb, dtype=np.float32), 1, nb, K, edge=edge_c))
    return out


def collapse_cases(V) -> List[Cand]:
    out = []
    name = f"collapse_both_rows@{V}"
    rng = _rng(name)
    s = (-rng.uniform(0, 200, size=(2, V))).astype(np.float32)

    def edge(c, tr, rows=(0, 1)):
        a = acc_of(c.scores, c.running)
        for r in rows:
            assert len(np.unique(a[r])) <= 8 and tr[r].n_eq > c.V // 16 and tr[r].n_eq > tr[r].rem, c.name    # ulp(1e9) = 64
    out.append(Cand(name, s, np.full(2, NEG_RUN), 1, 2, 4, edge=edge))

    name = f"collapse_first_step_row0_loses@{V}"
    rng = _rng(name)
    s = (-rng.uniform(0, 200, size=(4, V))).astype(np.float32)
    s[0] -= np.float32(3.0e9)                                             # beam 0 (running 0) below every collapsed value

    def edge4(c, tr):
        edge(c, tr, rows=(1, 2, 3))
        assert (expected_candidates(c.scores, c.running, c.B, c.nb, c.K, c.eos)[2] != 0).all(), c.name
    out.append(Cand(name, s, np.array([0, NEG_RUN, NEG_RUN, NEG_RUN], dtype=np.float32), 1, 4, 8, edge=edge4))
    return out


def grid_rows(rng, R, V, steps=40):
    """Log-probability-like rows on a coarse grid: many exact ties inside and across rows."""
    return (-rng.integers(1, steps, size=(R, V)) / 4.0).astype(np.float32)


def limit_cases(V) -> List[Cand]:
    out = []
    if V >= 1025:
        name = f"limit_nb16_k64@{V}"
        rng = _rng(name)
        B = 2
        s = grid_rows(rng, B * 16, V, steps=max(40, V // 3))           # about three of every value in a row
        run = (-rng.integers(0, 3, size=B * 16) / 4.0).astype(np.float32)
        top = expected_candidates(s, run, B, 16, 64, [])[1]
        eos = [int(top[5]), int(top[64 + 9]), V - 1]

        def edge(c, tr):
            assert c.nb == MAX_NB and c.K == MAX_K and c.nb * c.K == ROW_THREADS and len(c.eos) == 3, c.name
            assert 2 * sum(t.n_eq > t.rem for t in tr) >= len(tr), c.name
            beams = expected_candidates(c.scores, c.running, c.B, c.nb, c.K, c.eos)[2]
            assert len(np.unique(beams)) > 8, c.name                      # the merge draws from many lists
        out.append(Cand(name, s, run, B, 16, 64, eos, edge=edge))

    name = f"limit_nb1_k2@{V}"
    rng = _rng(name)
    s = (rng.standard_normal((3, V)) * 3).astype(np.float32)
    out.append(Cand(name, s, np.zeros(3, dtype=np.float32), 3, 1, 2, edge=lambda c, tr: None))
    return out


def k_equals_v_case() -> Cand:
    name = "k_equals_v@64"
    rng = _rng(name)
    s = grid_rows(rng, 4, 64, steps=12)

    def edge(c, tr):
        for k, t in zip(c.keys(), tr):
            assert c.K == c.V == MAX_K and t.thr == k.min() and t.idx_digits is None, c.name     # the whole row is taken
    return Cand(name, s, np.array([0, -0.25, -0.5, 0], dtype=np.float32), 1, 4, 64, edge=edge)


def _beams_are(want):
    def edge(c, tr):
        assert expected_candidates(c.scores, c.running, c.B, c.nb, c.K, c.eos)[2].tolist() == list(want), c.name
    return edge


def merge_cases(V) -> List[Cand]:
    out = []
    nb, K = 4, 8
    name = f"merge_equal_keys@{V}"
    rng = _rng(name)
    s = np.repeat(grid_rows(rng, 1, V, steps=6), nb, axis=0)

    def edge_eq(c, tr):
        _, tok, beam, _ = expected_candidates(c.scores, c.running, c.B, c.nb, c.K, c.eos)
        assert (beam == 0).all() and (np.diff(tok) > 0).all() and tr[0].n_eq > tr[0].rem, c.name  # one key: beam 0's lowest tokens
    out.append(Cand(name, s, np.zeros(nb, dtype=np.float32), 1, nb, K, edge=edge_eq))

    name = f"merge_same_token_across_beams@{V}"
    s = np.full((nb, V), -9.0, dtype=np.float32)
    s[:, V - 3] = -1.0
    s[:, 2] = -1.0

    def edge_tok(c, tr):
        _, tok, beam, _ = expected_candidates(c.scores, c.running, c.B, c.nb, c.K, c.eos)
        assert tok.tolist() == [2, c.V - 3] * 4 and beam.tolist() == [0, 0, 1, 1, 2, 2, 3, 3], c.name
    out.append(Cand(name, s, np.zeros(nb, dtype=np.float32), 1, nb, K, edge=edge_tok))

    name = f"merge_last_beam_wins@{V}"
    rng = _rng(name)
    s = (-rng.uniform(0, 10, size=(nb, V))).astype(np.float32)
    out.append(Cand(name, s, np.array([-50, -50, -50, 0], dtype=np.float32), 1, nb, K, edge=_beams_are([3] * K)))

    for what, val in (("even_shares", lambda j, i: 100.0 - (2 * j + i)), ("strict_interleave", lambda j, i: 100.0 - (nb * i + j))):
        name = f"merge_{what}@{V}"
        rng = _rng(name)
        s = (-rng.uniform(0, 10, size=(nb, V))).astype(np.float32)
        for j in range(nb):
            s[j, rng.choice(V, 2, replace=False)] = [val(j, 0), val(j, 1)]
        want = [0, 0, 1, 1, 2, 2, 3, 3] if what == "even_shares" else [0, 1, 2, 3] * 2
        out.append(Cand(name, s, np.zeros(nb, dtype=np.float32), 1, nb, K, edge=_beams_are(want)))
    return out


def three_prompt_case(V) -> Cand:
    """B = 3: a tie pattern, a collapsed prompt and a NaN prompt in one launch."""
    parts = [tie_case(f"p0@{V}", V, 4, [(list(range(250, 262)), 2), ([255, 256], 1)], one_prompt=True), collapse_cases(V)[0], nan_cases(V)[1]]
    assert all(p.nb == 2 and p.K == 4 for p in parts)

    def edge(c, tr):
        for i, p in enumerate(parts):
            p.edge(p, tr[2 * i:2 * i + 2])
    return Cand(f"three_prompts@{V}", np.concatenate([p.scores for p in parts]), np.concatenate([p.running for p in parts]), 3, 2, 4,
                edge=edge)


def eos_case(V) -> Cand:
    name = f"eos_ids@{V}"
    rng = _rng(name)
    nb, K = 2, 6
    s = (rng.standard_normal((nb, V)) * 3).astype(np.float32)
    _, tok, _, _ = expected_candidates(s, np.zeros(nb, dtype=np.float32), 1, nb, K, [])
    unsel = int(np.setdiff1d(np.arange(V), tok)[0])
    eos = [int(tok[1]), unsel, int(tok[1]), V + 3, int(tok[4])]         # selected, not selected, a duplicate, an id >= V

    def edge(c, tr):
        hit = expected_candidates(c.scores, c.running, c.B, c.nb, c.K, c.eos)[3]
        assert hit[1] == 1 and hit[4] == 1 and 2 <= hit.sum() < c.K, c.name
    return Cand(name, s, np.zeros(nb, dtype=np.float32), 1, nb, K, eos, edge=edge)


def _candidate_cases() -> List[Cand]:
    out = [k_equals_v_case()]
    for V in (97, 32769):
        out += merge_cases(V) + [eos_case(V)]
    for V in (1025, 32769):
        out += digit_cases(V)
    for V in (1025, 32768, 32769, 66000):
        out += tie_cases(V)
    for V in (1024, 32768, 32769, 66000):
        out += whole_row_cases(V)
    for V in (1025, 32769):
        out += nan_cases(V) + [three_prompt_case(V)]
    for V in (1025, 32768, 32769, 66000):
        out += collapse_cases(V)
    for V in (1025, 32769, 66000):
        out += limit_cases(V)
    names = [c.name for c in out]
    assert len(set(names)) == len(names)
    return out


_CASES = {}


def candidate_cases() -> List[Cand]:
    if "cand" not in _CASES:
        _CASES["cand"] = _candidate_cases()
    return _CASES["cand"]


def candidate_case_names() -> List[str]:
    return [c.name for c in candidate_cases()]


def case_by_name(name, which="cand"):
    pool = {"cand": candidate_cases, "lse": lse_cases, "select": select_cases, "proc": process_cases}[which]()
    return next(c for c in pool if c.name == name)


# ---- exact-lse rows ---------------------------------------------------------------------------------------------------------------------
LSE_GAP = 120.0                          # expf(-120) is far below half the smallest fp32 subnormal: exactly 0
LSE_WIDTHS = (1025, 32768, 32769, 66000)


def lse_case(kind, V) -> Cand:
    name = f"lse_{kind}@{V}"
    rng = _rng(name)
    nb, K = 4, 8
    m = np.array([3.5, -2.0, 0.0, 17.25], dtype=np.float32)
    if kind == "distinct":
        x = (m[:, None] - LSE_GAP - rng.uniform(0, 50, size=(nb, V))).astype(np.float32)
        run = np.array([0.0, -0.75, 40.0, -3.0], dtype=np.float32)
    elif kind == "ties":
        x = (m[:, None] - LSE_GAP - rng.integers(0, 6, size=(nb, V)) / 2.0).astype(np.float32)
        x[3, ::5] = -np.inf
        x[2, 11] = np.nan                                                 # a NaN logit is left out of the maximum and of the sum
        run = np.array([0.0, -0.5, 0.5, 0.0], dtype=np.float32)
    else:
        x = (m[:, None] - LSE_GAP - rng.uniform(0, 150, size=(nb, V))).astype(np.float32)
        run = np.array([0, NEG_RUN, NEG_RUN, NEG_RUN], dtype=np.float32)
    top = rng.integers(0, V, size=nb)
    x[np.arange(nb), top] = m
    if kind == "collapse":
        x[0, top[0]] = m[0]
        x[0, np.arange(V) != top[0]] = -np.inf                            # beam 0 keeps its maximum only: the collapsed rows fill the rest
    assert all((np.nan_to_num(np.delete(x[r], top[r]), nan=-np.inf) <= m[r] - LSE_GAP).all() for r in range(nb))

    def edge(c, tr):
        if kind != "distinct":
            assert sum(t.n_eq > t.rem for t in tr) >= 3, c.name
        if kind == "collapse":
            assert (expected_candidates(c.scores, c.running, c.B, c.nb, c.K, c.eos)[2][1:] != 0).all(), c.name
    return Cand(name, lse_scores(x, m), run, 1, nb, K, [int(top[1])], edge=edge, m=m, logits=x)


def lse_cases() -> List[Cand]:
    if "lse" not in _CASES:
        _CASES["lse"] = [lse_case(kind, V) for V in LSE_WIDTHS for kind in ("distinct", "ties", "collapse")]
    return _CASES["lse"]


# ---- the running beams ------------------------------------------------------------------------------------------------------------------
@dataclass(eq=False)
class Select:
    name: str
    score: np.ndarray                     # uint32 bits [B * K]
    token: np.ndarray
    beam: np.ndarray
    hit: np.ndarray
    B: int
    nb: int

    @property
    def K(self):
        return self.score.size // self.B


def select_cases() -> List[Select]:
    if "select" in _CASES:
        return _CASES["select"]
    out = []

    def mk(name, score, hit, B, nb):
        rng = _rng(name)
        n = score.size
        K = n // B
        beam = (rng.integers(0, nb, size=(B, K)) + np.arange(B)[:, None] * nb).reshape(-1).astype(np.int32)
        out.append(Select(name, np.asarray(score, dtype=np.float32).reshape(-1).view(np.uint32), rng.integers(0, 32000, size=n).astype(np.int32),
                          beam, np.asarray(hit, dtype=np.uint8).reshape(-1), B, nb))

    rng = _rng("select")
    desc = lambda B, K: -np.sort(rng.uniform(0, 150, size=(B, K)), axis=1).astype(np.float32)      # noqa: E731
    mk("limit_k64_nb16", desc(2, 64), rng.integers(0, 2, size=(2, 64)), 2, 16)
    s = desc(2, 64)
    mk("every_candidate_hit", s, np.ones((2, 64)), 2, 16)                 # a few values near -1e9: candidate order decides
    assert len(np.unique(s + NEG_RUN)) <= 4
    h = np.ones((1, 64))
    h[0, [63, 40]] = 0
    mk("two_survivors_at_the_end", desc(1, 64), h, 1, 16)
    z = np.array([[-0.0, 0.0, -0.0, 0.0, -1.0, 0.0, -0.0, -2.0]], dtype=np.float32)
    mk("signed_zeros", z, np.zeros((1, 8)), 1, 4)
    s = desc(1, 8)
    s[0, [0, 3]] = np.nan
    mk("nan_ranks_last", s, np.zeros((1, 8)), 1, 4)
    s = desc(1, 8)
    s[0, 1] = np.nan
    mk("nan_taken_when_k_equals_nb", s, np.zeros((1, 8)), 1, 8)
    mk("k_equals_nb", desc(3, 16), rng.integers(0, 2, size=(3, 16)), 3, 16)
    _CASES["select"] = out
    return out


# ---- the processors ---------------------------------------------------------------------------------------------------------------------
@dataclass(eq=False)
class Proc:
    """One launch of vly_logits_process: len = len_dev[r] + len_add per row, clamped to hist_ld."""
    name: str
    V: int
    x: np.ndarray                         # fp32 [R, V]
    hist: np.ndarray                      # int32 [R, hist_ld]
    len_dev: list
    len_add: int
    params: list                          # (penalty, n, min_len) per row
    eos: list
    tok: Optional[np.ndarray] = None
    lse: Optional[np.ndarray] = None      # log-softmax mode on exact-lse rows
    foreign: bool = False                 # ids outside [0, V): transformers' processors cannot express the case

    @property
    def R(self):
        return self.x.shape[0]

    @property
    def ld(self):
        return self.V + 5

    def lengths(self):
        return [d + self.len_add for d in self.len_dev]

    def expected(self):
        return expected_process(self.x, self.hist, self.lengths(), self.tok, self.params, self.eos, self.V, lse=self.lse)


def _rows(rng, R, V):
    x = (rng.standard_normal((R, V)) * 3).astype(np.float32)
    x[:, ::97] = -np.inf
    x[:, 5::1013] = np.nan
    return x


def loop_case(ln, V) -> Proc:
    """A history of ``ln`` ids: a small alphabet (n-grams repeat), ids unique to the second and third trips of the walks, ids in the
    bitmap words 0, 1023, 1024 and the last one, and a repeat of the final bigram that starts beyond position 1024 when ln allows."""
    name = f"len{ln}_v{V}"
    rng = _rng(name)
    R = 2
    words = (V + 31) // 32
    alpha = rng.choice(V, size=40, replace=False)
    hist = alpha[rng.integers(0, 40, size=(R, ln + 3))].astype(np.int32)
    x = _rows(rng, R, V)
    marks = list(dict.fromkeys([w * 32 + 3 for w in (0, 1023, 1024, words - 1) if w < words and w * 32 + 3 < V] + [V - 1]))
    late = [ln - 9, ROW_THREADS + 2] if ln > ROW_THREADS + 40 else []   # penalised in the last trip and in the second one only
    free = np.setdiff1d(np.arange(30, ROW_THREADS - 30), late)
    for r in range(R):
        spots = rng.choice(free, size=len(marks), replace=False)
        spots[len(marks) - len(late):] = late
        hist[r, spots] = marks
        x[r, marks] = [2.5, -1.5, 0.75, -0.25, 6.0][:len(marks)]
        a, b, c = V // 2 + r, V // 3 + r, V // 5 + r                      # (a, b) ends the row; (a, b, c) sits once early, once late
        hist[r, 20:23] = [a, b, c + 7]
        if ln > ROW_THREADS + 40:
            hist[r, ROW_THREADS + 30:ROW_THREADS + 33] = [a, b, c]
        hist[r, ln - 2:ln] = [a, b]
        x[r, [c, c + 7]] = 1.0
    return Proc(name, V, x, hist, [ln - 2] * R, 2, [(1.3, 3, ln + 1), (0.7, 3, ln)], [V - 2, 1])


def process_cases() -> List[Proc]:
    if "proc" in _CASES:
        return _CASES["proc"]
    out = [loop_case(1023, 32768), loop_case(1024, 32769), loop_case(1025, 262144), loop_case(2049, 262144), loop_case(2049, 32769),
           loop_case(2049, 1000)]

    V = 262144
    rng = _rng("one_id")
    x = _rows(rng, 2, V)
    x[0, V - 7], x[1, 33000] = 5.0, -5.0
    out.append(Proc("one_id_2049_times", V, x, np.stack([np.full(2049, V - 7), np.full(2049, 33000)]).astype(np.int32), [2049, 2049], 0,
                    [(2.0, 0, 0), (2.0, 0, 0)], []))

    V = 1000
    rng = _rng("ngram_sizes")
    hist = np.tile(np.array([7, 8, 7, 8, 12, 9, 11], dtype=np.int32), (4, 1))
    out.append(Proc("ngram_n1_nlen_nlen_plus_1", V, _rows(rng, 4, V), hist, [5, 5, 5, 4], 0,
                    [(1.0, 1, 0), (1.0, 5, 0), (1.0, 6, 0), (1.0, 4, 0)], []))
    hist = np.tile(np.array([3, 3, 3, 3, 3, 3], dtype=np.int32), (2, 1))   # n == len on a periodic row: the one window bans its last id
    out.append(Proc("ngram_n_equals_len_periodic", V, _rows(rng, 2, V), hist, [4, 6], 0, [(1.0, 4, 0), (1.0, 6, 0)], []))

    rng = _rng("ngram_tok")
    hist = np.array([[1, 2, 40, 40, 99, 5], [40, 41, 1, 40, 98, 5]], dtype=np.int32)      # position len - 1 holds a stale id
    out.append(Proc("ngram_banned_id_is_the_appended_token", V, _rows(rng, 2, V), hist, [4, 4], 1, [(1.0, 3, 0), (1.2, 2, 0)], [],
                    tok=np.array([40, 41], dtype=np.int32)))

    rng = _rng("foreign")
    big = 2 ** 31 - 1
    hist = np.array([[-200, 7, 9, 1, -200, 7, 0, 0],                      # foreign id inside a prefix that matches: 9 is banned
                     [4, 5, big, 2, 4, 5, 0, 0],                          # foreign id as the banned last id: nothing to ban
                     [V, 6, V, 6, V, 3, 0, 0],                            # id == V: skipped by the penalty, bigram (V, 6) bans nothing new
                     [1, -1, V + 31, big, -2 ** 31, 1, 0, 0]], dtype=np.int32)
    x = _rows(rng, 4, V)
    x[:, :12] = np.arange(1, 13, dtype=np.float32) - 4.5
    out.append(Proc("foreign_ids", V, x, hist, [6, 6, 5, 6], 0, [(1.5, 3, 9), (1.5, 3, 9), (0.5, 2, 9), (2.0, 1, 9)],
                    [-200, V, big, 8, -1], foreign=True))

    rng = _rng("clamp")
    hist = rng.integers(0, 6, size=(2, 12)).astype(np.int32)
    out.append(Proc("len_clamped_to_hist_ld_with_tok", V, _rows(rng, 2, V), hist, [40, 12], 3, [(1.3, 2, 13), (1.3, 2, 12)], [4, 5],
                    tok=np.array([3, 900], dtype=np.int32)))
    out.append(Proc("len_clamped_to_hist_ld", V, _rows(rng, 2, V), hist.copy(), [40, 13], 0, [(1.3, 2, 13), (1.3, 2, 12)], [4, 5]))
    out.append(Proc("len_zero_with_tok", V, _rows(rng, 2, V), hist.copy(), [0, 0], 0, [(1.3, 1, 1), (1.3, 1, 0)], [4, 5],
                    tok=np.array([3, 2], dtype=np.int32)))
    out.append(Proc("min_length_edges", V, _rows(rng, 2, V), hist.copy(), [6, 7], 0, [(1.0, 0, 7), (1.0, 0, 7)], [4, 999, 4]))

    V = 32769
    rng = _rng("lsm")
    m = np.array([4.0, -1.0], dtype=np.float32)
    x = (m[:, None] - LSE_GAP - rng.uniform(0, 30, size=(2, V))).astype(np.float32)
    x[0, 100], x[1, V - 1] = m
    hist = np.array([[100, 5, 5, V - 1, 32768], [V - 1, 5, 6, 5, 6]], dtype=np.int32)
    out.append(Proc("log_softmax_then_penalty", V, x, hist, [5, 5], 0, [(1.5, 0, 0), (0.5, 2, 6)], [9], lse=m))
    names = [c.name for c in out]
    assert len(set(names)) == len(names)
    _CASES["proc"] = out
    return out
