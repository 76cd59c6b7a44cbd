"""The sampling oracle is satisfiable and it bites (tests/sampling_oracle.py; no GPU).  sample_kernel and argmax_row are emulated in
numpy in the kernel's own order — uint32 keys, four 8-bit levels of integer counts and of uint64 floor(exp(s - m) 2^40) masses, the
status / rem / base hand-offs between levels, the Philox word layout, fp32 Gumbel noise, first-index ties; argmax_row per thread
(the float4 path's four unrolled slots and scalar tail, or the unaligned scalar loop), then the wave and block reduction — and the
emulation passes every probe of every family: the rows are satisfiable by the intended algorithm within the oracle's margins.  One
mutation at a time does not: each fails a named probe.

One mutation is read by its meaning, not its letter.  Inside the kernel ``above < p Z`` against ``above <= p Z`` differs only when a
cumulative fixed-point mass equals p Z exactly, which no row that respects the 1e-4 margin can produce; "top-p uses <=" is therefore
the other cut rule it stands for: a token is kept while the mass down to AND INCLUDING its own tie group is <= p (the token that
crosses p is dropped)."""
import numpy as np
import pytest

from tests import sampling_oracle as O
from tests.test_sampling_cpu import MASK, mass_above, philox4x32_10, scores

NONE = 0x7fffffff
MUTATIONS = {  # mutation -> (family, a fragment of the name of a probe that must fail)
    "topk_gt": ("A", "digit 3"),                    # top-k keeps > the k-th key instead of >=
    "three_digits": ("A", "digit 3"),               # the descent stops after three digits
    "topp_le": ("E", "digit"),                      # see the module's text
    "z_whole_row": ("F", "near miss"),              # Z of top-p over the whole row
    "pad_visible": ("G 4097", "G N=4097"),          # one padding column is read
    "skip_last_group": ("A", "last partial group"),
    "no_sign_fold": ("A", "- pair"),                # negative scores keyed without the complement
    "neg_zero_apart": ("B", "zeros tie"),           # -0 keyed below +0
    "ctr_plus_1": ("B", "kept"),
    "word_plus_1": ("B", "kept"),                   # Philox word (i + 1) & 3
    "shift_8": ("B", "kept"),                       # w >> 8
    "last_index_ties": ("greedy aligned", "tied maxima"),
    "k_above_count_keeps_nothing": ("D", "k = candidates + 1"),
    "all_nan_sentinel": ("H NaN 4097", "all NaN"),
}


# ---- the emulation ------------------------------------------------------------------------------------------------------------------------
def okey(s, mut=None):
    s = np.asarray(s, dtype=np.float32)
    u = (s if mut == "neg_zero_apart" else s + np.float32(0.0)).view(np.uint32)
    if mut == "no_sign_fold":
        k = u ^ np.uint32(0x80000000)
    else:
        k = np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000))
    return np.where(np.isnan(s), np.uint32(0), k).astype(np.uint32)


def okey_value(k, mut=None):
    k = np.asarray(k, dtype=np.uint32)
    if mut == "no_sign_fold":
        return (k ^ np.uint32(0x80000000)).view(np.float32)
    return O.key_value(k)


def better(v, i, best, bi, mut):
    return v > best or (v == best and (i > bi if mut == "last_index_ties" else i < bi))


def emu_argmax(r, aligned, mut=None):
    """argmax_row: every thread takes its elements in its own order, then the 64-lane butterfly, then the 16 waves in turn."""
    N = len(r)
    i = np.arange(N)
    if aligned:
        nv = N >> 2
        owner = np.where(i < (nv << 2), (i >> 2) & 1023, (i - (nv << 2)) & 1023)
    else:
        owner = i & 1023
    best = np.full(1024, -np.inf, dtype=np.float32)
    bi = np.full(1024, NONE, dtype=np.int64)
    valid = ~np.isnan(r)
    tie = -i if mut == "last_index_ties" else i
    order = np.lexsort((tie[valid], -r[valid].astype(np.float64), owner[valid]))     # per thread: value down, then index up
    own, first = np.unique(owner[valid][order], return_index=True)
    best[own], bi[own] = r[valid][order][first], i[valid][order][first]
    wave_v, wave_i = [], []
    for w in range(16):
        v, b = best[64 * w:64 * w + 64].copy(), bi[64 * w:64 * w + 64].copy()
        o = 32
        while o:
            ov, ob = v[np.arange(64) ^ o], b[np.arange(64) ^ o]
            take = np.array([better(ov[l], ob[l], v[l], b[l], mut) for l in range(64)])
            v, b = np.where(take, ov, v), np.where(take, ob, b)
            o >>= 1
        wave_v.append(v[0])
        wave_i.append(b[0])
    v, b = wave_v[0], wave_i[0]
    for w in range(1, 16):
        if better(wave_v[w], wave_i[w], v, b, mut):
            v, b = wave_v[w], wave_i[w]
    return int(b) if (b != NONE or mut == "all_nan_sentinel") else 0


def histogram(keys, masses, lo, prefix, mask, shift):
    sel = (keys >= lo) & ((keys & np.uint32(mask)) == np.uint32(prefix))
    d = ((keys[sel] >> np.uint32(shift)) & np.uint32(255)).astype(np.int64)
    cnt = np.bincount(d, minlength=256)
    ms = np.zeros(256, dtype=np.uint64)
    if masses is not None:
        np.add.at(ms, d, masses[sel])
    return cnt, ms


def emu_threshold(r, aligned, T, k, p, mut=None):
    """Everything of sample_kernel before the draw: ('token', t) for a greedy or fallback row, else ('thr', keys, thr)."""
    T, p = np.float32(T), np.float32(p)
    N = len(r)
    if not T >= np.float32(1e-4):
        return "token", emu_argmax(r, aligned, mut)
    with np.errstate(all="ignore"):
        keys = okey(r / T, mut)
    if mut == "skip_last_group":
        keys[4 * (N // 4):] = 0
    kmax = keys.max()
    m = okey_value(kmax, mut)
    if kmax == 0 or not np.isfinite(m):
        return "token", emu_argmax(r, aligned, mut)
    thr = 1
    if 0 < k < N:
        prefix = mask = 0
        rem, done = k, True
        for lev in range(3 if mut == "three_digits" else 4):
            shift = 24 - 8 * lev
            cnt, _ = histogram(keys, None, 1, prefix, mask, shift)
            if lev == 0 and rem > cnt.sum():
                done = False                                                    # L.status = 1: top-k is off
                if mut == "k_above_count_keeps_nothing":
                    thr = 0xffffffff
                break
            above = 0
            for d in range(255, -1, -1):
                if cnt[d] and above < rem <= above + cnt[d]:
                    digit, nrem = d, rem - above
                above += int(cnt[d])
            prefix |= digit << shift
            mask |= 0xff << shift
            rem = nrem
        if done:
            thr = prefix + 1 if mut == "topk_gt" else prefix
    if 0 < p < 1:
        with np.errstate(all="ignore"):
            e = np.exp((okey_value(keys, mut) - m).astype(np.float32)).astype(np.float32) * np.float32(2.0 ** 40)
        masses = np.where(keys >= 1, e, 0).astype(np.uint64)
        if mut == "topp_le":
            kk = keys[keys >= thr]
            uniq = np.unique(kk)[::-1]
            per = np.array([int(masses[keys == u].sum()) for u in uniq], dtype=object)
            pz = float(p) * float(per.sum())
            incl = np.cumsum(per)
            ok = [j for j in range(len(uniq)) if float(incl[j]) <= pz]
            return "thr", keys, int(uniq[ok[-1]] if ok else uniq[0])
        prefix = mask = 0
        base = 0
        for lev in range(4):
            shift = 24 - 8 * lev
            cnt, ms = histogram(keys, masses, thr, prefix, mask, shift)
            if lev == 0:
                total = int(ms.sum())
                if mut == "z_whole_row":
                    total = int(histogram(keys, masses, 1, 0, 0, shift)[1].sum())
                pz = float(p) * float(total)
            above = base
            for d in range(255, -1, -1):
                if cnt[d] and float(above) < pz:
                    digit, nbase = d, above
                above += int(ms[d])
            prefix |= digit << shift
            mask |= 0xff << shift
            base = nbase
        thr = prefix
    return "thr", keys, thr


def emu_draw(keys, thr, seed, c, mut=None):
    kept = np.flatnonzero(keys.astype(np.uint64) >= np.uint64(thr))
    if not len(kept):
        return NONE if mut == "all_nan_sentinel" else 0
    cc = (c + (mut == "ctr_plus_1")) & MASK
    g = (kept >> 2).astype(np.uint64)
    words = np.stack(philox4x32_10((g, np.full_like(g, cc), np.zeros_like(g), np.zeros_like(g)), (seed & MASK, seed >> 32)))
    x = words[(kept + (mut == "word_plus_1")) & 3, np.arange(len(kept))]
    with np.errstate(all="ignore"):
        u = ((2 * (x >> np.uint64(8 if mut == "shift_8" else 9)) + 1) & MASK).astype(np.float32) * np.float32(2.0 ** -24)
        z = okey_value(keys[kept], mut) + -np.log(-np.log(u))
    assert z.dtype == np.float32
    ok = ~np.isnan(z)
    if not ok.any():
        return NONE if mut == "all_nan_sentinel" else 0
    top = np.flatnonzero(ok & (z == z[ok].max()))
    return int(kept[top[-1] if mut == "last_index_ties" else top[0]])


def run_emulation(case, mut=None):
    L = O.layout(case)
    got, cache = [], {}
    for i, e in enumerate(case.entries):
        aligned = (case.offset + i * case.ld) % 4 == 0
        r = e.row.logits
        if mut == "pad_visible":
            r = np.concatenate([r, O.successor(case, L, i)[:1]])
        if case.null:
            got.append(emu_argmax(r, aligned, mut))
            continue
        key = (id(e.row), aligned, i if mut == "pad_visible" and case.ld == case.N else -1)
        if key not in cache:
            cache[key] = emu_threshold(r, aligned, L["T"][i], L["k"][i], L["p"][i], mut)
        res = cache[key]
        got.append(res[1] if res[0] == "token" else emu_draw(res[1], res[2], L["seed"][i], int(L["ctr"][i]) + O.CTR_ADD, mut))
    return np.array(got)


# ---- the tests ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", list(O.FAMILIES))
def test_emulation_passes_every_probe(family):
    for case in O.FAMILIES[family]():
        assert case.entries
        O.check(case, run_emulation(case))


@pytest.mark.parametrize("mut", list(MUTATIONS))
def test_mutation_fails_a_named_probe(mut):
    family, fragment = MUTATIONS[mut]
    failing, refused = [], 0
    for case in O.FAMILIES[family]():
        got = run_emulation(case, mut)
        failing += [e.what for e, t in zip(case.entries, got) if t != e.expect]
        try:
            O.check(case, got)
        except AssertionError:
            refused += 1
    assert refused, mut
    named = [w for w in failing if fragment in w]
    print(f"{mut}: {len(failing)} probes fail, e.g. {named[:2]}")
    assert named, (mut, failing[:4])


def test_builders_cannot_lie():
    """finish() refuses a row whose stated boundary is not host_kept's, and one whose top-p mass is inside the margin."""
    rng = np.random.default_rng(1)
    row = O.digit_row("lie", 4097, 2, False, (5, 9), 1.0, False, rng)
    row.k += 1
    with pytest.raises(AssertionError, match="kept set"):
        O.finish(row)
    row = O.digit_row("margin", 4097, 2, False, (5, 9), 1.0, True, rng)
    O.finish(row)
    s = scores(row.logits, row.T)
    row.p = float(np.float32(mass_above(s, ~np.isnan(s))[row.X[0]] - 5e-5))    # the first dropped token's mass is 5e-5 above p
    with pytest.raises(AssertionError, match="from p"):
        O.finish(row)


def test_every_probe_respects_the_draw_bound_and_the_sizes():
    counts = O.probe_counts()
    print(counts)
    for name, fam in O.FAMILIES.items():
        for case in fam():
            assert len(case.entries) * case.ld <= 2100 * 32768, case.name
            for e in case.entries:
                assert 0 <= e.expect < case.N and O.CTR_ADD <= e.c < O.BUDGET
                if e.row.fixed is None:
                    assert e.row.K[e.expect] and (e.row.K.sum() <= 16 or case.N <= 4097), e.what
    assert set(O.WIDTHS) == {1, 2, 3, 4, 5, 4093, 4096, 4097, 32765, 32767, 32768, 32769, 32772, 65541}


def test_replay_is_the_host_draw():
    from tests.test_sampling_cpu import host_draw
    rng = np.random.default_rng(2)
    logits = rng.standard_normal(300).astype(np.float32) * 3
    for c in range(20):
        t, ok = O.replay(logits, 0.7, 40, 0.9, 99, c)
        assert t == host_draw(logits, 0.7, 40, float(np.float32(0.9)), 99, c)[0] and isinstance(ok, bool)
