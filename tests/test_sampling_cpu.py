"""Seeded on-device sampling (vly_argmax with vly_sample_row, ops.sampling_rows): the host replicas the GPU tests compare
against — Philox4x32-10 and the float64 temperature / top-k / top-p / Gumbel-max reference — checked against published
known-answer vectors and against transformers' warpers, plus the host-side validation and the ABI of the entry point."""
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
MASK = 0xFFFFFFFF


def philox4x32_10(ctr, key):
    """Vectorised Philox4x32-10: ctr uint64 arrays (c0, c1, c2, c3) of 32-bit values, key (k0, k1) -> four uint64 arrays."""
    c0, c1, c2, c3 = (np.asarray(c, dtype=np.uint64) & MASK for c in ctr)
    k0, k1 = (np.asarray(k, dtype=np.uint64) & MASK for k in key)
    for rnd in range(10):
        if rnd:
            k0, k1 = (k0 + W0) & MASK, (k1 + W1) & MASK
        p0, p1 = np.uint64(M0) * c0, np.uint64(M1) * c2
        hi0, lo0 = p0 >> np.uint64(32), p0 & MASK
        hi1, lo1 = p1 >> np.uint64(32), p1 & MASK
        c0, c1, c2, c3 = hi1 ^ c1 ^ k0, lo1, hi0 ^ c3 ^ k1, lo0
    return c0, c1, c2, c3


def gumbel_noise(n, seed, ctr):
    """float64 Gumbel noise of elements 0 .. n-1 of one row: word i & 3 of Philox at counter (i >> 2, ctr, 0, 0)."""
    g = np.arange((n + 3) // 4, dtype=np.uint64)
    z = np.zeros_like(g)
    words = philox4x32_10((g, np.full_like(g, ctr & MASK), z, z), (seed & MASK, seed >> 32))
    x = np.stack(words, axis=1).reshape(-1)[:n]
    u = (2.0 * (x >> np.uint64(9)).astype(np.float64) + 1.0) * 2.0 ** -24
    return -np.log(-np.log(u))


def scores(logits, T):
    """s = l / T with IEEE fp32 division (the kernel's), as float64."""
    return (np.asarray(logits, np.float32) / np.float32(T)).astype(np.float64)


def mass_above(s, keep):
    """Softmax mass, over the kept tokens, strictly above each token's score (float64)."""
    e = np.where(keep, np.exp(s - s[keep].max()), 0.0)
    q = e / e.sum()
    order = np.argsort(-s, kind="stable")
    ss, qs = s[order], q[order]
    cum = np.concatenate([[0.0], np.cumsum(qs)])
    first = np.searchsorted(-ss, -ss, side="left")      # first position of each score's tie group in descending order
    out = np.empty_like(s)
    out[order] = cum[first]
    return out


def host_kept(logits, T, k, p):
    """Kept set of one row: top-k (ties kept, k clamped to N) then top-p (mass strictly above < p), float64."""
    s = scores(logits, T)
    keep = ~np.isnan(s)
    if 0 < k < keep.sum():
        kth = np.sort(s[keep])[::-1][k - 1]
        keep &= s >= kth
    if 0 < p < 1:
        keep &= mass_above(s, keep) < p
    return keep, s


def host_draw(logits, T, k, p, seed, ctr):
    """float64 replica of one draw: (token, kept set, perturbed scores)."""
    keep, s = host_kept(logits, T, k, p)
    z = np.where(keep, s + gumbel_noise(len(s), seed, ctr), -np.inf)
    return int(np.argmax(z)), keep, z


def test_philox_known_answers():
    """Random123's kat_vectors for philox4x32_10."""
    cases = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
             ((MASK,) * 4, (MASK, MASK), (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
             ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
              (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]
    for ctr, key, want in cases:
        got = tuple(int(w[0]) for w in philox4x32_10([np.array([c], np.uint64) for c in ctr], key))
        assert got == want, [hex(v) for v in got]


def test_uniforms_inside_open_interval():
    x = np.array([0, 511, 512, MASK], dtype=np.uint64)
    u = (2.0 * (x >> np.uint64(9)).astype(np.float64) + 1.0) * 2.0 ** -24
    assert (u > 0).all() and (u < 1).all() and u[0] == 2.0 ** -24 and u[-1] == 1 - 2.0 ** -24
    assert np.array_equal(u.astype(np.float32).astype(np.float64), u)          # exact in fp32


def test_host_reference_matches_transformers_warpers():
    transformers = pytest.importorskip("transformers")
    from transformers import TopKLogitsWarper, TopPLogitsWarper
    rng = np.random.default_rng(3)
    for trial in range(60):
        N = int(rng.integers(2, 400))
        logits = (rng.standard_normal(N) * rng.uniform(0.5, 4)).astype(np.float32)
        T = float(rng.choice([0.2, 0.7, 1.0, 1.5]))
        k = int(rng.choice([0, 1, 5, 50, N]))
        p = float(rng.choice([1.0, 0.9, 0.5, 1e-6]))
        keep, s = host_kept(logits, T, k, p)
        sc = torch.from_numpy(s)[None]
        ids = torch.zeros((1, 1), dtype=torch.long)
        if 0 < k:
            sc = TopKLogitsWarper(top_k=k)(ids, sc)
        if p < 1:
            sc = TopPLogitsWarper(top_p=p)(ids, sc)
        hf = torch.isfinite(sc[0]).numpy()
        assert np.array_equal(hf, keep), (trial, N, T, k, p, np.flatnonzero(hf != keep))
    assert transformers is not None


def test_host_draw_is_a_kept_token_with_the_filtered_distribution():
    rng = np.random.default_rng(5)
    logits = rng.standard_normal(16).astype(np.float32)
    keep, s = host_kept(logits, 0.7, 8, 0.9)
    q = np.where(keep, np.exp(s - s.max()), 0)
    q /= q.sum()
    counts = np.zeros(16)
    for c in range(20000):
        t, kept, _ = host_draw(logits, 0.7, 8, 0.9, 1234, c)
        counts[t] += 1
    assert counts[~keep].sum() == 0
    assert 0.5 * np.abs(counts / counts.sum() - q).sum() < 0.02


def test_sampling_rows_packs_and_broadcasts():
    from valley_amd import ops
    t = ops.sampling_rows([0.2, 1.5], 50, 0.9, [7, (1 << 64) - 1])
    assert t.dtype == torch.int32 and tuple(t.shape) == (2, 6)
    f = t.view(torch.float32)
    assert f[0, 0].item() == np.float32(0.2) and f[1, 0].item() == 1.5 and f[0, 2].item() == np.float32(0.9)
    assert t[:, 1].tolist() == [50, 50] and t[:, 5].tolist() == [0, 0]
    words = t[:, 3:5].numpy().astype(np.uint32).astype(np.uint64)
    assert words[0].tolist() == [7, 0] and words[1].tolist() == [MASK, MASK]
    assert tuple(ops.sampling_rows(0.0).shape) == (1, 6)


@pytest.mark.parametrize("bad", [dict(temperature=-0.1), dict(temperature=float("nan")), dict(temperature=float("inf")),
                                 dict(temperature=1.0, top_k=-1), dict(temperature=1.0, top_k=1.5),
                                 dict(temperature=1.0, top_p=0.0), dict(temperature=1.0, top_p=1.01),
                                 dict(temperature=1.0, top_p=float("nan")), dict(temperature=1.0, seed=-1),
                                 dict(temperature=1.0, seed=1 << 64), dict(temperature=[1.0, 1.0], seed=[1, 2, 3])])
def test_sampling_rows_rejects_invalid_values(bad):
    from valley_amd import ops
    with pytest.raises(ValueError):
        ops.sampling_rows(**bad)


def test_abi_version_and_sample_row_layout():
    from valley_amd import build, lib
    build.build(verbose=False)
    assert lib.ABI_VERSION == 8 == lib.load().vly_abi_version()
    hdr = open(os.path.join(ROOT, "include", "valley_hip.h")).read()
    m = re.search(r"typedef struct \{(.*?)\}\s*vly_sample_row;", hdr, flags=re.S)
    assert m, "vly_sample_row is not declared"
    body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            ty, names = decl.split(None, 1)
            fields += [(ty, n.strip()) for n in names.split(",")]
    assert fields == [("float", "temperature"), ("int32_t", "top_k"), ("float", "top_p"), ("uint32_t", "seed_lo"),
                      ("uint32_t", "seed_hi"), ("int32_t", "reserved")]
    assert 4 * len(fields) == 24
    assert len(lib._SIGS["vly_argmax"][1]) == 10
