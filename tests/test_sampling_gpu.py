"""Seeded on-device sampling on the MI355X: vly_argmax with per-row vly_sample_row parameters against the float64 host
replica of tests/test_sampling_cpu.py, its distribution, determinism and counter contract, and the layers above it —
DecodeSession(sampling=True), generate(top_k / top_p / seed) and ContinuousBatcher(sampling=True)."""
import numpy as np
import pytest
import torch

from tests import golden_cfg as G
from tests.test_sampling_cpu import host_draw, host_kept, mass_above, scores

pytestmark = pytest.mark.gpu


def dev():
    return torch.device("cuda:0")


def rows_of(ld, M, N, gen):
    """fp32 [M, N] view of an [M, ld] buffer (row stride ld) filled with logits."""
    buf = torch.randn((M, ld), generator=gen) * 3.0
    return buf.to(dev())[:, :N]


def first_max(x):
    """torch's first-maximal-index rule on the CPU, NaN never selected."""
    x = x.clone()
    x[torch.isnan(x)] = -float("inf")
    return x.argmax(-1)


@pytest.mark.parametrize("N,ld", [(1, 1), (7, 9), (1000, 1000), (32000, 32000), (32006, 32008), (32001, 32003), (70000, 70001)])
def test_greedy_identity(N, ld):
    from valley_amd import ops
    g = torch.Generator().manual_seed(N)
    M = 5
    x = rows_of(ld, M, N, g)
    x[0, N // 2] = x[0].max() + 1                       # ties at the maximum: the first one wins
    x[0, N - 1] = x[0, N // 2]
    x[1] = -float("inf")
    x[2, : N // 3] = float("nan")
    want = first_max(x.cpu())
    got = ops.argmax(x).cpu()
    assert got.tolist() == want.tolist()
    greedy = ops.sampling_rows([0.0] * M, 50, 0.5, 9, device=dev())
    assert ops.argmax(x, sampling=greedy, ctr=torch.zeros(M, dtype=torch.int32, device=dev()), ctr_add=3).cpu().tolist() \
        == want.tolist()


def test_exact_replica_mixed_rows():
    from valley_amd import ops
    rng = np.random.default_rng(7)
    Ts, ks, ps = [0.2, 0.7, 1.0, 1.5], [0, 1, 50, None], [1.0, 0.9, 0.5, 1e-6]
    checked = 0
    for N, ld in [(1000, 1000), (32000, 32000), (32006, 32008), (70000, 70000)]:
        M = 64
        buf = torch.from_numpy((rng.standard_normal((M, ld)) * rng.uniform(1, 4, (M, 1))).astype(np.float32))
        x = buf.to(dev())[:, :N]
        T = [Ts[i % 4] for i in range(M)]
        k = [N if ks[(i // 4) % 4] is None else ks[(i // 4) % 4] for i in range(M)]
        p = [ps[(i // 16) % 4] for i in range(M)]
        seed = [int(s) for s in rng.integers(0, 1 << 63, M)]
        ctr = torch.from_numpy(rng.integers(0, 1 << 20, M).astype(np.int32))
        sp = ops.sampling_rows(T, k, p, seed, device=dev())
        got = ops.argmax(x, sampling=sp, ctr=ctr.to(dev()), ctr_add=5).cpu().numpy()
        xc = buf[:, :N].numpy()
        for r in range(M):
            want, keep, z = host_draw(xc[r], T[r], k[r], p[r], seed[r], int(ctr[r]) + 5)
            t = int(got[r])
            assert 0 <= t < N
            if not keep[t]:                                  # only a top-p cut tie within 1e-5 of mass
                k_keep, s = host_kept(xc[r], T[r], k[r], 1.0)
                assert k_keep[t] and abs(mass_above(s, k_keep)[t] - p[r]) < 1e-5, (N, r, t)
                continue
            if t != want:
                top2 = np.sort(z[np.isfinite(z)])[-2:]
                assert top2[1] - top2[0] <= 1e-4 * max(1.0, abs(top2[1])), (N, r, t, want)
            checked += 1
    assert checked >= 250


def test_distribution_total_variation():
    from valley_amd import ops
    n, V = 200_000, 64
    row = torch.from_numpy((np.random.default_rng(11).standard_normal(V) * 2).astype(np.float32))
    x = row.to(dev())[None].expand(n, V)                  # one row, n draws (row stride 0 is not allowed: copy)
    x = x.contiguous()
    sp = ops.sampling_rows(0.7, 20, 0.9, 4242, device=dev()).expand(n, 6).contiguous()
    ctr = torch.arange(n, dtype=torch.int32, device=dev())
    got = ops.argmax(x, sampling=sp, ctr=ctr).cpu().numpy()
    s = scores(row.numpy(), 0.7)
    keep = s >= np.sort(s)[::-1][19]
    keep &= mass_above(s, keep) < 0.9
    q = np.where(keep, np.exp(s - s.max()), 0.0)
    q /= q.sum()
    counts = np.bincount(got, minlength=V).astype(np.float64)
    assert counts[~keep].sum() == 0
    assert 0.5 * np.abs(counts / n - q).sum() < 0.01


def test_determinism_and_counters():
    from valley_amd import ops
    g = torch.Generator().manual_seed(3)
    M, N = 1000, 32000
    x = rows_of(N, M, N, g)
    sp = ops.sampling_rows(1.0, 0, 1.0, 77, device=dev())
    sp = sp.expand(M, 6).contiguous()
    ctr = torch.full((M,), 100, dtype=torch.int32, device=dev())
    first = ops.argmax(x, sampling=sp, ctr=ctr).clone()
    for _ in range(20):
        assert torch.equal(ops.argmax(x, sampling=sp, ctr=ctr), first)
    nxt = ops.argmax(x, sampling=sp, ctr=ctr, ctr_add=1)
    assert float((nxt != first).float().mean()) >= 0.9
    # a row moved to another batch index with the same (seed, ctr) draws the same token
    sp2 = ops.sampling_rows([0.8] * 8, 40, 0.95, [5 + i for i in range(8)], device=dev())
    c2 = torch.arange(8, dtype=torch.int32, device=dev()) * 3
    a = ops.argmax(x[:8], sampling=sp2, ctr=c2).cpu()
    perm = torch.tensor([5, 2, 7, 0, 3, 6, 1, 4])
    b = ops.argmax(x[:8][perm.to(dev())].contiguous(), sampling=sp2[perm.to(dev())].contiguous(), ctr=c2[perm.to(dev())].contiguous())
    assert b.cpu().tolist() == a[perm].tolist()
    one = ops.argmax(x[3:4], sampling=sp2[3:4], ctr=c2[3:4])
    assert int(one[0]) == int(a[3])


def small_llama():
    from valley_amd.llama import HipLlama
    return HipLlama(1024, 8, 2752, 2, 32006, 1e-5).init_random(seed=5)


def run_session(ll, B, use_graph, sample_rows=None, steps=6, change_at=None):
    from valley_amd.decode import DecodeSession
    g = torch.Generator(device="cuda").manual_seed(21)
    S = 40
    cache = ll.new_cache(B, S + steps + 2)
    h = torch.randn((B * S, ll.H), generator=g, device="cuda") * 0.02
    x = ll.forward(h, B, S, cache)
    first = ll.logits(x.view(B, S, -1)[:, -1].contiguous())[:, :ll.V].argmax(-1)
    sess = DecodeSession(ll, cache, use_graph=use_graph, sampling=sample_rows is not None)
    if sample_rows is not None:
        sess.sample.copy_(sample_rows)
    sess.begin(first)
    toks = []
    for i in range(steps):
        if change_at is not None and i == change_at[0]:
            sess.sample.copy_(change_at[1])
        toks.append(sess.step().clone())
    torch.cuda.synchronize()
    sess.check()
    return torch.stack(toks).cpu(), sess


def test_decode_session_sampling_graph_equals_eager_and_greedy():
    from valley_amd import ops
    ll = small_llama()
    B = 4
    sp = ops.sampling_rows([0.7, 1.0, 1.5, 0.2], [0, 50, 0, 5], [0.9, 1.0, 1.0, 0.5], [1, 2, 3, 4], device=dev())
    tg, sess = run_session(ll, B, True, sp)
    te, _ = run_session(ll, B, False, sp)
    assert torch.equal(tg, te)
    # all rows greedy: the default session's tokens
    greedy = ops.sampling_rows([0.0] * B, device=dev())
    t0, _ = run_session(ll, B, True, None)
    t1, _ = run_session(ll, B, True, greedy)
    assert torch.equal(t0, t1)
    # sess.sample written between replays takes effect without a re-capture: greedy for three steps, then sampled — the
    # eager session's tokens, and no longer the greedy ones
    tc, s2 = run_session(ll, B, True, greedy, change_at=(3, sp))
    graph = s2.graph
    ref, _ = run_session(ll, B, False, greedy, change_at=(3, sp))
    assert torch.equal(tc, ref) and torch.equal(tc[:3], t0[:3])
    assert not torch.equal(tc[3:], t0[3:])
    assert s2.graph is graph is not None


def build_golden_model():
    from tests.test_model_gpu import build_golden_model as b
    return b()


def golden_inputs(case="decode"):
    T = G.GCFG["T"]
    ids, _ = G.golden_ids(case)
    img = torch.from_numpy(G.golden_pixels(T, "mixed")).view(1, T, 3, 224, 224).cuda()
    return torch.from_numpy(ids).cuda(), img


def test_generate_seeded_top_k():
    model = build_golden_model()
    ids, img = golden_inputs()
    kw = dict(images=img, max_new_tokens=12, do_sample=True, temperature=0.2, top_k=50)
    a = model.generate(ids, seed=123, **kw)
    b = model.generate(ids, seed=123, **kw)
    c = model.generate(ids, seed=123, use_graph=False, **kw)
    assert torch.equal(a, b) and torch.equal(a, c)
    others = [model.generate(ids, seed=s, temperature=1.5, **{k: v for k, v in kw.items() if k != "temperature"})
              for s in (1, 2, 3)]
    assert len({tuple(o[0].tolist()) for o in others}) > 1
    # every generated token is inside the top-50 of the full-recompute logits at its position
    for seq in [a] + others:
        out = model(input_ids=seq[:, :-1], images=img)
        lg = out.logits[0, ids.shape[1] - 1:]
        top = lg.topk(50, dim=-1).values[:, -1:]
        gen = seq[0, ids.shape[1]:]
        chosen = lg.gather(-1, gen[:, None])
        assert bool((chosen >= top - 0.09).all())                       # 2x the bf16 logit tolerance


def test_continuous_batcher_sampling():
    from valley_amd.serving import ContinuousBatcher
    model = build_golden_model()
    img = golden_inputs()[1]
    reqs = [golden_inputs(c)[0] for c in ("decode2", "decode", "decode2")]
    n = 6

    def serve(cb, plan):
        """plan: list of (request, slot-filler kwargs); returns tokens per plan entry."""
        slots, got = [], []
        for ids, kw in plan:
            s = cb.add(ids, images=img, **kw)
            slots.append(s)
            got.append([int(cb.sess.tok[s])])
        for _ in range(n - 1):
            toks = cb.step()
            for j, s in enumerate(slots):
                got[j].append(toks[s])
        for s in slots:
            cb.release(s)
        return got, slots

    seeded = dict(temperature=0.9, top_k=40, top_p=0.95, seed=2024)
    # seeded request in slot 0 beside greedy neighbours ...
    cb = ContinuousBatcher(model, slots=4, ctx_max=512, sampling=True)
    g1, s1 = serve(cb, [(reqs[0], seeded), (reqs[1], {}), (reqs[2], {})])
    # ... and in slot 2 beside other sampled requests
    cb2 = ContinuousBatcher(model, slots=4, ctx_max=512, sampling=True)
    g2, s2 = serve(cb2, [(reqs[1], dict(temperature=1.2, seed=1)), (reqs[2], dict(temperature=0.5, top_p=0.8, seed=2)),
                         (reqs[0], seeded)])
    assert s1[0] == 0 and s2[2] == 2
    assert g1[0] == g2[2]
    # greedy requests: the same tokens as in a default batcher
    cb3 = ContinuousBatcher(model, slots=4, ctx_max=512)
    g3, _ = serve(cb3, [(reqs[1], {}), (reqs[2], {})])
    assert g3 == g1[1:]
    with pytest.raises(ValueError):
        cb3.add(reqs[0], images=img, temperature=0.7)
