"""The beam and processor oracle on the MI355X (tests/beam_oracle.py): every constructed case through valley_amd.ops and the C ABI,
held to the host's answer bit for bit.  Candidates over scores (both instantiations of beam_rows_kernel<*, false>), candidates over
logits on rows whose log-sum-exp is exact (beam_rows_kernel<*, true>), the two libraries against each other on every case, the
log-sum-exp against float64, the running-beam selection, the KV reorder at its limits, and the processors round their loops and over
ids outside the vocabulary.  Inputs sit in wider buffers whose padding columns and guard row hold +inf / 3e38 / NaN; outputs are
followed by sentinels; every candidates launch runs twice on one scratch (the tickets are back at zero).

Measured on the device (score - (x - lse64)), the log-sum-exp test's figures are printed before they are asserted."""
import numpy as np
import pytest
import torch

from tests import beam_oracle as O

pytestmark = pytest.mark.gpu
GUARD = 64
LSE_BOUND = 2e-5                          # tests/test_beam_gpu.py's bound on log_softmax(x) + running against float64


def dev():
    return torch.device("cuda:0")


def up(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev())


def bits(t):
    return t.contiguous().view(torch.int32 if t.element_size() == 4 else torch.int16 if t.element_size() == 2 else torch.uint8)


def same(a, b):
    return a.shape == b.shape and torch.equal(bits(a), bits(b))


def guarded(n, dtype):
    """An output of n elements followed by GUARD sentinels: (whole buffer, the output view, a copy of the buffer as allocated)."""
    buf = torch.full((n + GUARD,), O.SENTINEL, dtype=dtype, device=dev())
    return buf, buf[:n], buf.clone()


def guards_intact(buf, n, orig):
    return torch.equal(bits(buf[n:]), bits(orig[n:]))


def candidates(case, values, running, lib):
    """Two launches of one candidates entry point on one scratch.  Returns the first launch's outputs as numpy (score as uint32)."""
    from valley_amd import ops
    fn = ops.logits_beam_candidates if lib == "logits" else ops.beam_candidates
    buf = up(O.padded(values, case.ld))
    orig = buf.clone()
    x = buf[:case.R, :case.V]
    run = up(np.asarray(running, dtype=np.float32))
    eos = up(np.asarray(case.eos, dtype=np.int32)) if case.eos else None
    scratch = ops.beam_scratch(case.B, case.nb, case.K, dev())
    n = case.B * case.K
    got = []
    for _ in range(2):
        outs = [guarded(n, dt) for dt in (torch.float32, torch.int32, torch.int32, torch.uint8)]
        fn(x, run, case.B, case.nb, case.K, eos, scratch, out=tuple(o[1] for o in outs))
        torch.cuda.synchronize()
        assert all(guards_intact(b, n, o) for b, _, o in outs), case.name
        got.append([v.cpu().numpy() for _, v, _ in outs])
    assert same(buf, orig), f"{case.name}: the input (poison columns, guard row) was written"
    for a, b in zip(*got):
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), f"{case.name}: the second launch on the same scratch differs"
    s, t, b, h = got[0]
    return s.view(np.uint32), t, b, h


def assert_candidates(case, got, want):
    for name, g, w in zip(("token", "beam", "hit", "score"), (got[1], got[2], got[3], got[0]), (want[1], want[2], want[3], want[0])):
        bad = np.flatnonzero(g != w)
        assert not len(bad), (f"{case.name} ({O.kernel_of(case.V)} form): {name} differs at {bad[:8].tolist()}: got "
                              f"{g[bad[:8]].tolist()}, want {w[bad[:8]].tolist()}")


@pytest.mark.parametrize("name", O.candidate_case_names())
def test_scored_candidates_are_exact(name):
    c = O.case_by_name(name)
    want = O.expected_candidates(c.scores, c.running, c.B, c.nb, c.K, c.eos)
    assert_candidates(c, candidates(c, c.scores, c.running, "logits"), want)


@pytest.mark.parametrize("name", [c.name for c in O.lse_cases()])
def test_beam_candidates_on_exact_lse_rows(name):
    """vly_beam_candidates against the host alone.  First, from the device's own output at running = 0: every row's maximum scores
    (m - lse) + 0 == +0.0 exactly, so lse == m (logf(1) == 0 and every other exponential flushed to 0)."""
    c = O.case_by_name(name, "lse")
    zero = np.zeros(c.R, dtype=np.float32)
    s0, t0, b0, _ = candidates(c, c.logits, zero, "beam")
    top = np.nanargmax(c.logits, axis=1)
    assert s0[:c.nb].tolist() == [0] * c.nb and t0[:c.nb].tolist() == top.tolist() and b0[:c.nb].tolist() == list(range(c.nb)), \
        f"{c.name}: lse != m on the device: scores {s0[:c.nb].view(np.float32).tolist()}"
    want = O.expected_candidates(c.scores, c.running, c.B, c.nb, c.K, c.eos)
    assert_candidates(c, candidates(c, c.logits, c.running, "beam"), want)


@pytest.mark.parametrize("name", O.candidate_case_names())
def test_beam_candidates_equal_process_then_scored(name):
    """vly_beam_candidates on the raw rows == vly_logits_process(log_softmax) then vly_logits_beam_candidates, bit for bit."""
    from valley_amd import ops
    c = O.case_by_name(name)
    a = candidates(c, c.scores, c.running, "beam")
    y = up(O.padded(c.scores, c.ld))
    orig = y.clone()
    params = ops.processor_rows(device=dev()).expand(c.R, 4).contiguous()
    ops.logits_process(y[:c.R, :c.V], params, torch.zeros((c.R, 1), dtype=torch.int32, device=dev()), log_softmax=True)
    torch.cuda.synchronize()
    assert same(y[:, c.V:], orig[:, c.V:]) and same(y[c.R], orig[c.R]), c.name
    b = candidates(c, y[:c.R, :c.V].cpu().numpy(), c.running, "logits")
    assert_candidates(c, a, b)


def lse_rows(V, seed):
    g = np.random.default_rng(seed)
    x = (g.standard_normal((8, V)) * 3).astype(np.float32)
    x[1, : V // 7] = -np.inf
    x[2, 11:40] = np.nan
    x[3] = -np.inf
    x[3, V - 2] = 5.0                                                     # a single finite value
    x[4, V // 2] = np.inf                                                 # lse = 0 from here on: the maximum is not finite
    x[5] = -np.inf
    x[6] = np.nan
    x[7, 3] = np.inf
    x[7, 9] = np.nan
    return x


@pytest.mark.parametrize("V", O.LSE_WIDTHS)
def test_lse_against_float64(V):
    from valley_amd import ops
    x = lse_rows(V, V)
    R = x.shape[0]
    ld = V + 3
    buf = up(O.padded(x, ld))
    orig = buf.clone()
    params = ops.processor_rows(device=dev()).expand(R, 4).contiguous()
    ops.logits_process(buf[:R, :V], params, torch.zeros((R, 1), dtype=torch.int32, device=dev()), log_softmax=True)
    torch.cuda.synchronize()
    assert same(buf[:, V:], orig[:, V:]) and same(buf[R], orig[R])
    y = buf[:R, :V].cpu().numpy()
    x64 = x.astype(np.float64)
    for r in range(4):
        ok = ~np.isnan(x64[r])
        mx = x64[r][ok].max()
        lse = mx + np.log(np.exp(x64[r][ok] - mx).sum())
        fin = np.isfinite(x64[r])
        err = float(np.abs(y[r][fin] - (x64[r][fin] - lse)).max())
        print(f"V={V} row {r}: max |y - (x - lse64)| = {err:.3e}")
        assert err < LSE_BOUND, (V, r, err)
        assert np.array_equal(np.isnan(y[r]), np.isnan(x[r])) and (y[r][np.isneginf(x[r])] == -np.inf).all(), (V, r)
    assert y[3, V - 2] == 0.0
    for r in range(4, 8):                                                 # lse = 0 exactly: the row comes back as it was
        assert np.array_equal(np.isnan(y[r]), np.isnan(x[r])) and np.array_equal(y[r][~np.isnan(x[r])], x[r][~np.isnan(x[r])]), (V, r)
    # the same quantity through vly_beam_candidates: the four finite rows as one prompt
    case = O.Cand(f"lse64@{V}", x[:4], np.array([0, -1.5, 0.25, -3], dtype=np.float32), 1, 4, 8)
    s, t, b, _ = candidates(case, case.scores, case.running, "beam")
    acc = np.full((4, V), -np.inf)
    for r in range(4):
        ok = ~np.isnan(x64[r])
        mx = x64[r][ok].max()
        acc[r][ok] = x64[r][ok] - (mx + np.log(np.exp(x64[r][ok] - mx).sum())) + float(case.running[r])
    order = np.argsort(-acc.reshape(-1), kind="stable")[:8]
    assert t.tolist() == (order % V).tolist() and b.tolist() == (order // V).tolist()
    err = float(np.abs(s.view(np.float32).astype(np.float64) - acc.reshape(-1)[order]).max())
    print(f"V={V} candidates: max |score - float64| = {err:.3e}")
    assert err < LSE_BOUND


@pytest.mark.parametrize("name", [c.name for c in O.select_cases()])
def test_select_is_exact(name):
    from valley_amd import ops
    c = O.case_by_name(name, "select")
    n = c.B * c.nb
    outs = [guarded(n, dt) for dt in (torch.int32, torch.int32, torch.float32)]
    ops.beam_select(up(c.score.view(np.float32)), up(c.token), up(c.beam), up(c.hit), c.B, c.nb, *[o[1] for o in outs])
    torch.cuda.synchronize()
    assert all(guards_intact(b, n, o) for b, _, o in outs)
    tok, parent, run = [v.cpu().numpy() for _, v, _ in outs]
    et, ep, er = O.expected_select(c.score, c.token, c.beam, c.hit, c.B, c.nb)
    assert tok.tolist() == et.tolist() and parent.tolist() == ep.tolist(), c.name
    run, er = run.view(np.uint32), er.view(np.uint32)
    nan = np.isnan(er.view(np.float32))
    assert np.array_equal(np.isnan(run.view(np.float32)), nan) and np.array_equal(run[~nan], er[~nan]), c.name


# ---- the KV reorder ---------------------------------------------------------------------------------------------------------------------
def reorder_parents(R, changed, g):
    """``changed`` rows get another row as parent, one row the parent -1 and one the parent R (left alone), the rest themselves."""
    parent = np.arange(R)
    rows = g.permutation(R)
    for r in rows[:changed]:
        parent[r] = (r + 1 + g.integers(0, R - 1)) % R
    return parent


REORDER = {
    "two_byte_r128_every_row": dict(R=128, dtype=torch.int16, changed=128, lo=3, pos=60, hi_add=2, run=1),
    "four_byte_r64_every_row": dict(R=64, dtype=torch.int32, changed=64, lo=3, pos=65, hi_add=5, run=1),
    "r13_five_rows_ragged_run": dict(R=13, dtype=torch.int16, changed=5, lo=3, pos=66, hi_add=4, run=25),
    "hi_clamped_to_ctx_max": dict(R=13, dtype=torch.int32, changed=13, lo=3, pos=60, hi_add=20, run=4),
    "hi_below_lo_nothing_moves": dict(R=13, dtype=torch.int16, changed=13, lo=3, pos=1, hi_add=1, run=9),
    "foreign_parents_left_alone": dict(R=13, dtype=torch.int16, changed=5, lo=0, pos=0, hi_add=70, run=25, foreign=True),
}


@pytest.mark.parametrize("name", list(REORDER))
def test_kv_reorder_at_its_limits(name):
    from valley_amd import ops
    k = REORDER[name]
    R, dtype = k["R"], k["dtype"]
    L, heads, ctx = 2, 2, 70
    g = np.random.default_rng(R + k["lo"] + k["pos"])
    eb = 2 if dtype == torch.int16 else 4
    parent = reorder_parents(R, k["changed"], g)
    if k.get("foreign"):
        same_rows = np.flatnonzero(parent == np.arange(R))
        parent[same_rows[0]], parent[same_rows[1]] = -1, R
    n = int(((parent != np.arange(R)) & (parent >= 0) & (parent < R)).sum())
    assert n == k["changed"] and O.reorder_run(n, eb) == k["run"], name
    if k["run"] > 1 and k["pos"] + k["hi_add"] <= ctx:
        assert (k["pos"] + k["hi_add"] - k["lo"]) % k["run"], name          # the last run is a partial one
    info = np.iinfo(np.int16 if eb == 2 else np.int32)
    host = [g.integers(info.min, info.max, size=(R + 1, heads, ctx, 128), dtype=info.dtype) for _ in range(2 * L)]   # row R: the guard
    bufs = [up(h) for h in host]
    ks, vs = [b[:R] for b in bufs[:L]], [b[:R] for b in bufs[L:]]
    table = ops.kv_beam_table(ks, vs, dev())
    pos = torch.tensor([k["pos"]], dtype=torch.int32, device=dev())
    ops.kv_beam_reorder(table, ks[0], up(parent.astype(np.int32)), k["lo"], k["hi_add"], pos_dev=pos)
    torch.cuda.synchronize()
    for b, h in zip(bufs, host):
        want = np.concatenate([O.expected_reorder(h[:R], parent.tolist(), k["lo"], k["pos"] + k["hi_add"]), h[R:]])
        assert np.array_equal(b.cpu().numpy(), want), name
    if name == "hi_below_lo_nothing_moves":
        assert all(np.array_equal(b.cpu().numpy(), h) for b, h in zip(bufs, host))


@pytest.mark.parametrize("R,dtype", [(129, torch.int16), (65, torch.int32)])
def test_kv_reorder_refuses_more_rows_than_it_can_stage(R, dtype):
    from valley_amd import lib_beam, ops
    bufs = [torch.full((R, 1, 4, 128), 7, dtype=dtype, device=dev()) for _ in range(2)]
    table = ops.kv_beam_table(bufs[:1], bufs[1:], dev())
    parent = torch.zeros(R, dtype=torch.int32, device=dev())
    rc = lib_beam.load().vly_kv_beam_reorder(table.data_ptr(), 1, R, 1, 4, bufs[0].element_size(), parent.data_ptr(), 0, None, 4,
                                            torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert rc == -22
    assert b"vly_kv_beam_reorder" in lib_beam.load().vly_beam_last_error()
    assert all(bool((b == 7).all()) for b in bufs)


# ---- the processors ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [c.name for c in O.process_cases()])
def test_process_loops_and_foreign_ids(name):
    from valley_amd import ops
    c = O.case_by_name(name, "proc")
    want_x, want_h = c.expected()
    R, V, hist_ld = c.R, c.V, c.hist.shape[1]
    params = ops.processor_rows([float(p) for p, _, _ in c.params], [n for _, n, _ in c.params], [m for _, _, m in c.params],
                                device=dev())
    length = up(np.asarray(c.len_dev, dtype=np.int32))
    eos = up(np.asarray(c.eos, dtype=np.int32)) if c.eos else None
    tok = None if c.tok is None else up(c.tok)
    hist_host = np.concatenate([c.hist, np.full((1, hist_ld), O.SENTINEL, dtype=np.int32)])
    for launch in range(2):                                               # twice on fresh inputs: nothing is carried between launches
        buf = up(O.padded(c.x, c.ld))
        orig = buf.clone()
        hist = up(hist_host)
        ops.logits_process(buf[:R, :V], params, hist[:R], length, c.len_add, tok=tok, eos=eos, log_softmax=c.lse is not None)
        torch.cuda.synchronize()
        assert same(buf[:, V:], orig[:, V:]) and same(buf[R], orig[R]), f"{name}: padding or guard row written"
        assert np.array_equal(hist.cpu().numpy(), np.concatenate([want_h, hist_host[R:]])), f"{name}: history after the append"
        got = buf[:R, :V].cpu().numpy()
        for r in range(R):
            bad = np.flatnonzero(got[r].view(np.uint32) != want_x[r].view(np.uint32))
            assert not len(bad), (f"{name} launch {launch} row {r}: ids {bad[:8].tolist()} got {got[r][bad[:8]].tolist()} want "
                                  f"{want_x[r][bad[:8]].tolist()}")
