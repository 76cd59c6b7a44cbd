"""CPU-side checks of token log-probabilities: the library and the wrappers refuse bad arguments before any launch, the float64 reference (tests/score_ref.py) agrees with
torch in float64, and — the mutation proof — a reference with the tie rule flipped or with NaN counted fails on the very
cases tests/test_score_gpu.py runs, so those cases can tell the difference."""
import numpy as np
import pytest
import torch

from tests import score_ref as SR


def test_bad_arguments_are_refused_by_the_library():
    """NULL logits, a top-n beyond 20, a target without its output: -22 with a message, before any launch."""
    from valley_amd import lib_score
    h = lib_score.load()
    assert h.vly_score_rows(None, 8, 8, 1, None, None, None, 0, None, None, None, 0, None) == -22
    assert b"vly_score_rows" in h.vly_score_last_error()
    assert h.vly_score_rows(256, 8, 8, 1, None, None, None, 21, 256, 256, None, 0, None) == -22
    assert h.vly_score_rows(256, 8, 9, 1, None, None, None, 0, None, None, None, 0, None) == -22          # V > ld
    assert h.vly_score_rows(256, 8, 8, 1, 256, None, None, 0, None, None, None, 0, None) == -22          # target, no output
    assert h.vly_score_rows(256, 8, 8, 1, None, None, None, 0, None, None, 256, 7, None) == -22          # copy_ld < V
    assert h.vly_score_record(256, 8, 8, 1, 256, 256, None, 1, 0, 256, 4, 0, None, None, None, None, None) == -22   # per row, no lengths
    assert h.vly_score_record(256, 8, 8, 1, 256, 256, None, 0, 0, 256, 4, 2, 256, 256, None, 256, None) == -22
    assert b"vly_score_record" in h.vly_score_last_error()
    assert h.vly_score_loss(256, 256, 0, 8, 256, 256, None) == -22
    assert h.vly_score_loss(256, None, 4, 8, 256, 256, None) == -22
    assert b"vly_score_loss" in h.vly_score_last_error()


def test_score_ops_check_their_arguments_before_any_launch():
    from valley_amd import lib, ops
    x = torch.zeros((4, 32))
    with pytest.raises(ValueError, match="top must be in"):
        ops.token_logprobs(x, top=21)
    with pytest.raises(ValueError, match="top must be in"):
        ops.token_logprobs(x, top=-1)
    with pytest.raises(ValueError, match="unit column stride"):
        ops.token_logprobs(torch.zeros((32, 4)).t())
    with pytest.raises(ValueError, match="unit column stride"):
        ops.token_logprobs(torch.zeros((4, 64))[:, ::2])
    with pytest.raises(ValueError, match="targets must hold 4"):
        ops.token_logprobs(x, torch.zeros((3,), dtype=torch.int32))
    with pytest.raises(ValueError, match="copy"):
        ops.token_logprobs(x, copy=torch.zeros((4, 31)))
    with pytest.raises(ValueError, match="262144"):
        ops.token_logprobs(torch.zeros((1, (1 << 18) + 1)))
    with pytest.raises(lib.ValleyHipError):                              # all shapes fine: no CPU compute path
        ops.token_logprobs(x, torch.zeros((4,), dtype=torch.int32), top=3)
    with pytest.raises(ValueError, match="lp_table"):
        ops.score_record(x, torch.zeros(4), torch.zeros((4,), dtype=torch.int32), torch.zeros((3, 8)))
    with pytest.raises(ValueError, match="go together"):
        ops.score_record(x, torch.zeros(4), torch.zeros((4,), dtype=torch.int32), torch.zeros((4, 8)),
                         top=(torch.zeros((4, 2), dtype=torch.int32), torch.zeros((4, 2))))
    with pytest.raises(ValueError, match="length must hold"):
        ops.score_record(x, torch.zeros(4), torch.zeros((4,), dtype=torch.int32), torch.zeros((4, 8)),
                         length=torch.zeros((3,), dtype=torch.int32))
    with pytest.raises(lib.ValleyHipError):
        ops.score_record(x, torch.zeros(4), torch.zeros((4,), dtype=torch.int32), torch.zeros((4, 8)))
    with pytest.raises(ValueError, match="labels"):
        ops.cross_entropy(x, torch.zeros((5,), dtype=torch.int32))
    with pytest.raises(lib.ValleyHipError):
        ops.cross_entropy(x, torch.zeros((4,), dtype=torch.int32))


def test_model_surface_refuses_what_the_feature_does_not_cover(monkeypatch):
    from valley_amd import decode, valley_model as vm

    class Stub(vm.ValleyLlamaForCausalLM):
        def __init__(self):                                             # the checks come before the model is touched
            pass

    m = Stub()
    ids = torch.zeros((1, 4), dtype=torch.long)
    with pytest.raises(ValueError, match="return_dict_in_generate"):
        m.generate(ids, output_logprobs=True)
    with pytest.raises(ValueError, match="num_beams"):
        m.generate(ids, output_logprobs=True, return_dict_in_generate=True, num_beams=2)
    with pytest.raises(ValueError, match="top_logprobs"):
        m.generate(ids, output_logprobs=True, return_dict_in_generate=True, top_logprobs=21)
    with pytest.raises(ValueError, match="output_logprobs"):
        m.generate(ids, return_dict_in_generate=True, top_logprobs=2)
    assert "logprobs" in decode.DecodeSession.__init__.__code__.co_varnames


@pytest.mark.parametrize("V", [1, 63, 1025, 4097])
def test_reference_matches_torch_float64(V):
    x, t = SR.rows_case(V)
    xt = torch.from_numpy(x[:, :V].astype(np.float64))
    clean = ~torch.isnan(xt).any(dim=1) & torch.isfinite(xt.max(dim=1).values)
    want = torch.log_softmax(xt, dim=-1)
    got = SR.lse(x[:, :V])
    for r in range(SR.ROWS):
        if bool(clean[r]):
            assert abs(got[r] - float(torch.logsumexp(xt[r], -1))) <= 1e-12 * max(1.0, abs(got[r]))
            lp = SR.target_logprobs(x[:, :V], np.full((SR.ROWS,), V - 1))[r]
            assert lp == pytest.approx(float(want[r, V - 1]), abs=1e-12, rel=1e-12) or (np.isinf(lp) and lp == float(want[r, V - 1]))
    assert got[1] == 0.0 and got[2] == 0.0                              # all -inf; a +inf maximum
    # NaNs are skipped: the row without them gives the same lse
    row = x[0, :V]
    if (~np.isnan(row)).any():
        assert got[0] == SR.lse(row[~np.isnan(row)][None])[0]
    tl = SR.target_logprobs(x[:, :V], t)
    assert tl[2] == 0.0 and tl[4] == 0.0                                # -100 and V: not counted


@pytest.mark.parametrize("n", [1, 5, 20])
def test_reference_topn_matches_torch_on_distinct_values_and_breaks_ties_low(n):
    g = np.random.default_rng(n)
    x = g.permutation(200).astype(np.float32).reshape(2, 100)           # distinct: torch.topk has one answer
    ids, lps = SR.topn(x, n)
    tv, ti = torch.topk(torch.from_numpy(x.astype(np.float64)), n, dim=-1)
    assert np.array_equal(ids, ti.numpy())
    want = torch.log_softmax(torch.from_numpy(x.astype(np.float64)), -1).gather(1, ti).numpy()
    assert np.allclose(lps, want, rtol=1e-12, atol=1e-12)
    x = SR.ties_case(256)
    ids, lps = SR.topn(x, n)
    for r in range(x.shape[0]):
        k = [i for i in ids[r] if i >= 0]
        vals = x[r, k].astype(np.float64)
        assert all(vals[j] > vals[j + 1] or (vals[j] == vals[j + 1] and k[j] < k[j + 1]) for j in range(len(k) - 1))
        assert len(k) == min(n, int((~np.isnan(x[r])).sum()))
        assert np.all(ids[r, len(k):] == -1) and np.all(np.isneginf(lps[r, len(k):]))
        # the same multiset of values as torch.topk over the non-NaN part
        fin = np.where(np.isnan(x[r]), -np.inf, x[r]).astype(np.float64)
        tv = torch.topk(torch.from_numpy(fin), len(k)).values.numpy() if k else np.zeros(0)
        assert np.array_equal(vals, tv)


@pytest.mark.parametrize("M", [1, 7, 1024, 5000])
def test_reference_loss_matches_torch_cross_entropy(M):
    V = 50
    g = torch.Generator().manual_seed(M)
    x = torch.randn((M, V), generator=g, dtype=torch.float64) * 3
    t = torch.randint(0, V, (M,), generator=g)
    t[::3] = SR.IGNORE
    if M == 1:
        t[0] = 4
    lp = SR.target_logprobs(x.numpy(), t.numpy())
    loss, n = SR.nll_mean(lp, t.numpy(), V)
    want = torch.nn.functional.cross_entropy(x, t, ignore_index=-100)
    assert n == int((t != SR.IGNORE).sum())
    assert loss == pytest.approx(float(want), rel=1e-12)
    loss, n = SR.nll_mean(lp, np.full((M,), SR.IGNORE), V)
    assert n == 0 and np.isnan(loss)
    assert bool(torch.isnan(torch.nn.functional.cross_entropy(x, torch.full((M,), -100), ignore_index=-100)))


def test_mutations_fail_on_the_gpu_tests_cases():
    """The GPU test's cases tell the rules apart: ties flipped to the higher index change the ids at every n it uses, and
    counting NaN changes the lse of the NaN row at every width it uses."""
    for V in (64, 1025):
        x = SR.ties_case(V)
        for n in (1, 5, 20):
            ids, _ = SR.topn(x, n)
            bad, _ = SR.topn(x, n, high_index_first=True)
            assert not np.array_equal(ids, bad), (V, n)
            assert not np.array_equal(ids[:3], bad[:3]), (V, n)        # on the plain rows already: a tie straddles rank n
    for V in SR.WIDTHS:
        x, t = SR.rows_case(V)
        good, bad = SR.lse(x[:, :V]), SR.lse(x[:, :V], count_nan=True)
        assert np.isnan(bad[0]) and not np.isnan(good[0]), V
        tl, tb = SR.target_logprobs(x[:, :V], t), SR.target_logprobs(x[:, :V], t, count_nan=True)
        if V > 1:                                                       # (at V = 1 the NaN row holds no value at all)
            assert np.isfinite(tl[0]) or np.isnan(x[0, V - 1])
            assert not np.array_equal(tl, tb, equal_nan=True), V
