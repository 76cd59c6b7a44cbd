"""The float64 truth of token log-probabilities (numpy): the log-sum-exp over a row's non-NaN values, the target rule, the
top-n with ties to the lower index, and the mean negative log-likelihood.  tests/test_score_cpu.py pins it to
torch.log_softmax / torch.topk / torch.nn.functional.cross_entropy in float64; tests/test_score_gpu.py checks the kernels of
libvalley_hip_score.so against it.  The cases both use are built here, so the mutation proof of the CPU test runs on exactly
the rows the GPU test runs on."""
import numpy as np

IGNORE = -100


def lse(x, count_nan=False):
    """x [R, V] -> float64 [R]: m + log(sum exp(x - m)) over the non-NaN values, 0 when the maximum is not finite (or the row
    holds no value).  ``count_nan``: the mutation — a NaN poisons its row, as a plain log-sum-exp would."""
    x = np.asarray(x, dtype=np.float64)
    out = np.zeros((x.shape[0],), dtype=np.float64)
    for r in range(x.shape[0]):
        row = x[r]
        if count_nan and np.isnan(row).any():
            out[r] = np.nan
            continue
        v = row[~np.isnan(row)]
        if v.size == 0:
            continue
        m = v.max()
        if not np.isfinite(m):
            continue
        out[r] = m + np.log(np.exp(v - m).sum())
    return out


def target_logprobs(x, targets, count_nan=False):
    """-> float64 [R]: x[r, t] - lse[r] for t = targets[r] in [0, V), 0 otherwise (-100 included)."""
    x = np.asarray(x, dtype=np.float64)
    L = lse(x, count_nan)
    out = np.zeros((x.shape[0],), dtype=np.float64)
    for r, t in enumerate(np.asarray(targets).tolist()):
        if 0 <= t < x.shape[1]:
            out[r] = x[r, t] - L[r]
    return out


def topn(x, n, high_index_first=False):
    """-> (ids int64 [R, n], lps float64 [R, n]): the n largest non-NaN values, best first, ties to the LOWER index; a row with
    fewer non-NaN values ends in -1 / -inf.  ``high_index_first``: the mutation — ties to the higher index."""
    x = np.asarray(x, dtype=np.float64)
    L = lse(x)
    ids = np.full((x.shape[0], n), -1, dtype=np.int64)
    lps = np.full((x.shape[0], n), -np.inf, dtype=np.float64)
    for r in range(x.shape[0]):
        idx = [i for i in range(x.shape[1]) if not np.isnan(x[r, i])]
        idx.sort(key=lambda i: (-x[r, i], -i if high_index_first else i))
        for k, i in enumerate(idx[:n]):
            ids[r, k] = i
            lps[r, k] = x[r, i] - L[r]
    return ids, lps


def nll_mean(target_lp, targets, V):
    """-> (loss float64, count): -(sum of target_lp over the targets in [0, V)) / count, NaN when count is 0."""
    t = np.asarray(targets)
    keep = (t >= 0) & (t < V)
    n = int(keep.sum())
    if n == 0:
        return float("nan"), 0
    return float(-np.asarray(target_lp, dtype=np.float64)[keep].sum() / n), n


# ---- the cases of the kernel tests ----------------------------------------------------------------------------------------
WIDTHS = (1, 63, 64, 1023, 1024, 1025, 4097, 32000, 32768, 32769, 40000)
ROWS = 5
PAD = 3


def rows_case(V, seed=0):
    """-> (x fp32 [5, V + 3] with poisoned padding, targets int32 [5]).  Row 0: random with NaNs sprinkled in; row 1: all -inf
    (lse 0); row 2: random with a +inf maximum (lse 0); row 3: one finite value among -inf; row 4: plain random."""
    g = np.random.default_rng(1000 + V + seed)
    x = (g.standard_normal((ROWS, V + PAD)) * 4.0).astype(np.float32)
    for i in g.integers(0, V, size=max(1, V // 50)):
        x[0, i] = np.nan
    x[1, :V] = -np.inf
    x[2, int(g.integers(0, V))] = np.inf
    one = int(g.integers(0, V))
    keep = x[3, one]
    x[3, :V] = -np.inf
    x[3, one] = keep
    x[:, V] = np.nan
    x[:, V + 1] = np.inf
    x[:, V + 2] = 1e30
    targets = np.array([V - 1, 0, IGNORE, one, V], dtype=np.int32)      # row 4: an id outside the row; row 2: ignored
    return x, targets


def rows_case_targets(V):
    """Further target vectors over the same rows: every special id of the contract on a plain row, and a NaN at a target."""
    return [np.array([0, V - 1, V - 1, 0, -1], dtype=np.int32), np.array([IGNORE, IGNORE, 0, V, 0], dtype=np.int32),
            np.array([V, -1, V, IGNORE, V - 1], dtype=np.int32)]


GRID = np.array([-np.inf, -8.0, -3.5, -2.0, -1.0, -0.5, -0.0, 0.0, 0.25, 0.5, 1.0, 1.5, 2.0, 3.0, 4.5, 6.0], dtype=np.float32)


def ties_case(V, seed=0):
    """x fp32 [6, V]: rows drawn from a 16-value grid (-0.0 and +0.0, -inf among them), so that every rank of a top-n with
    n <= 20 sits inside a run of equal values when V >= 64; row 3 holds NaNs, row 4 only 3 non-NaN values, row 5 none."""
    g = np.random.default_rng(77 + V + seed)
    x = GRID[g.integers(0, len(GRID), size=(6, V))].copy()
    x[3, g.integers(0, V, size=max(1, V // 8))] = np.nan
    x[4, :] = np.nan
    x[4, [V - 1, 0, V // 2]] = [1.0, 1.0, -np.inf]
    x[5, :] = np.nan
    return x


def loss_case(M, V=32000, seed=0):
    """target_lp fp32 [M] (negative, a wide range) and targets int32 [M] with about a third ignored or outside [0, V)."""
    g = np.random.default_rng(5 + M + seed)
    lp = (-np.abs(g.standard_normal(M)) * 10.0 ** g.integers(-3, 2, size=M)).astype(np.float32)
    t = g.integers(0, V, size=M).astype(np.int32)
    kind = g.integers(0, 6, size=M)
    t[kind == 0] = IGNORE
    t[kind == 1] = np.where(g.integers(0, 2, size=int((kind == 1).sum())) == 0, -1, V).astype(np.int32)
    t[0] = 5                                                            # at least one counted
    return lp, t
