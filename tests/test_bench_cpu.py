"""CPU checks of bench.py --dump-outputs: the sample of the prefill step's outputs does not depend on how the batch is split
into stream sub-batches, reads through views of padded buffers, and is written as float arrays under the size limit."""
import os
import sys
from types import SimpleNamespace

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


def test_prefill_dump_is_the_same_sample_for_any_split(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_LOGIT_ROWS", 17)
    monkeypatch.setattr(bench, "DUMP_KV_PER_LAYER", 300)
    S, V, L, B, heads = 20, 50, 3, 5, 2
    g = torch.Generator().manual_seed(0)
    logits = torch.randn(B, S, V + 7, generator=g)[:, :, :V]                 # a view of a V-padded buffer, as HipLlama.logits
    K = [torch.randn(B, heads, S + 4, 128, generator=g).bfloat16() for _ in range(L)]    # caches deeper than S
    Vc = [torch.randn(B, heads, S + 4, 128, generator=g).bfloat16() for _ in range(L)]

    def out(b0, b1):
        return SimpleNamespace(logits=logits[b0:b1], past_key_values=SimpleNamespace(k=[t[b0:b1] for t in K], v=[t[b0:b1] for t in Vc]))

    rows = torch.from_numpy(bench._sample(B * S, 17, "logits_rows"))
    idx = torch.from_numpy(bench._sample(B * heads * S * 128, 300, "kv"))
    want = {"logits_last": logits[:, -1].numpy(), "logits_rows": logits.reshape(B * S, V)[rows].numpy(),
            "kv_k": np.stack([t[:, :, :S].float().reshape(-1)[idx].numpy() for t in K]),
            "kv_v": np.stack([t[:, :, :S].float().reshape(-1)[idx].numpy() for t in Vc])}
    for cuts in ([0, B], [0, 2, B], [0, 1, 3, B]):
        got = bench.prefill_outputs([out(cuts[i], cuts[i + 1]) for i in range(len(cuts) - 1)], cuts, S)
        assert got.keys() == want.keys()
        for k in want:
            assert np.array_equal(got[k], want[k]), (cuts, k)
    bench.dump_outputs(str(tmp_path), got)
    for k in want:
        a = np.load(tmp_path / f"{k}.npy")
        assert a.dtype == np.float32 and np.array_equal(a, want[k])


def test_default_line_dump_fits_the_limit():
    """c3 (8 sequences x 336 positions, 40 layers) and the largest batch any configuration runs (64 sequences)."""
    V = bench.VOCAB_TEXT + 6
    for seqs, layers in ((8, 40), (64, 40)):
        nbytes = 4 * (seqs * V + bench.DUMP_LOGIT_ROWS * V + 2 * layers * bench.DUMP_KV_PER_LAYER)
        assert nbytes <= bench.DUMP_LIMIT_BYTES
