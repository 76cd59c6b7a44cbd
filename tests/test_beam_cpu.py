"""Beam search without a GPU: the host bookkeeping (valley_amd.beam) against transformers' own beam search on a tiny random
Llama, fed with candidates computed from the same model's logits the way the device computes them; the companion library's
host-side argument checks (its exports and ABI version: tests/test_companions_cpu.py); argument checks of generate()."""
import pytest
import torch


EOS = 7
V = 101


def tiny_llama(seed=0):
    from transformers import LlamaConfig, LlamaForCausalLM
    torch.manual_seed(seed)
    cfg = LlamaConfig(vocab_size=V, hidden_size=64, intermediate_size=128, num_hidden_layers=2, num_attention_heads=4,
                      num_key_value_heads=4, max_position_embeddings=128, pad_token_id=0, bos_token_id=1, eos_token_id=EOS)
    model = LlamaForCausalLM(cfg).eval()
    with torch.no_grad():
        model.lm_head.weight[EOS] *= 4.0                 # EOS is actually reached, at different lengths per beam
        model.lm_head.weight[EOS] += 0.05
    return model


class LastTokenIs:
    """A per-row stopping criterion: the candidate's last token is ``tok`` (a bool tensor, one per row)."""

    def __init__(self, tok):
        self.tok = tok

    def __call__(self, input_ids, scores, **kw):
        return input_ids[:, -1] == self.tok


class Row0Contains:
    """The reference's keyword criterion in shape: one Python bool for the whole batch, from row 0's generated part."""

    def __init__(self, start, tok):
        self.start, self.tok = start, tok

    def __call__(self, input_ids, scores, **kw):
        return bool((input_ids[0, self.start:] == self.tok).any())


def driver(model, ids, nb, max_new, eos, pad, length_penalty, early_stopping, nrs, criteria=()):
    """valley_amd.beam fed with top-K candidates of log_softmax(logits) + running, computed from the model's cached
    forward; the cache follows the running beams (what the device does with vly_kv_beam_reorder)."""
    from transformers import DynamicCache
    from valley_amd.beam import BeamSearch
    B, S = ids.shape
    st = BeamSearch(ids, nb, S + max_new, eos_ids=[eos] if eos is not None else None, pad_token_id=pad,
                    length_penalty=length_penalty, early_stopping=early_stopping, num_return_sequences=nrs)
    K, R = st.K, B * nb
    cache = DynamicCache()
    with torch.no_grad():
        out = model(input_ids=ids.repeat_interleave(nb, 0), past_key_values=cache, use_cache=True)
        running = st.initial_running()
        while True:
            logits = out.logits[:, -1, :].float()
            acc = (torch.log_softmax(logits, -1) + running[:, None]).view(B, nb * V)
            score, idx = torch.topk(acc, K)
            parent = idx // V + torch.arange(B)[:, None] * nb
            seqs = st.candidates(score.reshape(-1), (idx % V).reshape(-1), parent.reshape(-1))
            hits = st.eos_hits()
            for c in criteria:
                r = c(seqs, None)
                hits = hits | (r if isinstance(r, torch.Tensor) else torch.full_like(hits, bool(r)))
            st.advance(hits)
            if st.done:
                break
            running = st.run_score.reshape(-1).clone()
            cache.reorder_cache(st.run_ptr[:, :, st.cur_len - 1 - S].reshape(-1).long())
            tok = st.run_seq[:, :, st.cur_len - 1].reshape(R, 1)
            out = model(input_ids=tok, past_key_values=cache, use_cache=True)
    return st.result()


GRID = [(nb, B, lp, es, nrs) for nb in (2, 4) for B in (1, 2) for lp in (1.0, 0.0, 2.0, -0.5) for es in (False, True, "never")
        for nrs in sorted({1, nb})]


@pytest.fixture(scope="module")
def model():
    return tiny_llama()


@pytest.mark.parametrize("nb,B,lp,es,nrs", GRID)
@pytest.mark.parametrize("crit", [None, "row0", "last"])
def test_bookkeeping_matches_hf(model, nb, B, lp, es, nrs, crit):
    from transformers import StoppingCriteriaList
    g = torch.Generator().manual_seed(nb * 100 + B)
    S, max_new = 5, 9
    ids = torch.randint(8, V, (B, S), generator=g)
    criteria = {None: [], "row0": [Row0Contains(S, 13)], "last": [LastTokenIs(21)]}[crit]
    ref = model.generate(input_ids=ids, attention_mask=torch.ones_like(ids), num_beams=nb, do_sample=False,
                         max_new_tokens=max_new, eos_token_id=EOS, pad_token_id=0, length_penalty=lp, early_stopping=es,
                         num_return_sequences=nrs, return_dict_in_generate=True, output_scores=True,
                         stopping_criteria=StoppingCriteriaList(criteria) if criteria else None)
    seq, sc = driver(model, ids, nb, max_new, EOS, 0, lp, es, nrs, criteria)
    assert seq.shape == ref.sequences.shape
    assert torch.equal(seq, ref.sequences)
    torch.testing.assert_close(sc, ref.sequences_scores.float(), atol=1e-5, rtol=0)


def test_grid_reaches_eos_and_varied_lengths(model):
    """The bias on EOS makes hypotheses finish early: some returned sequences are padded, and lengths differ from greedy."""
    ids = torch.randint(8, V, (2, 5), generator=torch.Generator().manual_seed(3))
    seq, _ = driver(model, ids, 4, 9, EOS, 0, 1.0, False, 4)
    gen = seq[:, 5:]
    assert bool((gen == EOS).any())
    greedy = model.generate(input_ids=ids, attention_mask=torch.ones_like(ids), num_beams=1, do_sample=False, max_new_tokens=9,
                            eos_token_id=EOS, pad_token_id=0)
    assert not torch.equal(seq[::4][:, :greedy.shape[1]], greedy) or seq.shape[1] != greedy.shape[1]


def test_bookkeeping_without_eos_runs_to_max_length(model):
    ids = torch.randint(8, V, (1, 4), generator=torch.Generator().manual_seed(5))
    ref = model.generate(input_ids=ids, attention_mask=torch.ones_like(ids), num_beams=3, do_sample=False, max_new_tokens=6,
                         eos_token_id=None, pad_token_id=0, return_dict_in_generate=True, output_scores=True,
                         num_return_sequences=2)
    seq, sc = driver(model, ids, 3, 6, None, 0, 1.0, False, 2)
    assert seq.shape == (2, 10) and torch.equal(seq, ref.sequences)
    torch.testing.assert_close(sc, ref.sequences_scores.float(), atol=1e-5, rtol=0)


def test_bookkeeping_rejects_bad_arguments():
    from valley_amd.beam import BeamSearch
    ids = torch.zeros((1, 3), dtype=torch.long)
    with pytest.raises(ValueError):
        BeamSearch(ids, 2, 6, num_return_sequences=3)
    with pytest.raises(ValueError):
        BeamSearch(ids, 2, 6, early_stopping="sometimes")
    with pytest.raises(ValueError):
        BeamSearch(ids, 2, 3)


def test_beam_library_rejects_bad_arguments_without_a_gpu():
    """Argument checks run on the host: -22 and a message, no launch."""
    from valley_amd import lib_beam
    h = lib_beam.load()
    assert h.vly_beam_candidates(None, 10, 10, 1, 2, None, 4, None, 0, None, None, None, None, None, None) == -22
    assert b"vly_beam_candidates" in h.vly_beam_last_error()
    assert h.vly_beam_select(None, None, None, None, 1, 17, 34, None, None, None, None) == -22
    assert h.vly_kv_beam_reorder(None, 1, 2, 1, 8, 3, None, 0, None, 8, None) == -22
    assert b"vly_kv_beam_reorder" in h.vly_beam_last_error()
    assert h.vly_beam_scratch_bytes(2, 4, 8) >= 2 * 4 * 8 * 8
    assert h.vly_beam_scratch_bytes(0, 4, 8) == 0


def test_ops_beam_wrappers_reject_cpu_tensors():
    from valley_amd import lib, ops
    with pytest.raises(lib.ValleyHipError):
        ops.beam_select(torch.zeros(8), torch.zeros(8, dtype=torch.int32), torch.zeros(8, dtype=torch.int32),
                        torch.zeros(8, dtype=torch.uint8), 1, 2)
    with pytest.raises(ValueError):
        ops.kv_beam_table([torch.zeros((2, 1, 4, 128), dtype=torch.bfloat16)], [torch.zeros((2, 1, 4, 128))], "cpu")
    assert ops.beam_k(4, 0) == 8 and ops.beam_k(4, 1) == 8 and ops.beam_k(4, 2) == 12
