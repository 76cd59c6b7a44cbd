"""Logits processors without a GPU: the companion library's host-side argument checks (its exports and ABI version:
tests/test_companions_cpu.py); the
parameter table and its HF messages; and the reference loops of tests/test_logits_process_gpu.py (tests/logits_ref.py)
pinned to ``LlamaForCausalLM.generate`` on a tiny CPU Llama, greedy and beam, over a grid of processor settings."""
import pytest
import torch

from tests import logits_ref

EOS = 7
V = 101


def test_logits_library_rejects_bad_arguments_without_a_gpu():
    from valley_amd import lib_logits
    h = lib_logits.load()
    # logits_process(logits, ld, V, R, params, hist, hist_ld, len, per_row, len_add, tok, eos, n_eos, log_softmax, stream)
    assert h.vly_logits_process(None, 10, 10, 1, None, None, 8, None, 0, 0, None, None, 0, 0, None) == -22
    assert b"vly_logits_process" in h.vly_logits_last_error()
    assert h.vly_logits_process(64, 10, 11, 1, 64, 64, 8, None, 0, 0, None, None, 0, 0, None) == -22       # ld < V
    assert h.vly_logits_process(64, 1 << 19, 1 << 19, 1, 64, 64, 8, None, 0, 0, None, None, 0, 0, None) == -22   # V too wide
    assert h.vly_logits_process(64, 10, 10, 1, 64, 64, 8, None, 1, 0, None, None, 0, 0, None) == -22        # per-row, no len
    assert h.vly_logits_process(64, 10, 10, 1, 64, 64, 8, None, 0, 0, None, None, 2, 0, None) == -22        # n_eos, no eos
    assert h.vly_logits_history_gather(None, 2, 8, None, 0, None, 4, None) == -22
    assert h.vly_logits_history_gather(64, 8193, 8, 64, 0, None, 4, None) == -22
    assert b"vly_logits_history_gather" in h.vly_logits_last_error()
    assert h.vly_logits_beam_candidates(None, 10, 10, 1, 2, None, 4, None, 0, None, None, None, None, None, None) == -22
    assert b"vly_logits_beam_candidates" in h.vly_logits_last_error()
    assert h.vly_logits_beam_scratch_bytes(2, 4, 8) >= 2 * 4 * 8 * 8
    assert h.vly_logits_beam_scratch_bytes(0, 4, 8) == 0
    from valley_amd import lib_beam
    assert h.vly_logits_beam_scratch_bytes(3, 4, 12) == lib_beam.load().vly_beam_scratch_bytes(3, 4, 12)


def hf_message(fn):
    with pytest.raises(ValueError) as e:
        fn()
    return str(e.value)


def test_processor_rows_table_and_hf_messages():
    from transformers.generation.logits_process import (MinLengthLogitsProcessor, MinNewTokensLengthLogitsProcessor,
                                                        NoRepeatNGramLogitsProcessor, RepetitionPenaltyLogitsProcessor)
    from valley_amd import ops
    t = ops.processor_rows([1.3, None, 0.7], [0, 2, 3], 5, [None, 4, 0], prompt_len=[3, 3, 10])
    assert t.dtype == torch.int32 and tuple(t.shape) == (3, 4)
    assert t.view(torch.float32)[:, 0].tolist() == [pytest.approx(1.3), 1.0, pytest.approx(0.7)]
    assert t.view(torch.float32)[0, 0].item() == torch.tensor(1.3, dtype=torch.float32).item()
    assert t[:, 1].tolist() == [0, 2, 3] and t[:, 2].tolist() == [5, 7, 5] and t[:, 3].tolist() == [0, 0, 0]
    n = ops.processor_rows()
    assert n.tolist() == [[torch.tensor(1.0).view(torch.int32).item(), 0, 0, 0]]
    assert ops.processor_rows(1).view(torch.float32)[0, 0].item() == 1.0              # 1.0 is off, as in HF
    for bad in (0.0, -1.2, 2):
        assert hf_message(lambda: ops.processor_rows(bad)) == hf_message(lambda: RepetitionPenaltyLogitsProcessor(bad))
    for bad in (-1, 2.5):
        assert hf_message(lambda: ops.processor_rows(None, bad)) == hf_message(lambda: NoRepeatNGramLogitsProcessor(bad))
    assert hf_message(lambda: ops.processor_rows(min_length=-2)) == hf_message(lambda: MinLengthLogitsProcessor(-2, 7))
    assert hf_message(lambda: ops.processor_rows(min_new_tokens=-1)) == \
        hf_message(lambda: MinNewTokensLengthLogitsProcessor(3, -1, 7))
    with pytest.raises(ValueError):
        ops.processor_rows([1.1, 1.2], [2, 3, 4])


def test_ops_logits_wrappers_reject_cpu_tensors():
    from valley_amd import lib, ops
    x = torch.zeros((2, 16))
    p = ops.processor_rows([1.2, 1.2])
    h = torch.zeros((2, 8), dtype=torch.int32)
    with pytest.raises(lib.ValleyHipError):
        ops.logits_process(x, p, h, None, 4)
    with pytest.raises(lib.ValleyHipError):
        ops.logits_history_gather(h, torch.zeros(2, dtype=torch.int32), 0, 4)
    with pytest.raises(lib.ValleyHipError):
        ops.logits_beam_candidates(x, torch.zeros(2), 1, 2, 4, None, torch.zeros(1024, dtype=torch.uint8))


def test_generate_rejects_bad_processor_arguments_before_any_work():
    from valley_amd.generation import processor_table
    with pytest.raises(ValueError, match="penalty"):
        processor_table((0.0, None, None, None), 4, [7], "cpu")
    assert processor_table((None, None, None, None), 4, [7], "cpu") is None
    assert processor_table((1.0, 0, 3, 0), 4, [7], "cpu") is None           # nothing would act
    assert processor_table((None, None, 9, 2), 4, None, "cpu") is None      # no EOS: no min length
    t = processor_table((1.3, 2, None, 5), 4, [7], "cpu")
    assert t[0, 1].item() == 2 and t[0, 2].item() == 9


def test_completion_passes_the_processor_keys_through():
    import inspect
    from valley_amd.valley_model import ValleyLlamaForCausalLM
    src = inspect.getsource(ValleyLlamaForCausalLM.completion)
    for k in ("repetition_penalty", "no_repeat_ngram_size", "min_length", "min_new_tokens"):
        assert f'"{k}"' in src


# ---- the reference loops against transformers' generate ---------------------------------------------------------------------

def tiny_llama(seed=0):
    from transformers import LlamaConfig, LlamaForCausalLM
    torch.manual_seed(seed)
    cfg = LlamaConfig(vocab_size=V, hidden_size=64, intermediate_size=128, num_hidden_layers=2, num_attention_heads=4,
                      num_key_value_heads=4, max_position_embeddings=128, pad_token_id=0, bos_token_id=1, eos_token_id=EOS)
    model = LlamaForCausalLM(cfg).eval()
    with torch.no_grad():
        model.lm_head.weight[EOS] *= 4.0                 # EOS is reached early: min_new_tokens has something to keep out
        model.lm_head.weight[EOS] += 0.05
    return model


@pytest.fixture(scope="module")
def model():
    return tiny_llama()


def make_inputs(B, S, padded, seed):
    g = torch.Generator().manual_seed(seed)
    ids = torch.randint(8, V, (B, S), generator=g)
    ids[:, S // 2:] = ids[:, :S - S // 2]                # repeated content: n-grams of the prompt are banned
    mask = torch.ones_like(ids)
    if padded and B > 1:
        mask[1, :2] = 0
        ids[1, :2] = 0
    return ids, mask


def hf_stepper(model, ids, mask, nb=1):
    """step(tok) for logits_ref: a cached HF forward over the prompts repeated nb times, positions from the padding mask
    (what generate passes); ``reorder`` follows the beams."""
    from transformers import DynamicCache
    state = {"cache": DynamicCache(), "mask": mask.repeat_interleave(nb, 0)}
    rows = ids.repeat_interleave(nb, 0)

    def step(tok):
        with torch.no_grad():
            m = state["mask"]
            if tok is None:
                pos = (m.cumsum(-1) - 1).masked_fill(m == 0, 1)
                out = model(input_ids=rows, attention_mask=m, position_ids=pos, past_key_values=state["cache"], use_cache=True)
            else:
                m = torch.cat([m, torch.ones((m.shape[0], 1), dtype=m.dtype)], 1)
                state["mask"] = m
                pos = (m.sum(-1, keepdim=True) - 1)
                out = model(input_ids=tok[:, None], attention_mask=m, position_ids=pos, past_key_values=state["cache"],
                            use_cache=True)
        return out.logits[:, -1, :].float()

    def reorder(parent):
        state["cache"].reorder_cache(parent)
        state["mask"] = state["mask"].index_select(0, parent)
    return step, reorder


GRID = [(rp, n, mn) for rp in (None, 0.7, 1.3) for n in (0, 2, 3) for mn in (0, 6)]


@pytest.mark.parametrize("rp,n,mn", GRID)
@pytest.mark.parametrize("B,padded", [(1, False), (2, True)])
def test_greedy_loop_matches_hf_generate(model, rp, n, mn, B, padded):
    ids, mask = make_inputs(B, 8, padded, seed=B * 7 + n)
    kw = dict(repetition_penalty=rp, no_repeat_ngram_size=n or None, min_new_tokens=mn or None)
    ref = model.generate(input_ids=ids, attention_mask=mask, do_sample=False, num_beams=1, max_new_tokens=10, eos_token_id=EOS,
                         pad_token_id=0, **kw)
    step, _ = hf_stepper(model, ids, mask)
    procs = logits_ref.hf_processors(rp, n, None, mn, prompt_len=ids.shape[1], eos=EOS)
    got = logits_ref.greedy_loop(step, ids, 10, procs, eos=EOS, pad=0)
    assert torch.equal(got, ref)


@pytest.mark.parametrize("rp,n,mn", GRID)
@pytest.mark.parametrize("B,padded", [(1, False), (2, True)])
def test_beam_loop_matches_hf_generate(model, rp, n, mn, B, padded):
    ids, mask = make_inputs(B, 8, padded, seed=B * 11 + n)
    kw = dict(repetition_penalty=rp, no_repeat_ngram_size=n or None, min_new_tokens=mn or None)
    ref = model.generate(input_ids=ids, attention_mask=mask, do_sample=False, num_beams=3, max_new_tokens=8, eos_token_id=EOS,
                         pad_token_id=0, **kw)
    step, reorder = hf_stepper(model, ids, mask, nb=3)
    procs = logits_ref.hf_processors(rp, n, None, mn, prompt_len=ids.shape[1], eos=EOS)
    got, _ = logits_ref.beam_loop(step, reorder, ids, 3, 8, procs, eos=EOS, pad=0)
    assert torch.equal(got, ref)


def test_grid_processors_change_the_output(model):
    """The grid is not vacuous: each processor changes some greedy output of the tiny model."""
    ids, mask = make_inputs(2, 8, True, seed=3)
    for eos, kw in ((None, dict(repetition_penalty=1.3)), (None, dict(no_repeat_ngram_size=2)), (EOS, dict(min_new_tokens=6))):
        base = model.generate(input_ids=ids, attention_mask=mask, do_sample=False, max_new_tokens=10, eos_token_id=eos,
                              pad_token_id=0)
        other = model.generate(input_ids=ids, attention_mask=mask, do_sample=False, max_new_tokens=10, eos_token_id=eos,
                               pad_token_id=0, **kw)
        assert other.shape != base.shape or not torch.equal(other, base), kw
