"""Child process of tests/test_logits_process_gpu.py::test_processors_on_other_precisions (VALLEY_PRECISION=fp16 or fp32 in
the environment): generate() with logits processors on the fp16-storage library or the fp32 engine — greedy through the
captured, eager and generic routes, beam search with an EOS and min_new_tokens — against the test's reference loops
(tests/logits_ref.py).  Prints one JSON line."""
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
assert os.environ.get("VALLEY_PRECISION") in ("fp16", "fp32")


def main():
    from tests import logits_ref
    from tests.test_logits_process_gpu import beam_stepper, golden_model, inputs, ref_greedy
    from valley_amd import lib, ops, runtime
    ops.GEMM_MODE = "tiles"                                  # the GPU suite's pinned dispatch (tests/conftest.py)
    model = golden_model()
    ids, mask, img = inputs("main")
    S = ids.shape[1]
    kw = dict(repetition_penalty=1.3, no_repeat_ngram_size=2)
    ref = ref_greedy(model, ids, mask, img, 8, **kw)
    greedy = {str(ug): bool(torch.equal(model.generate(ids, images=img, attention_mask=mask, max_new_tokens=8, use_graph=ug,
                                                       **kw), ref)) for ug in (True, False, None)}
    # beams: the penalty and n-grams, then an EOS kept out by min_new_tokens
    step, reorder = beam_stepper(model, ids, mask, img, 4)
    bref, _ = logits_ref.beam_loop(step, reorder, ids, 4, 5, logits_ref.hf_processors(1.3, 2, prompt_len=S))
    beams = {str(ug): bool(torch.equal(model.generate(ids, images=img, attention_mask=mask, max_new_tokens=5, num_beams=4,
                                                      use_graph=ug, **kw), bref.cuda())) for ug in (True, None)}
    eos = int(bref[0, S + 1])
    step, reorder = beam_stepper(model, ids, mask, img, 4)
    eref, _ = logits_ref.beam_loop(step, reorder, ids, 4, 5, logits_ref.hf_processors(min_new_tokens=3, prompt_len=S, eos=eos),
                                   eos=eos)
    beams_eos = {str(ug): bool(torch.equal(model.generate(ids, images=img, attention_mask=mask, max_new_tokens=5, num_beams=4,
                                                          eos_token_id=eos, pad_token_id=0, min_new_tokens=3, use_graph=ug),
                                           eref.cuda())) for ug in (True, None)}
    print(json.dumps({"precision": runtime.PRECISION, "library": os.path.basename(lib.lib_path()), "engine": model.model.precision,
                      "greedy_equal_reference": greedy, "beams_equal_reference": beams, "beams_eos_equal_reference": beams_eos,
                      "eos_kept_out": bool(not (eref[:, S:S + 3] == eos).any())}))


if __name__ == "__main__":
    main()
