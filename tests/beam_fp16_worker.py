"""Child process of tests/test_beam_gpu.py::test_generate_beams_fp16_library (VALLEY_PRECISION=fp16 in the environment): beam
search on the fp16-storage library — generate(num_beams=4) through the captured session and through the generic forward, both
against the test's plain-torch beam search.  Prints one JSON line."""
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
assert os.environ.get("VALLEY_PRECISION") == "fp16"


def main():
    from tests.test_beam_gpu import golden_model, inputs, torch_beam
    from valley_amd import lib, ops
    ops.GEMM_MODE = "tiles"                                  # the GPU suite's pinned dispatch (tests/conftest.py)
    model = golden_model()
    ids, mask, img = inputs("main")
    ref, _ = torch_beam(model, ids, mask, img, 4, 5)
    kw = dict(images=img, attention_mask=mask, max_new_tokens=5, num_beams=4)
    a = model.generate(ids, use_graph=True, **kw)
    c = model.generate(ids, use_graph=None, **kw)
    print(json.dumps({"library": os.path.basename(lib.lib_path()), "dtype": str(model.dtype),
                      "graph_equals_reference": bool(torch.equal(a, ref)), "generic_equals_reference": bool(torch.equal(c, ref))}))


if __name__ == "__main__":
    main()
