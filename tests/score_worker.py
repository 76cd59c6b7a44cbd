"""Child process of tests/test_score_gpu.py: a plain generate() — no labels, no log-probabilities — never maps
libvalley_hip_score.so.  Prints one JSON line."""
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    from tests import golden_cfg as G
    from tests.test_model_gpu import build_golden_model
    from valley_amd import lib_score, ops
    ops.GEMM_MODE = "tiles"
    model = build_golden_model()
    T = G.GCFG["T"]
    ids, _ = G.golden_ids("decode")
    img = torch.from_numpy(G.golden_pixels(T, "mixed")).view(1, T, 3, 224, 224).cuda()
    seq = model.generate(torch.from_numpy(ids).cuda(), images=img, max_new_tokens=4)
    out = model.generate(torch.from_numpy(ids).cuda(), images=img, max_new_tokens=4, return_dict_in_generate=True)
    res = {"new_tokens": int(seq.shape[1] - ids.shape[1]), "same": bool(torch.equal(seq, out.sequences)),
           "has_logprobs": hasattr(out, "token_logprobs"), "score_lib_loaded": lib_score.loaded(),
           "score_lib_mapped": "libvalley_hip_score" in open("/proc/self/maps").read(), "ok": True}
    print(json.dumps(res))


main()
