"""Child process of tests/test_spec_gpu.py.  argv[1]:
  "fp16": VALLEY_PRECISION=fp16 is in the environment — one attention case through the oracle's three checks, the position
          invariance, and a speculative generation against plain greedy decoding, all on the fp16 storage type;
  "off":  a generation without the new arguments never loads libvalley_hip_spec.so.
Prints one JSON line."""
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def golden_inputs():
    from tests import golden_cfg as G
    from tests.test_model_gpu import build_golden_model
    model = build_golden_model()
    T = G.GCFG["T"]
    ids = torch.from_numpy(G.golden_ids("decode2")[0]).cuda()
    img = torch.from_numpy(G.golden_pixels(T, "mixed")).view(1, T, 3, 224, 224).cuda()
    return model, ids, img


def main():
    mode = sys.argv[1]
    res = {"mode": mode}
    if mode == "fp16":
        assert os.environ.get("VALLEY_PRECISION") == "fp16"
        from tests import test_spec_gpu as T
        from valley_amd import lib, runtime
        assert runtime.HALF == torch.float16 and T.HALF == torch.float16
        res["launches"] = T.attention_checks(T.C(1, 8, [249], 2, 320))
        T.test_spec_attention_position_invariance(250)
        T.test_spec_attention_agrees_with_rope_kv_and_llama_attention(250)
        model, ids, img = golden_inputs()
        want = model.generate(ids, images=img, max_new_tokens=16)
        got = model.generate(ids, images=img, max_new_tokens=16, prompt_lookup_num_tokens=3)
        res["tokens_equal"] = bool(torch.equal(got, want))
        res["storage"] = lib.load().vly_storage_dtype()
    else:
        from valley_amd import lib_spec
        model, ids, img = golden_inputs()
        seq = model.generate(ids, images=img, max_new_tokens=4)
        res["new_tokens"] = int(seq.shape[1] - ids.shape[1])
        res["spec_lib_loaded"] = lib_spec.loaded() or "valley_amd.spec" in sys.modules
    res["ok"] = True
    print(json.dumps(res))


main()
