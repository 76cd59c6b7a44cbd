"""Child process of tests/test_spec_sampling_gpu.py.  argv[1]:
  "fp16": VALLEY_PRECISION=fp16 is in the environment — a seeded sampled speculative generation (k = 3, T = 0.2) against the same
          seeded call without speculation, on the fp16 storage type;
  "off":  a plain seeded sampled generation loads neither libvalley_hip_spec.so nor libvalley_hip_spec_sample.so, and a greedy
          speculative one loads the first only.
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
    from valley_amd import lib, lib_spec, lib_spec_sample, runtime
    model, ids, img = golden_inputs()
    sampled = dict(do_sample=True, temperature=0.2, seed=7)
    if mode == "fp16":
        assert os.environ.get("VALLEY_PRECISION") == "fp16" and runtime.HALF == torch.float16
        want = model.generate(ids, images=img, max_new_tokens=24, **sampled)
        out = model.generate(ids, images=img, max_new_tokens=24, prompt_lookup_num_tokens=3, return_dict_in_generate=True, **sampled)
        res["tokens_equal"] = bool(torch.equal(out.sequences, want))
        res["new_tokens"] = int(out.sequences.shape[1] - ids.shape[1])
        res["steps_plus_accepted"] = out.speculation["steps"] + out.speculation["accepted"]
        res["storage"] = lib.load().vly_storage_dtype()
    else:
        seq = model.generate(ids, images=img, max_new_tokens=4, **sampled)
        res["new_tokens"] = int(seq.shape[1] - ids.shape[1])
        res["spec_lib_loaded"] = lib_spec.loaded() or "valley_amd.spec" in sys.modules
        res["spec_sample_lib_loaded"] = lib_spec_sample.loaded()
        model.generate(ids, images=img, max_new_tokens=12, prompt_lookup_num_tokens=3)
        res["greedy_lookup_loads_spec"] = lib_spec.loaded()
        res["greedy_lookup_loads_spec_sample"] = lib_spec_sample.loaded()
    res["ok"] = True
    print(json.dumps(res))


main()
