"""Child process of tests/test_spec_rows_gpu.py.  argv[1]:
  "fp16": VALLEY_PRECISION=fp16 is in the environment — the attention and RoPE bit-equality checks and the position invariance
          on the fp16 storage type, and one geometry of the speculating batcher against the plain one;
  "off":  a plain ContinuousBatcher run never loads libvalley_hip_spec_rows.so.
Prints one JSON line."""
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def golden_prompts():
    from tests import golden_cfg as G
    from tests import test_spec_rows_gpu as T
    from tests.test_model_gpu import build_golden_model
    model = build_golden_model()
    n = G.GCFG["T"]
    img = torch.from_numpy(G.golden_pixels(n, "mixed")).view(1, n, 3, 224, 224).cuda()
    prompts = {"decode2": (torch.from_numpy(G.golden_ids("decode2")[0]).cuda(), None, img),
               "repeat": (torch.tensor([T.REPEAT], dtype=torch.long).cuda(), None, None)}
    return model, prompts


def main():
    mode = sys.argv[1]
    res = {"mode": mode}
    from tests import test_spec_rows_gpu as T
    if mode == "fp16":
        assert os.environ.get("VALLEY_PRECISION") == "fp16"
        from valley_amd import lib, runtime
        assert runtime.HALF == torch.float16 and T.HALF == torch.float16
        w = T.make_world()
        res["positions"] = T.attention_bit_equality(w)
        T.attention_position_invariance(w)
        T.rope_bit_equality(w)
        model, prompts = golden_prompts()
        plan = [("repeat", 0, 12, {}), ("decode2", 1, 3, {}), ("repeat", 5, 6, {})]       # request 2 reuses request 1's slot
        want, _, _ = T.serve(model, prompts, plan, {}, False, 2, 320)
        got, stats, _ = T.serve(model, prompts, plan, dict(prompt_lookup_num_tokens=3), False, 2, 320)
        for r in range(3):
            assert got[r][:plan[r][2]] == want[r][:plan[r][2]], (r, got[r], want[r])
        res["accepted"] = sum(s["accepted"] for s in stats.values())
        res["storage"] = lib.load().vly_storage_dtype()
    else:
        from valley_amd import lib_spec_rows
        model, prompts = golden_prompts()
        got, _, _ = T.serve(model, prompts, [("decode2", 0, 4, {}), ("repeat", 1, 3, {})], {}, False, 2, 320)
        res["tokens"] = len(got[0])
        res["rows_lib_loaded"] = lib_spec_rows.loaded() or "libvalley_hip_spec_rows.so" in open("/proc/self/maps").read()
    res["ok"] = True
    print(json.dumps(res))


main()
