"""Child process of tests/test_wq_gpu.py.  argv[1]:
  "fp16": VALLEY_PRECISION=fp16 is in the environment — the kernel checks of tests/wq_checks.py on the fp16 storage type;
  "off":  an engine built without the switch holds no int8 weights and never loads libvalley_hip_wq.so.
Prints one JSON line."""
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    mode = sys.argv[1]
    res = {"mode": mode}
    if mode == "fp16":
        assert os.environ.get("VALLEY_PRECISION") == "fp16"
        from tests import wq_checks
        from valley_amd import lib, runtime
        assert runtime.HALF == torch.float16
        wq_checks.run_all()
        res["storage"] = lib.load().vly_storage_dtype()
    else:
        assert not os.environ.get("VALLEY_WEIGHT_QUANT")
        from tests import golden_cfg as G
        from tests.test_model_gpu import build_golden_model
        from valley_amd import lib_wq, ops
        ops.GEMM_MODE = "tiles"
        model = build_golden_model()
        ll = model.get_model().llama
        T = G.GCFG["T"]
        ids, _ = G.golden_ids("decode")
        img = torch.from_numpy(G.golden_pixels(T, "mixed")).view(1, T, 3, 224, 224).cuda()
        seq = model.generate(torch.from_numpy(ids).cuda(), images=img, max_new_tokens=4)
        res["new_tokens"] = int(seq.shape[1] - ids.shape[1])
        res["weight_quant"] = ll.weight_quant
        res["wq_keys"] = sorted(k for L in ll.layers for k in L if k.startswith("wq_"))
        res["wq_lib_loaded"] = lib_wq.loaded()
    res["ok"] = True
    print(json.dumps(res))


main()
