"""Child process of tests/test_suffix_gpu.py.  argv[1]:
  "fp16": VALLEY_PRECISION=fp16 is in the environment — one kernel case through the oracle's three checks and the turn-2
          generation through a prefix session on the split arm, all on the fp16 storage type;
  "off":  a generation without ``prefix=`` never loads libvalley_hip_suffix.so and never imports valley_amd.prefix.
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
        from tests import suffix_cases as SC
        from tests import test_suffix_gpu as T
        from valley_amd import lib, lib_suffix, runtime
        from valley_amd.prefix import PrefixSession
        assert runtime.HALF == torch.float16 and T.HALF == torch.float16
        res["launches"] = T.attention_checks(SC.BY_NAME[SC.FP16_CASE])
        model, ids, img = golden_inputs()
        s = PrefixSession(model, attention="split")
        one = model.generate(ids, images=img, prefix=s, max_new_tokens=SC.TURN1_NEW)
        ids2 = torch.tensor([SC.turn2_ids(ids[0].tolist(), one[0, ids.shape[1]:].tolist())], device=ids.device)
        n2 = len(SC.TURN2_TOKENS)
        before = s.stats["reused"]
        res["turn2_split"] = model.generate(ids2, images=img, prefix=s, max_new_tokens=n2)[0, ids2.shape[1]:].tolist()
        res["reused"] = s.stats["reused"] - before
        res["turn2_plain"] = model.generate(ids2, images=img, max_new_tokens=n2)[0, ids2.shape[1]:].tolist()
        res["storage"] = lib.load().vly_storage_dtype()
        res["suffix_lib_loaded"] = lib_suffix.loaded()
    else:
        from valley_amd import lib_suffix
        model, ids, img = golden_inputs()
        seq = model.generate(ids, images=img, max_new_tokens=4)
        res["new_tokens"] = int(seq.shape[1] - ids.shape[1])
        res["suffix_lib_loaded"] = lib_suffix.loaded()
        res["prefix_imported"] = "valley_amd.prefix" in sys.modules
    res["ok"] = True
    print(json.dumps(res))


main()
