"""A/B of the captured decode step with 16-bit and with INT8 projection weights: 13B shapes, random weights, ONE process, the two
engines share every tensor but the int8 copies, blocks of steps interleaved, the two arms in a fresh random order every round
(tools/ab_lib.py's pattern) so that clocks, neighbours and drift hit both alike.  Reports per-step ms (median of the blocks) and
the effective weight rate.

  python tools/wq_decode_ab.py [--tokens 256] [--rounds 3] [--batches 1,2,4,8] [--out profiles/r08/wq_decode_ab.jsonl]

--accuracy writes the accuracy record instead: the golden model of the test suite, once as it is and once
with int8 decode weights, on g5_decode's four teacher-forced one-token steps.

  python tools/wq_decode_ab.py --accuracy [--out profiles/r08/wq_accuracy_golden.txt]
"""
import argparse
import json
import os
import random
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def accuracy(out_path):
    """The four decode steps of tests/test_model_gpu.py::test_greedy_decode_vs_golden on two golden models, one of them quantized:
    both prefill with the 16-bit weights, then each step feeds the reference's token (g5_decode.npz) to both."""
    import numpy as np
    from tests import golden_cfg as G
    from tests.test_model_gpu import GOLD, build_golden_model
    g = np.load(os.path.join(GOLD, "g5_decode.npz"))
    T = G.GCFG["T"]
    ids, _ = G.golden_ids("decode")
    img = torch.from_numpy(G.golden_pixels(T, "mixed")).view(1, T, 3, 224, 224).cuda()
    models = [build_golden_model(), build_golden_model().quantize_decode_weights("int8")]
    outs = [m(input_ids=torch.from_numpy(ids).cuda(), images=img, use_cache=True) for m in models]
    n_gold = g["last_logits"].shape[1]                         # the fixture holds the logits IN FRONT of each of its steps
    lines = []
    for step in range(4):
        token = torch.from_numpy(g["tokens"][:, step]).cuda()
        ctx = ids.shape[1] + step
        mask = torch.ones(1, ctx + 1, dtype=torch.long).cuda()
        outs = [m(input_ids=token[:, None], use_cache=True, attention_mask=mask, past_key_values=o.past_key_values)
                for m, o in zip(models, outs)]
        l16, l8 = (o.logits[0, -1].float().cpu().numpy().astype(np.float64) for o in outs)
        gold = f"{np.abs(l8 - g['last_logits'][0, step + 1]).max():.4f}" if step + 1 < n_gold \
            else f"n/a (the fixture ends with the logits in front of step {n_gold - 1})"
        lines.append(f"step {step}: max |dlogit| int8 vs 16-bit {np.abs(l8 - l16).max():.4f}; greedy 16-bit {int(l16.argmax())} "
                     f"int8 {int(l8.argmax())}; fp32 reference vs int8 {gold}")
        print(lines[-1], flush=True)
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as f:
            f.write("\n".join(lines) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tokens", type=int, default=256)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--batches", type=str, default="1,2,4,8")
    ap.add_argument("--layers", type=int, default=40)
    ap.add_argument("--out", type=str, default="")
    ap.add_argument("--accuracy", action="store_true")
    args = ap.parse_args()
    if args.accuracy:
        return accuracy(args.out)
    from valley_amd import runtime
    from valley_amd.decode import DecodeSession
    from valley_amd.llama import HipLlama
    H, heads, I, L, V = 5120, 40, 13824, args.layers, 32006
    ref = HipLlama(H, heads, I, L, V, 1e-5, pack_weights=False, weight_quant="").init_random(seed=0)
    qe = HipLlama(H, heads, I, L, V, 1e-5, pack_weights=False, weight_quant="int8")
    qe.embed, qe.norm, qe.lm_head = ref.embed, ref.norm, ref.lm_head
    qe.layers = [dict(Ld) for Ld in ref.layers]
    qe._pack()
    qe.loaded = True
    proj = L * (4 * H * H + 3 * H * I)
    head = 2.0 * H * ref.Vpad                                   # lm_head stays 16-bit in both
    S0, n = 328, args.tokens
    lines = []
    rng = random.Random(0)
    for B in [int(b) for b in args.batches.split(",")]:
        sess = {}
        for name, ll in (("w16", ref), ("int8", qe)):
            cache = ll.new_cache(B, S0 + n + 8)
            cache.seq_len = S0                                  # (zero K / V: the attention streams the same bytes whatever they hold)
            s = DecodeSession(ll, cache, use_graph=True)
            s.begin(torch.zeros((B,), dtype=torch.int64, device=ll.device))
            sess[name] = (s, cache)
        times = {"w16": [], "int8": []}
        orders = []
        for rnd in range(args.rounds + 1):                      # round 0 warms both up and is dropped
            order = ["w16", "int8"]
            rng.shuffle(order)                                  # neither arm always runs behind the other
            orders.append(order[0])
            for name in order:
                s, cache = sess[name]
                cache.seq_len = S0
                s.pos.fill_(S0)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(n):
                    s.step()
                e1.record()
                torch.cuda.synchronize()
                if rnd:
                    times[name].append(e0.elapsed_time(e1) / n)
        ms16, ms8 = statistics.median(times["w16"]), statistics.median(times["int8"])
        rec = {"B": B, "tokens": n, "rounds": args.rounds, "dtype": str(runtime.HALF), "layers": L,
               "ms_per_step_w16": round(ms16, 4), "ms_per_step_int8": round(ms8, 4), "speedup": round(ms16 / ms8, 3),
               "blocks_w16": [round(t, 4) for t in times["w16"]], "blocks_int8": [round(t, 4) for t in times["int8"]], "first_arm_per_round": orders[1:],
               "weight_TBps_w16": round((2.0 * proj + head) / (ms16 * 1e-3) / 1e12, 2),
               "weight_TBps_int8": round((1.0 * proj + head) / (ms8 * 1e-3) / 1e12, 2),
               "note": "effective rate = weight bytes of the step (projections at 2 or 1 byte, lm_head at 2) / whole step time"}
        print(json.dumps(rec), flush=True)
        lines.append(json.dumps(rec))
        del sess
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
