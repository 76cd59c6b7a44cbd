"""A/B/C of the captured decode step with 16-bit, INT8 and INT4 projection weights: tools/wq_decode_ab.py's method with a third arm.
13B shapes, 40 distinct random layers, ONE process; the three engines share every tensor but their quantized copies; blocks of
captured steps, the arms in a fresh random order every round so that clocks, neighbours and drift hit all alike; median of the
blocks after a warm-up block.  Reports per-step ms, the spread between the blocks of each arm and the effective weight rate.

  python tools/w4_decode_ab.py [--tokens 256] [--rounds 3] [--batches 1,2,4,8] [--out profiles/r10/w4_decode_ab.jsonl]

--accuracy writes the accuracy record instead: the golden model of the test suite, once as it is, once with
int8 and once with int4 decode weights, on g5_decode's four teacher-forced one-token steps.

  python tools/w4_decode_ab.py --accuracy [--out profiles/r10/w4_accuracy_golden.txt]
"""
import argparse
import json
import os
import random
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

ARMS = ("w16", "int8", "int4")
# bytes per projection weight as each arm streams it (int4: a nibble plus one fp32 scale per 128 weights)
BYTES = {"w16": 2.0, "int8": 1.0, "int4": 0.5 + 4.0 / 128}


def accuracy(out_path):
    """The four decode steps of tests/test_model_gpu.py::test_greedy_decode_vs_golden on three golden models, two of them
    quantized: all prefill with the 16-bit weights, then each step feeds the reference's token (g5_decode.npz) to all."""
    import numpy as np
    from tests import golden_cfg as G
    from tests.test_model_gpu import GOLD, build_golden_model
    g = np.load(os.path.join(GOLD, "g5_decode.npz"))
    T = G.GCFG["T"]
    ids, _ = G.golden_ids("decode")
    img = torch.from_numpy(G.golden_pixels(T, "mixed")).view(1, T, 3, 224, 224).cuda()
    models = [build_golden_model(), build_golden_model().quantize_decode_weights("int8"),
              build_golden_model().quantize_decode_weights("int4")]
    outs = [m(input_ids=torch.from_numpy(ids).cuda(), images=img, use_cache=True) for m in models]
    lines = []
    for step in range(4):
        token = torch.from_numpy(g["tokens"][:, step]).cuda()
        ctx = ids.shape[1] + step
        mask = torch.ones(1, ctx + 1, dtype=torch.long).cuda()
        outs = [m(input_ids=token[:, None], use_cache=True, attention_mask=mask, past_key_values=o.past_key_values)
                for m, o in zip(models, outs)]
        l16, l8, l4 = (o.logits[0, -1].float().cpu().numpy().astype(np.float64) for o in outs)
        top2 = np.sort(l16)[-2:]
        lines.append(f"step {step}: max |dlogit| vs 16-bit: int8 {np.abs(l8 - l16).max():.4f}, int4 {np.abs(l4 - l16).max():.4f}; "
                     f"greedy 16-bit {int(l16.argmax())} int8 {int(l8.argmax())} int4 {int(l4.argmax())} "
                     f"(int4 agrees: {int(l4.argmax()) == int(l16.argmax())}); 16-bit top-2 gap {top2[1] - top2[0]:.4f}, "
                     f"logit range {l16.max() - l16.min():.2f}")
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
    engines = {"w16": ref}
    for mode in ("int8", "int4"):
        qe = HipLlama(H, heads, I, L, V, 1e-5, pack_weights=False, weight_quant=mode)
        qe.embed, qe.norm, qe.lm_head = ref.embed, ref.norm, ref.lm_head
        qe.layers = [dict(Ld) for Ld in ref.layers]
        qe._pack()
        qe.loaded = True
        engines[mode] = qe
    proj = L * (4 * H * H + 3 * H * I)
    head = 2.0 * H * ref.Vpad                                   # lm_head stays 16-bit in every arm
    S0, n = 328, args.tokens
    lines = []
    rng = random.Random(0)
    for B in [int(b) for b in args.batches.split(",")]:
        sess = {}
        for name in ARMS:
            ll = engines[name]
            cache = ll.new_cache(B, S0 + n + 8)
            cache.seq_len = S0                                  # (zero K / V: the attention streams the same bytes whatever they hold)
            s = DecodeSession(ll, cache, use_graph=True)
            s.begin(torch.zeros((B,), dtype=torch.int64, device=ll.device))
            sess[name] = (s, cache)
        times = {name: [] for name in ARMS}
        orders = []
        for rnd in range(args.rounds + 1):                      # round 0 warms every arm up and is dropped
            order = list(ARMS)
            rng.shuffle(order)                                  # no arm always runs behind another
            orders.append("".join(o[-1] for o in order))        # "684": w16, int8, int4 by their last character
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
        ms = {name: statistics.median(times[name]) for name in ARMS}
        spread = {name: (max(times[name]) - min(times[name])) / ms[name] for name in ARMS}
        margin = (ms["int8"] - ms["int4"]) / ms["int8"]
        rec = {"B": B, "tokens": n, "rounds": args.rounds, "dtype": str(runtime.HALF), "layers": L,
               **{f"ms_per_step_{name}": round(ms[name], 4) for name in ARMS},
               "speedup_int8_over_w16": round(ms["w16"] / ms["int8"], 3), "speedup_int4_over_w16": round(ms["w16"] / ms["int4"], 3),
               "speedup_int4_over_int8": round(ms["int8"] / ms["int4"], 3),
               "int4_margin_over_int8": round(margin, 4), "largest_block_spread": round(max(spread.values()), 4),
               "int4_shorter_than_int8_beyond_spread": bool(margin > max(spread.values())),
               **{f"blocks_{name}": [round(t, 4) for t in times[name]] for name in ARMS}, "arm_order_per_round": orders[1:],
               **{f"weight_TBps_{name}": round((BYTES[name] * proj + head) / (ms[name] * 1e-3) / 1e12, 2) for name in ARMS},
               "note": "effective rate = weight bytes of the step (projections at 2, 1 or 0.53125 bytes, lm_head at 2) / whole step "
                       "time; spread = (max - min) / median over one arm's blocks"}
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
