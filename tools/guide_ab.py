"""What a guided token costs per decode step: 13B shapes, 40 random layers, the captured step, ONE process, one session per arm
over shared weights, blocks of steps interleaved with the arms in a fresh random order every round (tools/constrain_ab.py's
pattern), a warm-up block and then --rounds blocks; medians, the blocks' spread, and the excess over the plain one-row step.

Arms: the plain one-row step (what an unguided token costs); the plain two-row per-row step (the second row alone: it exists
today); the guided pair (that two-row step plus vly_guide_apply and vly_guide_follow).

Every arm puts the position and the fed token back after each step (two tiny fills), so that the KV length is the same at every
step of every block.  vly_guide_apply alone is also timed: 100 launches captured in one graph on the step's own logits buffer
("kernel_us"; the launches rewrite the row in place, which costs what the first does).

  python tools/guide_ab.py [--steps 128] [--rounds 3] [--out profiles/r15/guide_ab.jsonl]
"""
import argparse
import json
import os
import random
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

ARMS = ["plain_1row", "plain_2rows", "guided_pair"]
C = 1000                                                        # the id every fed token holds


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=128)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--layers", type=int, default=40)
    ap.add_argument("--scale", type=float, default=1.5)
    ap.add_argument("--out", type=str, default="")
    args = ap.parse_args()
    from valley_amd import ops, runtime
    from valley_amd.decode import DecodeSession
    from valley_amd.llama import HipLlama
    H, heads, I, L, V = 5120, 40, 13824, args.layers, 32006
    ll = HipLlama(H, heads, I, L, V, 1e-5, pack_weights=False).init_random(seed=0)
    d = ll.device
    P, n = 328, args.steps                                      # every step runs at position P
    rng = random.Random(0)
    sess = {}
    for name in ARMS:
        B = 1 if name == "plain_1row" else 2
        cache = ll.new_cache(B, P + 8)
        cache.seq_len = P                                       # (zero K / V: the attention streams the same bytes whatever they hold)
        cache.key_valid = torch.ones((B, cache.ctx_max), dtype=torch.uint8, device=d)
        if name == "plain_1row":                                # generate()'s session of an unguided call: one shared position
            s = DecodeSession(ll, cache, use_graph=True)
            s.begin(torch.full((B,), C, dtype=torch.int64, device=d))
        else:                                                   # one position per row, as a pair needs them
            s = DecodeSession(ll, cache, use_graph=True, per_row_positions=True, guidance=name == "guided_pair")
            if s.guide is not None:
                s.guide.copy_(ops.guidance_rows(B, [(0, 1, args.scale, 0.1)]))
            s.pos.fill_(P)
            s.tok.fill_(C)
            s.begin()
        sess[name] = (s, cache)
    # the launch alone: 100 of them in one graph, on the guided step's own logits buffer
    s = sess["guided_pair"][0]
    x = s.logits[:, :V]
    x.copy_(torch.randn((2, V), device=d) * 3)
    ops.guide(x, s.guide)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(100):
            ops.guide(x, s.guide)
    ts = []
    for _ in range(5):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        g.replay()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1) * 10.0)                   # ms per 100 launches -> us per launch
    kernel_us = round(statistics.median(ts[1:]), 2)
    times = {a: [] for a in ARMS}
    for rnd in range(args.rounds + 1):                          # round 0 warms every arm up and is dropped
        order = list(ARMS)
        rng.shuffle(order)                                      # no arm always runs behind the same other
        for name in order:
            s, cache = sess[name]
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(n):
                cache.seq_len = P
                s.step()
                s.pos.fill_(P)
                s.tok.fill_(C)
            e1.record()
            torch.cuda.synchronize()
            if rnd:
                times[name].append(e0.elapsed_time(e1) / n)
    for s, _ in sess.values():
        s.check()
    med = {a: statistics.median(times[a]) for a in ARMS}
    rec = {"steps_per_block": n, "rounds": args.rounds, "dtype": str(runtime.HALF), "layers": L, "position": P, "scale": args.scale,
           "ms_per_step": {a: round(med[a], 4) for a in ARMS},
           "blocks_ms": {a: [round(t, 4) for t in times[a]] for a in ARMS},
           "spread_us": {a: round((max(times[a]) - min(times[a])) * 1e3, 1) for a in ARMS},
           "excess_us_over_plain_1row": {a: round((med[a] - med["plain_1row"]) * 1e3, 1) for a in ARMS},
           "excess_percent_of_plain_1row": {a: round((med[a] - med["plain_1row"]) / med["plain_1row"] * 100, 3) for a in ARMS},
           "new_launches_us": round((med["guided_pair"] - med["plain_2rows"]) * 1e3, 1),
           "guide_apply_kernel_us": kernel_us,
           "note": "every arm resets position and fed token after each step; guide_apply_kernel_us: "
                   "vly_guide_apply alone, 100 launches in one graph"}
    print(json.dumps(rec), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
