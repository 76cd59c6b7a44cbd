"""What the token constraints cost per decode step: 13B shapes, 40 random layers, the captured step, ONE process, one session
per arm over shared weights, blocks of steps interleaved with the arms in a fresh random order every round (tools/wq_decode_ab.py's
pattern), a warm-up block and then --rounds blocks; medians, the blocks' spread, and the excess over the plain arm.

Arms: the plain step; the step with neutral processors (the launch a constraint session always runs); one suppressed id; 1000
bad words of length 3; a trie of fan-out 4 walked to depth 2; a one-sequence trie walked to depth 64 (the longest walk there is).

Every arm, the plain one included, puts the position and the fed token back after each step (two tiny fills), so that the KV
length, the history length and the walk's depth are the same at every step of every block.  The kernel alone is also timed:
100 launches captured in one graph, per arm's tables and rows ("kernel_us").

  python tools/constrain_ab.py [--steps 128] [--rounds 3] [--batches 1,8] [--out profiles/r14/constrain_ab.jsonl]
"""
import argparse
import json
import os
import random
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

ARMS = ["plain", "neutral_processors", "suppress_1", "bad_words_1000x3", "trie_fan4_depth2", "trie_depth64"]
EOS, C = 2, 1000                                                # the id every history position and every fed token holds


def arm_tables(name, V, device):
    """(tables, generated ids the walk stands behind) of a constraint arm"""
    from valley_amd import ops
    rng = random.Random(1)
    if name == "suppress_1":
        return ops.constraint_tables(suppress_tokens=[7], eos=[EOS], V=V, device=device), 0
    if name == "bad_words_1000x3":
        words = [[rng.randrange(V), rng.randrange(V), rng.randrange(V)] for _ in range(1000)]
        return ops.constraint_tables(bad_words_ids=words, eos=[EOS], V=V, device=device), 0
    seqs = [[C + a, C + b] for a in range(4) for b in range(4)] if name == "trie_fan4_depth2" else [[C] * 64]
    t = ops.constraint_tables(eos=[EOS], V=V, capacity={"trie": len(ops.pack_trie(seqs, V))}, device=device)
    ops.constraint_trie(t, 0, seqs)
    return t, len(seqs[0])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=128)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--batches", type=str, default="1,8")
    ap.add_argument("--layers", type=int, default=40)
    ap.add_argument("--out", type=str, default="")
    args = ap.parse_args()
    from valley_amd import ops, runtime
    from valley_amd.decode import DecodeSession
    from valley_amd.llama import HipLlama
    H, heads, I, L, V = 5120, 40, 13824, args.layers, 32006
    ll = HipLlama(H, heads, I, L, V, 1e-5, pack_weights=False).init_random(seed=0)
    d = ll.device
    P, n = 328, args.steps                                      # every step runs at position P
    lines = []
    rng = random.Random(0)
    for B in [int(b) for b in args.batches.split(",")]:
        sess, kernel_us = {}, {}
        for name in ARMS:
            cache = ll.new_cache(B, P + 8)
            cache.seq_len = P                                   # (zero K / V: the attention streams the same bytes whatever they hold)
            kw = {}
            if name == "neutral_processors":
                kw = dict(processors=True)
            elif name != "plain":
                tables, depth = arm_tables(name, V, d)
                kw = dict(constraints=tables)
            s = DecodeSession(ll, cache, use_graph=True, **kw)
            if s.hist is not None:
                s.hist.fill_(C)
            if s.con is not None:
                rows = ops.constraint_rows(tables, B, begin=P + 1 - depth, max_length=0, trie_root=0 if depth else -1, device=d)
                s.con.copy_(rows)
                # the launch alone: 100 of them in one graph, on the step's own buffers
                x = torch.randn((B, V), device=d)
                length = torch.full((1,), P, dtype=torch.int32, device=d)
                ops.constrain(x, rows, tables, s.hist, length, 1)
                torch.cuda.synchronize()
                g = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g):
                    for _ in range(100):
                        ops.constrain(x, rows, tables, s.hist, length, 1)
                ts = []
                for _ in range(5):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    g.replay()
                    e1.record()
                    torch.cuda.synchronize()
                    ts.append(e0.elapsed_time(e1) * 10.0)       # ms per 100 launches -> us per launch
                kernel_us[name] = round(statistics.median(ts[1:]), 2)
            s.begin(torch.full((B,), C, dtype=torch.int64, device=d))
            sess[name] = (s, cache)
        times = {a: [] for a in ARMS}
        for rnd in range(args.rounds + 1):                      # round 0 warms every arm up and is dropped
            order = list(ARMS)
            rng.shuffle(order)                                  # no arm always runs behind the same other
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
        rec = {"B": B, "steps_per_block": n, "rounds": args.rounds, "dtype": str(runtime.HALF), "layers": L, "position": P,
               "ms_per_step": {a: round(med[a], 4) for a in ARMS},
               "blocks_ms": {a: [round(t, 4) for t in times[a]] for a in ARMS},
               "spread_us": {a: round((max(times[a]) - min(times[a])) * 1e3, 1) for a in ARMS},
               "excess_us_over_plain": {a: round((med[a] - med["plain"]) * 1e3, 1) for a in ARMS},
               "excess_percent_of_step": {a: round((med[a] - med["plain"]) / med["plain"] * 100, 3) for a in ARMS},
               "kernel_us": kernel_us,
               "note": "every arm resets position and fed token after each step; kernel_us: vly_constrain_apply alone, 100 launches in one graph"}
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
