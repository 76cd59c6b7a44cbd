"""What the end-of-generation test costs per token: 13B shapes, 40 random layers, the captured step, ONE process, one session per
arm over shared weights, generate()'s own loops (generation.token_loop / generation.block_loop) over blocks of --tokens tokens,
the arms interleaved in a fresh random order every round (tools/constrain_ab.py's pattern), a warm-up block and then --rounds
blocks; wall-clock medians per token (the host's share is what is measured), one row and four rows.

Arms: the reference's KeywordsStoppingCriteria(['###']) as a host callback over a toy tokenizer, the loop of the parent commit
(the baseline); stop_strings on the device at sync_every 1, 8 and 32; the bare captured step replayed with one synchronise at
the end (the floor).  The stop string never occurs (its one piece is an id a random model does not pick three times running),
so every block decodes all its tokens.  vly_stop_apply alone is also timed: 100 launches captured in one graph.

  python tools/stop_ab.py [--tokens 128] [--rounds 3] [--out profiles/r16/stop_ab.jsonl]
"""
import argparse
import json
import os
import random
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

ARMS = ["host_keywords", "stop_sync1", "stop_sync8", "stop_sync32", "bare_step"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tokens", type=int, default=128)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--layers", type=int, default=40)
    ap.add_argument("--out", type=str, default="")
    args = ap.parse_args()
    from tests.stop_tokenizer import ToyTokenizer
    from valley_amd import generation, ops, runtime
    from valley_amd.decode import DecodeSession
    from valley_amd.llama import HipLlama
    from valley_amd.video import KeywordsStoppingCriteria
    H, heads, I, L, V = 5120, 40, 13824, args.layers, 32006
    ll = HipLlama(H, heads, I, L, V, 1e-5, pack_weights=False).init_random(seed=0)
    d = ll.device
    P, n = 328, args.tokens                                     # every block starts behind a prompt of P tokens

    def piece(i):                                               # ids as words over a-g; the last id is the only '#'
        out = ""
        while True:
            i, r = divmod(i, 7)
            out = "abcdefg"[r] + out
            if i == 0:
                return out + " "
            i -= 1
    tk = ToyTokenizer(list("abcdefg") + [piece(i) for i in range(7, V - 1)] + ["#"])
    tables = ops.stop_tables(tk, ["###"], device=d)
    rng = random.Random(0)
    recs = []
    for B in (1, 4):
        prompt = torch.randint(7, V - 1, (B, P), device=d, generator=torch.Generator(device=d).manual_seed(B))
        first = torch.randint(7, V - 1, (B,), device=d, generator=torch.Generator(device=d).manual_seed(10 + B))
        sess = {}
        for name in ARMS:
            cache = ll.new_cache(B, P + n + 8)
            cache.seq_len = P                                   # (zero K / V: the attention streams the same bytes whatever they hold)
            s = DecodeSession(ll, cache, use_graph=True, **({"stop": tables} if name.startswith("stop") else {}))
            sess[name] = (s, cache)

        def block(name):
            s, cache = sess[name]
            cache.seq_len = P
            if s.stop_state is not None:
                s.stop_rows.copy_(ops.stop_rows(B, begin=P, pad=0, pad_after=True))
                s.stop_state.copy_(ops.stop_state(B))
            s.begin(first, prompt_ids=prompt if s.hist is not None else None)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            if name == "bare_step":
                for _ in range(n - 1):
                    s.step()
                made = n
            elif name in ("stop_sync8", "stop_sync32"):
                made = generation.block_loop(s, P, n, int(name[9:]), cache).shape[1]
            else:
                finished = torch.zeros((B,), dtype=torch.bool, device=d)

                def step(token):                                # _generate's session_step
                    token = s.step().to(torch.long).clone()
                    if bool(finished.any()):
                        token = torch.where(finished, torch.zeros_like(token), token)
                        s.tok.copy_(token.to(torch.int32))
                    return token
                crit = [KeywordsStoppingCriteria(["###"], tk, prompt)] if name == "host_keywords" else \
                    [lambda seqs, scores: s.stop_state[:, 0] != 0]
                seq = torch.cat([prompt, first[:, None]], dim=1)
                made = generation.token_loop(step, first, seq, finished, None, crit, n, cache, d).shape[1] - P
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e3 / made, made

        times, made = {a: [] for a in ARMS}, {}
        for rnd in range(args.rounds + 1):                      # round 0 warms every arm up and is dropped
            order = list(ARMS)
            rng.shuffle(order)                                  # no arm always runs behind the same other
            for name in order:
                ms, made[name] = block(name)
                if rnd:
                    times[name].append(ms)
        for s, _ in sess.values():
            s.check()
        med = {a: statistics.median(times[a]) for a in ARMS}
        recs.append({"rows": B, "tokens_per_block": made, "rounds": args.rounds, "dtype": str(runtime.HALF), "layers": L, "prompt": P,
                     "ms_per_token": {a: round(med[a], 4) for a in ARMS},
                     "blocks_ms": {a: [round(t, 4) for t in times[a]] for a in ARMS},
                     "spread_us": {a: round((max(times[a]) - min(times[a])) * 1e3, 1) for a in ARMS},
                     "saved_us_vs_host_keywords": {a: round((med["host_keywords"] - med[a]) * 1e3, 1) for a in ARMS},
                     "saved_percent_of_host_keywords": {a: round((med["host_keywords"] - med[a]) / med["host_keywords"] * 100, 3) for a in ARMS},
                     "note": "wall clock per token of generate()'s loops; host_keywords is the parent commit's loop (the baseline)"})
    # the launch alone: 100 of them in one graph, on a stop session's own buffers
    s = sess["stop_sync1"][0]
    ops.stop(s.tok, s.stop_rows, s.stop_state, tables, s.hist, s.pos, 0)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(100):
            ops.stop(s.tok, s.stop_rows, s.stop_state, tables, s.hist, s.pos, 0)
    ts = []
    for _ in range(5):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        g.replay()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1) * 10.0)                   # ms per 100 launches -> us per launch
    for r in recs:
        r["stop_apply_kernel_us"] = round(statistics.median(ts[1:]), 2)
        print(json.dumps(r), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            for r in recs:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
