"""What a verify step for several sequences costs: the continuous batcher's captured step of B rows against the captured
B x (k + 1)-row verify step of valley_amd.spec.SpecRowsSession, 13B shapes, random weights, ONE process.  Blocks of steps are
interleaved, the arms in a fresh random order every round (tools/spec_decode_ab.py's pattern), behind a warm-up block that is
dropped; the figure of an arm is the median of its blocks.

Arms, at every context, for the geometries (B, k) = (2, 1), (2, 3), (4, 1):
  plain{B}        DecodeSession(per_row_positions=True) of B rows and the step's one device-to-host read: the batcher's step,
                  the denominator
  rows{B(k+1)}    the same of B (k + 1) independent rows: what that many rows cost with the fused RoPE / attention
  specrows{B}x{k} SpecRowsSession(k, lookup=False) with nothing drafted: the full cost of a step that accepts nothing (draft and
                  accept kernels, the separate RoPE, the split attention of k + 1 queries per sequence, the step's read)
Derived per geometry: the excess over rows{B(k+1)}, and the break-even number of accepted tokens per slot and step,
t_specrows / t_plain{B} - 1 (a slot that accepts a tokens emits a + 1 per step).

  python tools/spec_rows_ab.py [--steps 192] [--rounds 3] [--contexts 336,1500] [--out profiles/r12/spec_rows_ab.jsonl]
"""
import argparse
import json
import os
import random
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

GEOMETRIES = ((2, 1), (2, 3), (4, 1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=192)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--contexts", type=str, default="336,1500")
    ap.add_argument("--layers", type=int, default=40)
    ap.add_argument("--out", type=str, default="")
    args = ap.parse_args()
    from valley_amd import runtime
    from valley_amd.decode import DecodeSession
    from valley_amd.llama import HipLlama
    from valley_amd.spec import SpecRowsSession
    H, heads, I, L, V = 5120, 40, 13824, args.layers, 32006
    ll = HipLlama(H, heads, I, L, V, 1e-5, pack_weights=False, weight_quant="").init_random(seed=0)
    n = args.steps
    lines = []
    rng = random.Random(0)
    for S0 in [int(c) for c in args.contexts.split(",")]:
        ctx = S0 + n + 16
        sess = {}

        def cache_of(B):
            cache = ll.new_cache(B, ctx)                     # (zero K / V: the attention streams the same bytes whatever they hold)
            cache.key_valid = torch.ones((B, ctx), dtype=torch.uint8, device=ll.device)
            return cache

        def plain(B):
            s = DecodeSession(ll, cache_of(B), use_graph=True, per_row_positions=True)
            s.pos.fill_(S0)
            s.begin()
            return s, lambda: s.tok.tolist()                 # the batcher's one read per step

        def specrows(B, k):
            s = SpecRowsSession(ll, cache_of(B), k, use_graph=True, lookup=False)
            s.hist.zero_()                                   # token 0 everywhere: the step feeds hist[pos]
            s.live.fill_(1)
            s.pos.fill_(S0)
            s.begin()
            s.draft_len.zero_()                              # nothing drafted: nothing accepted, one token per slot and step
            return s, None

        for B, k in GEOMETRIES:
            for name, make in ((f"plain{B}", lambda: plain(B)), (f"rows{B * (k + 1)}", lambda: plain(B * (k + 1))),
                               (f"specrows{B}x{k}", lambda: specrows(B, k))):
                if name not in sess:
                    sess[name] = make()
        times = {name: [] for name in sess}
        for rnd in range(args.rounds + 1):                   # round 0 warms every arm up and is dropped
            order = list(sess)
            rng.shuffle(order)                               # no arm always runs behind the same other
            for name in order:
                s, read = sess[name]
                s.pos.fill_(S0)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(n):
                    out = s.step()
                    if read is not None:
                        read()
                e1.record()
                torch.cuda.synchronize()
                assert s.pos.tolist() == [S0 + n] * s.pos.numel(), (name, s.pos.tolist())
                if read is None:
                    assert all(len(t) == 1 for t in out.values()) and len(out) == s.B, (name, out)
                if rnd:
                    times[name].append(e0.elapsed_time(e1) / n)
        ms = {name: statistics.median(t) for name, t in times.items()}
        for name in sess:
            rec = {"context": S0, "arm": name, "steps": n, "rounds": args.rounds, "dtype": str(runtime.HALF), "layers": L,
                   "ms_per_step": round(ms[name], 4), "blocks": [round(t, 4) for t in times[name]]}
            print(json.dumps(rec), flush=True)
            lines.append(json.dumps(rec))
        for B, k in GEOMETRIES:
            arm, rows, base = f"specrows{B}x{k}", f"rows{B * (k + 1)}", f"plain{B}"
            rec = {"context": S0, "summary": arm, "slots": B, "k": k, "ms_per_step": round(ms[arm], 4), f"ms_{base}": round(ms[base], 4),
                   f"ms_{rows}": round(ms[rows], 4), "excess_over_rows_ms": round(ms[arm] - ms[rows], 4),
                   "break_even_accepted_per_slot_step": round(ms[arm] / ms[base] - 1.0, 3)}
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
