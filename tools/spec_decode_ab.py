"""What a prompt-lookup verify step costs: the captured decode step of one sequence against the captured k + 1-row verify step of
valley_amd.spec.SpecDecodeSession, 13B shapes, random weights, ONE process, every arm on the same engine.  Blocks of steps are
interleaved, the arms in a fresh random order every round (tools/wq_decode_ab.py's pattern), with a warm-up block that is dropped;
the figure of an arm is the median of its blocks.

Arms, at every context:
  plain          DecodeSession, 1 row
  rows{k+1}      DecodeSession, k + 1 independent rows (what k + 1 rows cost with the fused norms and the fused RoPE / attention)
  spec{k}        SpecDecodeSession(k, lookup=False) with draft_len = 0: the full cost of a step that accepts nothing (draft and accept
                 kernels, the separate rope_kv, the split attention of k + 1 queries, the step's device-to-host read)
  spec{k}_pf     the same with VALLEY_SPEC_ATTN=prefill (vly_llama_attention(S = k + 1): one workgroup per head)
for k = 1, 3, 7.  Derived per k: the spec step's excess over rows{k+1}, and the break-even number of accepted tokens per step,
t_spec(k) / t_plain - 1 (a step that accepts a tokens emits a + 1).

--sampled adds the arms of speculation under seeded sampling (and drops rows{k+1} and spec{k}_pf, which they are not compared with):
  plain_{set}    DecodeSession(sampling=True), 1 row, the set's parameters
  spec{k}_{set}  SpecDecodeSession(k, lookup=False, sampling=True) with draft_len = 0: the counter launch and k + 1 sampled rows in
                 place of the argmax of k + 1 rows
for the sets T0.2 (T = 0.2), k50 (T = 1, top_k = 50) and p0.9 (T = 0.8, top_p = 0.9).  Derived: the excess over spec{k} (the existing
arm is the reference) and the break-even against the sampled one-row step, t_spec_set(k) / t_plain_set - 1.

  python tools/spec_decode_ab.py [--tokens 256] [--rounds 3] [--contexts 336,1500] [--out profiles/r09/spec_decode_ab.jsonl]
  python tools/spec_decode_ab.py --sampled --out profiles/r11/spec_sampled_ab.jsonl
"""
import argparse
import json
import os
import random
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

KS = (1, 3, 7)
SETS = {"T0.2": (0.2, 0, 1.0), "k50": (1.0, 50, 1.0), "p0.9": (0.8, 0, 0.9)}     # (temperature, top_k, top_p)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tokens", type=int, default=256)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--contexts", type=str, default="336,1500")
    ap.add_argument("--layers", type=int, default=40)
    ap.add_argument("--out", type=str, default="")
    ap.add_argument("--sampled", action="store_true", help="the arms of speculation under seeded sampling")
    args = ap.parse_args()
    from valley_amd import ops, runtime
    from valley_amd.decode import DecodeSession
    from valley_amd.llama import HipLlama
    from valley_amd.spec import SpecDecodeSession
    H, heads, I, L, V = 5120, 40, 13824, args.layers, 32006
    ll = HipLlama(H, heads, I, L, V, 1e-5, pack_weights=False, weight_quant="").init_random(seed=0)
    n = args.tokens
    lines = []
    rng = random.Random(0)
    for S0 in [int(c) for c in args.contexts.split(",")]:
        ctx = S0 + n + 16
        sess = {}

        def plain(B, params=None):
            cache = ll.new_cache(B, ctx)
            cache.seq_len = S0                               # (zero K / V: the attention streams the same bytes whatever they hold)
            s = DecodeSession(ll, cache, use_graph=True, sampling=params is not None)
            if params is not None:
                s.sample.copy_(ops.sampling_rows(*params, seed=[1] * B, device=ll.device))
            s.begin(torch.zeros((B,), dtype=torch.int64, device=ll.device))
            return s, cache

        def spec(k, attn, params=None):
            os.environ["VALLEY_SPEC_ATTN"] = attn            # read when the session is made
            cache = ll.new_cache(1, ctx)
            cache.seq_len = S0
            s = SpecDecodeSession(ll, cache, k, use_graph=True, lookup=False, sampling=params is not None)
            if params is not None:
                s.sample.copy_(ops.sampling_rows(*params, seed=[1] * (k + 1), device=ll.device))
            s.begin(torch.zeros((1,), dtype=torch.int64, device=ll.device))
            s.draft_len.zero_()                              # nothing drafted: nothing accepted, one token per step
            return s, cache

        sess["plain"] = plain(1)
        for name, params in SETS.items() if args.sampled else ():
            sess[f"plain_{name}"] = plain(1, params)
        for k in KS:
            sess[f"spec{k}"] = spec(k, "split")
            if args.sampled:
                for name, params in SETS.items():
                    sess[f"spec{k}_{name}"] = spec(k, "split", params)
            else:
                sess[f"rows{k + 1}"] = plain(k + 1)
                sess[f"spec{k}_pf"] = spec(k, "prefill")
        os.environ.pop("VALLEY_SPEC_ATTN", None)
        times = {name: [] for name in sess}
        for rnd in range(args.rounds + 1):                   # round 0 warms every arm up and is dropped
            order = list(sess)
            rng.shuffle(order)                               # no arm always runs behind the same other
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
                assert cache.seq_len == S0 + n, (name, cache.seq_len)
                if rnd:
                    times[name].append(e0.elapsed_time(e1) / n)
        ms = {name: statistics.median(t) for name, t in times.items()}
        for name in sess:
            rec = {"context": S0, "arm": name, "tokens": n, "rounds": args.rounds, "dtype": str(runtime.HALF), "layers": L,
                   "ms_per_step": round(ms[name], 4), "blocks": [round(t, 4) for t in times[name]]}
            print(json.dumps(rec), flush=True)
            lines.append(json.dumps(rec))
        for k in KS if args.sampled else ():
            for name in SETS:
                arm = f"spec{k}_{name}"
                rec = {"context": S0, "summary": arm, "k": k, "ms_per_step": round(ms[arm], 4), "ms_spec": round(ms[f"spec{k}"], 4),
                       "ms_plain": round(ms["plain"], 4), "ms_plain_sampled": round(ms[f"plain_{name}"], 4),
                       "excess_over_spec_ms": round(ms[arm] - ms[f"spec{k}"], 4),
                       "break_even_accepted_per_step": round(ms[arm] / ms[f"plain_{name}"] - 1.0, 3),
                       "break_even_greedy": round(ms[f"spec{k}"] / ms["plain"] - 1.0, 3)}
                print(json.dumps(rec), flush=True)
                lines.append(json.dumps(rec))
        for k in () if args.sampled else KS:
            for arm in (f"spec{k}", f"spec{k}_pf"):
                rec = {"context": S0, "summary": arm, "k": k, "ms_per_step": round(ms[arm], 4), "ms_plain": round(ms["plain"], 4),
                       f"ms_rows{k + 1}": round(ms[f"rows{k + 1}"], 4), "excess_over_rows_ms": round(ms[arm] - ms[f"rows{k + 1}"], 4),
                       "break_even_accepted_per_step": round(ms[arm] / ms["plain"] - 1.0, 3)}
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
