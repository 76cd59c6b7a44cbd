"""Decode throughput with on-device sampling against greedy decoding and the torch host-sampling path.

    python tools/decode_sampling_time.py [--steps 256] [--batches 1,8] [--layers 40]
    python tools/decode_sampling_time.py --kernel [--iters 200]     # only the token-selection launches (run under
                                                                    # rocprofv3 --kernel-trace --stats for their times)

The decode mode builds a 13B-shaped HipLlama (hidden 5120, 40 heads, 13824, 40 layers, V 32000; random weights), prefills a
prefix of --prefix positions, and times --steps hipGraph decode steps (DecodeSession) per case:
  greedy   the default captured step (argmax)
  graph    DecodeSession(sampling=True): T 0.2, top-k 50, top-p 0.9 drawn inside the captured step
  host     the greedy graph + softmax / torch.multinomial on the step's logits, the token copied back (generate()'s path
           without top_k / top_p / seed)
and prints one JSON line per (case, batch)."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402


def kernel_mode(iters):
    from valley_amd import ops
    d = torch.device("cuda:0")
    V, Vpad = 32000, 32000
    for B in (1, 8):
        x = (torch.randn((B, Vpad), device=d) * 3)[:, :V]
        sp = ops.sampling_rows([0.2] * B, 50, 0.9, list(range(B)), device=d)
        ctr = torch.zeros((B,), dtype=torch.int32, device=d)
        out = torch.empty((B,), dtype=torch.int32, device=d)
        for _ in range(iters):
            ops.argmax(x, out=out)                                       # greedy (NULL parameters)
            ops.argmax(x, sampling=sp, ctr=ctr, ctr_add=1, out=out)      # sampled
        torch.cuda.synchronize()
    print(json.dumps({"kernel_mode": "done", "iters": iters}))


def decode_mode(args):
    from valley_amd import ops
    from valley_amd.decode import DecodeSession
    from valley_amd.llama import HipLlama
    d = torch.device("cuda:0")
    ll = HipLlama(5120, 40, 13824, args.layers, 32000, 1e-5).init_random(seed=1)
    for B in [int(b) for b in args.batches.split(",")]:
        S = args.prefix
        for case in ("greedy", "graph", "host"):
            cache = ll.new_cache(B, S + args.steps + args.warmup + 4)
            h = torch.randn((B * S, ll.H), generator=torch.Generator(device="cuda").manual_seed(3), device=d) * 0.02
            x = ll.forward(h, B, S, cache)
            first = ll.logits(x.view(B, S, -1)[:, -1].contiguous())[:, :ll.V].argmax(-1)
            sess = DecodeSession(ll, cache, use_graph=True, sampling=case == "graph")
            if case == "graph":
                sess.sample.copy_(ops.sampling_rows([0.2] * B, 50, 0.9, list(range(B)), device=d))
            sess.begin(first)

            def step():
                t = sess.step()
                if case == "host":
                    p = torch.softmax(sess.logits[:, :ll.V] / 0.2, dim=-1)
                    sess.tok.copy_(torch.multinomial(p, num_samples=1).view(B).to(torch.int32))
                return t

            for _ in range(args.warmup):
                step()
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0 = time.perf_counter()
            e0.record()
            for _ in range(args.steps):
                step()
            e1.record()
            torch.cuda.synchronize()
            wall = time.perf_counter() - t0
            sess.check()
            ms = e0.elapsed_time(e1) / args.steps
            print(json.dumps({"case": case, "batch": B, "layers": args.layers, "prefix": S, "steps": args.steps,
                              "ms_per_step": round(ms, 4), "tokens_per_s": round(B * 1e3 / ms, 2),
                              "wall_ms_per_step": round(wall / args.steps * 1e3, 4)}), flush=True)
            del sess, cache


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kernel", action="store_true")
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--steps", type=int, default=256)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--prefix", type=int, default=600)
    ap.add_argument("--layers", type=int, default=40)
    ap.add_argument("--batches", default="1,8")
    args = ap.parse_args()
    if args.kernel:
        kernel_mode(args.iters)
    else:
        decode_mode(args)


if __name__ == "__main__":
    main()
