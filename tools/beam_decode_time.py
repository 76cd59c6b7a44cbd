"""Per-step time of beam-search decoding (DecodeSession(beams=...)) against greedy decoding at the same row count.

    python tools/beam_decode_time.py [--steps 256] [--beams 1,4,8] [--prefix 336] [--layers 40]
    python tools/beam_decode_time.py --kernel [--iters 200]      # only the three beam launches (run under
                                                                 # rocprofv3 --kernel-trace --stats for their times)

The decode mode builds a 13B-shaped HipLlama (hidden 5120, 40 heads, 13824, 40 layers, V 32000; random weights), prefills
one prompt of --prefix positions, expands it into nb beam rows (vly_kv_beam_reorder with lo = 0) and times --steps
captured beam steps with no EOS: candidates + select + the KV reorder of the generated positions + pos += 1 inside the
graph.  Each nb is also timed as the greedy session of nb rows (the same forward, argmax instead of the beam kernels): the
difference is the beam overhead.  One JSON line per (nb, mode); the per-step time is averaged over the steps, so the
reorder's share (which grows with the generated length) is its mean over 0 .. steps generated tokens."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402


def kernel_mode(iters):
    """The three beam kernels at the 13B shapes: B = 1, nb = 4, V 32000, 256 generated positions behind a 336-token prompt."""
    from valley_amd import ops
    d = torch.device("cuda:0")
    B, nb, V, L, heads, S, gen = 1, 4, 32000, 40, 40, 336, 256
    R, K = B * nb, ops.beam_k(nb, 0)
    x = (torch.randn((R, V), device=d) * 3).contiguous()
    running = torch.randn((R,), device=d) - 5
    scratch = ops.beam_scratch(B, nb, K, d)
    ks = [torch.zeros((R, heads, S + gen + 1, 128), dtype=torch.bfloat16, device=d) for _ in range(L)]
    vs = [torch.zeros_like(k) for k in ks]
    table = ops.kv_beam_table(ks, vs, d)
    parent = torch.tensor([0, 0, 1, 3], dtype=torch.int32, device=d)       # two rows change: 1 <- 0 and 2 <- 1
    pos = torch.tensor([S + gen - 1], dtype=torch.int32, device=d)
    for _ in range(iters):
        c = ops.beam_candidates(x, running, B, nb, K, None, scratch)
        ops.beam_select(*c, B, nb)
        ops.kv_beam_reorder(table, ks[0], parent, S, 1, pos_dev=pos)
    torch.cuda.synchronize()
    print(json.dumps({"kernel_mode": "done", "iters": iters, "reorder_positions": gen, "changed_rows": 2}))


def decode_mode(args):
    from valley_amd import ops
    from valley_amd.decode import DecodeSession
    from valley_amd.llama import HipKVCache, HipLlama
    d = torch.device("cuda:0")
    ll = HipLlama(5120, 40, 13824, args.layers, 32000, 1e-5).init_random(seed=1)
    S = args.prefix
    for nb, mode in [(int(b), m) for b in args.beams.split(",") for m in ("greedy", "beam")]:
        if nb == 1 and mode == "beam":
            continue
        cache = ll.new_cache(nb, S + args.steps + args.warmup + 4)
        h = torch.randn((S, ll.H), generator=torch.Generator(device="cuda").manual_seed(3), device=d) * 0.02
        x = ll.forward(h, 1, S, HipKVCache.rows_of(cache, 0, 1))
        table = ops.kv_beam_table(cache.k, cache.v, d)
        ops.kv_beam_reorder(table, cache.k[0], torch.zeros((nb,), dtype=torch.int32, device=d), 0, S)
        cache.seq_len = S
        logits = ll.logits(x.view(1, S, -1)[:, -1].contiguous()).repeat_interleave(nb, 0).contiguous()
        if mode == "greedy":
            sess = DecodeSession(ll, cache, use_graph=True)
            sess.begin(logits.argmax(-1))
        else:
            K = ops.beam_k(nb, 0)
            running = torch.full((nb,), -1e9, device=d)
            running[0] = 0
            cand = ops.beam_candidates(logits, running, 1, nb, K, None, ops.beam_scratch(1, nb, K, d))
            sess = DecodeSession(ll, cache, use_graph=True, beams=(1, nb, S, []))
            ops.beam_select(*cand, 1, nb, tok=sess.tok, parent=sess.parent, running=sess.running)
            sess.begin(sess.tok.clone())
        for _ in range(args.warmup):
            sess.step()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        moved = 0
        t0 = time.perf_counter()
        e0.record()
        for _ in range(args.steps):
            sess.step()
        e1.record()
        torch.cuda.synchronize()
        wall = time.perf_counter() - t0
        sess.check()
        if mode == "beam":
            moved = int((sess.parent.cpu() != torch.arange(nb)).sum())
        ms = e0.elapsed_time(e1) / args.steps
        print(json.dumps({"nb": nb, "mode": mode, "layers": args.layers, "prefix": S, "steps": args.steps, "ms_per_step": round(ms, 4),
                          "wall_ms_per_step": round(wall / args.steps * 1e3, 4), "rows_moved_last_step": moved}), flush=True)
        del sess, cache


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kernel", action="store_true")
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--steps", type=int, default=256)
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--prefix", type=int, default=336)
    ap.add_argument("--layers", type=int, default=40)
    ap.add_argument("--beams", default="1,4,8")
    args = ap.parse_args()
    if args.kernel:
        kernel_mode(args.iters)
    else:
        decode_mode(args)


if __name__ == "__main__":
    main()
