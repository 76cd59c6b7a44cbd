"""Per-step time of decoding with HF's logits processors inside the captured step (DecodeSession(processors=True)) against
the same session without them.

    python tools/logits_decode_time.py [--steps 256] [--rows 1,8] [--beams 4] [--prefix 336] [--layers 40]
    python tools/logits_decode_time.py --kernel [--iters 200]     # only the processor launches (run under
                                                                  # rocprofv3 --kernel-trace --stats for their times)

The decode mode builds a 13B-shaped HipLlama (hidden 5120, 40 heads, 13824, 40 layers, V 32000; random weights), prefills
one prompt of --prefix positions into every row and times --steps captured steps: greedy sessions of each --rows count and
beam sessions of each --beams count, each without processors and with all three on (repetition_penalty 1.2,
no_repeat_ngram_size 3, min_new_tokens 16 with an EOS id).  One JSON line per (mode, rows, processors)."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

S_PROMPT, V = 336, 32000


def kernel_mode(iters):
    """vly_logits_process at B in {1, 4, 8} (logit mode) and nb = 4 (history gather + log-softmax mode + scored candidates),
    all processors on, 336 + 256 positions of history."""
    from valley_amd import ops
    d = torch.device("cuda:0")
    g = torch.Generator(device="cuda").manual_seed(5)
    L = S_PROMPT + 256
    eos = torch.tensor([2], dtype=torch.int32, device=d)
    pos = torch.tensor([L - 1], dtype=torch.int32, device=d)

    def rows(B):
        return (torch.randn((B, V), generator=g, device=d) * 3,
                torch.randint(3, V, (B, L + 8), generator=g, device=d, dtype=torch.int32),
                ops.processor_rows(1.2, 3, None, 16, prompt_len=S_PROMPT, device=d).expand(B, 4).contiguous(),
                torch.randint(3, V, (B,), generator=g, device=d, dtype=torch.int32))
    for B in (1, 4, 8):
        x, hist, params, tok = rows(B)
        for _ in range(iters):
            ops.logits_process(x, params, hist, pos, 1, tok=tok, eos=eos)
    nb = 4
    x, hist, params, tok = rows(nb)
    K = ops.beam_k(nb, 1)
    parent = torch.tensor([0, 0, 1, 3], dtype=torch.int32, device=d)
    running = torch.randn((nb,), generator=g, device=d) - 5
    scratch = ops.beam_scratch(1, nb, K, d)
    for _ in range(iters):
        ops.logits_history_gather(hist, parent, S_PROMPT, 0, len_dev=pos)
        ops.logits_process(x, params, hist, pos, 1, tok=tok, eos=eos, log_softmax=True)
        ops.logits_beam_candidates(x, running, 1, nb, K, eos, scratch)
    torch.cuda.synchronize()
    print(json.dumps({"kernel_mode": "done", "iters": iters, "history": L}))


def decode_mode(args):
    from valley_amd import ops
    from valley_amd.decode import DecodeSession
    from valley_amd.llama import HipKVCache, HipLlama
    d = torch.device("cuda:0")
    ll = HipLlama(5120, 40, 13824, args.layers, V, 1e-5).init_random(seed=1)
    S = args.prefix
    eos = [2]
    runs = [("greedy", int(b)) for b in args.rows.split(",") if b] + [("beam", int(b)) for b in args.beams.split(",") if b]
    for (mode, n), proc in [(r, p) for r in runs for p in (False, True)]:
        cache = ll.new_cache(n, S + args.steps + args.warmup + 4)
        h = torch.randn((S, ll.H), generator=torch.Generator(device="cuda").manual_seed(3), device=d) * 0.02
        x = ll.forward(h, 1, S, HipKVCache.rows_of(cache, 0, 1))
        table = ops.kv_beam_table(cache.k, cache.v, d)
        ops.kv_beam_reorder(table, cache.k[0], torch.zeros((n,), dtype=torch.int32, device=d), 0, S)
        cache.seq_len = S
        logits = ll.logits(x.view(1, S, -1)[:, -1].contiguous()).repeat_interleave(n, 0).contiguous()
        prompt = torch.randint(3, V, (1, S), generator=torch.Generator().manual_seed(4)).repeat(n, 1).to(d)
        params = ops.processor_rows(1.2, 3, None, 16, prompt_len=S, device=d).expand(n, 4)
        if mode == "greedy":
            sess = DecodeSession(ll, cache, use_graph=True, processors=proc, processor_eos=eos)
            if proc:
                sess.proc.copy_(params)
            sess.begin(logits.argmax(-1), prompt_ids=prompt if proc else None)
        else:
            K = ops.beam_k(n, len(eos))
            running = torch.full((n,), -1e9, device=d)
            running[0] = 0
            cand = ops.beam_candidates(logits, running, 1, n, K, torch.tensor(eos, dtype=torch.int32, device=d),
                                       ops.beam_scratch(1, n, K, d))
            sess = DecodeSession(ll, cache, use_graph=True, beams=(1, n, S, eos), processors=proc)
            if proc:
                sess.proc.copy_(params)
            ops.beam_select(*cand, 1, n, tok=sess.tok, parent=sess.parent, running=sess.running)
            sess.begin(sess.tok.clone(), prompt_ids=prompt if proc else None)
        for _ in range(args.warmup):
            sess.step()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        e0.record()
        for _ in range(args.steps):
            sess.step()
        e1.record()
        torch.cuda.synchronize()
        wall = time.perf_counter() - t0
        sess.check()
        ms = e0.elapsed_time(e1) / args.steps
        print(json.dumps({"mode": mode, "rows": n, "processors": proc, "layers": args.layers, "prefix": S, "steps": args.steps,
                          "ms_per_step": round(ms, 4), "wall_ms_per_step": round(wall / args.steps * 1e3, 4)}), flush=True)
        del sess, cache


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kernel", action="store_true")
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--steps", type=int, default=256)
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--prefix", type=int, default=S_PROMPT)
    ap.add_argument("--layers", type=int, default=40)
    ap.add_argument("--rows", default="1,8")
    ap.add_argument("--beams", default="4")
    args = ap.parse_args()
    if args.kernel:
        kernel_mode(args.iters)
    else:
        decode_mode(args)


if __name__ == "__main__":
    main()
