"""What conversation KV reuse costs and saves at 13B shapes (40 heads, 40 random layers), ONE process, on tools/spec_rows_ab.py's
method: the arms of a point are interleaved, in a fresh random order every round, behind a warm-up block that is dropped; the
figure of an arm is the median of its blocks and the blocks themselves are reported (their spread is the noise).

Kernel: the attention launch of S new queries over ``past`` cached keys, S in {8, 16, 32, 64} x past in {336, 1500}
  prefill      ops.llama_attention (llama_attn2_kernel: what a forward over a filled cache launches today)
  split        ops.suffix_attention (the shipped libvalley_hip_suffix.so)
  <name>       --variants name=path[,name=path]: other builds of the same library (the split rule's constants,
               -DVLY_SUFFIX_TILES_PER_SPLIT=n), called through the same binding
  A block walks the 40 layers' caches (1.3 GB at 1564 keys: no launch finds its keys in a cache the one before left).
Turn: a 32-token turn over a context of 336 / 1500 tokens (the 8-frame visual block in it)
  scratch          the whole prompt through the model's forward into an empty cache, tower included: what every turn costs today
  session_prefill  PrefixSession(attention="prefill").prefill: 32 tokens behind the cached context
  session_split    PrefixSession(attention="split").prefill: the same on the split kernel
  (two different 32-token suffixes alternate, so every timed call reuses exactly the context and computes 32 tokens)

  python tools/prefix_ab.py [--rounds 3] [--reps 8] [--turn-reps 4] [--variants tps1=...so] [--out profiles/r13/prefix_ab.jsonl]
"""
import argparse
import ctypes
import json
import os
import random
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

QUERIES = (8, 16, 32, 64)
PASTS = (336, 1500)
HEADS, LAYERS = 40, 40


def timed(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


def interleave(arms, rounds, reps, rng):
    """arms: name -> callable (one unit of work).  -> name -> [ms per unit of every block behind the warm-up round]"""
    times = {name: [] for name in arms}
    for rnd in range(rounds + 1):                            # round 0 warms every arm up and is dropped
        order = list(arms)
        rng.shuffle(order)                                   # no arm always runs behind the same other
        for name in order:
            t = timed(arms[name], reps)
            if rnd:
                times[name].append(t)
    return times


def variant_call(path):
    from valley_amd import lib_suffix
    from valley_amd.lib import bind
    lib = ctypes.CDLL(path)
    bind(lib, path, lib_suffix.SIGS)
    assert lib.vly_suffix_abi_version() == lib_suffix.ABI_VERSION
    return lib.vly_suffix_attention


def kernel_points(args, emit, rng):
    from valley_amd import ops, runtime
    dev = torch.device("cuda:0")
    variants = dict(v.split("=", 1) for v in args.variants.split(",") if v)
    calls = {name: variant_call(path) for name, path in variants.items()}
    g = torch.Generator(device=dev).manual_seed(5)
    dt = 1 if runtime.HALF == torch.float16 else 0
    for past in PASTS:
        ctx = past + max(QUERIES)
        ks = [torch.randn((1, HEADS, ctx, 128), generator=g, device=dev).to(runtime.HALF) for _ in range(LAYERS)]
        vs = [torch.randn((1, HEADS, ctx, 128), generator=g, device=dev).to(runtime.HALF) for _ in range(LAYERS)]
        for S in QUERIES:
            qkv = torch.randn((S, 3 * HEADS * 128), generator=g, device=dev).to(runtime.HALF)
            out = torch.empty((S, HEADS * 128), dtype=runtime.HALF, device=dev)
            scratch = ops.suffix_scratch(1, S, HEADS, dev)
            stream = torch.cuda.current_stream().cuda_stream

            def prefill():
                for k, v in zip(ks, vs):
                    ops.llama_attention(qkv, k, v, None, 1, S, HEADS, past, out=out)

            def split():
                for k, v in zip(ks, vs):
                    ops.suffix_attention(qkv, k, v, None, 1, S, HEADS, past, scratch, out=out)

            def raw(fn):
                def run():
                    for k, v in zip(ks, vs):
                        rc = fn(qkv.data_ptr(), k.data_ptr(), v.data_ptr(), None, 0, out.data_ptr(), 1, S, HEADS, past, None, ctx, dt,
                                scratch.data_ptr(), stream)
                        assert rc == 0, rc
                return run

            arms = {"prefill": prefill, "split": split, **{name: raw(fn) for name, fn in calls.items()}}
            # the arms agree before they are timed (faster and different is not faster)
            prefill()
            want = out.float().clone()
            for name in arms:
                if name != "prefill":
                    out.zero_()
                    arms[name]()
                    err = float((out.float() - want).abs().max())
                    assert err < 2e-2, (name, S, past, err)
            times = interleave(arms, args.rounds, args.reps, rng)
            for name, t in times.items():
                emit({"part": "kernel", "S": S, "past": past, "arm": name, "heads": HEADS, "dtype": str(runtime.HALF),
                      "launches_per_block": args.reps * LAYERS, "us_per_launch": round(statistics.median(t) * 1e3 / LAYERS, 2),
                      "blocks_us": [round(x * 1e3 / LAYERS, 2) for x in t]})
        del ks, vs
        torch.cuda.empty_cache()
    assert int(scratch[-HEADS:].abs().sum()) == 0


def turn_points(args, emit, rng):
    from valley_amd import ops, runtime
    from valley_amd import valley_model as vm
    from valley_amd import weights as W
    from valley_amd.prefix import PrefixSession
    dev = torch.device("cuda:0")
    T, H, I, vocab_text = 8, 5120, 13824, 32000
    config = vm.ValleyConfig(vocab_size=vocab_text + 6, hidden_size=H, intermediate_size=I, num_hidden_layers=LAYERS,
                             num_attention_heads=HEADS, num_key_value_heads=HEADS, rms_norm_eps=1e-5, max_position_embeddings=2048)
    config.use_mm_proj, config.mm_hidden_size, config.mm_vision_select_layer = True, 1024, -2
    model = vm.ValleyLlamaForCausalLM(config, device=dev)
    mm = model.get_model()
    mm.llama.init_random(seed=0)
    tower = vm.build_vision_tower(None, device=dev)
    tower.init_random(seed=0, layers=23)
    for k, v in W.SPECIAL_IDS(vocab_text).items():
        setattr(tower.config, k, v)
    mm.initialize_vision_modules(tower, -2)
    g = torch.Generator(device=dev).manual_seed(1234)
    frames = torch.randn((1, T, 3, 224, 224), generator=g, device=dev).to(runtime.HALF)
    head = torch.from_numpy(W.synthetic_prompt(7, T, vocab_text)).view(1, -1)                # 320 + T tokens, the visual block in it
    gen = torch.Generator().manual_seed(7)
    for ctx in PASTS:
        text = torch.randint(3, vocab_text, (1, ctx - head.shape[1]), generator=gen)
        base = torch.cat([head, text], 1).to(dev)
        tails = [torch.randint(3, vocab_text, (1, 32), generator=gen).to(dev) for _ in range(2)]
        tails[1][0, 0] = (tails[0][0, 0] + 1 - 3) % (vocab_text - 3) + 3                       # the suffixes differ at their first token
        prompts = [torch.cat([base, t], 1) for t in tails]
        cache = mm.llama.new_cache(1, ctx + 32)
        sessions = {arm: PrefixSession(model, attention=arm) for arm in ("prefill", "split")}
        for s in sessions.values():
            s.prefill(base, frames)
        flip = {"scratch": 0, "prefill": 0, "split": 0}

        def scratch():
            cache.truncate(0)
            flip["scratch"] ^= 1
            model(input_ids=prompts[flip["scratch"]], images=frames, past_key_values=cache, use_cache=True)

        def through(arm):
            def run():
                flip[arm] ^= 1
                sessions[arm].prefill(prompts[flip[arm]], frames)
            return run

        arms = {"scratch": scratch, "session_prefill": through("prefill"), "session_split": through("split")}
        for _ in range(12):                                  # the GEMM tuner's trials of the new row counts end before anything is timed
            for fn in arms.values():
                fn()
            torch.cuda.synchronize()
            if not ops.tuning_pending():
                break
        times = interleave(arms, args.rounds, args.turn_reps, rng)
        for arm, s in sessions.items():
            assert s.stats["tower_runs"] == 1 and s.cache.seq_len == ctx + 32, (arm, s.stats)
        for name, t in times.items():
            emit({"part": "turn", "context": ctx, "new_tokens": 32, "frames": T, "arm": name, "layers": LAYERS, "dtype": str(runtime.HALF),
                  "calls_per_block": args.turn_reps, "ms_per_turn": round(statistics.median(t), 3), "blocks_ms": [round(x, 3) for x in t],
                  "tuning_pending": int(ops.tuning_pending())})
        del cache, sessions
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=8, help="walks over the 40 layers per kernel block")
    ap.add_argument("--turn-reps", type=int, default=4, help="turns per block")
    ap.add_argument("--variants", type=str, default="")
    ap.add_argument("--parts", type=str, default="kernel,turn")
    ap.add_argument("--out", type=str, default="")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "prefix_ab.py measures on the GPU: there is no other figure to report"
    lines = []

    def emit(rec):
        print(json.dumps(rec), flush=True)
        lines.append(json.dumps(rec))
        if args.out:                                         # (kept as it grows: a later part's failure loses nothing)
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                f.write("\n".join(lines) + "\n")

    rng = random.Random(0)
    if "kernel" in args.parts:
        kernel_points(args, emit, rng)
    if "turn" in args.parts:
        turn_points(args, emit, rng)


if __name__ == "__main__":
    main()
