"""In-process interleaved A/B of tile hints 197 and 194 on the 13B gate|up shape (2688 x 27648 x 5120, SwiGLU) with block-packed weights
as the model runs them: three rotating weight copies, arms in random order per repetition, device events; checks the arms agree.
Usage (GPU): python tools/ab_gate_up_packed.py"""
import random, statistics, sys, os
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from valley_amd import ops
D = "cuda:0"
M, N, K = 2688, 27648, 5120
a = torch.randn((M, K), device=D).to(torch.bfloat16)
ws = [ops.PackedWeight((torch.randn((N, K), device=D) * 0.02).to(torch.bfloat16)) for _ in range(3)]
outs = {t: torch.empty((M, N // 2), device=D, dtype=torch.bfloat16) for t in (197, 194)}
times = {197: [], 194: []}
rng = random.Random(0)
for rep in range(45):
    arms = [197, 194]
    rng.shuffle(arms)
    for t in arms:
        w = ws[(rep * 2 + arms.index(t)) % 3]
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        ops.gemm_mfma(a, w, epilogue=2, out=outs[t], tile_hint=t)
        e1.record()
        torch.cuda.synchronize()
        if rep >= 5:
            times[t].append(e0.elapsed_time(e1) * 1e3)
for w in ws[:1]:
    r = [ops.gemm_mfma(a, w, epilogue=2, tile_hint=t) for t in (197, 194)]
    torch.cuda.synchronize()
    print("bit-identical:", torch.equal(r[0], r[1]))
fl = 2.0 * M * N * K
for t in (197, 194):
    med = statistics.median(times[t])
    print(f"hint {t}: median {med:.1f} us  min {min(times[t]):.1f}  max {max(times[t]):.1f}  {fl / med / 1e6:.0f} TFLOP/s  (n={len(times[t])})")
print(f"194 vs 197: {statistics.median(times[197]) / statistics.median(times[194]) - 1:+.2%} faster per launch")
