"""Child process of tests/test_gemv_exact_gpu.py for the decode GEMV branches that only an environment switch selects (the
switches are read once per process).  argv[1]:
  "A": VLY_GEMV_ROWS=4 VLY_GEMV_MFMA=0 — the four-row kernel at small shapes on any device, and the VALU MR = 4 / 8 kernels at
       aligned shapes;
  "B": VLY_GEMV_MFMA=1 — gemv_mfma_kernel, the matrix-core form that loads its fragments straight from global memory.
Every check asserts through the dispatch mirror of tests/gemv_oracle.py that its call reaches the kernel it names.  VALLEY_PRECISION
is inherited: the same checks run on the fp16 library.  Prints one JSON line."""
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    which = sys.argv[1]
    from tests import gemv_oracle as G
    from valley_amd import lib, ops
    ops.GEMM_MODE = "tiles"
    want = G.WORKER_A_ENV if which == "A" else G.WORKER_B_ENV
    have = {k: v for k, v in os.environ.items() if k.startswith("VLY_GEMV_")}
    assert have == want and "VALLEY_HIP_LIB" not in os.environ, (have, want)
    reached, calls = set(), 0
    if which == "A":
        for s in G.WORKER_A_FOUR:
            for M in s.Ms:
                G.check_linear(M, s.N, s.K, f"gemv_kernel<MR={M},KS=4,NR=4>", reached=reached)
                calls += 1
        for s in G.WORKER_A_VALU:
            for M in s.Ms:
                G.check_linear(M, s.N, s.K, f"gemv_kernel<MR={4 if M <= 4 else 8},KS={4 if s.K >= 2048 else 1},NR=2>", full=False, reached=reached)
                calls += 1
        for M in (1, 2):
            G.check_epilogues(M, 1032, 2048, f"gemv_kernel<MR={M},KS=4,NR=4>", reached=reached)
        for M in (3, 8):
            G.check_epilogues(M, 1032, 2048, f"gemv_kernel<MR={4 if M <= 4 else 8},KS=4,NR=2>", reached=reached)
    else:
        for s in G.WORKER_B:
            for M in s.Ms:
                G.check_linear(M, s.N, s.K, "gemv_mfma", full=M in (3, 16), reached=reached)
                calls += 1
        for N, K in G.WORKER_B_EPILOGUE:
            for M in (3, 8, 11, 16):
                G.check_epilogues(M, N, K, "gemv_mfma", reached=reached)
    torch.cuda.synchronize()
    print(json.dumps({"which": which, "ok": True, "reached": sorted(reached), "linear_checks": calls,
                      "storage": lib.load().vly_storage_dtype(), "cus": G.cu_count()}))


main()
