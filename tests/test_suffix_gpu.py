"""GPU checks of the split suffix attention (include/valley_hip_suffix.h, ops.suffix_attention) on the cases of
tests/suffix_cases.py:

* the three exact checks of tests/attention_oracle.py — (a) the output row is V[target] bit for bit, (b) replacing everything
  invisible leaves the bits, (c) count_c / n within one ulp of the storage type.  They hold for this kernel as they hold for
  llama_attn2_kernel inside a split (same arithmetic), and across splits because the merge's weights exp2(m_s - m) are exactly
  1 or 0 under (a), exactly 1 (0 for a split whose keys are all masked or in the query's future) under (c), and a masked or
  future split contributes 0 x finite = 0 under (b);
* launches alternate between the host position and ``past_dev`` (then with a WRONG host value); after every launch the caches
  are bitwise untouched and the ticket counters are zero; two launches give equal bits;
* on dense data the error against the fp64 reference is at most 1.5 x ops.llama_attention's on the same inputs;
* a child process repeats one case and the turn-2 generation on the fp16 library; another shows that a plain ``generate``
  never loads the library.

Measured figures are printed before they are asserted."""
import json
import os
import subprocess
import sys

import pytest
import torch

from tests import attention_oracle as AO
from tests import suffix_cases as SC
from valley_amd.runtime import HALF

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"


def pack_qkv(inp):
    """The rotated q in the q slot of a q | k | v buffer whose other two thirds hold data the kernel must not read."""
    c = inp.case
    Hq = c.heads * 128
    qkv = torch.full((c.B * c.S, 3 * Hq), 3.0, dtype=HALF, device=DEV)
    qkv[:, :Hq] = inp.q.to(DEV).reshape(c.B * c.S, Hq)
    return qkv


class SuffixRun:
    """``run(inp)`` of the oracle's checks.  Even launches pass the position on the device with a wrong host value (key_valid
    widened with ones to the cache's depth, as that form requires), odd ones pass it on the host."""

    def __init__(self):
        self.launches = 0
        self.scratch = {}

    def __call__(self, inp):
        from valley_amd import ops
        c = inp.case
        B, S, heads, past = c.B, c.S, c.heads, c.past
        qkv = pack_qkv(inp)
        k0, v0 = inp.k.to(DEV).contiguous(), inp.v.to(DEV).contiguous()
        k, v = k0.clone(), v0.clone()
        valid = None if inp.valid is None else inp.valid.to(DEV)
        key = (B, S, heads)
        if key not in self.scratch:
            self.scratch[key] = ops.suffix_scratch(B, S, heads, DEV)
        scratch = self.scratch[key]
        on_device = self.launches % 2 == 0
        self.launches += 1
        if on_device:
            if valid is not None and valid.shape[1] < c.ctx_max:
                wide = torch.ones((B, c.ctx_max), dtype=torch.uint8, device=DEV)
                wide[:, :valid.shape[1]] = valid
                valid = wide
            wrong = 0 if past != 0 else min(1, c.ctx_max - S)
            out = ops.suffix_attention(qkv, k, v, valid, B, S, heads, wrong, scratch,
                                       past_dev=torch.tensor([past], dtype=torch.int32, device=DEV))
        else:
            out = ops.suffix_attention(qkv, k, v, valid, B, S, heads, past, scratch)
        assert torch.equal(AO.bits(k), AO.bits(k0)) and torch.equal(AO.bits(v), AO.bits(v0)), "the caches are read-only"
        assert int(scratch[-B * heads:].abs().sum()) == 0, "ticket counters not back at zero"
        return out.view(B, S, heads, 128)


def attention_checks(case):
    run = SuffixRun()
    AO.check_pointer(case, run, HALF, DEV)
    AO.check_count(case, run, HALF, DEV)
    AO.check_invisible(case, run, HALF, DEV)
    inp = AO.build_dense(case, HALF, DEV)
    a, b = run(inp), run(inp)                                # (one through the device-side position, one through the host's)
    assert torch.equal(AO.bits(a), AO.bits(b)), "two launches differ"
    return run.launches


@pytest.mark.parametrize("case", SC.CASES, ids=lambda c: c.name)
def test_suffix_attention_exact(case):
    n = attention_checks(case)
    print(f"{case.name}: {n} launches")


def _errors(out, ref):
    d = out.double().cpu() - ref
    return float(d.abs().max()), float(d.norm() / ref.norm())


@pytest.mark.parametrize("name", SC.DENSE)
def test_dense_error_against_the_prefill_kernel(name):
    """Both kernels round P and the output to 16 bits; the merge adds a handful of fp32 roundings.  1.5 covers how far the
    maximum over a few thousand elements moves between two correct kernels."""
    from valley_amd import ops
    case = SC.BY_NAME[name]
    inp = AO.build_dense(case, HALF, DEV)
    ref = AO.reference(inp)
    got = SuffixRun()(inp)
    valid = None if inp.valid is None else inp.valid.to(DEV)
    base = ops.llama_attention(pack_qkv(inp), inp.k.to(DEV).contiguous(), inp.v.to(DEV).contiguous(), valid, case.B, case.S, case.heads,
                               case.past).view(case.B, case.S, case.heads, 128)
    (ma, l2), (ma0, l20) = _errors(got, ref), _errors(base, ref)
    print(f"{name}: suffix max-abs {ma:.3e} rel-L2 {l2:.3e}; llama_attention {ma0:.3e} {l20:.3e}; ratios {ma / ma0:.3f} {l2 / l20:.3f}")
    assert ma <= 1.5 * ma0 and l2 <= 1.5 * l20


def test_scratch_size_is_the_librarys():
    from valley_amd import lib_suffix, ops
    for B, S, heads in ((1, 64, 40), (2, 31, 4)):
        s = ops.suffix_scratch(B, S, heads, DEV)
        assert s.numel() * 4 == lib_suffix.load().vly_suffix_scratch_bytes(B, S, heads) and int(s.abs().sum()) == 0


# ---- the fp16 storage type, and a run that never reuses ------------------------------------------------------------------------
def _worker(mode, env_extra):
    env = {k: v for k, v in os.environ.items() if k not in ("VALLEY_PRECISION", "VALLEY_SUFFIX_ATTN")}
    env.update(env_extra)
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "suffix_worker.py"), mode], capture_output=True, text=True, env=env,
                       timeout=600)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    return json.loads(p.stdout.strip().splitlines()[-1])


def test_suffix_on_the_fp16_library():
    res = _worker("fp16", {"VALLEY_PRECISION": "fp16"})
    print(res)
    assert res["ok"] and res["storage"] == 1 and res["turn2_split"] == SC.TURN2_TOKENS and res["turn2_plain"] == SC.TURN2_TOKENS
    assert res["reused"] == 289 and res["suffix_lib_loaded"] is True


def test_plain_generate_never_loads_the_suffix_library():
    res = _worker("off", {})
    assert res["ok"] and res["new_tokens"] == 4 and res["suffix_lib_loaded"] is False and res["prefix_imported"] is False
