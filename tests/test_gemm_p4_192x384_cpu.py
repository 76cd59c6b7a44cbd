"""Compile-time gate of tile hint 194 (gemm_p4_kernel<192, 384, SwiGLU>, no GPU needed): 72 accumulator blocks per wave, 64 in a0 .. a255
and 8 in v224 .. v255, all named by inline asm.  The ISA hipcc emits must show no scratch, no compiler instruction on any of those
registers, and a descriptor that allocates them; and the audit that checks it must catch a compiler instruction in them."""
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def test_192x384_instantiation_passes_the_accumulator_audit():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "agpr_audit.py")], capture_output=True, text=True, timeout=1200)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("gemm_p4_kernel<192, 384, 2, 0, false>")]
    assert len(line) == 1, r.stdout[-3000:]
    # 72 blocks x 2 K steps x (first K tile + the loop's K tile); 64 blocks read from AGPRs per tile; the 32 VGPRs by name
    assert re.search(r"mfma\s+288\s+acc reads\s+256\s+compiler AGPR / scratch instructions: 0\s+ok\s+\(\+32 accumulation VGPRs by name\)", line[0]), line
    assert re.search(r"kernels with accumulators by name audited, 0 findings", r.stdout)


def _kernel(body, desc_accum_offset=256):
    return "\n".join(["_ZN12_GLOBAL__N_114gemm_p4_kernelILi192ELi384ELi2ELi0ELb0EEEvPKt:", *body, "\ts_endpgm",
                      "\t.amdhsa_next_free_vgpr 512", f"\t.amdhsa_accum_offset {desc_accum_offset}"]) + "\n"


GOOD = [";;#ASMSTART", "\tv_mfma_f32_16x16x32_bf16 a[0:3], v[0:3], v[4:7], 0", ";;#ASMEND",
        ";;#ASMSTART", "\tv_mfma_f32_16x16x32_bf16 v[0xe0:0xe3], v[8:11], v[4:7], 0", ";;#ASMEND",
        ";;#ASMSTART", "\tv_mfma_f32_16x16x32_bf16 v[0xfc:0xff], v[8:11], v[4:7], v[0xfc:0xff]", ";;#ASMEND",
        ";;#ASMSTART", "\tv_accvgpr_read_b32 v12, a[0]", ";;#ASMEND",
        ";;#ASMSTART", "\tv_mov_b32 v13, v[0xe0]", ";;#ASMEND",
        "\tv_add_u32_e32 v14, v13, v12"]


def _audit(text, tmp_path):
    from valley_amd.agpr_audit import audit_asm
    p = tmp_path / "k.s"
    p.write_text(text)
    return audit_asm(str(p), "gemm_p4_kernel")


def test_audit_accepts_named_vgpr_blocks(tmp_path):
    report, kernels, bad = _audit(_kernel(GOOD), tmp_path)
    assert (kernels, bad) == (1, 0), report
    assert "+32 accumulation VGPRs by name" in report[0]


def test_audit_flags_the_compiler_in_the_vgpr_blocks(tmp_path):
    for extra in ("\tv_mov_b32 v230, 0", "\tv_add_u32_e32 v14, v[0xf0], v12", "\tscratch_store_dword off, v[0xe4], s0"):
        report, kernels, bad = _audit(_kernel(GOOD + [extra]), tmp_path)
        assert kernels == 1 and bad >= 1, (extra, report)
    # an asm statement whose compiler-chosen operand lands in the blocks, and a block read into a block register
    for extra in ([";;#ASMSTART", "\tv_mfma_f32_16x16x32_bf16 v[0xe0:0xe3], v[0xf0:0xf3], v[4:7], v[0xe0:0xe3]", ";;#ASMEND"],
                  [";;#ASMSTART", "\tv_mov_b32 v[0xe8], v[0xe0]", ";;#ASMEND"]):
        report, kernels, bad = _audit(_kernel(GOOD + extra), tmp_path)
        assert kernels == 1 and bad >= 1, (extra, report)
    # a descriptor whose arch VGPRs stop below the blocks
    report, kernels, bad = _audit(_kernel(GOOD, desc_accum_offset=224), tmp_path)
    assert bad >= 1, report
