"""Audit of the kernels that own their accumulation registers BY NAME (gemm_p4_kernel's rolled instantiations, gemm_p32_kernel,
gemm_p16_kernel): in the ISA hipcc emits for them no instruction OUTSIDE an inline-asm block may name an accumulation register — the
compiler has no value there, and a spill or copy of its own into a0 .. a255 silently corrupts a tile.  Also required: no scratch.
valley_amd.build runs this on the ISA of EVERY library it builds (the fp16 library was shipped unaudited) and fails the
build on a finding; tools/agpr_audit.py is the command-line form.
Kernels that hold accumulator blocks in ARCH VGPRs as well (gemm_p4_kernel<192, 384, ...>: v224 .. v255, reserved at its entry) are
held to the same rule for those: from the lowest VGPR an asm MFMA accumulates into up to v255, no instruction outside an inline-asm block
names a register, inside one only the MFMAs (as D / C) and the v_mov_b32 reads of the blocks (as source) do, and the descriptor's arch
VGPRs (accum_offset) cover them."""
import re
import subprocess

AUDITED = {"gemm_bf16.hip": "gemm_p4_kernel", "gemm_p32.hip": "gemm_p32_kernel", "gemm_p16.hip": "gemm_p16_kernel"}


def audit_asm(asm_path, kern):
    """-> (lines of report, number of audited kernels, number of findings)"""
    asm = open(asm_path).read().splitlines()
    bad = kernels = 0
    report = []
    i = 0
    areg = re.compile(r"\ba(\[(\d+|0x[0-9a-f]+)(:(\d+|0x[0-9a-f]+))?\]|\d+\b)")
    while i < len(asm):
        m = re.match(r"^(_ZN\S*" + kern + r"\S*):", asm[i])
        if not m:
            i += 1
            continue
        name = subprocess.run(["c++filt", m.group(1)], capture_output=True, text=True).stdout.strip()
        name = re.sub(r"\(anonymous namespace\)::", "", name).split("(")[0].replace("void ", "")
        j = i + 1
        in_asm = False
        outside, n_mfma, n_rd, n_mfma_compiler = [], 0, 0, 0
        while j < len(asm) and "s_endpgm" not in asm[j]:
            ln = asm[j]
            if ";;#ASMSTART" in ln:
                in_asm = True
            elif ";;#ASMEND" in ln:
                in_asm = False
            else:
                code = ln.split(";")[0]
                if in_asm:
                    if "v_mfma" in code:
                        n_mfma += 1
                    if "v_accvgpr_read" in code:
                        n_rd += 1
                elif areg.search(code) and not code.strip().startswith("."):
                    outside.append((j - i, code.strip()))
                    if "v_mfma" in code:
                        n_mfma_compiler += 1
                if "scratch_" in code:
                    outside.append((j - i, code.strip()))
            j += 1
        # the kernel descriptor must allocate every accumulation register the asm names (it does so only because of the clobber list
        # at the kernel's entry): next_free_vgpr - accum_offset >= highest named register + 1
        named = [int(x, 0) for ln in asm[i:j] for x in re.findall(r"\ba\[(?:\d+|0x[0-9a-f]+):(\d+|0x[0-9a-f]+)\]", ln.split(";")[0])]
        desc = "\n".join(asm[j:j + 120])
        nf = re.search(r"\.amdhsa_next_free_vgpr\s+(\d+)", desc)
        ao = re.search(r"\.amdhsa_accum_offset\s+(\d+)", desc)
        lit = n_mfma > 0 and n_mfma_compiler == 0 and "v_mfma" not in "\n".join(c for _, c in outside)
        if lit and named and nf and ao and int(nf.group(1)) - int(ao.group(1)) < max(named) + 1:
            outside.append((0, f"descriptor allocates {int(nf.group(1)) - int(ao.group(1))} accumulation registers, the asm names a{max(named)}"))
        if lit and not (nf and ao):
            outside.append((0, "kernel descriptor not found behind the kernel"))
        if n_mfma_compiler:              # the compiler manages this kernel's accumulators (builtin MFMAs): not audited
            lit = False
        vbad, n_vacc = _audit_vgpr_blocks(asm[i + 1:j], desc) if lit else ([], 0)
        outside += vbad
        if lit:
            kernels += 1
            status = "ok" if not outside else "FAIL"
            report.append(f"{name:48s} mfma {n_mfma:4d}  acc reads {n_rd:4d}  compiler AGPR / scratch instructions: {len(outside)}  {status}"
                          + (f"  (+{n_vacc} accumulation VGPRs by name)" if n_vacc else ""))
            for off, code in outside[:8]:
                report.append(f"    +{off}: {code}")
            bad += len(outside)
        i = j
    return report, kernels, bad


def audit_plain(asm_path):
    """Kernels that own no accumulation register by name (the beam-search library): no instruction of any kernel names an
    accumulation register or touches scratch.  -> (lines of report, number of kernels, number of findings)"""
    asm = open(asm_path).read().splitlines()
    areg = re.compile(r"\ba(\[(\d+|0x[0-9a-f]+)(:(\d+|0x[0-9a-f]+))?\]|\d+\b)")
    report, kernels, bad = [], 0, 0
    i = 0
    while i < len(asm):
        m = re.match(r"^(_Z\S*kernel\S*):", asm[i])
        if not m:
            i += 1
            continue
        j, found = i + 1, []
        while j < len(asm) and "s_endpgm" not in asm[j]:
            code = asm[j].split(";")[0]
            if (areg.search(code) and not code.strip().startswith(".")) or "scratch_" in code or "v_accvgpr" in code:
                found.append((j - i, code.strip()))
            j += 1
        kernels += 1
        bad += len(found)
        report.append(f"{m.group(1)[:60]:60s} accumulation-register / scratch instructions: {len(found)}  {'FAIL' if found else 'ok'}")
        report += [f"    +{off}: {code}" for off, code in found[:8]]
        i = j
    return report, kernels, bad


_VREG = re.compile(r"\bv(?:\[(\d+|0x[0-9a-f]+)(?::(\d+|0x[0-9a-f]+))?\]|(\d+)\b)")


def _vregs(code):
    """-> [(first, last)] of every VGPR (range) an instruction names: v7, v[7], v[0xe0], v[4:7]"""
    return [(int(a, 0), int(b or a, 0)) if a else (int(c), int(c)) for a, b, c in _VREG.findall(code)]


def _audit_vgpr_blocks(body, desc):
    """Accumulator blocks in arch VGPRs, named by the asm (an asm MFMA whose D is v[..]): -> (findings as (offset, text), registers)"""
    lines, in_asm = [], False
    for k, ln in enumerate(body):
        if ";;#ASMSTART" in ln:
            in_asm = True
        elif ";;#ASMEND" in ln:
            in_asm = False
        else:
            code = ln.split(";")[0].strip()
            if code and not code.startswith("."):
                lines.append((k + 1, code, in_asm))
    dsts = [_vregs(c)[0] for _, c, a in lines if a and c.startswith("v_mfma") and re.match(r"v_mfma\S*\s+v\[", c)]
    if not dsts:
        return [], 0
    base = min(d[0] for d in dsts)
    top = max(d[1] for d in dsts)
    bad = []
    for off, code, in_asm in lines:
        regs = [r for r in _vregs(code) if r[1] >= base]
        if not regs:
            continue
        if not in_asm:
            bad.append((off, code))                      # the compiler's own instruction in the blocks' registers
        elif code.startswith("v_mfma"):
            ops = _vregs(code)                           # D, A, B[, C]: A and B never in the range, C (if a register) is D
            if len(ops) < 3 or ops[1][1] >= base or ops[2][1] >= base or (len(ops) > 3 and ops[3] != ops[0]):
                bad.append((off, code))
        elif code.startswith("v_mov_b32"):
            ops = _vregs(code)                           # a block read: destination outside, source inside
            if len(ops) != 2 or ops[0][1] >= base or ops[1][0] < base:
                bad.append((off, code))
        else:
            bad.append((off, code))
    ao = re.search(r"\.amdhsa_accum_offset\s+(\d+)", desc)
    if not ao or int(ao.group(1)) < top + 1:
        bad.append((0, f"descriptor's arch VGPRs ({ao.group(1) if ao else '?'}) do not cover v{top} the asm accumulates into"))
    return bad, top + 1 - base
