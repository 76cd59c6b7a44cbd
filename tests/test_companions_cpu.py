"""The contract every companion library shares, checked once over valley_amd.build.COMPANIONS: a companion exports exactly its
header and its binding's table, the main libraries export exactly valley_hip.h, no library carries another companion's names,
a missing, incomplete or mis-versioned library fails loudly, and a companion is mapped on first use, once, never on import."""
import os
import re
import subprocess
import sys

import pytest

from valley_amd import build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = [c.name for c in build.COMPANIONS]
# per companion: the number of exports, entry points named outright, and what the missing-library error says of the feature
EXPECT = {
    "beam": (6, {"vly_beam_candidates", "vly_beam_select", "vly_kv_beam_reorder"}, "Beam search has no non-HIP path."),
    "logits": (6, {"vly_logits_process", "vly_logits_history_gather", "vly_logits_beam_candidates"},
               "The logits processors have no non-HIP path."),
    "wq": (6, set(), "INT8 weight-only decode has no non-HIP path."),
    "score": (5, set(), "Token log-probabilities and the loss have no non-HIP path."),
    "spec": (5, set(), "Speculative decoding has no non-HIP path."),
    "w4": (6, set(), "INT4 weight-only decode has no non-HIP path."),
    "spec_sample": (3, {"vly_spec_counters", "vly_spec_sample_abi_version", "vly_spec_sample_last_error"},
                    "Speculative decoding under sampling has no non-HIP path."),
}


def header_text(header):
    return open(os.path.join(ROOT, "include", header)).read()


def header_symbols(header, prefix="vly_"):
    """The functions a public header declares whose names begin with ``prefix`` (block comments do not count)."""
    txt = re.sub(r"/\*.*?\*/", "", header_text(header), flags=re.S)
    return sorted(set(re.findall(r"\b(%s[a-z0-9_]+)\s*\(" % re.escape(prefix), txt)))


def exported(path):
    """The vly_* functions a shared library defines, by ``nm -D``."""
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    return sorted(ln.split()[-1] for ln in out.splitlines() if re.search(r" T vly_[a-z0-9_]+$", ln))


def binding(name):
    import importlib
    return importlib.import_module(f"valley_amd.lib_{name}")


@pytest.fixture(scope="module")
def built():
    build.build(verbose=False)


def test_the_table_is_the_seven_companions():
    assert sorted(NAMES) == sorted(EXPECT) and len(NAMES) == 7
    for c, const in zip(build.COMPANIONS, (build.LIB_BEAM, build.LIB_LOGITS, build.LIB_WQ, build.LIB_SCORE, build.LIB_SPEC, build.LIB_W4,
                                           build.LIB_SPEC_SAMPLE)):
        assert c.lib == const == os.path.join(build.LIBDIR, f"libvalley_hip_{c.name}.so")
        assert c.header == f"valley_hip_{c.name}.h" and binding(c.name).lib_path() == c.lib
        # editing the shared prologue or anything a unit includes recompiles it
        assert "companion_capi.hpp" in build.COMPANION_SHARED
        for s in c.sources:
            src = open(os.path.join(build.CSRC, s)).read()
            assert set(re.findall(r'#include "([a-z0-9_]+\.(?:hpp|inc))"', src)) <= set(c.deps) | set(build.COMPANION_SHARED), s


@pytest.mark.parametrize("c", build.COMPANIONS, ids=NAMES)
def test_companion_exports_exactly_its_header(built, c):
    mod, up = binding(c.name), c.name.upper()
    count, named, _ = EXPECT[c.name]
    names = header_symbols(c.header)
    assert len(names) == count
    assert exported(c.lib) == names == sorted(mod.EXPORTS)
    assert named <= set(names)
    assert {f"vly_{c.name}_abi_version", f"vly_{c.name}_last_error"} <= set(names)
    assert getattr(mod.load(), f"vly_{c.name}_abi_version")() == mod.ABI_VERSION == 1
    assert re.search(rf"#define VLY_{up}_ABI_VERSION 1\b", header_text(c.header))


def header_macro(header, macro):
    return int(re.search(rf"#define {macro} (\d+)\b", header_text(header)).group(1))


def test_mirrored_header_constants(built):
    from valley_amd import lib_score, lib_spec, lib_spec_sample, lib_w4, lib_wq, ops
    for macro, a, b in (("MAX_QUERIES", lib_spec.MAX_QUERIES, ops.SPEC_MAX_QUERIES), ("MAX_DRAFT", lib_spec.MAX_DRAFT, ops.SPEC_MAX_DRAFT),
                        ("MAX_NGRAM", lib_spec.MAX_NGRAM, ops.SPEC_MAX_NGRAM), ("SPLITS", lib_spec.SPLITS, ops.SPEC_SPLITS),
                        ("PARTIAL", lib_spec.PARTIAL, ops.SPEC_PARTIAL)):
        assert header_macro("valley_hip_spec.h", f"VLY_SPEC_{macro}") == a == b, macro
    assert lib_spec.SPLITS == ops.DECODE_SPLITS
    assert header_macro("valley_hip_score.h", "VLY_SCORE_MAX_TOP") == 20 and lib_score.MAX_TOP == 20
    assert header_macro("valley_hip_spec_sample.h", "VLY_SPEC_SAMPLE_MAX_DRAFT") == lib_spec_sample.MAX_DRAFT == \
        ops.SPEC_MAX_DRAFT == lib_spec.MAX_DRAFT
    assert re.search(r"int vly_spec_counters\(const int32_t \*pos_dev, int k, int ctx_max, int32_t \*ctr, void \*stream\);",
                     header_text("valley_hip_spec_sample.h"))
    # the companion spec_sample joins is what it was: no new export there, the same ABI version
    assert "vly_spec_counters" not in exported(build.LIB_SPEC) and len(exported(build.LIB_SPEC)) == 5
    assert lib_spec.load().vly_spec_abi_version() == 1
    # host-side probes of the fused-norm GEMVs' shape rule
    assert lib_wq.load().vly_wq_gemv_rmsnorm_supported(2, 5120) == 1
    assert lib_wq.load().vly_wq_gemv_rmsnorm_supported(3, 5120) == 0
    assert lib_w4.load().vly_w4_gemv_rmsnorm_supported(2, 5120) == 1
    assert lib_w4.load().vly_w4_gemv_rmsnorm_supported(3, 5120) == 0
    assert lib_w4.load().vly_w4_gemv_rmsnorm_supported(1, 4160) == 0     # K % 128


def test_main_libraries_export_exactly_valley_hip_h(built):
    """The shipped libraries still export exactly valley_hip.h's default section (52 names, ABI 8), the experimental ones more."""
    from tests.test_abi_cpu import header_symbols as main_symbols
    from valley_amd import lib
    names = main_symbols()
    assert len(names) == 52 and lib.ABI_VERSION == 8
    assert exported(build.LIB) == names == exported(build.LIB_F16)
    assert set(names) <= set(exported(build.LIB_EXP)) and set(names) <= set(exported(build.LIB_EXP_F16))


def test_no_library_carries_another_companions_names(built):
    """Every ordered pair (library, other companion) of the 4 main variants and the 7 companions."""
    mains = {"main": build.LIB, "main_f16": build.LIB_F16, "exp": build.LIB_EXP, "exp_f16": build.LIB_EXP_F16}
    libs = {**mains, **{c.name: c.lib for c in build.COMPANIONS}}
    symbols = {k: exported(p) for k, p in libs.items()}
    pairs = 0
    for holder, got in symbols.items():
        own = set(header_symbols(f"valley_hip_{holder}.h")) if holder in NAMES else set()
        for c in build.COMPANIONS:
            if c.name == holder:
                continue
            pairs += 1
            # (vly_spec_counters and vly_spec_sample_* begin with the spec library's prefix, and are spec_sample's by its header)
            assert not [n for n in got if n.startswith(f"vly_{c.name}_") and n not in own], (holder, c.name)
            assert not set(got) & set(header_symbols(c.header)), (holder, c.name)
    assert pairs == 4 * 7 + 7 * 6
    for holder in mains:
        assert not [n for n in symbols[holder] if "beam" in n or "logits_" in n], holder


@pytest.mark.parametrize("name", NAMES)
def test_missing_library_fails_loudly(monkeypatch, tmp_path, name):
    from valley_amd import lib
    mod = binding(name)
    mod.reset()
    monkeypatch.setenv(f"VALLEY_HIP_{name.upper()}_LIB", str(tmp_path / "nope.so"))
    with pytest.raises(lib.ValleyHipError, match=re.escape(EXPECT[name][2])) as e:
        mod.load()
    assert str(e.value) == (f"{tmp_path / 'nope.so'} not found: build it with `python -m valley_amd.build` (hipcc --offload-arch=gfx950). "
                            f"{EXPECT[name][2]}")
    assert not mod.loaded()


def stub_library(tmp_path, stem, functions):
    """A host-only shared object that defines ``functions`` ({name: the int it returns}); no device code."""
    src = tmp_path / f"{stem}.cpp"
    src.write_text("".join(f'extern "C" int {n}(void) {{ return {v}; }}\n' for n, v in functions.items()))
    out = tmp_path / f"{stem}.so"
    subprocess.run([build.hipcc(), "-x", "c++", "-shared", "-fPIC", str(src), "-o", str(out)], check=True, capture_output=True)
    return str(out)


def test_incomplete_and_mis_versioned_libraries_fail_loudly(monkeypatch, tmp_path):
    from valley_amd import lib, lib_spec_sample
    from valley_amd.companion import Companion

    def fresh():
        return Companion("spec_sample", lib_spec_sample.SIGS, lib_spec_sample.ABI_VERSION, build.LIB_SPEC_SAMPLE, "(stub)",
                         label="spec-sample")

    short = stub_library(tmp_path, "short", {"vly_spec_sample_abi_version": 1, "vly_spec_sample_last_error": 0})
    monkeypatch.setenv("VALLEY_HIP_SPEC_SAMPLE_LIB", short)
    c = fresh()
    with pytest.raises(lib.ValleyHipError) as e:
        c.load()
    assert str(e.value) == f"{short} does not export vly_spec_counters" and not c.loaded()
    stale = stub_library(tmp_path, "stale", {"vly_spec_sample_abi_version": 2, "vly_spec_sample_last_error": 0, "vly_spec_counters": 0})
    monkeypatch.setenv("VALLEY_HIP_SPEC_SAMPLE_LIB", stale)
    c = fresh()
    with pytest.raises(lib.ValleyHipError) as e:
        c.load()
    assert str(e.value) == "spec-sample ABI mismatch: library 2 vs binding 1" and not c.loaded()
    # the other labels are the companions' names
    assert all(binding(n).COMPANION.label == n for n in NAMES if n != "spec_sample") and lib_spec_sample.COMPANION.label == "spec-sample"


def test_a_companion_loads_once(built):
    from valley_amd import lib
    for name in NAMES:
        mod = binding(name)
        h = mod.load()
        assert mod.load() is h and mod.loaded()
        mod.check(0, "nothing")
        with pytest.raises(lib.ValleyHipError, match=r"probe failed \(rc=-22\): "):
            mod.check(-22, "probe")


def test_importing_the_package_maps_no_companion(built):
    code = ("import valley_amd, valley_amd.ops\n"
            f"names = {NAMES!r}\n"
            "import importlib\n"
            "mods = [importlib.import_module('valley_amd.lib_' + n) for n in names]\n"
            "assert not any(m.loaded() for m in mods), [m.loaded() for m in mods]\n"
            "maps = open('/proc/self/maps').read()\n"
            "assert not any('libvalley_hip_' + n + '.so' in maps for n in names)\n"
            "print('lazy')\n")
    out = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.strip().endswith("lazy"), out.stderr[-2000:]
