"""The int8 GEMM's measuring builds instantiate the product kernel (igemm_nt_mod_kernel<TBN, NST,
Probe>, csrc/ozaki.hpp) with a probe policy of tools/microbench/igemm_probes.hpp: no copy of the
kernel is left under tools/microbench, every target still compiles for gfx950, and the tool that
gates "the library's kernels did not change" (tools/asm_equal.py) tells equal from different."""
import json
import os
import re
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

from conftest import ROOT
from microbench_build import MICROBENCH, build_target, makefile_targets


def test_every_igemm_target_compiles_for_gfx950(tmp_path):
    targets = makefile_targets()
    assert set(targets) >= {"igemm_FULL", "igemm_FULL5", "igemm_N128", "igemm_NO_DMA", "igemm_NO_MFMA",
                            "igemm_NO_LDSREAD", "igemm_EPI_ONLY", "igemm_NO_DMA_NO_BAR", "igemm_MFMA_ONLY",
                            "igemm_STAMPS", "coresid", "igemm_zbatch"}
    before = sorted(os.listdir(MICROBENCH))
    with ThreadPoolExecutor(max_workers=4) as pool:
        done = list(pool.map(lambda t: build_target(t, tmp_path), targets))
    failed = {t: r.stderr[-800:] for t, (out, r) in zip(targets, done) if r.returncode != 0 or not os.path.exists(out)}
    assert not failed, failed
    assert sorted(os.listdir(MICROBENCH)) == before   # into the temporary directory, not into the tree


def test_no_copy_of_the_kernel_under_microbench():
    assert not os.path.exists(os.path.join(MICROBENCH, "igemm_ablate.hpp"))
    assert not os.path.exists(os.path.join(MICROBENCH, "igemm_stamps.hpp"))
    for name in sorted(os.listdir(MICROBENCH)):
        path = os.path.join(MICROBENCH, name)
        if not name.endswith((".hip", ".hpp", ".h", ".cpp")):
            continue
        text = open(path, encoding="utf-8").read()
        kernels = re.findall(r"__global__\b[^;{]*?\bvoid\s+(\w+)\s*\(", text, flags=re.S)
        assert not [k for k in kernels if k.startswith("igemm_")], (name, kernels)
    # the regex sees the product kernel where it is defined
    oz = open(os.path.join(ROOT, "2d-gp_amd", "csrc", "ozaki.hpp"), encoding="utf-8").read()
    assert "igemm_nt_mod_kernel" in re.findall(r"__global__\b[^;{]*?\bvoid\s+(\w+)\s*\(", oz, flags=re.S)


_ASM = """\t.text
\t.protected\t{name}
\t.type\t{name},@function
{name}:                                 ; @{name}
; %bb.0:
\ts_mov_b32 s0, 0
.LBB{idx}_1:
\t{insn}
\ts_cbranch_scc1 .LBB{idx}_1
\ts_endpgm
.Lfunc_end{idx}:
\t.size\t{name}, .Lfunc_end{idx}-{name}
\t.amdhsa_kernel {name}
\t\t.amdhsa_group_segment_fixed_size {lds}
\t\t.amdhsa_next_free_vgpr 254
\t.end_amdhsa_kernel
"""
_OLD = "_ZN4gp2d19igemm_nt_mod_kernelILi256ELi4EEEvPKaS2_PhliiNS_9IgemmProdEPKiS6_NS_6IgemmZE"
_NEW = "_ZN4gp2d19igemm_nt_mod_kernelILi256ELi4ENS_12IgemmNoProbeEEEvPKaS3_PhliiNS_9IgemmProdEPKiS7_NS_6IgemmZE"


def _asm_equal(tmp_path, old, new):
    a, b, out = tmp_path / "old.s", tmp_path / "new.s", tmp_path / "verdict.json"
    a.write_text(old)
    b.write_text(new)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "asm_equal.py"), str(a), str(b), "-o", str(out)],
                       capture_output=True, text=True)
    return r.returncode, json.loads(out.read_text())


def test_asm_equal_tells_equal_from_different(tmp_path):
    other = _ASM.format(name="_ZN4gp2d5otherEv", idx=0, insn="v_add_u32_e32 v0, v0, v1", lds=0)
    old = other + _ASM.format(name=_OLD, idx=1, insn="v_mfma_i32_16x16x64_i8 v[0:3], v[4:7], v[8:11], v[0:3]", lds=131072)
    # the renamed kernel, a shifted block-label number: equal
    same = _ASM.format(name=_NEW, idx=5, insn="v_mfma_i32_16x16x64_i8 v[0:3], v[4:7], v[8:11], v[0:3]", lds=131072) + other
    rc, doc = _asm_equal(tmp_path, old, same)
    assert rc == 0 and doc["kernels"] == 2 and doc["equal"] == 2 and doc["all_equal"]
    # one operand of one instruction differs
    rc, doc = _asm_equal(tmp_path, old, same.replace("v[4:7], v[8:11]", "v[4:7], v[12:15]"))
    assert rc == 1 and doc["equal"] == 1 and not doc["all_equal"]
    assert [r["verdict"] for r in doc["per_kernel"] if "igemm" in r["kernel"]] == ["DIFFERENT"]
    # a resource directive differs
    rc, doc = _asm_equal(tmp_path, old, same.replace("fixed_size 131072", "fixed_size 65536"))
    assert rc == 1 and doc["equal"] == 1
    # a kernel is missing
    rc, doc = _asm_equal(tmp_path, old, other)
    assert rc == 1 and not doc["all_equal"]
