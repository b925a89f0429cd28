"""Build a tools/microbench target outside the tree: the Makefile's own command (make -n), with
the output moved into a directory of the caller's."""
import os
import subprocess

from conftest import ROOT

MICROBENCH = os.path.join(ROOT, "tools", "microbench")


def makefile_targets():
    """The int8 GEMM bench's targets (the Makefile's IG list) plus the two other users of the kernel."""
    for line in open(os.path.join(MICROBENCH, "Makefile")):
        if line.startswith("IG = "):
            return line.split()[2:] + ["coresid", "igemm_zbatch"]
    raise AssertionError("tools/microbench/Makefile has no IG list")


def build_target(target, outdir):
    """Compile `target` for gfx950 into outdir; returns (path, CompletedProcess)."""
    dry = subprocess.run(["make", "-n", "-B", target], cwd=MICROBENCH, capture_output=True, text=True, check=True)
    cmds = [c for c in dry.stdout.splitlines() if c.strip()]
    assert len(cmds) == 1 and cmds[0].endswith(" -o " + target), cmds
    out = os.path.join(str(outdir), target)
    cmd = cmds[0][:-len(target)] + out
    return out, subprocess.run(cmd, shell=True, cwd=MICROBENCH, capture_output=True, text=True)
