"""The int8 GEMM bench and its stamp build run the product kernel (igemm_nt_mod_kernel<256, 4,
Probe>) and compute what it computes: igemm_FULL (IgemmNoProbe) and igemm_STAMPS (IgemmStamps)
at 1024 × 512, the plain product and the product with the epilogue add, every output checked
against the CPU by the bench itself.

At that size there are four row blocks with K loops of 4, 8, 12 and 16 slabs and two column
blocks; the first loop equals the ring's prologue: one FULL step, then the written-out tail.
The kernel's rule: a tile of nsl slabs runs nsl − (NST − 1) FULL steps (NST = 4 ring stages),
and only FULL steps are stamped — 1, 5, 9, 13 per wave, mean 7.

The ablation builds are not run: their outputs are meaningless by design."""
import math
import os
import re
import subprocess

import pytest

from microbench_build import build_target

N, NC, NST = 1024, 512, 4
FULL_STEPS = [256 * (bi + 1) // 64 - (NST - 1) for bi in range(N // 256)]   # [1, 5, 9, 13]


def _run(target, tmp_path):
    """Build into tmp_path, run once as a child under its own time limit; returns its output."""
    exe, built = build_target(target, tmp_path)
    assert built.returncode == 0, built.stderr[-800:]
    env = dict(os.environ, IGEMM_N=str(N), IGEMM_NC=str(NC), IGEMM_ADD="1")
    r = subprocess.run([exe], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (target, r.returncode, r.stdout[-800:], r.stderr[-800:])
    return r.stdout


def _differing(out):
    """{'plain': (bad, checked), 'add': (bad, checked)} from the bench's check lines."""
    found = re.findall(r": (plain|add) product: (\d+) of (\d+) outputs differ", out)
    return {k: (int(b), int(c)) for k, b, c in found}


@pytest.mark.gpu
def test_full_and_stamp_builds_compute_the_products(tmp_path):
    assert FULL_STEPS == [1, 5, 9, 13]
    out = _run("igemm_FULL", tmp_path)   # a failure here ends the test before the next child starts
    print(out)
    assert _differing(out) == {"plain": (0, N * NC), "add": (0, N * NC)}, out

    out = _run("igemm_STAMPS", tmp_path)
    print(out)
    assert _differing(out) == {"plain": (0, N * NC), "add": (0, N * NC)}, out
    for what in ("plain", "add"):
        m = re.search(r"stamps %s: (\d+) waves, stamped steps per wave mean ([\d.]+) min (\d+) max (\d+)" % what, out)
        assert m, out
        assert int(m.group(1)) == (N // 256) * (NC // 256) * 8
        assert float(m.group(2)) == sum(FULL_STEPS) / len(FULL_STEPS) == 7.0
        assert (int(m.group(3)), int(m.group(4))) == (min(FULL_STEPS), max(FULL_STEPS))
        shares = [float(s) for s in re.findall(r"^  %s seg \d .* share (\S+)" % what, out, flags=re.M)]
        assert len(shares) == 6 and all(math.isfinite(s) and 0 <= s <= 1 for s in shares), shares
        assert abs(sum(shares) - 1.0) <= 6 * 0.5e-4 + 1e-9, shares   # six figures printed to four decimals
