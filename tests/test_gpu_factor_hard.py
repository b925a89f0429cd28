"""The FP64 factor chain (gp2d_potrf, gp2d_trtri, gp2d_potrf_inv, the batched pair, gp2d_potrs_inv,
gp2d_dfact_panel) through the raw ABI at real conditioning and at failure.

Accuracy: on Gram matrices of condition 2e3 … 5e10, a graded matrix of 1e16 and the benign matrix of
the older tests (tests/factor_ref.py), the factor's scaled residual ρ, the inverse's componentwise
forward error φ against the longdouble inverse of the very L it was given, and the solve against its
derived per-component bound.  The yardstick is a float64 numpy emulation of the project's own
algorithm (blocked inverse-panel Cholesky, recursive-doubling inverse) and LAPACK; a kernel may be
4× worse than the worse of them — three summation orders differ by at most 1.2× on the benign rows,
a pivot short of a dozen bits or a dropped k slab moves ρ by orders of magnitude.

Failure: `info` is LAPACK's — the 1-based order of the first pivot that is not > 0 — at panel edges,
block edges, the first and the last row, for NaN inputs, per problem of a batch, as a global order in
the distributed panel step and in the error that engine.fit raises; and a failed call leaves nothing
behind that changes the next one.  The references are proven in tests/test_factor_ref_cpu.py.

With GP2D_FACTOR_HARD_OUT set to a path, the measured figures are written there as JSON
(profiles/factor_hard.json is one such run)."""
import ctypes
import functools
import hashlib
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import scipy.linalg.lapack as lapack

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
if not torch.cuda.is_available():  # pragma: no cover
    pytest.skip("no HIP device", allow_module_level=True)

import factor_ref as F  # noqa: E402
from gp2d import _native as N  # noqa: E402
from gp2d import engine as E  # noqa: E402

if not F.have_longdouble():  # pragma: no cover
    pytest.skip("np.longdouble is no wider than float64 on this host", allow_module_level=True)

L_ = N.lib()
DEV = torch.device("cuda")
NB = F.NB
MARGIN = 4.0
MEASURED = {}


def P(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def S():
    return ctypes.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)


def zeros(*shape, dtype=torch.float64):
    return torch.zeros(shape, dtype=dtype, device=DEV)


def workspace(nbytes):
    return zeros(nbytes // 8 + 2)


def note(name, group, **kv):
    MEASURED.setdefault(name, {"n": int(F.matrix(name).shape[0])}).setdefault(group, {}).update(kv)


@pytest.fixture(scope="module", autouse=True)
def _write_measured():
    yield
    out = os.environ.get("GP2D_FACTOR_HARD_OUT")
    if out and MEASURED:
        with open(out, "w") as f:
            json.dump(MEASURED, f, indent=1, sort_keys=True)


def factor(K, entry="potrf"):
    """gp2d_potrf (A ← L) or gp2d_potrf_inv (A ← W) on the full symmetric K.  Returns (A, dinv, info);
    info starts as 7: the call resets it."""
    n = K.shape[0]
    A = torch.tensor(np.array(K, dtype=np.float64), device=DEV)
    dinv, info = zeros(n // NB, NB, NB), torch.full((1,), 7, dtype=torch.int32, device=DEV)
    if entry == "potrf":
        N.check(L_.gp2d_potrf(P(A), n, n, P(dinv), P(info), None, 0, S()), "gp2d_potrf")
    else:
        wb = int(L_.gp2d_potrf_inv_workspace(n))
        N.check(L_.gp2d_potrf_inv(P(A), n, n, P(dinv), P(info), P(workspace(wb)), wb, S()), "gp2d_potrf_inv")
    torch.cuda.synchronize()
    return A, dinv, int(info.item())


def trtri(Lt, dinv):
    """gp2d_trtri on a copy of the device L, with the factor's diagonal inverses or without."""
    n = Lt.shape[0]
    A = Lt.clone()
    wb = int(L_.gp2d_trtri_workspace(n))
    N.check(L_.gp2d_trtri(P(A), n, n, P(dinv), P(workspace(wb)), wb, S()), "gp2d_trtri")
    torch.cuda.synchronize()
    return A


# Everything below is computed once per matrix and left unchanged.
@functools.lru_cache(maxsize=None)
def hip_factor(name):
    """(L on the device, dinv) of the named matrix from gp2d_potrf, info asserted zero."""
    A, dinv, info = factor(F.matrix(name))
    assert info == 0, (name, info)
    return A, dinv


@functools.lru_cache(maxsize=None)
def hip_inverse(name, with_dinv=True):
    Lt, dinv = hip_factor(name)
    return trtri(Lt, dinv if with_dinv else None)


@functools.lru_cache(maxsize=None)
def host_rho(name):
    """(ρ of the yardstick, ρ of LAPACK) on the named matrix."""
    K = F.matrix(name)
    Lb, ib = F.blocked_chol(K)
    Ll, il = lapack.dpotrf(K, lower=1, clean=1)
    assert (ib, il) == (0, 0)
    return F.rho(K, Lb), F.rho(K, Ll)


@functools.lru_cache(maxsize=None)
def inverse_ref(name):
    """The longdouble inverse of the HIP L of the named matrix, with the yardstick's and dtrtri's φ."""
    Lh = hip_factor(name)[0].cpu().numpy()
    ref = F.InverseRef(Lh)
    Wt, info = lapack.dtrtri(Lh, lower=1)
    assert info == 0
    return ref, ref.phi(F.blocked_inv(Lh)), ref.phi(Wt)


def bits(t):
    return hashlib.sha256(np.ascontiguousarray(t.cpu().numpy()).tobytes()).hexdigest()


# ---------------------------------------------------------------------- a. factor backward error
def check_factor(name, Lh, info, what):
    K = F.matrix(name)
    n = K.shape[0]
    assert info == 0, (what, info)
    assert np.array_equal(np.triu(Lh, 1), np.zeros_like(Lh)), f"{what}: the strict upper triangle is not zero"
    assert np.all(np.isfinite(Lh))
    ry, rl = host_rho(name)
    rh = F.rho(K, Lh)
    nu = n * F.U
    msg = f"{what}: rho/(n u) hip {rh / nu:.3f}, yardstick {ry / nu:.3f}, LAPACK {rl / nu:.3f}"
    print(msg)
    assert rh <= MARGIN * max(ry, rl), msg
    return rh / nu, ry / nu, rl / nu


@pytest.mark.parametrize("name", F.NAMES)
def test_factor_backward_error(name):
    Lt, _ = hip_factor(name)
    rh, ry, rl = check_factor(name, Lt.cpu().numpy(), 0, name)
    note(name, "rho_over_nu", hip=rh, yardstick=ry, lapack=rl)


# ------------------------------------------------------------------------------ b. every schedule
_SCHED_CHILD = r'''
import ctypes, hashlib, json, sys
import numpy as np, torch
sys.path[:0] = sys.argv[1:4]
import factor_ref as F
from gp2d import _native as N
L_ = N.lib()
K = np.array(F.matrix("G4"))
n = K.shape[0]
A = torch.tensor(K, device="cuda")
dinv = torch.empty((n // 128, 128, 128), dtype=torch.float64, device="cuda")
info = torch.full((1,), 7, dtype=torch.int32, device="cuda")
s = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
P = lambda t: ctypes.c_void_p(t.data_ptr())
N.check(L_.gp2d_potrf(P(A), n, n, P(dinv), P(info), None, 0, s), "potrf")
Lg = A.cpu().numpy()
print(json.dumps(dict(info=int(info.item()), upper=float(np.abs(np.triu(Lg, 1)).max()),
                      finite=bool(np.isfinite(Lg).all()), rho=F.rho(K, Lg),
                      sha=hashlib.sha256(Lg.tobytes()).hexdigest())))
'''


@functools.lru_cache(maxsize=None)
def schedule_run(G, split):
    from conftest import PKG, ROOT
    env = dict(os.environ, GP2D_POTRF_G=str(G), GP2D_POTRF_SPLIT=str(split))
    out = subprocess.run([sys.executable, "-c", _SCHED_CHILD, os.path.join(ROOT, "tests"), ROOT, PKG], env=env,
                         capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-2000:]
    return json.loads(out.stdout.strip().splitlines()[-1])


@pytest.mark.parametrize("G,split", [(2, 0), (4, 0), (4, 1)])
def test_factor_backward_error_every_schedule(G, split):
    """G4 (five blocks: a ragged four-panel group) under each trailing-update schedule of potrf_impl,
    in a fresh process each (the schedule is read once per process)."""
    r = schedule_run(G, split)
    n = F.matrix("G4").shape[0]
    ry, rl = host_rho("G4")
    msg = f"G={G} split={split}: rho/(n u) hip {r['rho'] / (n * F.U):.3f}, yardstick {ry / (n * F.U):.3f}"
    print(msg)
    assert r["info"] == 0 and r["upper"] == 0.0 and r["finite"], r
    assert r["rho"] <= MARGIN * max(ry, rl), msg
    note("G4", "rho_over_nu", **{f"hip_G{G}_split{split}": r["rho"] / (n * F.U)})


def test_split_changes_no_bit_on_hard_data():
    assert schedule_run(4, 0)["sha"] == schedule_run(4, 1)["sha"]


# ----------------------------------------------------------------------- c. inverse forward error
@pytest.mark.parametrize("with_dinv", [True, False])
@pytest.mark.parametrize("name", ["G2", "G3", "G4", "GR"])
def test_inverse_forward_error(name, with_dinv):
    W = hip_inverse(name, with_dinv).cpu().numpy()
    assert np.array_equal(np.triu(W, 1), np.zeros_like(W)) and np.all(np.isfinite(W))
    ref, py, pt = inverse_ref(name)
    ph = ref.phi(W)
    msg = f"{name} dinv={with_dinv}: phi hip {ph:.3e}, yardstick {py:.3e}, dtrtri {pt:.3e}"
    print(msg)
    note(name, "phi", yardstick=py, dtrtri=pt, **{"hip_dinv" if with_dinv else "hip_nodinv": ph})
    assert ph <= MARGIN * py, msg


# ------------------------------------------------------------------------------------- d. solve
@pytest.mark.parametrize("name", ["G3", "G4"])
def test_solve_within_its_bound(name):
    Wt = hip_inverse(name)
    n = Wt.shape[0]
    y = np.random.default_rng(5).normal(size=n)
    yt, alpha = torch.tensor(y, device=DEV), zeros(n)
    pb = int(L_.gp2d_potrs_workspace(n))
    N.check(L_.gp2d_potrs_inv(P(Wt), n, n, P(yt), P(alpha), P(workspace(pb)), pb, S()), "gp2d_potrs_inv")
    torch.cuda.synchronize()
    want, b = F.solve_ref(Wt.cpu().numpy(), y)
    ratio = np.abs(alpha.cpu().numpy().astype(F.LD) - want) / b
    worst = float(np.max(ratio))
    print(f"{name}: max |d alpha|_i / b_i = {worst:.3e}")
    note(name, "solve", max_err_over_bound=worst)
    assert np.all(ratio <= 1), (int(np.argmax(ratio)), worst)


# ------------------------------------------------------------------ e. paths agree on hard data
def test_paths_agree_on_hard_data():
    """gp2d_potrf + gp2d_trtri, gp2d_potrf_inv and the batched pair (nprob = 3 on [G3, GR, P]) give
    one set of bits for W and dinv at cond 6e9 and 1e16."""
    names = ["G3", "GR", "P"]
    n, B = 384, 3
    buf = torch.stack([torch.tensor(np.array(F.matrix(k)), device=DEV) for k in names]).contiguous()
    dinv, info = zeros(B, n // NB, NB, NB), torch.full((B,), 7, dtype=torch.int32, device=DEV)
    N.check(L_.gp2d_potrf_batched(P(buf), n, n, n * n, B, P(dinv), P(info), S()), "gp2d_potrf_batched")
    Lb = buf.clone()
    wb = int(L_.gp2d_trtri_batched_workspace(n, B))
    N.check(L_.gp2d_trtri_batched(P(buf), n, n, n * n, B, P(dinv), P(workspace(wb)), wb, S()), "gp2d_trtri_batched")
    torch.cuda.synchronize()
    assert info.tolist() == [0] * B
    for b, name in enumerate(names):
        Lt, d1 = hip_factor(name)
        W1 = hip_inverse(name)
        W2, d2, i2 = factor(F.matrix(name), "potrf_inv")
        assert i2 == 0
        assert torch.equal(Lb[b], Lt), name
        assert torch.equal(W1, W2) and torch.equal(d1, d2), name
        assert torch.equal(buf[b], W1) and torch.equal(dinv[b], d1), name
        assert bool(torch.isfinite(W1).all())


# ------------------------------------------------------------------------- f. info is LAPACK's
@functools.lru_cache(maxsize=None)
def healthy_bits():
    """The bits of a fresh run of each entry on P."""
    out = {}
    for entry in ("potrf", "potrf_inv"):
        A, dinv, info = factor(F.matrix("P"), entry)
        assert info == 0
        out[entry] = (bits(A), bits(dinv))
    return out


def check_info(K, want):
    """Both entries report `want` on K; a healthy call after each returns info 0 and a fresh run's bits."""
    for entry in ("potrf", "potrf_inv"):
        _, _, info = factor(K, entry)
        assert info == want, (entry, info, want)
        A, dinv, info = factor(F.matrix("P"), entry)
        assert info == 0 and (bits(A), bits(dinv)) == healthy_bits()[entry], entry


@pytest.mark.parametrize("j", [0, 31, 32, 63, 64, 127, 128, 129, 255, 256, 383])
def test_info_of_a_planted_pivot(j):
    check_info(F.plant(F.matrix("P"), j), j + 1)


def test_info_of_two_plants_is_the_first():
    check_info(F.plant(F.matrix("P"), 140, 300), 141)
    check_info(F.plant(F.matrix("P"), 31, 32), 32)


# the diagonal; below it in one 32-panel, in one block, across a block edge, in different blocks
@pytest.mark.parametrize("i,j", [(0, 0), (200, 200), (383, 383), (45, 40), (100, 3), (128, 127), (300, 10),
                                 (383, 129)])
def test_info_of_a_nan(i, j):
    """netlib's pivot test `not (d > 0)` fails a NaN: one at K[j, j] fails pivot j, one at K[i, j],
    i > j, of the lower triangle reaches row i of L only and fails pivot i.  (The installed LAPACK
    lets NaN through and returns 0, so the reference is factor_ref.chol_ld.)"""
    K = np.array(F.matrix("P"))
    K[i, j] = np.nan
    assert F.chol_ld(K)[1] == i + 1
    check_info(K, i + 1)


def test_info_batched_is_each_problems_own():
    n, B = 384, 4
    plants = [5, 130, None, 383]
    mats = [F.matrix("P") if j is None else F.plant(F.matrix("P"), j) for j in plants]
    buf = torch.stack([torch.tensor(np.array(m), device=DEV) for m in mats]).contiguous()
    dinv, info = zeros(B, n // NB, NB, NB), torch.full((B,), 7, dtype=torch.int32, device=DEV)
    N.check(L_.gp2d_potrf_batched(P(buf), n, n, n * n, B, P(dinv), P(info), S()), "gp2d_potrf_batched")
    torch.cuda.synchronize()
    assert info.tolist() == [6, 131, 0, 384]
    assert (bits(buf[2]), bits(dinv[2])) == healthy_bits()["potrf"]


@pytest.mark.parametrize("j", [5, 511, 512, 700])
def test_info_dfact_panel_is_a_global_order(j):
    """gp2d_dfact_panel at n = 1024 (two super-columns of 512) on one rank, the step sequence of
    test_gpu_strides.test_dfact_one_rank: a pivot planted in either super-column is reported as its
    order in the whole matrix, and the first failure is kept."""
    n = 1024
    SB = int(L_.gp2d_dfact_sb())
    assert SB == 512
    nsb = n // SB
    A = torch.tensor(F.plant(F.spd(n, n), j), device=DEV)
    wb, pd = int(L_.gp2d_dfact_workspace(n)), int(L_.gp2d_dfact_panel_doubles(n))
    panels = [zeros(pd) for _ in range(2)]
    info, work = torch.zeros(1, dtype=torch.int32, device=DEV), workspace(wb)
    seen = []

    def step(s):
        N.check(L_.gp2d_dfact_panel(P(A), n, n, s, P(panels[s % 2]), P(info), P(work), wb, S()), "gp2d_dfact_panel")
        torch.cuda.synchronize()
        seen.append(int(info.item()))
    step(0)
    for s in range(nsb):
        N.check(L_.gp2d_dfact_update(P(A), n, n, s, P(panels[s % 2]), 1, 0, s + 1, nsb, S()), "gp2d_dfact_update")
        if s + 1 < nsb:
            step(s + 1)
        N.check(L_.gp2d_dfact_invstep(P(A), n, n, s, P(panels[s % 2]), 1, 0, P(work), wb, S()), "gp2d_dfact_invstep")
    torch.cuda.synchronize()
    assert seen == ([j + 1, j + 1] if j < SB else [0, j + 1]), seen
    assert int(info.item()) == j + 1


def test_fit_error_carries_the_order_of_potrf():
    """engine.fit on 64 points (2·64 rows, one block) with a negative noise: the LinAlgError's
    message carries the order that gp2d_potrf reports on the same padded matrix — 12, the
    extended-precision order too (pivots 1–11 ≥ 0.02, pivot 12 = −0.037: no rounding decides)."""
    x = np.random.default_rng(11).uniform(0, 20, (64, 2))
    ks, noise = E.KernelSpec(kind="df", l_df=3.0), -0.02
    npad = E.padded_points(64)
    n = 2 * npad
    assert n == 128
    X = torch.tensor(x, device=DEV)
    desc = ks.desc()
    K = zeros(n, n)
    N.check(L_.gp2d_assemble(P(X), 64, npad, P(X), 64, npad, ctypes.byref(desc), noise, 1, P(K), n, S()),
            "gp2d_assemble")
    torch.cuda.synchronize()
    Kh = K.cpu().numpy()
    want = F.chol_ld(Kh)[1]
    assert want == 12
    assert factor(Kh)[2] == want and factor(Kh, "potrf_inv")[2] == want
    with pytest.raises(np.linalg.LinAlgError) as ei:
        E.fit(ks, x, np.zeros(128), noise=noise)
    m = re.search(r"leading minor of order (\d+)", str(ei.value))
    assert m and int(m.group(1)) == want, str(ei.value)
