"""The leave-one-out objective, host side: the numpy reference's closed forms against brute-force
refits and central differences of the brute force, the C ABI's export, workspace query and argument
checks (no HIP device), and hyper's objective= argument handling.

Gates.  Closed form against refit: 1e-10 relative, tests/test_cv_cpu.py's gate for the same two
routes.  Analytic gradient against a central difference (step 1e-5 relative) of the brute force:
tests/test_gpu_lml.py's gates for finite-difference references — per entry |fd − g| ≤ 1e-5·|g| +
1e-6·|value| (test_lml_grad_full_size_fd) and 1e-6 in the `rel` norm (largest deviation over
largest entry), the latter on the whole vector and on the kernel-parameter sub-vector without the
noise entry, which is 10³ to 10⁵ times the others.
"""
import ctypes
import os
import re

import numpy as np
import pytest

import cv_ref as C
import loo_ref as R
import sum_ref as S
from conftest import ROOT

GATE = 1e-10
N_FD = 60


@pytest.fixture(autouse=True, scope="module")
def loo_entry():
    """Everything here pins gp2d_loo_grad's reference, its C entry or the objective switch built on
    it: a library without the entry fails the whole module."""
    from gp2d import _native as N
    assert "gp2d_loo_grad" in N.EXPORTS and hasattr(N.lib(), "gp2d_loo_grad")


# ---------------------------------------------------------------- parameter vectors of the cases
def pack(terms, weights, noise):
    th = []
    for t, w in zip(terms, weights):
        th += [w, t["l_df"], t["l_cf"], t["ratio"]] + ([t["var_t"], t["l_t"]] if S.is_st(t) else [])
    return np.array(th + [noise])


def unpack(th, terms):
    out, ws, i = [], [], 0
    for t in terms:
        new = dict(t, l_df=th[i + 1], l_cf=th[i + 2], ratio=th[i + 3])
        ws.append(th[i])
        i += 4
        if S.is_st(t):
            new.update(var_t=th[i], l_t=th[i + 1])
            i += 2
        out.append(new)
    return out, ws, th[i]


def used_mask(terms):
    """Which entries of pack() the kernels depend on (a df kind ignores l_cf and ratio, …)."""
    m = []
    for t in terms:
        k = t["kind"]
        m += [True, k in ("df", "mixed"), k in ("cf", "mixed"), k == "mixed"] + ([True, True] if S.is_st(t) else [])
    return np.array(m + [True])


def central_difference(f, th, used):
    g = np.zeros(th.size)
    for i in np.flatnonzero(used):
        h = 1e-5 * abs(th[i])
        up, dn = th.copy(), th.copy()
        up[i] += h
        dn[i] -= h
        g[i] = (f(up) - f(dn)) / (2 * h)
    return g


def gate_fd(what, val, g, fd):
    kernel = slice(0, g.size - 1)
    e = dict(whole=R.rel(g, fd), kernel=R.rel(g[kernel], fd[kernel]),
             entry=float(np.max(np.abs(fd - g) - 1e-5 * np.abs(g))), entry_gate=1e-6 * abs(val))
    print(f"{what}: analytic vs central difference {e}")
    assert np.all(np.abs(fd - g) <= 1e-5 * np.abs(g) + 1e-6 * abs(val)), (what, g, fd)
    assert e["whole"] < 1e-6 and e["kernel"] < 1e-6, (what, e)


VECTOR_CASES = {
    "df": ([R.term("df")], [1.0], 2),
    "cf": ([R.term("cf")], [1.0], 2),
    "mixed": ([R.term("mixed")], [1.0], 2),
    "st": ([R.term("mixed", st=True)], [1.0], 3),
    "sum": (R.SUM_TERMS, R.SUM_WEIGHTS, 2),
}


@pytest.mark.parametrize("name", sorted(VECTOR_CASES))
def test_vector_closed_form_equals_refits_and_differences(name):
    terms, weights, dim = VECTOR_CASES[name]
    x, y = R.data(N_FD, dim=dim)
    val, g = R.loo_value_grad(terms, weights, x, y, C.NOISE)
    brute = R.loo_refit_sum(terms, weights, x, y, C.NOISE)
    print(f"{name}: closed form {val!r} vs refits {brute!r}")
    assert abs(val - brute) < GATE * max(1.0, abs(brute))
    used = used_mask(terms)
    assert np.all(g[~used] == 0.0)

    def f(th):
        t, w, nz = unpack(th, terms)
        return R.loo_refit_sum(t, w, x, y, nz)

    gate_fd(name, val, g, central_difference(f, pack(terms, weights, C.NOISE), used))
    if len(terms) == 1:   # the library's order for a kernel that is not a sum: no weight entry
        v1, g1 = R.loo_value_grad_single(terms[0], x, y, C.NOISE)
        assert v1 == val and np.array_equal(g1, g[1:])


def test_ard_closed_form_equals_refits_and_differences():
    x, y = R.data(N_FD, bd=1)
    var, ls = C.ARD_VARIANCES, C.ARD_LENGTHSCALES
    val, g = R.ard_value_grad(x, y, var, ls, C.NOISE)
    brute = R.ard_refit(x, y, var, ls, C.NOISE)
    print(f"ard: closed form {val!r} vs refits {brute!r}")
    assert abs(val - brute) < GATE * max(1.0, abs(brute))
    th0 = np.array([var[0], *ls[0], var[1], *ls[1], C.NOISE])

    def f(th):
        return R.ard_refit(x, y, (th[0], th[3]), (tuple(th[1:3]), tuple(th[4:6])), th[6])

    gate_fd("ard", val, g, central_difference(f, th0, np.ones(th0.size, bool)))


@pytest.mark.parametrize("n", [130])
def test_closed_form_equals_refits_larger(n):
    x, y = R.data(n)
    terms, weights = VECTOR_CASES["mixed"][:2]
    val, _ = R.loo_value_grad(terms, weights, x, y, C.NOISE)
    brute = R.loo_refit_sum(terms, weights, x, y, C.NOISE)
    assert abs(val - brute) < GATE * max(1.0, abs(brute))
    # the objective is summary[0] of the cross-validation reference
    assert val == pytest.approx(C.cv_points("vector2d", n)["mean_lpd"] * n, rel=1e-12)
    # the value-only closed form an optimiser calls, both block sizes
    assert R.value_from_K(S.ky(terms, weights, x, C.NOISE), y, 2) == pytest.approx(val, rel=1e-12)
    xa, ya = R.data(n, bd=1)
    K = R.ard_ky(xa, C.ARD_VARIANCES, C.ARD_LENGTHSCALES, C.NOISE)
    ref = R.ard_value_grad(xa, ya, C.ARD_VARIANCES, C.ARD_LENGTHSCALES, C.NOISE)[0]
    assert R.value_from_K(K, ya, 1) == pytest.approx(ref, rel=1e-12)


# ---------------------------------------------------------------- the C entry on the host
def header_prototype(name):
    txt = open(os.path.join(ROOT, "include", "gp2d.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    m = re.search(rf"\b{name}\s*\(([^)]*)\)", txt)
    assert m, name
    return [p.split()[-1].lstrip("*") for p in m.group(1).split(",")]


def test_loo_symbols_and_prototype():
    from gp2d import _native as N
    L = N.lib()
    for s in ("gp2d_loo_grad_workspace", "gp2d_loo_grad"):
        assert s in N.EXPORTS and hasattr(L, s), s
    assert L.gp2d_abi_version() == 11
    params = header_prototype("gp2d_loo_grad")
    assert params == ["W", "n", "wld", "alpha", "y", "xtr", "ntr", "ntr_pad", "k", "value_dev", "grad_dev",
                      "info_dev", "work", "work_bytes", "stream"]
    assert "wld" in params and "ldw" not in params
    assert len(params) == len(N._SIGS["gp2d_loo_grad"][1])
    from gp2d import engine as E
    from gp2d import hyper as H
    from gp2d.krig import Krig
    assert callable(E.loo_device) and callable(E.loo_log_likelihood) and callable(Krig.loo_log_likelihood)
    assert H.OBJECTIVES == ("lml", "loo")


def test_loo_workspace_query():
    from gp2d import _native as N
    L = N.lib()
    assert L.gp2d_loo_grad_workspace(0) == 0 and L.gp2d_loo_grad_workspace(-128) == 0
    assert L.gp2d_loo_grad_workspace(192) == 0            # not a multiple of the GEMM tile
    for n in (128, 384, 8192):
        wb = L.gp2d_loo_grad_workspace(n)
        # P and B, r, s, three c arrays, the triangular products' and the pair loop's workspaces
        assert wb >= 8 * (2 * n * n + 5 * n) + L.gp2d_potrs_workspace(n)
        assert wb <= 8 * (2 * n * n) + L.gp2d_lml_grad_workspace(n) - 8 * n * n + L.gp2d_potrs_workspace(n) + 8 * 5 * n
        assert wb % 8 == 0


def test_loo_argument_errors_are_reported():
    from gp2d import _native as N
    L = N.lib()
    p16, p8 = ctypes.c_void_p(16), ctypes.c_void_p(8)   # never dereferenced: the checks fail first
    big = 1 << 40
    mixed = N.vector_kernel_desc(N.KIND_MIXED, 5.0, 4.0, 0.5)
    ard = N.ard_kernel_desc([0.8, 0.2], [[5.0, 7.0], [12.0, 9.0]])

    def call(n=256, wld=256, ntr=100, ntr_pad=128, k=mixed, W=p16, alpha=p16, y=p16, xtr=p16, value=p16,
             grad=p16, info=p16, work=p16, wb=big):
        return L.gp2d_loo_grad(W, n, wld, alpha, y, xtr, ntr, ntr_pad, ctypes.byref(k) if k is not None else None,
                               value, grad, info, work, wb, None)

    def err():
        return L.gp2d_last_error()

    assert call(wld=255) < 0 and b"wld" in err()
    assert call(wld=254) < 0 and b"wld" in err()
    assert call(wld=257) < 0 and b"wld" in err() and b"even" in err()
    assert call(W=p8) < 0 and b"16-byte aligned" in err() and b"W" in err()
    assert call(wb=L.gp2d_loo_grad_workspace(256) - 1) < 0 and b"workspace" in err()
    assert call(work=None) < 0 and b"workspace" in err()
    assert call(work=p8) < 0 and b"workspace" in err() and b"16-byte" in err()
    for name in ("W", "alpha", "y", "xtr", "value", "info"):
        assert call(**{name: None}) < 0 and b"NULL" in err(), name
    assert call(n=384) < 0 and b"ntr_pad" in err()                      # n ≠ bd·ntr_pad
    assert call(k=ard) < 0 and b"ntr_pad" in err()                      # bd = 1: n = 256 ≠ 128
    assert call(n=192, wld=192, ntr_pad=96) < 0 and b"ntr_pad" in err()  # not whole point tiles
    assert call(n=64, wld=64, ntr=10, ntr_pad=64, k=ard) < 0 and b"multiple of 128" in err()
    assert call(ntr=0) < 0 and b"ntr" in err()
    assert call(ntr=129) < 0 and b"ntr" in err()
    bad = N.vector_kernel_desc(N.KIND_DIVFREE, -1.0)
    assert call(k=bad) < 0 and b"l_df" in err()
    assert call(k=None) < 0
    # the value-only form is a valid call as far as the host can tell: it fails only for want of a device
    rc = call(grad=None, ntr=0)
    assert rc < 0 and b"ntr" in err()


# ---------------------------------------------------------------- hyper's objective= argument
def _problem():
    from gp2d import engine as E
    x, y = R.data(20)
    return E.KernelSpec(kind="df", l_df=5.0), x, y


def test_hyper_refuses_bad_objectives_before_any_device_call():
    from gp2d import hyper as H
    from gp2d import krig
    ks, x, y = _problem()
    for fn in (H.optimize, H.optimize_restarts):
        with pytest.raises(ValueError, match="objective"):
            fn(ks, x, y, 0.01, objective="rmse")
        with pytest.raises(ValueError, match="objective='loo'.*trend='linear'"):
            fn(ks, x, y, 0.01, objective="loo", trend="linear")
        with pytest.raises(ValueError, match="objective"):
            fn(ks, x, y, 0.01, objective="lgo")            # sweep alone scores 'lgo'
    with pytest.raises(ValueError, match="objective"):
        H.Objective(ks, x, y, 0.01, ("l_df",), objective="rmse")
    with pytest.raises(ValueError, match="objective='loo'.*trend='constant'"):
        H.Objective(ks, x, y, 0.01, ("l_df",), objective="loo", trend="constant")
    settings = [dict(l_df=4.0), dict(l_df=6.0)]
    with pytest.raises(ValueError, match="objective"):
        H.sweep(ks, x, y, settings, noise=0.01, objective="rmse")
    with pytest.raises(ValueError, match="objective='loo'.*trend='constant'"):
        H.sweep(ks, x, y, settings, noise=0.01, objective="loo", trend="constant")
    with pytest.raises(ValueError, match="labels"):
        H.sweep(ks, x, y, settings, noise=0.01, objective="lgo")
    with pytest.raises(ValueError, match="gradient"):
        H.sweep(ks, x, y, settings, noise=0.01, objective="lgo", labels=np.arange(20) % 4, eval_gradient=True)
    with pytest.raises(ValueError, match="trend"):
        H.sweep(ks, x, y, settings, noise=0.01, objective="lgo", labels=np.arange(20) % 4, trend="constant")
    with pytest.raises(ValueError, match="labels"):
        H.sweep(ks, x, y, settings, noise=0.01, objective="loo", labels=np.arange(20) % 4)
    k = krig.Krig("df", l_df=3.0, noise=0.05)
    k._X, k._y, k.gp = x, y, object()   # a model that looks fitted: the refusal comes before the device
    for fn in (k.optimize, k.optimize_restarts):
        with pytest.raises(ValueError, match="objective"):
            fn(objective="rmse")


def test_opt_result_fields():
    from gp2d import engine as E
    from gp2d import hyper as H
    r = H.OptResult(E.KernelSpec(kind="df", l_df=5.0), 0.01, -3.5)
    assert (r.objective, r.value, r.lml) == ("lml", -3.5, -3.5)
    r = H.OptResult(E.KernelSpec(kind="df", l_df=5.0), 0.01, -3.5, objective="loo", value=2.0)
    assert (r.objective, r.value, r.lml) == ("loo", 2.0, -3.5)
