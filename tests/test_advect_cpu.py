"""Advection through the fitted flow, without a device: the numpy reference tests/advect_ref.py
checked against itself (order of convergence, the tangent against central differences of its own
discrete flow map, area conservation), engine.ftle's closed form, and gp2d_advect's host checks.

The flow is advect_ref.oracle_flow(200): oracle.OracleFit of tracks(200) — f1 = sin(x2/7),
f2 = cos(x1/9), noise 0.01, l_df 5, l_cf 4 — for the div-free and the mixed (ratio 0.35) kernel; 300
start points on [−5, 50] × [−5, 65], the first five on training points; T = 20, vel_scale 1.
Measured here: ‖F‖₂ up to 10.6 (df) and 17.4 (mixed), displacements up to 21.
"""
import ctypes
import functools

import numpy as np
import pytest

import advect_ref as A

KINDS = [("df", 1.0), ("mixed", 0.35)]
T_END = 20.0


@functools.lru_cache(maxsize=None)
def flow(kind, ratio):
    return A.oracle_flow(200, kind, ratio)


def starts():
    return A.seeds(A.tracks(200)[0])


@functools.lru_cache(maxsize=None)
def run(kind, ratio, nsteps, tangent):
    return A.advect(flow(kind, ratio), starts(), 0.0, T_END / nsteps, nsteps, tangent=tangent)


@pytest.mark.parametrize("kind,ratio", KINDS)
def test_reference_converges_at_fourth_order(kind, ratio):
    """The position error of 20, 40 and 80 steps against 160: each halving of the step divides it
    by 2⁴ = 16 up to the next order's share — between 12 and 20."""
    end = run(kind, ratio, 160, False).path[-1]
    err = [float(np.max(np.abs(run(kind, ratio, n, False).path[-1] - end))) for n in (20, 40, 80)]
    print(f"{kind}: errors {err}, ratios {err[0] / err[1]:.1f} {err[1] / err[2]:.1f}")
    assert err[2] >= 1e-6      # what a wrong stage weight or time would be measured against
    assert 12.0 < err[0] / err[1] < 20.0 and 12.0 < err[1] / err[2] < 20.0, err


@pytest.mark.parametrize("kind,ratio", KINDS)
def test_tangent_is_the_derivative_of_the_discrete_flow_map(kind, ratio):
    """An RK method applied to the variational equation is the derivative of its own map, so F
    equals central differences (δ = 1e-5) of the reference's 40-step map without truncation error
    in the step: to 1e-7 (the differences' own δ² and rounding/δ terms)."""
    f = flow(kind, ratio)
    x0 = starts()
    F = run(kind, ratio, 40, True).tangent[-1]
    delta = 1e-5
    fd = np.empty_like(F)
    for b in range(2):
        e = np.zeros(2)
        e[b] = delta
        hi = A.advect(f, x0 + e, 0.0, T_END / 40, 40, tangent=False).path[-1]
        lo = A.advect(f, x0 - e, 0.0, T_END / 40, 40, tangent=False).path[-1]
        fd[:, :, b] = (hi - lo) / (2 * delta)
    err = float(np.max(np.abs(F - fd)))
    print(f"{kind}: max |F − central differences| = {err:.2e}, max ‖F‖₂ = {run(kind, ratio, 40, True).fmax:.1f}")
    assert err < 1e-7


def test_divfree_flow_conserves_area():
    """det F = exp(∫ div μ dt): 1 for the div-free kernel up to the scheme's O(h⁴) (|det F − 1| < 1e-5
    at 40 steps), far from 1 for the mixed kernel, whose mean flow has divergence."""
    det = np.linalg.det(run("df", 1.0, 40, True).tangent[-1])
    detm = np.linalg.det(run("mixed", 0.35, 40, True).tangent[-1])
    print(f"df: max |det F − 1| = {np.max(np.abs(det - 1)):.2e}; mixed: {np.max(np.abs(detm - 1)):.2e}")
    assert np.max(np.abs(det - 1.0)) < 1e-5
    assert np.max(np.abs(detm - 1.0)) > 0.1


def test_reference_records_and_backward_time():
    """Run.records lists gp2d_advect's records; integrating back from the end returns to the start
    to the scheme's accuracy."""
    r = run("df", 1.0, 40, False)
    assert list(r.records(8)) == [0, 8, 16, 24, 32, 40] and list(r.records(7)) == [0, 7, 14, 21, 28, 35, 40]
    assert list(r.records(40)) == [0, 40]
    back = A.advect(flow("df", 1.0), r.path[-1], T_END, -T_END / 40, 40, tangent=False).path[-1]
    assert np.max(np.abs(back - starts())) < 1e-3
    assert r.umax > 0.5 and np.max(np.abs(r.path[-1] - r.path[0])) > 10.0


def test_ftle_closed_form():
    """engine.ftle on F = R(θ)·diag(e^{aT}, e^{−aT})·R(φ)ᵀ gives a to 1e-14, on CPU tensors, numpy arrays and
    over leading dimensions; advect_ref.ftle (numpy's eigensolver) agrees."""
    torch = pytest.importorskip("torch")
    from gp2d import engine as E
    rng = np.random.default_rng(3)
    a, T = rng.uniform(0.02, 0.2, (4, 5)), 20.0

    def rot(t):
        return np.stack([np.stack([np.cos(t), -np.sin(t)], -1), np.stack([np.sin(t), np.cos(t)], -1)], -2)

    D = np.zeros((4, 5, 2, 2))
    D[..., 0, 0], D[..., 1, 1] = np.exp(a * T), np.exp(-a * T)
    F = rot(rng.uniform(0, 6, (4, 5))) @ D @ np.swapaxes(rot(rng.uniform(0, 6, (4, 5))), -1, -2)
    out = E.ftle(torch.as_tensor(F), T)
    assert out.shape == (4, 5) and out.dtype == torch.float64
    assert np.max(np.abs(out.numpy() - a)) < 1e-14
    assert np.max(np.abs(E.ftle(F, -T).numpy() - a)) < 1e-14       # |duration|
    assert np.max(np.abs(E.ftle(F[0, 0], T).numpy() - a[0, 0])) < 1e-14
    assert np.max(np.abs(A.ftle(F, T) - a)) < 1e-13
    assert float(E.ftle(np.eye(2), 5.0)) == 0.0


def test_advect_abi_refusals():
    """gp2d_advect_records' count and gp2d_advect's host checks, which run before any device work
    (the pointers are never dereferenced) and name their parameter."""
    from gp2d import _native as N
    L = N.lib()
    assert L.gp2d_advect_records(40, 7) == 7 and L.gp2d_advect_records(40, 8) == 6
    assert L.gp2d_advect_records(0, 1) == 1 and L.gp2d_advect_records(1, 100) == 2
    assert L.gp2d_advect_records(-1, 1) < 0 and b"nsteps" in L.gp2d_last_error()
    assert L.gp2d_advect_records(4, 0) < 0 and b"save_every" in L.gp2d_last_error()

    one = ctypes.c_void_p(1)   # never dereferenced: the argument checks fail first
    good = N.vector_kernel_desc(N.KIND_DIVFREE, 5.0)
    trend = N.trend_desc(1, (0.0, 0.0), 1.0)

    def call(k=good, n=128, ntr=50, npad=64, trend=None, block=None, m=10, t0=0.0, dt=0.5, nsteps=4, save_every=2,
             s=1.0, alpha=one, xtr=one, x0=one, path=one):
        return L.gp2d_advect(alpha, n, xtr, ntr, npad, ctypes.byref(k), None if trend is None else ctypes.byref(trend),
                             block, x0, m, t0, dt, nsteps, save_every, s, path, None, None)

    def refused(what, **kw):
        rc = call(**kw)
        assert rc < 0 and what in L.gp2d_last_error(), (kw, rc, L.gp2d_last_error())

    refused(b"advect: k ", k=N.ard_kernel_desc([1.0], [[1.0, 2.0]]))
    refused(b"advect: k ", k=N.vector_kernel_desc(N.KIND_SCALAR, 5.0))
    refused(b"advect: k ", k=N.vector_kernel_desc(N.KIND_DIVFREE, -1.0))
    refused(b"advect: k ", k=N.vector_sum_kernel_desc([good, N.vector_kernel_desc(N.KIND_SCALAR, 5.0)], [1.0, 1.0])[0])
    refused(b"advect: n ", n=256)
    refused(b"advect: ntr ", ntr=0)
    refused(b"advect: ntr ", ntr=65)
    refused(b"advect: nsteps", nsteps=-1)
    refused(b"advect: save_every", save_every=0)
    refused(b"advect: dt ", dt=0.0)
    refused(b"advect: dt ", dt=float("nan"))
    refused(b"advect: t0 ", t0=float("inf"))
    refused(b"advect: vel_scale", s=float("inf"))
    refused(b"block", trend=trend, block=None)
    refused(b"trend", trend=None, block=ctypes.c_void_p(64))
    refused(b"64-byte", trend=trend, block=ctypes.c_void_p(8))
    refused(b"order", trend=N.trend_desc(2, (0.0, 0.0), 1.0), block=ctypes.c_void_p(64))
    refused(b"advect: x0", x0=None)
    refused(b"advect: path", path=None)
    refused(b"advect: alpha", alpha=None)
    assert call(m=0) == 0                                # nothing to do: no launch, no device needed
    assert call(m=0, dt=0.0, nsteps=0) == 0              # dt is not read without steps
