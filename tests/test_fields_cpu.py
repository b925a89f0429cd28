"""Derived fields (divergence, vorticity) without a device: the closed forms of tests/field_ref.py
against finite differences of the oracle's vector kernel, the library's prior variances, and the
argument checks of gp2d_predict_field (include/gp2d.h).

Tolerances: cross-covariances 1e-7 relative to the matrix max-norm against a 4-point central
difference (the gate and stencil of test_gpu_st.test_st_kernel_grad_dense); prior variances 1e-6
against a second difference at zero lag; gp2d_field_prior_var 1e-15 against 8·w/ℓ⁴.
"""
import ctypes
import math

import numpy as np
import pytest

import field_ref as F
from oracle import gp2d_oracle as O

L_DF, L_CF = 5.0, 3.0
KINDS = [("df", 1.0), ("cf", 0.0), ("mixed", 0.7)]


def rel(a, b):
    return float(np.max(np.abs(np.asarray(a) - np.asarray(b))) / max(np.max(np.abs(b)), 1e-300))


def _dK(xa, g, axis, h, **kw):
    """∂K(xa, g)/∂g_axis by the 4-point central stencil: the four (N, M) blocks K11, K12, K21, K22."""
    Ks = []
    for t in (-2, -1, 1, 2):
        gs = g.copy()
        gs[:, axis] += t * h
        Ks.append(O.vector_kernel(xa, gs, **kw))
    D = (Ks[0] - 8 * Ks[1] + 8 * Ks[2] - Ks[3]) / (12 * h)
    n, m = xa.shape[0], g.shape[0]
    return D[:n, :m], D[:n, m:], D[n:, :m], D[n:, m:]


@pytest.mark.parametrize("kind,ratio", KINDS)
def test_cross_covariance_is_the_derivative_of_the_kernel(kind, ratio):
    rng = np.random.default_rng(3)
    xa = rng.uniform(0, 10, (40, 2))
    g = rng.uniform(0, 10, (30, 2))
    g[:3] = xa[:3]                         # zero lag, where both fields' cross-covariances vanish
    kw = dict(kind=kind, l_df=L_DF, l_cf=L_CF, ratio=ratio)
    h = 1e-3
    a11, a12, a21, a22 = _dK(xa, g, 0, h, **kw)   # ∂/∂g1 of cov(f_p(x), f_q(g))
    b11, b12, b21, b22 = _dK(xa, g, 1, h, **kw)   # ∂/∂g2
    fd = {"divergence": np.concatenate([a11 + b12, a21 + b22], 0),      # ∂g1 K_p1 + ∂g2 K_p2
          "vorticity": np.concatenate([a12 - b11, a22 - b21], 0)}       # ∂g1 K_p2 − ∂g2 K_p1
    scale = max(np.max(np.abs(m)) for m in (a11, a12, a21, a22, b11, b12, b21, b22))
    for field in F.FIELDS:
        C = F.cross(xa, g, field, kind, L_DF, L_CF, ratio)
        assert C.shape == (80, 30)
        w = F.weights(kind, ratio)[0 if field == "vorticity" else 1]
        if w == 0.0:   # vanishes by kind: exactly zero in closed form, rounding noise in the differences
            assert not C.any()
            assert np.max(np.abs(fd[field])) < 1e-7 * scale, (kind, field)
        else:
            assert rel(C, fd[field]) < 1e-7, (kind, field)


def _k0(d1, d2, **kw):
    """The 2×2 block K(d) of the oracle at lag d = (d1, d2)."""
    return O.vector_kernel(np.array([[d1, d2]]), np.zeros((1, 2)), **kw)


@pytest.mark.parametrize("kind,ratio", KINDS)
def test_prior_variance_is_the_second_derivative_at_zero_lag(kind, ratio):
    """cov(∂_p f_a(g), ∂_q f_b(g')) = −∂_p∂_q K_ab(g − g'), so at g = g':
    Var δ = −(∂11 K11 + 2 ∂12 K12 + ∂22 K22)(0),  Var ζ = −(∂11 K22 − 2 ∂12 K12 + ∂22 K11)(0)."""
    kw = dict(kind=kind, l_df=L_DF, l_cf=L_CF, ratio=ratio)
    h = 1e-3
    K0 = _k0(0.0, 0.0, **kw)
    d11 = (_k0(h, 0, **kw) - 2 * K0 + _k0(-h, 0, **kw)) / h ** 2
    d22 = (_k0(0, h, **kw) - 2 * K0 + _k0(0, -h, **kw)) / h ** 2
    d12 = (_k0(h, h, **kw) - _k0(h, -h, **kw) - _k0(-h, h, **kw) + _k0(-h, -h, **kw)) / (4 * h ** 2)
    fd = {"divergence": -(d11[0, 0] + 2 * d12[0, 1] + d22[1, 1]),
          "vorticity": -(d11[1, 1] - 2 * d12[0, 1] + d22[0, 0])}
    scale = max(np.max(np.abs(d)) for d in (d11, d12, d22))
    for field in F.FIELDS:
        pv = F.prior_var(field, kind, L_DF, L_CF, ratio)
        if pv == 0.0:
            assert abs(fd[field]) < 1e-6 * scale, (kind, field)
        else:
            assert abs(pv - fd[field]) < 1e-6 * abs(fd[field]), (kind, field, pv, fd[field])


def test_field_prior_var_abi():
    from gp2d import _native as N
    from gp2d import engine as E
    L = N.lib()
    codes = {"divergence": N.FIELD_DIVERGENCE, "vorticity": N.FIELD_VORTICITY}
    assert (N.FIELD_DIVERGENCE, N.FIELD_VORTICITY) == (1, 2) and E.FIELDS == F.FIELDS
    kinds = {"df": N.KIND_DIVFREE, "cf": N.KIND_CURLFREE, "mixed": N.KIND_MIXED}
    for kind, ratio in KINDS:
        k = N.vector_kernel_desc(kinds[kind], L_DF, L_CF, ratio)
        st = N.vector_st_kernel_desc(kinds[kind], L_DF, L_CF, ratio, 2.0, 1.5)
        spec = E.KernelSpec(kind=kind, l_df=L_DF, l_cf=L_CF, ratio=ratio)
        for field, code in codes.items():
            w_df, w_cf = F.weights(kind, ratio)
            want = 8.0 * w_cf / L_CF ** 4 if field == "divergence" else 8.0 * w_df / L_DF ** 4
            assert want == F.prior_var(field, kind, L_DF, L_CF, ratio)
            assert L.gp2d_field_prior_var(ctypes.byref(k), code) == pytest.approx(want, rel=1e-15, abs=0.0)
            assert L.gp2d_field_prior_var(ctypes.byref(st), code) == pytest.approx(2.0 * want, rel=1e-15, abs=0.0)
            assert spec.field_prior_var(field) == pytest.approx(want, rel=1e-15, abs=0.0)
    k = N.vector_kernel_desc(N.KIND_MIXED, L_DF, L_CF, 0.7)
    for bad in (0, 3, -1):
        assert math.isnan(L.gp2d_field_prior_var(ctypes.byref(k), bad))
    scalar = N.vector_kernel_desc(N.KIND_SCALAR, L_DF)
    ard = N.ard_kernel_desc([0.8], [[3.0, 4.0]])
    for code in codes.values():
        assert math.isnan(L.gp2d_field_prior_var(ctypes.byref(scalar), code))
        assert math.isnan(L.gp2d_field_prior_var(ctypes.byref(ard), code))
        assert math.isnan(L.gp2d_field_prior_var(None, code))
    # the Python surface refuses the same kernels, and unknown names, with a ValueError
    with pytest.raises(ValueError):
        E.KernelSpec(kind="scalar").field_prior_var("vorticity")
    with pytest.raises(ValueError):
        E.KernelSpec(family="ard", variances=(1.0,), lengthscales=((5.0, 5.0),)).field_prior_var("divergence")
    with pytest.raises(ValueError):
        spec.field_prior_var("strain")


def test_predict_field_argument_errors_are_reported():
    """Every argument error of gp2d_predict_field comes before any device work: the pointers here
    are never dereferenced (the style of test_host_cpu.test_argument_errors_are_reported)."""
    from gp2d import _native as N
    L = N.lib()
    one = ctypes.c_void_p(1)
    big = 1 << 40
    good = N.vector_kernel_desc(N.KIND_MIXED, 5.0, 4.0, 0.35)

    def call(k=good, field=N.FIELD_VORTICITY, n=256, npad=128, chunk=128, wbytes=big):
        return L.gp2d_predict_field(one, n, n, one, one, 100, npad, one, 10, ctypes.byref(k), field, 1, one, one,
                                    chunk, one, wbytes, None)

    assert L.gp2d_predict_field_workspace(256, 128) == L.gp2d_predict_workspace(256, 128, 1) > 256 * 128 * 8
    assert L.gp2d_predict_field_workspace(256, 256) == L.gp2d_predict_workspace(256, 256, 1)
    assert call(k=N.vector_kernel_desc(N.KIND_SCALAR, 5.0)) < 0 and b"vector kernels only" in L.gp2d_last_error()
    assert call(k=N.ard_kernel_desc([1.0], [[5.0, 5.0]])) < 0 and b"vector kernels only" in L.gp2d_last_error()
    assert call(k=N.vector_kernel_desc(N.KIND_DIVFREE, -1.0)) < 0 and b"l_df" in L.gp2d_last_error()
    for bad in (0, 3):
        assert call(field=bad) < 0 and b"field" in L.gp2d_last_error()
    assert call(chunk=64) < 0 and b"chunk" in L.gp2d_last_error()
    assert call(chunk=0) < 0 and b"chunk" in L.gp2d_last_error()
    assert call(n=100, npad=50) < 0 and b"multiple of 128" in L.gp2d_last_error()
    assert call(n=256, npad=64) < 0 and b"ntr_pad" in L.gp2d_last_error()
    assert call(wbytes=8) < 0 and b"workspace" in L.gp2d_last_error()
    assert call(wbytes=L.gp2d_predict_field_workspace(256, 128) - 1) < 0 and b"workspace" in L.gp2d_last_error()
