"""The velocity gradient tensor without a device: the closed forms of tests/grad_ref.py against
finite differences of the oracle's vector kernels, their recombination to tests/field_ref.py, the
library's 4 × 4 prior, the workspace formula and argument checks of gp2d_predict_grad
(include/gp2d.h), and the Gaussian moments of engine.flow_diagnostics.

Tolerances: cross-covariances 1e-7 relative to the matrix max-norm against the 4-point central
difference of test_fields_cpu.py (its stencil and gate); the prior 1e-6 against second differences
at zero lag (its gate); recombination to δ and ζ 1e-15 of the max-norm; gp2d_grad_prior_cov 1e-15
relative; Okubo–Weiss moments within 5 standard errors of 2e5 seeded draws.
"""
import ctypes
import math

import numpy as np
import pytest

import field_ref as F
import grad_ref as R
from oracle import gp2d_oracle as O

L_DF, L_CF = 5.0, 3.0
KINDS = [("df", 1.0), ("cf", 0.0), ("mixed", 0.7)]
ST = dict(var_t=2.0, l_t=1.5)


def rel(a, b):
    return float(np.max(np.abs(np.asarray(a) - np.asarray(b))) / max(np.max(np.abs(b)), 1e-300))


def _dK(kernel, xa, g, col, h, **kw):
    """∂K(xa, g)/∂g[:, col] by the 4-point central stencil: the four (N, M) blocks K11, K12, K21, K22."""
    Ks = []
    for t in (-2, -1, 1, 2):
        gs = g.copy()
        gs[:, col] += t * h
        Ks.append(kernel(xa, gs, **kw))
    D = (Ks[0] - 8 * Ks[1] + 8 * Ks[2] - Ks[3]) / (12 * h)
    n, m = xa.shape[0], g.shape[0]
    return D[:n, :m], D[:n, m:], D[n:, :m], D[n:, m:]


def _fd_cross(kernel, xa, g, first, **kw):
    """(2N, M, 4) finite-difference cov(f_p(xa), ∂f_a/∂x_b (g)) = ∂K_pa/∂g_b; `first`: the column of x1."""
    n, m = xa.shape[0], g.shape[0]
    out = np.empty((2 * n, m, 4))
    for b in range(2):
        k11, k12, k21, k22 = _dK(kernel, xa, g, first + b, 1e-3, **kw)
        out[:n, :, 0 + b], out[:n, :, 2 + b] = k11, k12     # p = 1: a = 1, 2
        out[n:, :, 0 + b], out[n:, :, 2 + b] = k21, k22     # p = 2
    return out


@pytest.mark.parametrize("kind,ratio", KINDS)
@pytest.mark.parametrize("st", [False, True])
def test_cross_covariance_is_the_derivative_of_the_kernel(kind, ratio, st):
    rng = np.random.default_rng(3)
    xa = rng.uniform(0, 10, (40, 2))
    g = rng.uniform(0, 10, (30, 2))
    g[:3] = xa[:3]                         # zero lag, where every cross-covariance vanishes
    kw = dict(kind=kind, l_df=L_DF, l_cf=L_CF, ratio=ratio)
    if st:
        xa = np.concatenate([rng.uniform(0, 4, (40, 1)), xa], 1)
        g = np.concatenate([rng.uniform(-1, 5, (30, 1)), g], 1)
        fd = _fd_cross(O.vector_st_kernel, xa, g, 1, **kw, **ST)
        C = R.cross(xa, g, kind, L_DF, L_CF, ratio, **ST)
    else:
        fd = _fd_cross(O.vector_kernel, xa, g, 0, **kw)
        C = R.cross(xa, g, kind, L_DF, L_CF, ratio)
    assert C.shape == (80, 30, 4)
    if not st:
        assert not C[:3, :3][np.eye(3, dtype=bool)].any()    # d = 0: odd in d
    err = rel(C, fd)
    print(f"{kind} st={st}: closed form vs central difference {err:.2e}")
    assert err < 1e-7, (kind, st, err)


@pytest.mark.parametrize("kind,ratio", KINDS)
@pytest.mark.parametrize("st", [False, True])
def test_recombination_gives_divergence_and_vorticity(kind, ratio, st):
    rng = np.random.default_rng(4)
    xa = rng.uniform(0, 10, (40, 2))
    g = rng.uniform(0, 10, (30, 2))
    g[:3] = xa[:3]
    kw = {}
    if st:
        xa = np.concatenate([rng.uniform(0, 4, (40, 1)), xa], 1)
        g = np.concatenate([rng.uniform(-1, 5, (30, 1)), g], 1)
        kw = ST
    C = R.cross(xa, g, kind, L_DF, L_CF, ratio, **kw)
    scale = np.max(np.abs(C))
    for field in F.FIELDS:
        want = F.cross(xa, g, field, kind, L_DF, L_CF, ratio, **kw)
        got = C @ R.LINEAR[field]
        err = float(np.max(np.abs(got - want))) / scale
        print(f"{kind} st={st} {field}: {err:.2e}")
        assert err <= 1e-15, (kind, field, err)
    P = R.prior(kind, L_DF, L_CF, ratio, **({"var_t": ST["var_t"]} if st else {}))
    for field in F.FIELDS:
        a = R.LINEAR[field]
        assert a @ P @ a == pytest.approx(F.prior_var(field, kind, L_DF, L_CF, ratio, ST["var_t"] if st else None),
                                          rel=1e-15, abs=1e-18)


def _k0(d1, d2, **kw):
    """The 2×2 block K(d) of the oracle at lag d = (d1, d2)."""
    return O.vector_kernel(np.array([[d1, d2]]), np.zeros((1, 2)), **kw)


@pytest.mark.parametrize("kind,ratio", KINDS)
def test_prior_is_the_second_derivative_at_zero_lag(kind, ratio):
    """cov(∂_b f_a(g), ∂_d f_c(g')) = −∂_b∂_d K_ac(g − g') at g = g'."""
    kw = dict(kind=kind, l_df=L_DF, l_cf=L_CF, ratio=ratio)
    h = 1e-3
    K0 = _k0(0.0, 0.0, **kw)
    d11 = (_k0(h, 0, **kw) - 2 * K0 + _k0(-h, 0, **kw)) / h ** 2
    d22 = (_k0(0, h, **kw) - 2 * K0 + _k0(0, -h, **kw)) / h ** 2
    d12 = (_k0(h, h, **kw) - _k0(h, -h, **kw) - _k0(-h, h, **kw) + _k0(-h, -h, **kw)) / (4 * h ** 2)
    dd = {(0, 0): d11, (1, 1): d22, (0, 1): d12, (1, 0): d12}
    fd = np.empty((4, 4))
    for a in range(2):
        for b in range(2):
            for c in range(2):
                for d in range(2):
                    fd[2 * a + b, 2 * c + d] = -dd[b, d][a, c]
    P = R.prior(kind, L_DF, L_CF, ratio)
    err = rel(P, fd)
    print(f"{kind}: prior vs second difference {err:.2e}")
    assert err < 1e-6, (kind, err)


def test_grad_prior_cov_abi():
    from gp2d import _native as N
    from gp2d import engine as E
    L = N.lib()
    assert E.GRADIENT_COMPONENTS == R.COMPONENTS == ("du_dx", "du_dy", "dv_dx", "dv_dy")
    kinds = {"df": N.KIND_DIVFREE, "cf": N.KIND_CURLFREE, "mixed": N.KIND_MIXED}
    codes = {"divergence": N.FIELD_DIVERGENCE, "vorticity": N.FIELD_VORTICITY}
    out = (ctypes.c_double * 16)()
    for kind, ratio in KINDS:
        k = N.vector_kernel_desc(kinds[kind], L_DF, L_CF, ratio)
        st = N.vector_st_kernel_desc(kinds[kind], L_DF, L_CF, ratio, 2.0, 1.5)
        for desc, var_t in ((k, None), (st, 2.0)):
            assert L.gp2d_grad_prior_cov(ctypes.byref(desc), out) == 0
            P = np.array(out).reshape(4, 4)
            want = R.prior(kind, L_DF, L_CF, ratio, var_t)
            assert rel(P, want) <= 1e-15
            assert np.array_equal(P, P.T)
            ev = np.linalg.eigvalsh(P)
            assert ev.min() >= -1e-15 * ev.max()
            for field, code in codes.items():
                a = R.LINEAR[field]
                assert a @ P @ a == pytest.approx(L.gp2d_field_prior_var(ctypes.byref(desc), code), rel=1e-15, abs=1e-18)
        spec = E.KernelSpec(kind=kind, l_df=L_DF, l_cf=L_CF, ratio=ratio)
        got = spec.grad_prior_cov()
        assert got.shape == (4, 4) and rel(got, R.prior(kind, L_DF, L_CF, ratio)) <= 1e-15
    # singular directions: no divergence in a df prior, no vorticity in a cf prior
    assert not (E.KernelSpec(kind="df", l_df=L_DF).grad_prior_cov() @ R.LINEAR["divergence"]).any()
    assert not (E.KernelSpec(kind="cf", l_cf=L_CF).grad_prior_cov() @ R.LINEAR["vorticity"]).any()
    # bad input: < 0 and NaNs
    scalar = N.vector_kernel_desc(N.KIND_SCALAR, L_DF)
    ard = N.ard_kernel_desc([0.8], [[3.0, 4.0]])
    bad_len = N.vector_kernel_desc(N.KIND_DIVFREE, -1.0)
    for desc in (scalar, ard, bad_len):
        out[:] = [0.0] * 16
        assert L.gp2d_grad_prior_cov(ctypes.byref(desc), out) < 0
        assert all(math.isnan(v) for v in out)
    assert L.gp2d_grad_prior_cov(None, out) < 0 and all(math.isnan(v) for v in out)
    assert L.gp2d_grad_prior_cov(ctypes.byref(scalar), None) < 0
    with pytest.raises(ValueError, match="vector kernel"):
        E.KernelSpec(kind="scalar").grad_prior_cov()
    with pytest.raises(ValueError, match="vector kernel"):
        E.KernelSpec(family="ard", variances=(1.0,), lengthscales=((5.0, 5.0),)).grad_prior_cov()


def test_predict_grad_workspace_is_its_layout():
    """C (n × 4·chunk) | the mean's partials ((n/128 + 1) × 4·chunk) | the Gram partials
    ((n/128 + 1) × 10·chunk), in doubles."""
    from gp2d import _native as N
    L = N.lib()
    for n, chunk in [(128, 64), (256, 128), (384, 192), (2048, 1024), (8192, 8192)]:
        seg = n // 128 + 1
        assert L.gp2d_predict_grad_workspace(n, chunk) == 8 * (n * 4 * chunk + seg * 4 * chunk + seg * 10 * chunk)
    # twice the columns of the velocity predict's K*ᵀ
    assert L.gp2d_predict_grad_workspace(256, 128) > 2 * 256 * 2 * 128 * 8


def test_predict_grad_argument_errors_are_reported():
    """Every argument error of gp2d_predict_grad comes before any device work: the pointers here
    are never dereferenced (the style of test_fields_cpu.test_predict_field_argument_errors_are_reported)."""
    from gp2d import _native as N
    L = N.lib()
    one = ctypes.c_void_p(1)
    big = 1 << 40
    good = N.vector_kernel_desc(N.KIND_MIXED, 5.0, 4.0, 0.35)

    def call(k=good, n=256, npad=128, ntr=100, ldw=None, chunk=64, wbytes=big, m=10, work=one):
        return L.gp2d_predict_grad(one, n, n if ldw is None else ldw, one, one, ntr, npad, one, m, ctypes.byref(k), 1,
                                   one, one, chunk, work, wbytes, None)

    assert call(k=N.vector_kernel_desc(N.KIND_SCALAR, 5.0)) < 0 and b"vector kernels only" in L.gp2d_last_error()
    assert call(k=N.ard_kernel_desc([1.0], [[5.0, 5.0]])) < 0 and b"vector kernels only" in L.gp2d_last_error()
    assert call(k=N.vector_kernel_desc(N.KIND_DIVFREE, -1.0)) < 0 and b"l_df" in L.gp2d_last_error()
    assert call(n=256, npad=64) < 0 and b"ntr_pad" in L.gp2d_last_error()
    assert call(n=100, npad=50) < 0 and b"multiple of 128" in L.gp2d_last_error()
    assert call(n=0, npad=0) < 0 and b"multiple of 128" in L.gp2d_last_error()
    assert call(ntr=129) < 0 and b"point count" in L.gp2d_last_error()
    assert call(ldw=128) < 0 and b"ldw" in L.gp2d_last_error()
    for bad in (0, -64, 32, 96):
        assert call(chunk=bad) < 0 and b"chunk" in L.gp2d_last_error()
    assert call(chunk=1 << 28) < 0 and b"out of range" in L.gp2d_last_error()   # 4·chunk columns: an int
    assert call(wbytes=8) < 0 and b"workspace" in L.gp2d_last_error()
    assert call(wbytes=L.gp2d_predict_grad_workspace(256, 64) - 1) < 0 and b"workspace" in L.gp2d_last_error()
    assert call(work=None) < 0 and b"workspace" in L.gp2d_last_error()
    # nothing to predict: no device call, no error
    assert call(m=0, wbytes=L.gp2d_predict_grad_workspace(256, 64)) == 0
    assert call(m=-3) == 0


def test_flow_diagnostics_moments():
    """The linear diagnostics are exactly aᵀμ, aᵀΣa; the Okubo–Weiss mean and variance are the
    moments of gᵀAg for g ~ N(μ, Σ): within 5 standard errors of 2e5 seeded draws (the standard
    error of the sample variance from the sample's fourth central moment)."""
    torch = pytest.importorskip("torch")
    from gp2d import engine as E
    rng = np.random.default_rng(11)
    mu = np.array([0.3, -0.2, 0.25, 0.1])
    B = rng.normal(0, 0.15, (4, 4))
    S = B @ B.T + 0.01 * np.eye(4)
    assert set(E.DIAGNOSTICS) == set(R.LINEAR) | {"okubo_weiss"}
    out = E.flow_diagnostics(mu, S)
    for name, a in R.LINEAR.items():
        assert out[name][0] == pytest.approx(a @ mu, rel=1e-15, abs=1e-17)
        assert out[name][1] == pytest.approx(a @ S @ a, rel=1e-14)
    g = rng.multivariate_normal(mu, S, size=200_000, method="cholesky")
    ow = (g[:, 0] - g[:, 3]) ** 2 + 4 * g[:, 1] * g[:, 2]
    nd = ow.size
    m1, v = ow.mean(), ow.var(ddof=1)
    se_mean = math.sqrt(v / nd)
    m4 = np.mean((ow - m1) ** 4)
    se_var = math.sqrt((m4 - v * v * (nd - 3) / (nd - 1)) / nd)
    em, ev = out["okubo_weiss"]
    print(f"OW mean {em:.6f} vs {m1:.6f} ± {se_mean:.1e}; var {ev:.6f} vs {v:.6f} ± {se_var:.1e}")
    assert abs(em - m1) < 5 * se_mean
    assert abs(ev - v) < 5 * se_var
    # batches, torch tensors, names and the mean-only form agree with the single point
    M = np.stack([mu, 2 * mu, -mu])
    C = np.stack([S, 0.5 * S, S])
    ref = R.diagnostics(M, C)
    for kind in ("numpy", "torch"):
        a, c = (M, C) if kind == "numpy" else (torch.as_tensor(M), torch.as_tensor(C))
        got = E.flow_diagnostics(a, c)
        for name in E.DIAGNOSTICS:
            for u, w in zip(got[name], ref[name]):
                assert np.asarray(u).shape == (3,) and rel(np.asarray(u), w) < 1e-14, (kind, name)
        assert float(np.asarray(got["okubo_weiss"][0])[0]) == pytest.approx(em, rel=1e-14)
        only = E.flow_diagnostics(a, None, names=("shear_strain", "okubo_weiss"))
        assert set(only) == {"shear_strain", "okubo_weiss"} and only["shear_strain"][1] is None
        assert rel(np.asarray(only["okubo_weiss"][0]), np.einsum("ma,ab,mb->m", M, R.OW, M)) < 1e-14
    with pytest.raises(ValueError, match="diagnostic must be one of"):
        E.flow_diagnostics(mu, S, names=("strain",))
