"""The velocity gradient tensor of the fitted flow with its 4 × 4 posterior covariance per point
(gp2d_predict_grad, engine.predict_gradient, engine.flow_diagnostics, Krig.predict_gradient /
predict_diagnostics), against the numpy reference tests/grad_ref.py.  Shapes and inputs are those
of test_gpu_fields.py.

Tolerances: cross-covariance entries and the W = I Gram 1e-13 relative to the max-norm (the gate of
test_gpu_fields.test_field_cross_covariance); posterior mean / covariance 1e-10 relative normwise
(the gate of test_gpu_fields for the same fits; the reference's own `solve_triangular` and `inv`
recipes differ by ≤ 2.7e-14 normwise on these inputs and the smallest posterior diagonal is 2.8 %
of its prior, so the gate hides nothing); agreement with predict_field 1e-10 of the field's prior
(absolute: aᵀΣa cancels); sharded and whole predictions bit-identical.
"""
import ctypes
import dataclasses
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
if not torch.cuda.is_available():  # pragma: no cover
    pytest.skip("no HIP device", allow_module_level=True)

import field_ref as F  # noqa: E402
import grad_ref as R  # noqa: E402
from gp2d import _native as N  # noqa: E402
from gp2d import engine as E  # noqa: E402
from gp2d.krig import Krig  # noqa: E402
from oracle import gp2d_oracle as O  # noqa: E402

L_DF, L_CF, NOISE = 5.0, 4.0, 0.01
CASES = [("df", 1.0), ("cf", 0.0), ("mixed", 0.35)]
DEV = torch.device("cuda")


def rel(a, b):
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    return float(np.max(np.abs(a - b)) / max(np.max(np.abs(b)), 1e-300))


def normwise(a, b):
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    return float(np.linalg.norm((a - b).ravel()) / max(np.linalg.norm(b.ravel()), 1e-300))


def spec(kind, ratio):
    return E.KernelSpec(kind=kind, l_df=L_DF, l_cf=L_CF, ratio=ratio)


@functools.lru_cache(maxsize=None)
def tracks(n, sd=0.05):
    rng = np.random.default_rng(n)
    x = np.stack([rng.uniform(0, 45, n), rng.uniform(0, 60, n)], 1)
    y = np.concatenate([np.sin(x[:, 1] / 7), np.cos(x[:, 0] / 9)]) + sd * rng.normal(0, 1, 2 * n)
    return x, y


def targets(x, m=700, seed=1):
    """m points on [−5, 50] × [−5, 65], the first five on training points (d = 0)."""
    rng = np.random.default_rng(seed)
    g = np.stack([rng.uniform(-5, 50, m), rng.uniform(-5, 65, m)], 1)
    k = min(5, x.shape[0]) if m > 5 else 0
    g[:k] = x[:k]
    return g


@functools.lru_cache(maxsize=None)
def reference(n, kind, ratio):
    """(mean (700, 4), cov (700, 4, 4), prior (4, 4)) at targets(tracks(n)) from the oracle's Cholesky fit."""
    x, y = tracks(n)
    fit = O.OracleFit(x, y, kind, L_DF, L_CF, ratio, NOISE)
    mo, co = R.fit_predict_grad(fit.L, fit.alpha, x, targets(x), kind, L_DF, L_CF, ratio)
    for a in (mo, co):
        a.setflags(write=False)
    return mo, co, R.prior(kind, L_DF, L_CF, ratio)


@functools.lru_cache(maxsize=None)
def fitted(n, kind, ratio, variance="f64"):
    x, y = tracks(n)
    return E.fit(spec(kind, ratio), x, y, NOISE, variance=variance)


def check_covariances(cov, prior, what):
    """Exact symmetry, diag ≤ prior·(1 + 1e-12), eigenvalues ≥ −1e-12·max|prior|."""
    assert np.array_equal(cov, cov.transpose(0, 2, 1)), what
    diag = np.einsum("maa->ma", cov)
    assert (diag <= np.diag(prior) * (1 + 1e-12)).all(), what
    ev = np.linalg.eigvalsh(cov)
    assert ev.min() >= -1e-12 * np.max(np.abs(prior)), (what, ev.min())


def check_posterior(gp, n, kind, ratio, chunk=256):
    x, _ = tracks(n)
    mo, co, prior = reference(n, kind, ratio)
    mu, cov = E.predict_gradient(gp, targets(x), chunk=chunk)
    assert mu.shape == (700, 4) and cov.shape == (700, 4, 4)
    mu, cov = mu.cpu().numpy(), cov.cpu().numpy()
    em, ec = normwise(mu, mo), normwise(cov, co)
    dmin = np.min(np.einsum("maa->ma", cov)[:, np.diag(prior) > 0] / np.diag(prior)[np.diag(prior) > 0])
    print(f"{kind} N={n}: mean normwise {em:.2e}, cov normwise {ec:.2e}, min diag/prior {dmin:.3f}")
    assert em < 1e-10 and ec < 1e-10, (kind, n, em, ec)
    check_covariances(cov, prior, (kind, n))
    assert rel(gp.kernel.grad_prior_cov(), prior) <= 1e-15


# ---- 1. the cross-covariance and the column layout alone -----------------------------------
def check_identity_fit(na, m, kind, ratio, l_cf):
    """W = I, α = e_k for every row k: the assembled matrix and the Gram of its columns."""
    rng = np.random.default_rng(na + 7 * m)
    xa = np.stack([rng.uniform(0, 45, na), rng.uniform(0, 60, na)], 1)
    g = targets(xa, m, seed=na)
    npad = E.padded_points(na)
    n = 2 * npad
    assert n % 128 == 0 and npad == {1: 64, 37: 64, 130: 192}[na]
    ks = E.KernelSpec(kind=kind, l_df=L_DF, l_cf=l_cf, ratio=ratio)
    X = torch.as_tensor(xa, device=DEV)
    eye = torch.eye(n, dtype=torch.float64, device=DEV)
    C = torch.empty((n, m, 4), dtype=torch.float64, device=DEV)
    cov = None
    for k in range(n):
        gp = E.GPFit(kernel=ks, noise=NOISE, x=X, n_train=na, n_pad=npad, W=eye, alpha=eye[k].contiguous(), device=DEV)
        mu, c = E.predict_gradient(gp, g, compute_cov=(k == 0))
        C[k] = mu
        cov = c if k == 0 else cov
    C = C.cpu().numpy()
    ref = R.cross(xa, g, kind, L_DF, l_cf, ratio)
    valid = np.r_[0:na, npad:npad + na]
    assert rel(C[valid], ref) < 1e-13
    pad = np.setdiff1d(np.arange(n), valid)
    assert not C[pad].any()
    want = R.prior(kind, L_DF, l_cf, ratio) - np.einsum("nma,nmb->mab", ref, ref)
    assert rel(cov.cpu().numpy(), want) < 1e-13


@pytest.mark.parametrize("kind,ratio", CASES)
@pytest.mark.parametrize("na,m", [(1, 1), (37, 100), (130, 64)])
def test_grad_cross_covariance_and_layout(kind, ratio, na, m):
    """With W = I and α = e_k the predicted mean is row k of the assembled matrix, un-permuted from
    the epilogue's column layout, for all four components, and the covariance is prior − the Gram
    of the reference's columns: every row of the buffer — the padded ones, which must be exact
    zeros, included — against grad_ref.cross.  (1, 1): a single point; (37, 100): ragged tiles,
    targets across the 16-target and 64-column group boundaries, which pins the permutation;
    (130, 64): na_pad = 192, the second component's rows start past a 64-point tile."""
    check_identity_fit(na, m, kind, ratio, L_CF)


def test_grad_cross_covariance_equal_lengths():
    """A mixed kernel with ℓ_cf = ℓ_df takes the kernel's other path: one exp serves both parts."""
    check_identity_fit(37, 100, "mixed", 0.35, L_DF)


# ---- 2. posterior against the reference ----------------------------------------------------
@pytest.mark.parametrize("kind,ratio", CASES)
@pytest.mark.parametrize("n", [130, 300, 1000])
def test_grad_posterior_vs_reference(kind, ratio, n):
    check_posterior(fitted(n, kind, ratio), n, kind, ratio)   # chunk = 256: three chunks, the last 188 targets


# ---- 3. the same δ and ζ as predict_field --------------------------------------------------
@pytest.mark.parametrize("kind,ratio", CASES)
def test_grad_agrees_with_predict_field(kind, ratio):
    x, _ = tracks(300)
    g = targets(x)
    gp = fitted(300, kind, ratio)
    mu, cov = E.predict_gradient(gp, g, chunk=256)
    diag = E.flow_diagnostics(mu, cov)
    prior = gp.kernel.grad_prior_cov()
    pmax = np.max(np.abs(prior))
    for field in F.FIELDS:
        fm, fv = (t.cpu().numpy() for t in E.predict_field(gp, g, field, chunk=256))
        dm, dv = (t.cpu().numpy() for t in diag[field])
        fprior = gp.kernel.field_prior_var(field)
        if fprior == 0.0:   # the field vanishes by kind: predict_field gives exact zeros
            em, ev = float(np.max(np.abs(dm))) / float(np.max(np.abs(mu.cpu().numpy()))), float(np.max(np.abs(dv))) / pmax
            print(f"{kind} {field}: |mean| {em:.2e} of the gradient's max, |var| {ev:.2e} of max|prior|")
            assert not fm.any() and not fv.any()
            assert em < 1e-10 and ev <= 1e-10
        else:
            em, ev = normwise(dm, fm), float(np.max(np.abs(dv - fv))) / fprior
            print(f"{kind} {field}: mean normwise {em:.2e}, var abs/prior {ev:.2e}")
            assert em < 1e-10 and ev < 1e-10, (kind, field, em, ev)


# ---- 4. a fit of the int8 engine gives the same tensor -------------------------------------
def test_grad_from_ozaki_fit():
    """The ozaki fit keeps x, α and W in Morton order; predict_gradient uses them as they are."""
    gp = fitted(300, "mixed", 0.35, "ozaki")
    assert gp.perm is not None and gp.W is not None
    check_posterior(gp, 300, "mixed", 0.35)


# ---- 5. sharding ---------------------------------------------------------------------------
def test_grad_sharded_is_bit_identical():
    """Two shards of 150 (not a multiple of 16: the second shard's targets sit at other lane
    positions and in other 16-groups) at chunk 128 against all 300 at chunk 1024."""
    x, _ = tracks(300)
    g = targets(x, 300)
    gp = fitted(300, "mixed", 0.35)
    mu, cov = (t.cpu().numpy() for t in E.predict_gradient(gp, g, chunk=1024))
    parts = []
    for lo, hi in ((0, 150), (150, 300)):
        parts.append([t.cpu().numpy() for t in E.predict_gradient(gp, g[lo:hi], chunk=128)])
    assert np.array_equal(mu, np.concatenate([p[0] for p in parts]))
    assert np.array_equal(cov, np.concatenate([p[1] for p in parts]))


# ---- 6. spatio-temporal product ------------------------------------------------------------
def st_tracks(n, seed):
    """The (T, Y, X) tracks of test_gpu_st.py: observations [v; u]."""
    rng = np.random.default_rng(seed)
    X = np.stack([rng.uniform(0, 6, n), rng.uniform(0, 45, n), rng.uniform(0, 60, n)], 1)
    v = np.cos(X[:, 2] / 9) + 0.1 * X[:, 0] + rng.normal(0, 0.05, n)
    u = np.sin(X[:, 1] / 7) - 0.05 * X[:, 0] + rng.normal(0, 0.05, n)
    return X, np.concatenate([v, u])


def test_grad_spatio_temporal():
    import scipy.linalg as sla
    X, y = st_tracks(300, seed=300)
    rng = np.random.default_rng(1)
    G = np.stack([rng.uniform(-1, 7, 700), rng.uniform(-5, 50, 700), rng.uniform(-5, 65, 700)], 1)
    G[:5] = X[:5]
    assert G[:, 0].min() < 0 and G[:, 0].max() > 6          # times outside the tracks' [0, 6]
    kw = dict(kind="mixed", l_df=L_DF, l_cf=L_CF, ratio=0.35, var_t=2.0, l_t=1.5)
    K = O.vector_st_kernel(X, X, **kw)
    K[np.diag_indices_from(K)] += NOISE
    Lo = np.linalg.cholesky(K)
    alpha = sla.cho_solve((Lo, True), y)
    ks = E.KernelSpec(family="vector_st", **kw)
    gp = E.fit(ks, X, y, NOISE)
    mo, co = R.fit_predict_grad(Lo, alpha, X, G, "mixed", L_DF, L_CF, 0.35, var_t=2.0, l_t=1.5)
    prior = R.prior("mixed", L_DF, L_CF, 0.35, var_t=2.0)
    mu, cov = (t.cpu().numpy() for t in E.predict_gradient(gp, G, chunk=256))
    em, ec = normwise(mu, mo), normwise(cov, co)
    print(f"st: mean normwise {em:.2e}, cov normwise {ec:.2e}")
    assert em < 1e-10 and ec < 1e-10, (em, ec)
    check_covariances(cov, prior, "st")
    assert rel(ks.grad_prior_cov(), prior) <= 1e-15


# ---- 7. the raw ABI writes 4m and 16m doubles ----------------------------------------------
@pytest.mark.parametrize("m", [1, 100, 300])
def test_grad_raw_abi_writes_exactly_its_outputs(m):
    """NaN-filled buffers with a guard zone behind the outputs: exactly 4m and 16m doubles are
    written (padded targets write nothing), and compute_cov = 0 leaves cov untouched."""
    L = N.lib()
    x, _ = tracks(130)
    gp = fitted(130, "mixed", 0.35)
    G = torch.as_tensor(np.ascontiguousarray(targets(x, m)), device=DEV)
    guard = 256
    chunk = 128   # m = 300: three chunks, the last 44 targets
    wbytes = int(L.gp2d_predict_grad_workspace(gp.n, chunk))
    work = torch.empty(wbytes // 8, dtype=torch.float64, device=DEV)
    desc = gp.kernel.desc()

    def run(compute_cov):
        mean = torch.full((4 * m + guard,), float("nan"), dtype=torch.float64, device=DEV)
        cov = torch.full((16 * m + guard,), float("nan"), dtype=torch.float64, device=DEV)
        N.check(L.gp2d_predict_grad(E._ptr(gp.W), gp.n, gp.W.stride(0), E._ptr(gp.alpha), E._ptr(gp.x), gp.n_train,
                                    gp.n_pad, E._ptr(G), m, ctypes.byref(desc), compute_cov, E._ptr(mean), E._ptr(cov),
                                    chunk, E._ptr(work), wbytes, E._stream_handle(DEV)), "gp2d_predict_grad")
        return mean.cpu().numpy(), cov.cpu().numpy()

    mean, cov = run(1)
    assert not np.isnan(mean[:4 * m]).any() and np.isnan(mean[4 * m:]).all()
    assert not np.isnan(cov[:16 * m]).any() and np.isnan(cov[16 * m:]).all()
    mean0, cov0 = run(0)
    assert np.array_equal(mean0[:4 * m], mean[:4 * m]) and np.isnan(mean0[4 * m:]).all()
    assert np.isnan(cov0).all()
    mu, c = E.predict_gradient(gp, G)
    assert np.array_equal(mu.cpu().numpy().reshape(-1), mean[:4 * m])
    assert np.array_equal(c.cpu().numpy().reshape(-1), cov[:16 * m])


# ---- 8. the Krig surface and the sign convention -------------------------------------------
def test_krig_gradient_and_diagnostics_grid():
    """The noise-free 1000-point fit and the 12 × 9 grid of test_gpu_fields.test_krig_predict_fields_grid.
    A centred difference of the predicted velocity grid (dx = 0.5) carries its own truncation error
    dx²/6·|f‴|: an absolute error set by the third derivatives of the whole flow, not by the size of
    the component it estimates.  For the observed u = sin(y/7), v = cos(x/9) the components ∂u/∂y
    and ∂v/∂x are ≈ ±0.1 while ∂u/∂x and ∂v/∂y are ≈ 1e-3, their differences' truncation error
    (≈ 2e-5) being 2.0 % and 0.8 % of themselves but 1.6e-4 and 6.6e-5 of the tensor (measured;
    ∂u/∂y and ∂v/∂x: 9.5e-4 and 6.8e-4 of themselves).  So each component's error is
    taken relative to the max-norm of the differenced tensor on the interior (gate 1e-3), and the
    signs are compared where a component is bounded away from zero (min |fd| > half its max)."""
    x, y = tracks(1000, sd=0.0)
    kr = Krig(kernel="df", l_df=5.0, noise=NOISE).fit(x, y)
    gx, gy = 10.0 + 0.5 * np.arange(12), 40.0 + 0.5 * np.arange(9)
    XX, YY = np.meshgrid(gx, gy)
    pts = np.stack([XX.reshape(-1), YY.reshape(-1)], 1)
    mu, cov = kr.predict_gradient(pts)
    assert isinstance(mu, np.ndarray) and mu.shape == (108, 4) and cov.shape == (108, 4, 4)
    dm, dc = E.predict_gradient(kr.gp, pts, chunk=kr.chunk)
    assert np.array_equal(mu, dm.cpu().numpy()) and np.array_equal(cov, dc.cpu().numpy())
    out = kr.predict_diagnostics_grid(gx, gy)
    assert set(out) == set(E.DIAGNOSTICS)
    want = E.flow_diagnostics(dm, dc)
    for name in E.DIAGNOSTICS:
        a, v = out[name]
        assert a.shape == v.shape == (9, 12)
        assert np.array_equal(a, want[name][0].cpu().numpy().reshape(9, 12)), name
        assert np.array_equal(v, want[name][1].cpu().numpy().reshape(9, 12)), name
    flat = kr.predict_diagnostics(pts, names=("shear_strain",))
    assert set(flat) == {"shear_strain"} and np.array_equal(flat["shear_strain"][0].reshape(9, 12), out["shear_strain"][0])
    # (∂u/∂x, ∂u/∂y, ∂v/∂x, ∂v/∂y) for points (x, y) and components (u, v): rows of the grid are y
    uf, vf, _, _ = kr.predict_grid(gx, gy)
    fd = np.stack([(uf[1:-1, 2:] - uf[1:-1, :-2]) / 1.0, (uf[2:, 1:-1] - uf[:-2, 1:-1]) / 1.0,
                   (vf[1:-1, 2:] - vf[1:-1, :-2]) / 1.0, (vf[2:, 1:-1] - vf[:-2, 1:-1]) / 1.0], -1)
    gm = mu.reshape(9, 12, 4)[1:-1, 1:-1]
    scale = np.max(np.abs(fd))
    compared = 0
    for c, name in enumerate(E.GRADIENT_COMPONENTS):
        err = float(np.max(np.abs(gm[..., c] - fd[..., c])))
        print(f"{name} vs centred difference: {err / scale:.2e} of the tensor's max-norm, "
              f"{err / np.max(np.abs(fd[..., c])):.2e} of its own; range [{fd[..., c].min():.3g}, {fd[..., c].max():.3g}]")
        assert err / scale < 1e-3, name
        if np.min(np.abs(fd[..., c])) > 0.5 * np.max(np.abs(fd[..., c])):
            assert np.array_equal(np.sign(gm[..., c]), np.sign(fd[..., c])), name
            compared += 1
    assert compared == 2   # ∂u/∂y > 0 and ∂v/∂x < 0 on this grid


# ---- 9. what has no gradient predict -------------------------------------------------------
def test_predict_gradient_refuses_scalar_ard_and_planes_only_fits():
    x, y = tracks(130)
    gp = fitted(130, "df", 1.0)
    g = targets(x, 10)
    with pytest.raises(ValueError, match="vector kernel"):
        E.predict_gradient(dataclasses.replace(gp, kernel=E.KernelSpec(kind="scalar")), g)
    ard = E.KernelSpec(family="ard", variances=(1.0,), lengthscales=((5.0, 5.0),))
    with pytest.raises(ValueError, match="vector kernel"):
        E.predict_gradient(dataclasses.replace(gp, kernel=ard), g)
    with pytest.raises(ValueError, match="W"):
        E.predict_gradient(dataclasses.replace(gp, W=None, n_mat=gp.n), g)
    sc = Krig(kernel="scalar", l_df=5.0, noise=NOISE).fit(x, y)
    with pytest.raises(ValueError, match="vector kernel"):
        sc.predict_gradient(g)
    with pytest.raises(ValueError, match="vector kernel"):
        sc.predict_diagnostics(g)
    # the existing surface is unchanged: strain is no predict_field field
    assert E.FIELDS == ("divergence", "vorticity")
    with pytest.raises(ValueError, match="field must be one of"):
        E.predict_field(gp, g, "strain")
