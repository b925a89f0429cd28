"""Joint posterior covariance and conditional simulations (gp2d_predict_cov, engine.predict_cov,
engine.jitchol, engine.sample_posterior, Krig.predict_cov / sample / sample_grid) against the numpy
reference tests/cov_ref.py.

Tolerances: entries 1e-13 relative to the matrix max-norm where only kernel evaluation and one
product are involved (the gate of test_gpu_fields.test_field_cross_covariance); the posterior
1e-10 relative normwise, the project's gate (the reference's own `chol` and `inv` recipes differ by
≤ 8.4e-14 on these inputs, tests/test_cov_cpu.py); the ensemble check's bound comes from the
distribution of a product of Gaussians (cov_ref.ensemble_bound), not from the samples.
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

import cov_ref as C  # noqa: E402
from gp2d import _native as N  # noqa: E402
from gp2d import engine as E  # noqa: E402
from gp2d.krig import Krig  # noqa: E402
from oracle import gp2d_oracle as O  # noqa: E402

L_DF, L_CF, NOISE = C.L_DF, C.L_CF, C.NOISE
DEV = torch.device("cuda")


def rel(a, b):
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    return float(np.max(np.abs(a - b)) / max(np.max(np.abs(b)), 1e-300))


def spec(kind, ratio):
    return E.KernelSpec(kind=kind, l_df=L_DF, l_cf=L_CF, ratio=ratio)


def okw(kind, ratio):
    return dict(kind=kind, l_df=L_DF, l_cf=L_CF, ratio=ratio)


@functools.lru_cache(maxsize=None)
def oracle_fit(n, kind, ratio):
    x, y = C.tracks(n)
    return O.OracleFit(x, y, kind, L_DF, L_CF, ratio, NOISE)


@functools.lru_cache(maxsize=None)
def reference(n, m, kind, ratio):
    """(targets, Σ, mean) of the oracle's Cholesky fit of tracks(n) at targets(m); read-only."""
    fit = oracle_fit(n, kind, ratio)
    g = C.targets(fit.x, m)
    return g, C.posterior_cov(fit, g), C.posterior_mean(fit, g)


def hand_fit(kind, ratio, xa, w):
    """A GPFit with W = w·I (w = 0: Σ is the prior; w = 1: V = K*ᵀ) and α = 0."""
    na = xa.shape[0]
    npad = E.padded_points(na)
    n = 2 * npad
    W = torch.zeros((n, n), dtype=torch.float64, device=DEV)
    W.diagonal().fill_(float(w))
    return E.GPFit(kernel=spec(kind, ratio), noise=NOISE, x=torch.as_tensor(xa, device=DEV), n_train=na, n_pad=npad,
                   W=W, alpha=torch.zeros(n, dtype=torch.float64, device=DEV), device=DEV)


def hand_points(na, m):
    rng = np.random.default_rng(na + 7 * m)
    xa = np.stack([rng.uniform(0, 45, na), rng.uniform(0, 60, na)], 1)
    return xa, C.targets(xa, m, seed=na)


# (na, m): one tile | mp = 128, q = 256: the first off-diagonal tile, ragged columns | npad = mp =
# 192, q = 384: the v component starts in the middle of a 128-tile on the K axis and on the output
# axes | a full 64-point component, no padding
HAND_SHAPES = [(1, 1), (37, 100), (130, 130), (130, 64)]


# ---- 1. the kernel alone -------------------------------------------------------------------
@pytest.mark.parametrize("kind,ratio", C.CASES)
@pytest.mark.parametrize("na,m", HAND_SHAPES)
def test_prior_epilogue(kind, ratio, na, m):
    """W = 0: Σ is K(g, g) — the epilogue's prior, the mirror and the slicing of the padding."""
    xa, g = hand_points(na, m)
    mean, cov = E.predict_cov(hand_fit(kind, ratio, xa, 0.0), g)
    assert mean.shape == (2 * m,) and cov.shape == (2 * m, 2 * m)
    assert not mean.any()
    assert rel(cov.cpu().numpy(), O.vector_kernel(g, g, **okw(kind, ratio))) < 1e-13


@pytest.mark.parametrize("kind,ratio", C.CASES)
@pytest.mark.parametrize("na,m", HAND_SHAPES)
def test_tn_product(kind, ratio, na, m):
    """W = I: Σ = K(g, g) − K*·K*ᵀ, the TN product over every training row."""
    xa, g = hand_points(na, m)
    _, cov = E.predict_cov(hand_fit(kind, ratio, xa, 1.0), g)
    Ks = O.vector_kernel(g, xa, **okw(kind, ratio))
    assert rel(cov.cpu().numpy(), O.vector_kernel(g, g, **okw(kind, ratio)) - Ks @ Ks.T) < 1e-13


def raw_cov(gp, g, diag_add=0.0, ld_extra=0):
    """gp2d_predict_cov through the C ABI: the whole padded q × ldc buffer (NaN where not written)."""
    L = N.lib()
    G = torch.as_tensor(np.ascontiguousarray(g), device=DEV)
    m = G.shape[0]
    mp = E.padded_points(m)
    q = 2 * mp
    ldc = q + ld_extra
    wbytes = int(L.gp2d_predict_cov_workspace(gp.n, m))
    work = torch.empty(wbytes // 8 + 1, dtype=torch.float64, device=DEV)
    mean = torch.empty(2 * m, dtype=torch.float64, device=DEV)
    cov = torch.full((q, ldc), float("nan"), dtype=torch.float64, device=DEV)
    desc = gp.kernel.desc()
    N.check(L.gp2d_predict_cov(E._ptr(gp.W), gp.n, gp.n, E._ptr(gp.alpha), E._ptr(gp.x), gp.n_train, gp.n_pad,
                               E._ptr(G), m, ctypes.byref(desc), float(diag_add), E._ptr(mean), E._ptr(cov), ldc,
                               E._ptr(work), wbytes, E._stream_handle(DEV)), "gp2d_predict_cov")
    return cov.cpu().numpy(), m, mp


@pytest.mark.parametrize("na,m", HAND_SHAPES)
@pytest.mark.parametrize("ld_extra", [0, 1])
def test_raw_buffer_padding_and_symmetry(na, m, ld_extra):
    """The padded buffer as gp2d_potrf takes it: identity rows and columns for the padded points,
    exactly symmetric, nothing written past column q (also with an odd leading dimension)."""
    xa, g = hand_points(na, m)
    buf, m, mp = raw_cov(hand_fit("mixed", 0.35, xa, 1.0), g, diag_add=0.25, ld_extra=ld_extra)
    q = 2 * mp
    cov = buf[:, :q]
    assert np.isnan(buf[:, q:]).all() and not np.isnan(cov).any()
    assert np.array_equal(cov, cov.T)
    valid = np.r_[0:m, mp:mp + m]
    pad = np.setdiff1d(np.arange(q), valid)
    eye = np.eye(q)
    assert np.array_equal(cov[pad], eye[pad]) and np.array_equal(cov[:, pad], eye[:, pad])
    Ks = O.vector_kernel(g, xa, **okw("mixed", 0.35))
    ref = O.vector_kernel(g, g, **okw("mixed", 0.35)) - Ks @ Ks.T + 0.25 * np.eye(2 * m)
    assert rel(cov[np.ix_(valid, valid)], ref) < 1e-13


# ---- 2. posterior against the reference -----------------------------------------------------
def check_posterior(gp, n, m, kind, ratio, bit_identical_mean=True):
    g, ref, mo = reference(n, m, kind, ratio)
    kss = O.kernel_diag(**okw(kind, ratio))
    mean, cov = E.predict_cov(gp, g)
    pm, pv = E.predict(gp, g)
    pm0 = E.predict(gp, g, compute_var=False)[0]
    cov_h, mean_h = cov.cpu().numpy(), mean.cpu().numpy()
    ec, em = rel(cov_h, ref), rel(mean_h, mo)
    ed = float(np.max(np.abs(np.diag(cov_h) - pv.cpu().numpy()))) / kss
    lam = float(np.linalg.eigvalsh(cov_h)[0])
    print(f"{kind} N={n} m={m}: cov rel {ec:.2e}, mean rel {em:.2e}, diag vs predict {ed:.2e} kss, "
          f"smallest eigenvalue {lam:.3e} ({lam / kss:.2e} kss)")
    assert ec < 1e-10 and em < 1e-10
    assert ed <= 1e-12
    if bit_identical_mean:
        assert torch.equal(mean, pm0) and torch.equal(mean, pm)
    assert np.array_equal(cov_h, cov_h.T)
    assert lam >= -1e-12 * kss
    return cov_h


@pytest.mark.parametrize("kind,ratio", C.CASES)
@pytest.mark.parametrize("n,m", [(130, 130), (300, 200), (1000, 300)])
def test_posterior_vs_reference(kind, ratio, n, m):
    x, y = C.tracks(n)
    check_posterior(E.fit(spec(kind, ratio), x, y, NOISE), n, m, kind, ratio)


# ---- 3. more posterior cases -----------------------------------------------------------------
def test_posterior_from_ozaki_fit():
    """The ozaki fit keeps x, α and W in Morton order; predict_cov uses them as they are (the
    engine's own mean comes from the int8 path's K* kernel, so it is compared at the gate)."""
    x, y = C.tracks(300)
    gp = E.fit(spec("mixed", 0.35), x, y, NOISE, variance="ozaki")
    assert gp.perm is not None and gp.W is not None
    check_posterior(gp, 300, 200, "mixed", 0.35, bit_identical_mean=False)
    g = reference(300, 200, "mixed", 0.35)[0]
    assert rel(E.predict_cov(gp, g)[0].cpu().numpy(), E.predict(gp, g, compute_var=False)[0].cpu().numpy()) < 1e-10


def st_tracks(n, seed):
    """The (T, Y, X) tracks of test_gpu_fields.st_tracks: observations [v; u]."""
    rng = np.random.default_rng(seed)
    X = np.stack([rng.uniform(0, 6, n), rng.uniform(0, 45, n), rng.uniform(0, 60, n)], 1)
    v = np.cos(X[:, 2] / 9) + 0.1 * X[:, 0] + rng.normal(0, 0.05, n)
    u = np.sin(X[:, 1] / 7) - 0.05 * X[:, 0] + rng.normal(0, 0.05, n)
    return X, np.concatenate([v, u])


def test_posterior_spatio_temporal():
    import scipy.linalg as sla
    X, y = st_tracks(300, seed=300)
    rng = np.random.default_rng(1)
    G = np.stack([rng.uniform(-1, 7, 200), rng.uniform(-5, 50, 200), rng.uniform(-5, 65, 200)], 1)
    G[:5] = X[:5]
    assert G[:, 0].min() < 0 and G[:, 0].max() > 6          # times outside the tracks' [0, 6]
    kw = dict(kind="mixed", l_df=L_DF, l_cf=L_CF, ratio=0.35, var_t=2.0, l_t=1.5)
    K = O.vector_st_kernel(X, X, **kw)
    K[np.diag_indices_from(K)] += NOISE
    Lo = np.linalg.cholesky(K)
    alpha = sla.cho_solve((Lo, True), y)
    Ks = O.vector_st_kernel(G, X, **kw)
    ref = C.cov_from_factor(Lo, O.vector_st_kernel(G, G, **kw), Ks)
    gp = E.fit(E.KernelSpec(family="vector_st", **kw), X, y, NOISE)
    mean, cov = E.predict_cov(gp, G)
    cov_h = cov.cpu().numpy()
    ec, em = rel(cov_h, ref), rel(mean.cpu().numpy(), Ks @ alpha)
    print(f"st: cov rel {ec:.2e}, mean rel {em:.2e}")
    assert ec < 1e-10 and em < 1e-10
    assert torch.equal(mean, E.predict(gp, G, compute_var=False)[0])
    assert np.array_equal(cov_h, cov_h.T)


def test_diag_add_moves_only_the_diagonal():
    x, y = C.tracks(130)
    g = reference(130, 130, "df", 1.0)[0]
    gp = E.fit(spec("df", 1.0), x, y, NOISE)
    a = E.predict_cov(gp, g)[1].cpu().numpy()
    b = E.predict_cov(gp, g, diag_add=NOISE)[1].cpu().numpy()
    off = ~np.eye(260, dtype=bool)
    assert np.array_equal(a[off], b[off])
    # fl(k + noise) − acc against fl(k − acc), and the two subtractions here: four roundings of
    # values below 2⁻⁴, 2⁻⁵⁷ each
    assert np.max(np.abs(np.diag(b) - np.diag(a) - NOISE)) <= 1e-16


# ---- 4. jitchol -------------------------------------------------------------------------------
def test_jitchol_first_retry():
    A = torch.eye(256, dtype=torch.float64, device=DEV)
    A[200, 200] = -1e-8
    A0 = A.cpu().numpy()
    L, jit = E.jitchol(A)
    assert L is A
    assert jit == float(np.mean(np.diag(A0))) * 1e-6
    Lh = L.cpu().numpy()
    assert not np.triu(Lh, 1).any()
    assert rel(Lh @ Lh.T, A0 + jit * np.eye(256)) < 1e-14
    # a positive definite matrix takes no jitter
    L2, jit2 = E.jitchol(torch.eye(128, dtype=torch.float64, device=DEV) * 4.0)
    assert jit2 == 0.0 and torch.equal(L2, torch.eye(128, dtype=torch.float64, device=DEV) * 2.0)


def test_jitchol_gives_up():
    """−1 on the diagonal outlasts the schedule (1e-6 … 1e-2): a status word each time, then
    LinAlgError; the device goes on working."""
    A = torch.eye(256, dtype=torch.float64, device=DEV)
    A[200, 200] = -1.0
    with pytest.raises(np.linalg.LinAlgError):
        E.jitchol(A, maxtries=5)
    with pytest.raises(ValueError):
        E.jitchol(torch.eye(100, dtype=torch.float64, device=DEV))
    torch.cuda.synchronize()
    assert E.jitchol(torch.eye(128, dtype=torch.float64, device=DEV))[1] == 0.0


# ---- 5. sample_posterior ----------------------------------------------------------------------
def schedule(diag_mean, tries=5):
    return [0.0] + [diag_mean * 1e-6 * 10.0 ** t for t in range(tries)]


def on_schedule(jit, diag_mean):
    return any(jit == 0.0 if s == 0.0 else abs(jit / s - 1.0) < 1e-12 for s in schedule(diag_mean))


def test_samples_from_identity_normals_are_the_factor():
    x, y = C.tracks(300)
    g = C.targets(x, 100)
    gp = E.fit(spec("mixed", 0.35), x, y, NOISE)
    mean, cov = E.predict_cov(gp, g)
    z = torch.eye(200, dtype=torch.float64, device=DEV)
    samples, info = E.sample_posterior(gp, g, 200, z=z)
    assert samples.shape == (200, 200) and set(info) == {"jitter", "tries"}
    D = (samples - mean[None, :]).t().cpu().numpy()   # L in the component order
    assert not np.triu(D, 1).any()
    cov_h = cov.cpu().numpy()
    assert on_schedule(info["jitter"], float(np.mean(np.diag(cov_h))))
    assert rel(D @ D.T, cov_h + info["jitter"] * np.eye(200)) < 1e-12
    with pytest.raises(ValueError, match="shape"):
        E.sample_posterior(gp, g, 100, z=z)


def test_samples_on_a_dense_grid():
    """Σ of the 12 × 9 grid is singular to rounding (test_cov_cpu.test_dense_grid_needs_jitter):
    the call succeeds, with no jitter or with one of the schedule's values."""
    x, y = C.tracks(300)
    g = C.grid_points()
    gp = E.fit(E.KernelSpec(kind="df", l_df=5.0), x, y, NOISE)
    cov = E.predict_cov(gp, g)[1].cpu().numpy()
    samples, info = E.sample_posterior(gp, g, 16, seed=3)
    print(f"dense grid: jitter {info['jitter']:.3e} after {info['tries']} retries")
    assert samples.shape == (16, 216) and bool(torch.isfinite(samples).all())
    assert on_schedule(info["jitter"], float(np.mean(np.diag(cov))))
    assert (info["tries"] == 0) == (info["jitter"] == 0.0) and 0 <= info["tries"] <= 5
    again, _ = E.sample_posterior(gp, g, 16, seed=3)
    other, _ = E.sample_posterior(gp, g, 16, seed=4)
    assert torch.equal(samples, again) and not torch.equal(samples, other)


def test_sample_ensemble_covariance():
    """S = 4096 draws at 8 random targets: every entry of the sample covariance about the known
    mean within 6·√((Σ_ii·Σ_jj + Σ_ij²)/S) of the reference's Σ_ij (numpy normals pass the same
    check at ≤ 3.3σ, test_cov_cpu.test_ensemble_bound_holds_for_numpy_normals)."""
    x, y = C.tracks(300)
    g = C.targets(x, 8, seed=8)
    fit = O.OracleFit(x, y, "df", 5.0, L_CF, 1.0, NOISE)
    ref = C.posterior_cov(fit, g)
    gp = E.fit(E.KernelSpec(kind="df", l_df=5.0), x, y, NOISE)
    samples, info = E.sample_posterior(gp, g, 4096, seed=11)
    assert info["jitter"] == 0.0 and samples.shape == (4096, 16)
    d = samples.cpu().numpy() - C.posterior_mean(fit, g)[None, :]
    dev = np.abs(d.T @ d / 4096 - ref) / C.ensemble_bound(ref, 4096, k=1.0)
    print(f"largest deviation {dev.max():.2f} sigma")
    assert np.all(dev <= 6.0)


# ---- 6. surface and refusals -------------------------------------------------------------------
def test_krig_surface():
    x, y = C.tracks(1000, sd=0.0)
    kr = Krig(kernel="df", l_df=5.0, noise=NOISE).fit(x, y)
    pts = C.grid_points()
    M = pts.shape[0]
    mu, cov = kr.predict_cov(pts)
    assert isinstance(mu, np.ndarray) and mu.shape == (2 * M, 1) and cov.shape == (2 * M, 2 * M)
    assert np.array_equal(mu, kr.predict(pts, compute_var=False)[0])
    s = kr.sample(pts, 5, seed=2)
    assert isinstance(s, np.ndarray) and s.shape == (5, 2 * M)
    us, vs = kr.sample_grid(C.GRID_X, C.GRID_Y, 5, seed=2)
    assert us.shape == vs.shape == (5, 9, 12)
    # the flattening is predict_grid's: the same draws, laid out as uf and vf are
    assert np.array_equal(us, s[:, :M].reshape(5, 9, 12)) and np.array_equal(vs, s[:, M:].reshape(5, 9, 12))
    uf, vf, uvar, vvar = kr.predict_grid(C.GRID_X, C.GRID_Y)
    assert np.array_equal(uf, mu[:M, 0].reshape(9, 12)) and np.array_equal(vf, mu[M:, 0].reshape(9, 12))
    # and each draw stays within 6 posterior standard deviations (the retry's jitter included) of
    # the mean grid, point by point — the fields vary by far more across the grid
    jit = float(np.mean(np.diag(cov))) * 1e-2   # the schedule's last value bounds the jitter
    assert np.all(np.abs(us - uf[None]) <= 6.0 * np.sqrt(uvar + jit)[None])
    assert np.all(np.abs(vs - vf[None]) <= 6.0 * np.sqrt(vvar + jit)[None])


def test_refusals():
    x, y = C.tracks(130)
    gp = E.fit(spec("df", 1.0), x, y, NOISE)
    g = C.targets(x, 10)
    ard = E.KernelSpec(family="ard", variances=(1.0,), lengthscales=((5.0, 5.0),))
    for call in (lambda f: E.predict_cov(f, g), lambda f: E.sample_posterior(f, g, 3)):
        with pytest.raises(ValueError, match="vector kernel"):
            call(dataclasses.replace(gp, kernel=E.KernelSpec(kind="scalar")))
        with pytest.raises(ValueError, match="vector kernel"):
            call(dataclasses.replace(gp, kernel=ard))
        with pytest.raises(ValueError, match="W"):
            call(dataclasses.replace(gp, W=None, n_mat=gp.n))
    sc = Krig(kernel="scalar", l_df=5.0, noise=NOISE).fit(x, y)
    with pytest.raises(ValueError, match="vector kernel"):
        sc.predict_cov(g)
    with pytest.raises(ValueError, match="vector kernel"):
        sc.sample(g, 2)
