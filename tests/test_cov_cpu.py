"""Joint posterior covariance, the parts that need no device: the numpy reference tests/cov_ref.py
against the oracle, how far the reference's two recipes are apart on the GPU tests' inputs (so
that test_gpu_cov.py's 1e-10 gate hides nothing), the conditioning of Σ on random targets and on a
dense grid, the ensemble bound of the sampling test on numpy normals, and gp2d_predict_cov's
argument checks."""
import ctypes
import functools

import numpy as np
import pytest

import cov_ref as C
from oracle import gp2d_oracle as O

SHAPES = [(130, 100), (130, 130), (300, 200), (1000, 300)]   # (N, m)


@functools.lru_cache(maxsize=None)
def fits(n, kind, ratio):
    x, y = C.tracks(n)
    return (O.OracleFit(x, y, kind, C.L_DF, C.L_CF, ratio, C.NOISE),
            O.OracleFit(x, y, kind, C.L_DF, C.L_CF, ratio, C.NOISE, method="inv"))


@functools.lru_cache(maxsize=None)
def sigma(n, m, kind, ratio):
    g = C.targets(C.tracks(n)[0], m)
    return g, C.posterior_cov(fits(n, kind, ratio)[0], g)


@pytest.mark.parametrize("kind,ratio", C.CASES)
@pytest.mark.parametrize("n,m", SHAPES)
def test_helper_diagonal_is_the_oracle_variance(kind, ratio, n, m):
    fit = fits(n, kind, ratio)[0]
    g, cov = sigma(n, m, kind, ratio)
    kss = O.kernel_diag(**fit.kw)
    mu, var = fit.predict(g)
    assert cov.shape == (2 * m, 2 * m)
    assert np.max(np.abs(np.diag(cov) - var)) <= 1e-12 * kss
    assert np.max(np.abs(C.posterior_mean(fit, g) - mu)) <= 1e-12 * np.max(np.abs(mu))
    assert np.array_equal(C.prior(fit.kw, g), C.prior(fit.kw, g).T)


@pytest.mark.parametrize("kind,ratio", C.CASES)
@pytest.mark.parametrize("n,m", SHAPES)
def test_recipes_agree(kind, ratio, n, m):
    """chol (what the library computes) against GP_laser's inv recipe: ≤ 8.4e-14 normwise."""
    g, a = sigma(n, m, kind, ratio)
    b = C.posterior_cov(fits(n, kind, ratio)[1], g, recipe="inv")
    spread = np.max(np.abs(a - b)) / np.max(np.abs(a))
    print(f"{kind} N={n} m={m}: chol vs inv {spread:.2e}")
    assert spread < 1e-12


@pytest.mark.parametrize("kind,ratio", C.CASES)
@pytest.mark.parametrize("n,m", SHAPES)
def test_random_targets_stay_positive_definite(kind, ratio, n, m):
    _, cov = sigma(n, m, kind, ratio)
    lam = np.linalg.eigvalsh(0.5 * (cov + cov.T))[0]
    print(f"{kind} N={n} m={m}: smallest eigenvalue {lam:.3e}")
    assert lam >= 1.5e-12
    np.linalg.cholesky(cov)   # no jitter needed


def test_dense_grid_needs_jitter():
    """12 × 9 points half a unit apart under ℓ = 5: Σ is singular to rounding (smallest eigenvalue
    −3.6e-16 here), plain Cholesky fails and 1e-10·mean(diag) repairs it — far below the first step
    of the jitchol schedule (1e-6), so sample_posterior's retry always ends at its first step."""
    x, y = C.tracks(300)
    fit = O.OracleFit(x, y, "df", 5.0, C.L_CF, 1.0, C.NOISE)
    cov = C.posterior_cov(fit, C.grid_points())
    lam = np.linalg.eigvalsh(0.5 * (cov + cov.T))
    print(f"dense grid: eigenvalues {lam[0]:.3e} .. {lam[-1]:.3e}")
    assert abs(lam[0]) < 1e-14 and lam[-1] > 0.1
    with pytest.raises(np.linalg.LinAlgError):
        np.linalg.cholesky(cov)
    np.linalg.cholesky(cov + 1e-10 * np.mean(np.diag(cov)) * np.eye(cov.shape[0]))


def test_ensemble_bound_holds_for_numpy_normals():
    """The sampling test's check on the reference itself: m = 8 random targets, S = 4096 draws
    L·z of numpy normals; every entry of the sample covariance within the 6σ bound, with room
    (the largest deviation over five seeds is 3.3σ)."""
    x, y = C.tracks(300)
    fit = O.OracleFit(x, y, "df", 5.0, C.L_CF, 1.0, C.NOISE)
    cov = C.posterior_cov(fit, C.targets(x, 8, seed=8))
    L = np.linalg.cholesky(cov)
    one_sigma = C.ensemble_bound(cov, 4096, k=1.0)
    for seed in range(5):
        d = L @ np.random.default_rng(seed).standard_normal((16, 4096))
        worst = np.max(np.abs(d @ d.T / 4096 - cov) / one_sigma)
        print(f"seed {seed}: largest deviation {worst:.2f} sigma")
        assert worst < 4.5


def test_predict_cov_argument_errors():
    from gp2d import _native as N
    L = N.lib()
    one = ctypes.c_void_p(1)   # never dereferenced: the argument checks fail first
    big = 1 << 40
    k = N.vector_kernel_desc(N.KIND_DIVFREE, 5.0)

    def call(kern=k, n=256, ntr_pad=128, m=100, ldc=256, wbytes=big):
        return L.gp2d_predict_cov(one, n, n, one, one, 100, ntr_pad, one, m, ctypes.byref(kern), 0.0, one, one,
                                  ldc, one, wbytes, None)

    assert L.gp2d_predict_cov_workspace(256, 100) == 8 * (2 * 256 * 256 + 3 * 256)
    assert L.gp2d_predict_cov_workspace(384, 130) == 8 * (2 * 384 * 384 + 4 * 384)
    rc = call(n=384)
    assert rc < 0 and b"n must equal 2" in L.gp2d_last_error()
    rc = call(ldc=255)
    assert rc < 0 and b"ldc" in L.gp2d_last_error()
    rc = call(wbytes=L.gp2d_predict_cov_workspace(256, 100) - 1)
    assert rc < 0 and b"workspace" in L.gp2d_last_error()
    rc = call(kern=N.vector_kernel_desc(N.KIND_SCALAR, 5.0))
    assert rc < 0 and b"vector kernels only" in L.gp2d_last_error()
    rc = call(kern=N.ard_kernel_desc([1.0], [[5.0, 5.0]]))
    assert rc < 0 and b"vector kernels only" in L.gp2d_last_error()
    rc = call(kern=N.vector_kernel_desc(N.KIND_DIVFREE, -1.0))
    assert rc < 0 and b"l_df" in L.gp2d_last_error()
    assert call(m=0) == 0   # nothing to predict
