"""numpy reference for the joint posterior covariance of the vector GP at a set of target points:
a plain helper module of tests/test_cov_cpu.py and tests/test_gpu_cov.py.

    Σ = Kss − Ks·K_y⁻¹·Ksᵀ,   Kss = K(g, g),  Ks = K(g, x)        (GP_laser.py:128-129)

component-major like every matrix of the oracle: rows and columns [u(g_1..g_m), v(g_1..g_m)].
Two recipes: 'chol' — V = solve_triangular(L, Ksᵀ), Σ = Kss − VᵀV, what the library computes with
W = L⁻¹ (and sklearn's predict(return_cov=True), _gpr.py:454-460); 'inv' — the reference's own
np.dot(Ks, np.dot(Ki, Ks.T)) with Ki = np.linalg.inv(K_y).  test_cov_cpu.py measures how far the two
are apart on the GPU tests' inputs.
"""
import numpy as np

from oracle import gp2d_oracle as O


L_DF, L_CF, NOISE = 5.0, 4.0, 0.01
CASES = [("df", 1.0), ("cf", 0.0), ("mixed", 0.35)]
# the dense 12 × 9 grid of test_gpu_fields.test_krig_predict_fields_grid
GRID_X, GRID_Y = 10.0 + 0.5 * np.arange(12), 40.0 + 0.5 * np.arange(9)


def tracks(n, sd=0.05):
    """The observations of test_gpu_fields.tracks (that module needs a device to import)."""
    rng = np.random.default_rng(n)
    x = np.stack([rng.uniform(0, 45, n), rng.uniform(0, 60, n)], 1)
    y = np.concatenate([np.sin(x[:, 1] / 7), np.cos(x[:, 0] / 9)]) + sd * rng.normal(0, 1, 2 * n)
    return x, y


def targets(x, m=700, seed=1):
    """test_gpu_fields.targets: m points on [−5, 50] × [−5, 65], the first five on training points."""
    rng = np.random.default_rng(seed)
    g = np.stack([rng.uniform(-5, 50, m), rng.uniform(-5, 65, m)], 1)
    k = min(5, x.shape[0]) if m > 5 else 0
    g[:k] = x[:k]
    return g


def grid_points():
    X, Y = np.meshgrid(GRID_X, GRID_Y)
    return np.stack([X.reshape(-1), Y.reshape(-1)], 1)


def prior(fit_kw, g, st=None):
    """K(g, g) of an OracleFit's kernel keywords (st: dict(var_t, l_t) for the (t, x1, x2) product)."""
    return O.vector_kernel(g, g, **fit_kw) if st is None else O.vector_st_kernel(g, g, **fit_kw, **st)


def cross(fit_kw, g, x, st=None):
    """Ks = K(g, x): (2m, 2N)."""
    return O.vector_kernel(g, x, **fit_kw) if st is None else O.vector_st_kernel(g, x, **fit_kw, **st)


def cov_from_factor(L, Kss, Ks):
    """Kss − VᵀV with V = L⁻¹·Ksᵀ for a lower Cholesky factor L of K_y."""
    import scipy.linalg as sla
    V = sla.solve_triangular(L, Ks.T, lower=True)
    return Kss - V.T @ V


def cov_from_inverse(Ki, Kss, Ks):
    """The GP_laser recipe: Kss − np.dot(Ks, np.dot(Ki, Ks.T))."""
    return Kss - np.dot(Ks, np.dot(Ki, Ks.T))


def posterior_cov(fit, xg, recipe="chol"):
    """Joint latent covariance (2m, 2m) of an oracle.OracleFit at the points xg.  recipe 'chol'
    needs a fit made with method='chol', recipe 'inv' one made with method='inv'."""
    xg = np.asarray(xg, dtype=np.float64).reshape(-1, 2)
    Kss, Ks = prior(fit.kw, xg), cross(fit.kw, xg, fit.x)
    if recipe == "inv":
        return cov_from_inverse(fit.Ki, Kss, Ks)
    return cov_from_factor(fit.L, Kss, Ks)


def posterior_mean(fit, xg):
    xg = np.asarray(xg, dtype=np.float64).reshape(-1, 2)
    return cross(fit.kw, xg, fit.x) @ fit.alpha


def ensemble_bound(cov, n_samples, k=6.0):
    """Entrywise k-sigma bound on |sample covariance − Σ| for n_samples zero-mean Gaussian draws:
    Var(x_i·x_j) = Σ_ii·Σ_jj + Σ_ij² (Isserlis), so the mean of S products has standard deviation
    √((Σ_ii·Σ_jj + Σ_ij²)/S)."""
    d = np.diag(cov)
    return k * np.sqrt((np.outer(d, d) + cov * cov) / n_samples)
