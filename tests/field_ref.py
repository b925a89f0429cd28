"""numpy reference for the derived fields of the vector GP (divergence, vorticity): a plain
helper module of tests/test_fields_cpu.py and tests/test_gpu_fields.py.

Points are (x1, x2), components (f1, f2) = the first and second half of the observation vector.
    divergence δ = ∂f1/∂x1 + ∂f2/∂x2,    vorticity ζ = ∂f2/∂x1 − ∂f1/∂x2.
With d = x − g (training minus target point), r² = d1² + d2² and
    h_p(d; ℓ) = exp(−r²/2ℓ²) · d_p · (4 − r²/ℓ²) / ℓ⁴:
    cov(f_p(x), δ(g)) = w_cf · h_p(d; ℓ_cf)
    cov(f_1(x), ζ(g)) = −w_df · h_2(d; ℓ_df),   cov(f_2(x), ζ(g)) = +w_df · h_1(d; ℓ_df)
    Var δ = 8·w_cf/ℓ_cf⁴,   Var ζ = 8·w_df/ℓ_df⁴
(w_df, w_cf) = (1, 0) | (0, 1) | (ratio, 1 − ratio) for df | cf | mixed.  The spatio-temporal
product (points (t, x1, x2)) multiplies the cross-covariances by var_t·exp(−Δt²/2ℓ_t²) and the
prior variances by var_t.  test_fields_cpu.py checks these closed forms against central
differences of oracle.vector_kernel.
"""
import numpy as np

FIELDS = ("divergence", "vorticity")


def weights(kind, ratio):
    """(w_df, w_cf) of a kind 'df' | 'cf' | 'mixed'."""
    return {"df": (1.0, 0.0), "cf": (0.0, 1.0), "mixed": (ratio, 1.0 - ratio)}[kind]


def _h(d1, d2, length):
    c = (d1 * d1 + d2 * d2) / length ** 2
    s = np.exp(-0.5 * c) * (4.0 - c) / length ** 4
    return s * d1, s * d2


def cross(xa, g, field, kind, l_df, l_cf, ratio, var_t=None, l_t=None):
    """(2N, M) covariance of the observations [f1(xa); f2(xa)] with `field` at the points g.
    var_t, l_t: the spatio-temporal product; xa and g then carry t in their first column."""
    assert field in FIELDS
    xa, g = np.asarray(xa, dtype=np.float64), np.asarray(g, dtype=np.float64)
    tf = 1.0
    if var_t is not None:
        tf = var_t * np.exp(-0.5 * np.square(xa[:, 0][:, None] - g[:, 0][None, :]) / l_t ** 2)
        xa, g = xa[:, 1:], g[:, 1:]
    d1 = xa[:, 0][:, None] - g[:, 0][None, :]
    d2 = xa[:, 1][:, None] - g[:, 1][None, :]
    w_df, w_cf = weights(kind, ratio)
    if field == "divergence":
        h1, h2 = _h(d1, d2, l_cf)
        return np.concatenate([w_cf * h1 * tf, w_cf * h2 * tf], 0)
    h1, h2 = _h(d1, d2, l_df)
    return np.concatenate([-w_df * h2 * tf, w_df * h1 * tf], 0)


def prior_var(field, kind, l_df, l_cf, ratio, var_t=None):
    assert field in FIELDS
    w_df, w_cf = weights(kind, ratio)
    v = 8.0 * w_cf / l_cf ** 4 if field == "divergence" else 8.0 * w_df / l_df ** 4
    return v * (1.0 if var_t is None else var_t)


def fit_predict_field(L, alpha, xa, g, field, kind, l_df, l_cf, ratio, var_t=None, l_t=None):
    """Posterior of `field` at g from a Cholesky fit of the velocity observations (oracle.OracleFit's
    L and alpha, or any lower factor of K_y with alpha = K_y⁻¹y): mean = Cᵀα, var = prior − ‖L⁻¹C‖²."""
    import scipy.linalg as sla
    C = cross(xa, g, field, kind, l_df, l_cf, ratio, var_t, l_t)
    V = sla.solve_triangular(L, C, lower=True)
    return C.T @ alpha, prior_var(field, kind, l_df, l_cf, ratio, var_t) - np.einsum("ij,ij->j", V, V)
