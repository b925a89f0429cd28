"""numpy reference for the velocity gradient tensor of the vector GP: a plain helper module of
tests/test_grad_cpu.py and tests/test_gpu_grad.py.

Points are (x1, x2), components (f1, f2) = the first and second half of the observation vector.
    ∇f = (g0, g1, g2, g3) = (∂f1/∂x1, ∂f1/∂x2, ∂f2/∂x1, ∂f2/∂x2),  component c = 2a + b
(a the field component, b the direction).  With d = x − g (training minus target point),
r² = d1² + d2², a = 1/ℓ² and E = exp(−a r²/2):
    T_pqb(d; ℓ) = E·[a²(δ_pq d_b + δ_pb d_q + δ_qb d_p) − a³ d_p d_q d_b]
    h_b(d; ℓ)   = Σ_c T_ccb = E·a²·d_b·(4 − a r²)
    cov(f_p(x), ∂f_a/∂x_b (g)) = w_cf·T_pab(d; ℓ_cf) + w_df·(δ_pa·h_b(d; ℓ_df) − T_pab(d; ℓ_df))
    cov(∂_b f_a, ∂_d f_c)(0)   = w_cf/ℓ_cf⁴·S_acbd + w_df/ℓ_df⁴·(4 δ_ac δ_bd − S_acbd),
    S_pqbd = δ_pq δ_bd + δ_pb δ_qd + δ_pd δ_qb
(w_df, w_cf) = (1, 0) | (0, 1) | (ratio, 1 − ratio) for df | cf | mixed.  The spatio-temporal
product (points (t, x1, x2)) multiplies the cross-covariances by var_t·exp(−Δt²/2ℓ_t²) and the
prior by var_t.  test_grad_cpu.py checks these closed forms against central differences of
oracle.vector_kernel.  The tensors are formed from the index formulas as written, with einsum over
Kronecker deltas, not from expanded per-component expressions.
"""
import numpy as np

from field_ref import weights

COMPONENTS = ("du_dx", "du_dy", "dv_dx", "dv_dy")
# the linear diagnostics as aᵀ∇f
LINEAR = {"divergence": np.array([1.0, 0.0, 0.0, 1.0]), "vorticity": np.array([0.0, -1.0, 1.0, 0.0]),
          "normal_strain": np.array([1.0, 0.0, 0.0, -1.0]), "shear_strain": np.array([0.0, 1.0, 1.0, 0.0])}
# Okubo–Weiss (g0 − g3)² + 4·g1·g2 = gᵀAg
OW = np.array([[1.0, 0, 0, -1], [0, 0, 2, 0], [0, 2, 0, 0], [-1, 0, 0, 1.0]])

_I2 = np.eye(2)


def _T(d, length):
    """T_pqb at the lags d (N, M, 2): (2, 2, 2, N, M)."""
    a = 1.0 / length ** 2
    E = np.exp(-0.5 * a * np.sum(d * d, -1))
    lin = (np.einsum("pq,nmb->pqbnm", _I2, d) + np.einsum("pb,nmq->pqbnm", _I2, d)
           + np.einsum("qb,nmp->pqbnm", _I2, d))
    cub = np.einsum("nmp,nmq,nmb->pqbnm", d, d, d)
    return E * (a ** 2 * lin - a ** 3 * cub)


def cross(xa, g, kind, l_df, l_cf, ratio, var_t=None, l_t=None):
    """(2N, M, 4) covariance of the observations [f1(xa); f2(xa)] with the four components of ∇f at
    the points g.  var_t, l_t: the spatio-temporal product; xa and g then carry t in their first
    column."""
    xa, g = np.asarray(xa, dtype=np.float64), np.asarray(g, dtype=np.float64)
    tf = 1.0
    if var_t is not None:
        tf = var_t * np.exp(-0.5 * np.square(xa[:, 0][:, None] - g[:, 0][None, :]) / l_t ** 2)
        xa, g = xa[:, 1:], g[:, 1:]
    d = xa[:, None, :] - g[None, :, :]
    w_df, w_cf = weights(kind, ratio)
    C = np.zeros((2, 2, 2) + d.shape[:2])           # [p, a, b, n, m]
    if w_cf != 0.0:
        C += w_cf * _T(d, l_cf)
    if w_df != 0.0:
        T = _T(d, l_df)
        h = np.einsum("ccbnm->bnm", T)
        C += w_df * (np.einsum("pa,bnm->pabnm", _I2, h) - T)
    C = C * tf
    n, m = d.shape[:2]
    return C.transpose(0, 3, 4, 1, 2).reshape(2 * n, m, 4)


def prior(kind, l_df, l_cf, ratio, var_t=None):
    """(4, 4) prior covariance of ∇f at one point."""
    w_df, w_cf = weights(kind, ratio)
    S = (np.einsum("ac,bd->abcd", _I2, _I2) + np.einsum("ab,cd->abcd", _I2, _I2)
         + np.einsum("ad,cb->abcd", _I2, _I2))
    D = 4.0 * np.einsum("ac,bd->abcd", _I2, _I2)
    P = np.zeros((2, 2, 2, 2))
    if w_cf != 0.0:
        P += w_cf / l_cf ** 4 * S
    if w_df != 0.0:
        P += w_df / l_df ** 4 * (D - S)
    return P.reshape(4, 4) * (1.0 if var_t is None else var_t)


def fit_predict_grad(L, alpha, xa, g, kind, l_df, l_cf, ratio, var_t=None, l_t=None):
    """Posterior of ∇f at g from a Cholesky fit of the velocity observations (oracle.OracleFit's L
    and alpha, or any lower factor of K_y with alpha = K_y⁻¹y): mean (M, 4) = Cᵀα and cov
    (M, 4, 4) = prior − VᵀV per point, V = L⁻¹C."""
    import scipy.linalg as sla
    C = cross(xa, g, kind, l_df, l_cf, ratio, var_t, l_t)
    n2, m, _ = C.shape
    V = sla.solve_triangular(L, C.reshape(n2, 4 * m), lower=True).reshape(n2, m, 4)
    return np.einsum("nmc,n->mc", C, alpha), prior(kind, l_df, l_cf, ratio, var_t) - np.einsum("nma,nmb->mab", V, V)


def diagnostics(mean, cov):
    """{name: (mean, var)} of the linear diagnostics and the Okubo–Weiss parameter from (…, 4)
    means and (…, 4, 4) covariances: aᵀμ, aᵀΣa; μᵀAμ + tr(AΣ), 2·tr(AΣAΣ) + 4·μᵀAΣAμ."""
    out = {k: (mean @ a, np.einsum("a,...ab,b->...", a, cov, a)) for k, a in LINEAR.items()}
    AS = OW @ cov
    Am = mean @ OW
    out["okubo_weiss"] = (np.einsum("...a,...a->...", Am, mean) + np.trace(AS, axis1=-2, axis2=-1),
                          2.0 * np.trace(AS @ AS, axis1=-2, axis2=-1) + 4.0 * np.einsum("...a,...ab,...b->...", Am, cov, Am))
    return out
