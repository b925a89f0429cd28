"""numpy float64 reference for the leave-one-out objective and its gradient (gp2d_loo_grad): a plain
helper module of tests/test_loo_cpu.py and tests/test_gpu_loo.py.

With P = K_y⁻¹, α = P·y and P_ii the bd × bd diagonal block of point i (cv_ref's conventions):
    Σ_i = P_ii⁻¹,  r_i = Σ_i·α_i,  lpd_i = log N(r_i; 0, Σ_i),  L_LOO = Σ_i lpd_i
    ∂L_LOO/∂θ = ½ tr((α sᵀ + s αᵀ − P·D·P) ∂K_y/∂θ),  s = P·r,  D = blockdiag(r_i r_iᵀ + Σ_i)
(Rasmussen & Williams §5.4.2).  Two independent routes: the closed forms above from one inverse of
K_y (value_grad_from_K), and the brute force (loo_refit): remove point i, refit, take the density of
the held-out observation.  The derivative matrices are sum_ref's analytic ones for the vector and
spatio-temporal families and the ARD RBF's own.  Gradients are in the library's order, noise last.
"""
import numpy as np

import cv_ref as C
import sum_ref as S
from oracle import gp2d_oracle as O


def value_grad_from_K(K, y, bd, dKs):
    """(L_LOO, gradient) from K_y, the stacked observations and the list of ∂K_y/∂θ matrices without
    the noise's (the identity), whose entry comes last."""
    n = K.shape[0] // bd
    Li = np.linalg.inv(np.linalg.cholesky(K))
    P = Li.T @ Li
    alpha = P @ y
    value, r, D = 0.0, np.zeros(bd * n), np.zeros_like(K)
    for i in range(n):
        idx = C.components([i], n, bd)
        mean, cov, lpd = C.closed_group(P, alpha, y, idx)
        value += lpd
        r[idx] = y[idx] - mean
        D[np.ix_(idx, idx)] = np.outer(r[idx], r[idx]) + cov
    s = P @ r
    M = np.outer(alpha, s) + np.outer(s, alpha) - P @ D @ P
    g = [0.5 * np.sum(M * dK) for dK in dKs] + [0.5 * np.trace(M)]
    return float(value), np.array(g)


def value_from_K(K, y, bd):
    """L_LOO alone, the 1 × 1 / 2 × 2 blocks in closed form (what an optimiser of the value calls)."""
    n = K.shape[0] // bd
    Li = np.linalg.inv(np.linalg.cholesky(K))
    P = Li.T @ Li
    alpha = P @ y
    i = np.arange(n)
    if bd == 1:
        p = P[i, i]
        return float(np.sum(-0.5 * alpha * alpha / p + 0.5 * np.log(p)) - 0.5 * n * C.LOG_2PI)
    puu, pvu, pvv = P[i, i], P[n + i, i], P[n + i, n + i]
    au, av = alpha[:n], alpha[n:]
    det = puu * pvv - pvu * pvu
    quad = (pvv * au * au - 2.0 * pvu * au * av + puu * av * av) / det   # α_iᵀ·P_ii⁻¹·α_i
    return float(np.sum(-0.5 * quad + 0.5 * np.log(det)) - n * C.LOG_2PI)


def loo_refit(K, y, bd):
    """The brute force: Σ_i log p(y_i | y_−i) by one refit per held-out point."""
    n = K.shape[0] // bd
    return float(sum(C.refit_without(K, y, C.components([i], n, bd))[2] for i in range(n)))


# ---------------------------------------------------------------- vector and spatio-temporal families
def loo_value_grad(terms, weights, x, y, noise):
    """A sum of vector kernels (sum_ref's term dicts): (L_LOO, gradient) in the library's order, per
    term (weight_t, l_df_t, l_cf_t, ratio_t[, var_t_t, l_t_t]), then noise."""
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64).reshape(-1)
    return value_grad_from_K(S.ky(terms, weights, x, noise), y, 2, S.grad_matrices(terms, weights, x, x))


def loo_value_grad_single(term, x, y, noise):
    """One vector kernel that is not a sum: the library's order has no weight entry."""
    val, g = loo_value_grad([term], [1.0], x, y, noise)
    return val, g[1:]


def loo_refit_sum(terms, weights, x, y, noise):
    return loo_refit(S.ky(terms, weights, np.asarray(x, dtype=np.float64), noise), np.asarray(y).reshape(-1), 2)


# ---------------------------------------------------------------- ARD
def ard_ky(X, variances, lengthscales, noise):
    K = O.ard_rbf(X, X, variances, lengthscales)
    return K + noise * np.eye(K.shape[0])


def ard_grad_matrices(X, variances, lengthscales):
    """∂K/∂(var_t, ls_t0..) per term: ∂k/∂var_t = e_t, ∂k/∂ls_td = var_t·e_t·Δ_d²/ls_td³."""
    X = np.atleast_2d(np.asarray(X, dtype=np.float64))
    out = []
    for v, ls in zip(variances, lengthscales):
        e = O.ard_rbf(X, X, [1.0], [ls])
        out.append(e)
        for d in range(X.shape[1]):
            D2 = np.square(X[:, d][:, None] - X[:, d][None, :])
            out.append(v * e * D2 / ls[d] ** 3)
    return out


def ard_value_grad(X, y, variances, lengthscales, noise):
    """(L_LOO, gradient) of Σ_t var_t·RBF(ls_t) + noise: per term (var_t, ls_t[0..D)), then noise."""
    X = np.atleast_2d(np.asarray(X, dtype=np.float64))
    y = np.asarray(y, dtype=np.float64).reshape(-1)
    return value_grad_from_K(ard_ky(X, variances, lengthscales, noise), y, 1,
                             ard_grad_matrices(X, variances, lengthscales))


def ard_refit(X, y, variances, lengthscales, noise):
    X = np.atleast_2d(np.asarray(X, dtype=np.float64))
    return loo_refit(ard_ky(X, variances, lengthscales, noise), np.asarray(y, dtype=np.float64).reshape(-1), 1)


# ---------------------------------------------------------------- the shared cases of both test files
def term(kind, l_df=C.L_DF, l_cf=C.L_CF, ratio=C.RATIO, st=False):
    """A sum_ref term dict at cv_ref's shared settings; a df or cf kind carries the library's ratio."""
    t = dict(kind=kind, l_df=l_df, l_cf=l_cf, ratio={"df": 1.0, "cf": 0.0}.get(kind, ratio))
    if st:
        t.update(var_t=C.VAR_T, l_t=C.L_T)
    return t


SUM_TERMS = [term("df", l_df=9.0), term("mixed", l_df=3.0, l_cf=4.0, ratio=0.4)]
SUM_WEIGHTS = [0.7, 0.3]


def data(n, dim=2, bd=2):
    """cv_ref's seeded points and observations."""
    x = C.points(n, dim=dim)
    return x, C.observations(x, bd)


def rel(a, b):
    """The project's gradient norm: largest deviation over largest entry."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.max(np.abs(a - b)) / max(np.max(np.abs(b)), 1e-300))
