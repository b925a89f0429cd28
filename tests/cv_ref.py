"""numpy float64 reference for the cross-validation entries (gp2d_cv_points, gp2d_cv_groups).

K_y comes from the oracle's kernels; two independent routes to a held-out prediction:
  * the closed forms from one Cholesky of K_y — with P = K_y⁻¹ and α = P·y, the observations y_G
    given all the others are N(y_G − P_GG⁻¹·α_G, P_GG⁻¹) (Rasmussen & Williams §5.4.2, block form);
  * the brute force the reference performs: remove G, refit, predict at G (refit_without).
Components are stacked [u…, v…] (bd·N entries); a group is an array of POINT indices and holds
every component of its points.

Shared settings of the tests: mixed kernel, ℓ_df = 5, ℓ_cf = 7, ratio 0.6, noise 0.0025, points
uniform in [0, 40]², seeded.
"""
import functools

import numpy as np

from oracle import gp2d_oracle as O

L_DF, L_CF, RATIO, NOISE = 5.0, 7.0, 0.6, 0.0025
ARD_VARIANCES, ARD_LENGTHSCALES = (0.8, 0.2), ((5.0, 7.0), (12.0, 9.0))
VAR_T, L_T = 1.0, 3.0
LOG_2PI = float(np.log(2.0 * np.pi))


def points(n, seed=2016, dim=2):
    """n points uniform in [0, 40]² (dim 3: a leading time column uniform in [0, 6])."""
    rng = np.random.default_rng(seed + n)
    xy = rng.uniform(0.0, 40.0, (n, 2))
    if dim == 2:
        return xy
    return np.concatenate([rng.uniform(0.0, 6.0, (n, 1)), xy], 1)


def observations(x, bd, seed=7):
    """A smooth field at the last two columns of x plus N(0, 0.05²) noise, stacked [u…, v…]."""
    rng = np.random.default_rng(seed + x.shape[0])
    a, b = x[:, -2], x[:, -1]
    f = [np.sin(b / 7.0) + 0.3 * np.cos(a / 5.0), np.cos(a / 9.0) - 0.2 * np.sin(b / 6.0)][:bd]
    return np.concatenate(f) + rng.normal(0.0, 0.05, bd * x.shape[0])


def ky(family, x, noise=NOISE):
    """(K_y, bd) of the shared settings for a kernel family."""
    if family == "vector2d":
        K, bd = O.vector_kernel(x, x, kind="mixed", l_df=L_DF, l_cf=L_CF, ratio=RATIO), 2
    elif family == "ard":
        K, bd = O.ard_rbf(x, x, ARD_VARIANCES, ARD_LENGTHSCALES), 1
    elif family == "vector_st":
        K, bd = O.vector_st_kernel(x, x, kind="mixed", l_df=L_DF, l_cf=L_CF, ratio=RATIO, var_t=VAR_T, l_t=L_T), 2
    else:
        raise ValueError(family)
    return K + noise * np.eye(K.shape[0]), bd


@functools.lru_cache(maxsize=None)
def problem(family, n):
    """(x, y, K_y, bd, P, α) of the shared settings; computed once, read-only."""
    x = points(n, dim=3 if family == "vector_st" else 2)
    K, bd = ky(family, x)
    y = observations(x, bd)
    Li = np.linalg.inv(np.linalg.cholesky(K))
    P = Li.T @ Li
    out = (x, y, K, bd, P, P @ y)
    for a in out:
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return out


def components(G, n, bd):
    """Indices into the stacked vector of every component of the points G."""
    G = np.asarray(G, dtype=np.int64).reshape(-1)
    return np.concatenate([c * n + G for c in range(bd)])


def log_density(r, cov):
    """log N(r; 0, cov)."""
    L = np.linalg.cholesky(cov)
    z = np.linalg.solve(L, r)
    return float(-0.5 * z @ z - np.sum(np.log(np.diag(L))) - 0.5 * r.size * LOG_2PI)


def closed_group(P, alpha, y, idx):
    """(mean, cov, lpd) of y[idx] given the rest, from the precision matrix."""
    cov = np.linalg.inv(P[np.ix_(idx, idx)])
    cov = 0.5 * (cov + cov.T)
    r = cov @ alpha[idx]
    return y[idx] - r, cov, log_density(r, cov)


def refit_without(K, y, idx):
    """The brute force: drop the observations idx, refit on the rest, predict the dropped
    observations (noise included).  (mean, cov, lpd)."""
    keep = np.setdiff1d(np.arange(K.shape[0]), idx)
    L = np.linalg.cholesky(K[np.ix_(keep, keep)])
    A = np.linalg.solve(L, K[np.ix_(keep, idx)])
    mean = A.T @ np.linalg.solve(L, y[keep])
    cov = K[np.ix_(idx, idx)] - A.T @ A
    cov = 0.5 * (cov + cov.T)
    return mean, cov, log_density(y[idx] - mean, cov)


def scores(resid, lpd_sum, chi2_sum, npts, n, bd):
    """The host scores of engine.cv_points / cv_groups from residuals stacked [u…, v…] (NaN for
    points that were not held out)."""
    r = resid.reshape(bd, n)
    return dict(rmse_u=float(np.sqrt(np.nansum(r[0] ** 2) / npts)),
                rmse_v=float(np.sqrt(np.nansum(r[1] ** 2) / npts)) if bd == 2 else 0.0,
                mean_lpd=float(lpd_sum / npts), msll_chi2=float(chi2_sum / npts))


@functools.lru_cache(maxsize=None)
def cv_points(family, n):
    """Closed-form leave-one-point-out results: dict mean, var, cuv, lpd, resid + the scores."""
    _, y, _, bd, P, alpha = problem(family, n)
    mean, var = np.empty(bd * n), np.empty(bd * n)
    cuv, lpd = np.zeros(n), np.empty(n)
    chi2 = 0.0
    for i in range(n):
        idx = components([i], n, bd)
        m, c, lpd[i] = closed_group(P, alpha, y, idx)
        mean[idx], var[idx] = m, np.diag(c)
        if bd == 2:
            cuv[i] = c[0, 1]
        chi2 += float(alpha[idx] @ (c @ alpha[idx]))
    resid = y - mean
    return dict(mean=mean, var=var, cuv=cuv if bd == 2 else None, lpd=lpd, resid=resid,
                **scores(resid, lpd.sum(), chi2, n, n, bd))


def cv_groups(family, n, labels):
    """Closed-form leave-group-out results for integer labels (negative: in no group): dict mean,
    var, resid (NaN where not held out), lpd per group, labels (sorted unique ids) + the scores."""
    _, y, _, bd, P, alpha = problem(family, n)
    labels = np.asarray(labels, dtype=np.int64)
    ids = np.unique(labels[labels >= 0])
    mean, var = np.full(bd * n, np.nan), np.full(bd * n, np.nan)
    lpd = np.empty(ids.size)
    chi2 = 0.0
    for g, lab in enumerate(ids):
        idx = components(np.flatnonzero(labels == lab), n, bd)
        m, c, lpd[g] = closed_group(P, alpha, y, idx)
        mean[idx], var[idx] = m, np.diag(c)
        chi2 += float(alpha[idx] @ (c @ alpha[idx]))
    resid = y - mean
    return dict(mean=mean, var=var, resid=resid, lpd=lpd, labels=ids,
                **scores(resid, lpd.sum(), chi2, int(np.sum(labels >= 0)), n, bd))
