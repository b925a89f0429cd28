"""numpy float64 reference for a background flow estimated with the fit (universal kriging, DESIGN.md
§3.11): a plain helper module of tests/test_trend_cpu.py and tests/test_gpu_trend.py.

Basis coordinates ξ = (x1 − c1)/s, η = (x2 − c2)/s of a point's two spatial (last two) coordinates,
c the mean of the training points, s the largest |coordinate − centre| over both axes, and
    u = β0 + β2·ξ + β3·η,   v = β1 + β4·ξ + β5·η          order 0: q = 2, order 1: q = 6.
H (q × 2N) is the basis at the observations [u…, v…].  Two routes to the same posterior:

  formulas    the library's: L = chol(K_y), W = L⁻¹, G = W·Hᵀ, z = W·y, A = GᵀG, β̂ = A⁻¹Gᵀz,
              α′ = Wᵀ(z − Gβ̂), B0 = WᵀG;  mean = k*ᵀα′ + h*ᵀβ̂,  var = prior − ‖W k*‖² + rᵀA⁻¹r,
              r = h* − B0ᵀk*;
  augmented   independent of them: M = [[K_y, Hᵀ], [H, 0]] solved by LU with a few steps of
              long-double iterative refinement.  M·[α′; β̂] = [y; 0], M⁻¹'s corner is −A⁻¹, and
              var = prior − [k*; h*]ᵀ·M⁻¹·[k*; h*].

The restricted likelihood is −½‖z − Gβ̂‖² − Σ log L_ii − ½ log|A| − ½(n − q) log 2π and its gradient
½ tr((α′α′ᵀ − K_y⁻¹ + B0·A⁻¹·B0ᵀ)·∂K_y/∂θ).  Kernels are tests/sum_ref.py's (a plain kernel is the
one-term sum of weight 1), derived fields tests/field_ref.py's through it.
"""
import functools

import numpy as np
import scipy.linalg as sla

import sum_ref as S

ORDERS = {"constant": 0, "linear": 1}
NOISE = 0.0025
SIZES = (100, 130)
M_TARGETS = 70

# the kernels of the tests: plain mixed vector2d, its spatio-temporal product, the two-term sum
T2D = (dict(kind="mixed", l_df=8.0, l_cf=8.0, ratio=0.6), dict(kind="df", l_df=2.0, l_cf=1.0, ratio=1.0))
TST = (dict(kind="mixed", l_df=8.0, l_cf=8.0, ratio=0.6, var_t=1.0, l_t=3.0),)
CASES = {"vector2d": (T2D[:1], (1.0,)), "vector_st": (TST, (1.0,)), "sum": (T2D, (1.0, 0.05))}


def q_of(order: int) -> int:
    return 2 if order == 0 else 6


def centre_scale(x):
    sp = np.asarray(x, dtype=np.float64)[:, -2:]
    c = sp.mean(0)
    return c, float(np.abs(sp - c).max())


def basis(x, order, centre, scale):
    """H (q × 2N) at the points x for the components [u…, v…]."""
    sp = np.asarray(x, dtype=np.float64)[:, -2:]
    n = sp.shape[0]
    xi, eta = (sp[:, 0] - centre[0]) / scale, (sp[:, 1] - centre[1]) / scale
    one, zero = np.ones(n), np.zeros(n)
    rows = [np.concatenate([one, zero]), np.concatenate([zero, one])]
    if order == 1:
        rows += [np.concatenate([xi, zero]), np.concatenate([eta, zero]),
                 np.concatenate([zero, xi]), np.concatenate([zero, eta])]
    return np.stack(rows)


def field_basis(field, order, scale, m):
    """h_δ = (0,0,1,0,0,1)/s, h_ζ = (0,0,0,−1,1,0)/s as (q × m); zero at order 0."""
    h = np.zeros(q_of(order))
    if order == 1:
        h[[2, 5] if field == "divergence" else [3, 4]] = ([1.0, 1.0] if field == "divergence" else [-1.0, 1.0])
        h /= scale
    return np.repeat(h[:, None], m, 1)


def refined_solve(M, B, steps=3):
    """M⁻¹·B by LU in float64 with `steps` of iterative refinement whose residual is formed in
    long double."""
    lu = sla.lu_factor(M)
    Ml, Bl = M.astype(np.longdouble), B.astype(np.longdouble)
    X = sla.lu_solve(lu, B).astype(np.longdouble)
    for _ in range(steps):
        R = (Bl - Ml @ X).astype(np.float64)
        X = X + sla.lu_solve(lu, R).astype(np.longdouble)
    return X.astype(np.float64)


class Fit:
    """A trend fit of a sum of vector kernels by both routes (route = 'formulas' | 'augmented')."""

    def __init__(self, terms, weights, x, y, noise, order, centre=None, scale=None, route="formulas"):
        self.terms, self.weights = list(terms), [float(w) for w in weights]
        self.x, self.noise, self.order = np.asarray(x, dtype=np.float64), float(noise), int(order)
        self.y = np.asarray(y, dtype=np.float64).reshape(-1)
        c, s = centre_scale(self.x)
        self.centre = np.asarray(c if centre is None else centre, dtype=np.float64)
        self.scale = float(s if scale is None else scale)
        self.q = q_of(order)
        self.H = basis(self.x, order, self.centre, self.scale)
        self.K = S.ky(self.terms, self.weights, self.x, self.noise)
        self.L = np.linalg.cholesky(self.K)
        self.route = route
        n, q = self.K.shape[0], self.q
        if route == "formulas":
            G = sla.solve_triangular(self.L, self.H.T, lower=True)
            z = sla.solve_triangular(self.L, self.y, lower=True)
            self.A = G.T @ G
            self.Ainv = np.linalg.inv(self.A)
            self.beta = np.linalg.solve(self.A, G.T @ z)
            self.alpha = sla.solve_triangular(self.L, z - G @ self.beta, lower=True, trans="T")
            self.B0 = sla.solve_triangular(self.L, G, lower=True, trans="T")
            self.rss = float(np.sum((z - G @ self.beta) ** 2))
        else:
            self.M = np.block([[self.K, self.H.T], [self.H, np.zeros((q, q))]])
            rhs = np.zeros((n + q, 1 + q))
            rhs[:n, 0] = self.y
            rhs[n:, 1:] = np.eye(q)
            X = refined_solve(self.M, rhs)
            self.alpha, self.beta = X[:n, 0], X[n:, 0]
            self.Ainv = -X[n:, 1:]
            self.Ainv = 0.5 * (self.Ainv + self.Ainv.T)
            self.A = np.linalg.inv(self.Ainv)
            self.B0 = X[:n, 1:] @ self.A          # M⁻¹'s off-diagonal block is B0·A⁻¹
            self.rss = float(self.y @ self.alpha)  # (y − Hᵀβ̂)ᵀK_y⁻¹(y − Hᵀβ̂) = yᵀα′ since H·α′ = 0

    # ---- posteriors: cross-covariance Ks (m' × 2N rows = target columns), prior, basis Hs (q × m')
    def _posterior(self, Ks, prior, Hs):
        mean = Ks @ self.alpha + Hs.T @ self.beta
        if self.route == "formulas":
            V = sla.solve_triangular(self.L, Ks.T, lower=True)
            R = Hs - self.B0.T @ Ks.T
            return mean, prior - np.einsum("ij,ij->j", V, V) + np.einsum("ij,ij->j", R, self.Ainv @ R)
        C = np.concatenate([Ks.T, Hs], 0)
        return mean, prior - np.einsum("ij,ij->j", C, refined_solve(self.M, C))

    def _select(self, term):
        if term is None:
            return self.terms, self.weights
        return [self.terms[term]], [self.weights[term]]

    def predict(self, xg, term=None):
        """(mean, latent var), [u…, v…]; term=t: term t's contribution alone (h* = 0)."""
        xg = np.asarray(xg, dtype=np.float64)
        terms, weights = self._select(term)
        Ks = S.k_sum(terms, weights, xg, self.x)
        prior = sum(w * S.term_diag(t) for t, w in zip(terms, weights))
        Hs = basis(xg, self.order, self.centre, self.scale)
        return self._posterior(Ks, prior, Hs if term is None else np.zeros_like(Hs))

    def trend_at(self, xg):
        """h*ᵀβ̂ at the points xg, [u…, v…]."""
        return basis(xg, self.order, self.centre, self.scale).T @ self.beta

    def trend_var(self, xg):
        """h*ᵀA⁻¹h* at the points xg, [u…, v…]."""
        Hs = basis(xg, self.order, self.centre, self.scale)
        return np.einsum("ij,ij->j", Hs, self.Ainv @ Hs)

    def predict_field(self, xg, field, term=None):
        xg = np.asarray(xg, dtype=np.float64)
        ref = S.Fit.__new__(S.Fit)
        ref.terms, ref.weights, ref.x = self.terms, self.weights, self.x
        C = ref.field_cross(xg, field, term)
        prior = ref.field_prior(field, term)
        Hs = field_basis(field, self.order, self.scale, xg.shape[0])
        return self._posterior(C.T, prior, Hs if term is None else np.zeros_like(Hs))

    # ---- the restricted likelihood and its gradient
    def reml(self) -> float:
        n = self.K.shape[0]
        return float(-0.5 * self.rss - np.sum(np.log(np.diag(self.L))) - 0.5 * np.linalg.slogdet(self.A)[1]
                     - 0.5 * (n - self.q) * np.log(2.0 * np.pi))

    def reml_grad(self, plain: bool):
        """Gradient in the library's order: a sum's per term (weight, own entries) then noise; plain:
        the one term's own entries (l_df, l_cf, ratio[, var_t, l_t]) then noise."""
        Ki = sla.cho_solve((self.L, True), np.eye(self.K.shape[0]))
        Mw = np.outer(self.alpha, self.alpha) - Ki + self.B0 @ self.Ainv @ self.B0.T
        dKs = S.grad_matrices(self.terms, self.weights, self.x, self.x)
        if plain:
            dKs = dKs[1:]
        g = [0.5 * np.einsum("ij,ji->", Mw, dK) for dK in dKs]
        g.append(0.5 * np.trace(Mw))
        return np.array(g)


def reml(terms, weights, x, y, noise, order, centre, scale) -> float:
    return Fit(terms, weights, x, y, noise, order, centre, scale).reml()


# ---------------------------------------------------------------- the shared data
@functools.lru_cache(maxsize=None)
def data(n, st):
    """(x, y, xg): tests/test_gpu_sum.py's two-scale observations [u…, v…] at n points and its 70
    targets (the first three on observations), plus a background flow of order 1 m/s with a linear
    shear, so that β̂ is far from zero.  Shared by the tests, which never modify them."""
    rng = np.random.default_rng(2016 + n)
    x = np.stack([rng.uniform(0, 60, n), rng.uniform(0, 45, n)], 1)
    xg = np.stack([rng.uniform(-3, 63, M_TARGETS), rng.uniform(-3, 48, M_TARGETS)], 1)
    xg[:3] = x[:3]
    if st:
        x = np.concatenate([rng.uniform(0, 6, (n, 1)), x], 1)
        xg = np.concatenate([rng.uniform(-1, 7, (M_TARGETS, 1)), xg], 1)
        xg[:3] = x[:3]
    a, b = x[:, -2], x[:, -1]
    y = np.concatenate([np.sin(b / 7) + 0.2 * np.sin(a / 1.5), np.cos(a / 9) + 0.2 * np.cos(b / 1.5)])
    y = y + rng.normal(0, 0.05, 2 * n)
    y = y + np.concatenate([0.8 + 0.010 * (a - 30.0) - 0.006 * (b - 22.0),
                            -0.5 + 0.004 * (a - 30.0) + 0.012 * (b - 22.0)])
    return x, y, xg


def case_data(case, n):
    return data(n, case == "vector_st")


@functools.lru_cache(maxsize=None)
def ref(case, n, order, route="formulas"):
    terms, weights = CASES[case]
    x, y, _ = case_data(case, n)
    return Fit(terms, weights, x, y, NOISE, order, route=route)
