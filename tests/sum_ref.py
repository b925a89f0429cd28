"""numpy float64 reference for sums of vector kernels (GP2D_FAMILY_VECTOR_SUM): a plain helper
module of tests/test_sum_cpu.py and tests/test_gpu_sum.py.

A sum is K = Σ_t w_t·K_t with each K_t one of the oracle's vector kernels (oracle.vector_kernel on
(x1, x2) points, oracle.vector_st_kernel on (t, x1, x2) points); the noise is added once.  A term
is a dict: kind, l_df, l_cf, ratio, and for the spatio-temporal product var_t, l_t.  With
y = Σ_t f_t + ε, cov(f_t(g), y) = w_t·K_t(g, X), so from one Cholesky of K_y (L, α = K_y⁻¹y):
    whole       mean K*·α,          var Σ_t w_t·diag_t − ‖L⁻¹·K*ᵀ‖²
    term t      mean w_t·K_t*·α,    var w_t·diag_t − ‖L⁻¹·w_t·K_t*ᵀ‖²
and the same with tests/field_ref.py's closed forms for the divergence and the vorticity.
The LML gradient is ½ tr((ααᵀ − K_y⁻¹)·∂K_y/∂θ) (oracle._trace_grad) with analytic ∂K_t, in the
library's order: per term (weight_t, l_df_t, l_cf_t, ratio_t[, var_t_t, l_t_t]), then noise;
entries a kind does not use are 0.  tests/test_sum_cpu.py checks it against central differences of
lml() itself.
"""
import numpy as np
import scipy.linalg as sla

import field_ref as F
from oracle import gp2d_oracle as O


def is_st(term) -> bool:
    return "var_t" in term


def _kw(term):
    return dict(kind=term["kind"], l_df=term["l_df"], l_cf=term["l_cf"], ratio=term["ratio"])


def term_k(term, xa, xb):
    """K_t(xa, xb), component-major (2Na, 2Nb)."""
    if is_st(term):
        return O.vector_st_kernel(xa, xb, var_t=term["var_t"], l_t=term["l_t"], **_kw(term))
    return O.vector_kernel(xa, xb, **_kw(term))


def term_diag(term) -> float:
    d = O.kernel_diag(O.kind_code(term["kind"]), l_df=term["l_df"], l_cf=term["l_cf"], ratio=term["ratio"])
    return float(d * (term["var_t"] if is_st(term) else 1.0))


def k_sum(terms, weights, xa, xb):
    return sum(w * term_k(t, xa, xb) for t, w in zip(terms, weights))


def ky(terms, weights, x, noise):
    K = k_sum(terms, weights, x, x)
    return K + noise * np.eye(K.shape[0])


class Fit:
    """One Cholesky fit of the sum: L, α, and every posterior the tests compare against."""

    def __init__(self, terms, weights, x, y, noise):
        self.terms, self.weights = list(terms), [float(w) for w in weights]
        self.x, self.noise = np.asarray(x, dtype=np.float64), float(noise)
        self.y = np.asarray(y, dtype=np.float64).reshape(-1)
        self.K = ky(self.terms, self.weights, self.x, self.noise)
        self.L = np.linalg.cholesky(self.K)
        self.alpha = sla.cho_solve((self.L, True), self.y)

    def _select(self, term):
        if term is None:
            return self.terms, self.weights
        return [self.terms[term]], [self.weights[term]]

    def predict(self, xg, term=None):
        """(mean, latent var), [u…, v…]; term=t: term t's contribution alone."""
        terms, weights = self._select(term)
        Ks = k_sum(terms, weights, xg, self.x)
        V = sla.solve_triangular(self.L, Ks.T, lower=True)
        prior = sum(w * term_diag(t) for t, w in zip(terms, weights))
        return Ks @ self.alpha, prior - np.einsum("ij,ij->j", V, V)

    def field_cross(self, xg, field, term=None):
        terms, weights = self._select(term)
        return sum(w * F.cross(self.x, xg, field, t["kind"], t["l_df"], t["l_cf"], t["ratio"],
                               t.get("var_t"), t.get("l_t")) for t, w in zip(terms, weights))

    def field_prior(self, field, term=None):
        terms, weights = self._select(term)
        return sum(w * F.prior_var(field, t["kind"], t["l_df"], t["l_cf"], t["ratio"], t.get("var_t"))
                   for t, w in zip(terms, weights))

    def predict_field(self, xg, field, term=None):
        C = self.field_cross(np.asarray(xg, dtype=np.float64), field, term)
        V = sla.solve_triangular(self.L, C, lower=True)
        return C.T @ self.alpha, self.field_prior(field, term) - np.einsum("ij,ij->j", V, V)


# ---------------------------------------------------------------- LML and its gradient
def lml(terms, weights, x, y, noise) -> float:
    return float(O.lml_from_K(ky(terms, weights, x, noise), y)[0])


def _spatial_parts(xa, xb, l_df, l_cf):
    """The div-free and curl-free 2×2 SE blocks f, g as (3, Na, Nb) arrays of (k11, k12, k22), and
    their derivatives in ℓ_df and ℓ_cf.  With u = 1/ℓ², E = exp(−r²u/2), P_ab = d_a·d_b:
        f = u·E·Q,  Q = P·u + δ·(1 − r²u):   ∂f/∂u = E·[Q·(1 − u·r²/2) + u·(P − δ·r²)]
        g = u·E·G,  G = δ − P·u:              ∂g/∂u = E·[G·(1 − u·r²/2) − u·P]
    and ∂/∂ℓ = ∂/∂u · (−2u/ℓ)."""
    d1 = xa[:, 0][:, None] - xb[:, 0][None, :]
    d2 = xa[:, 1][:, None] - xb[:, 1][None, :]
    r2 = d1 * d1 + d2 * d2
    P = np.stack([d1 * d1, d1 * d2, d2 * d2])
    D = np.array([1.0, 0.0, 1.0])[:, None, None]
    u = 1.0 / l_df ** 2
    E = np.exp(-0.5 * r2 * u)
    Q = P * u + D * (1.0 - r2 * u)
    f = u * E * Q
    df = E * (Q * (1.0 - 0.5 * u * r2) + u * (P - D * r2)) * (-2.0 * u / l_df)
    v = 1.0 / l_cf ** 2
    Ec = np.exp(-0.5 * r2 * v)
    G = D - P * v
    g = v * Ec * G
    dg = Ec * (G * (1.0 - 0.5 * v * r2) - v * P) * (-2.0 * v / l_cf)
    return f, df, g, dg


def _blocks(b):
    return np.block([[b[0], b[1]], [b[1], b[2]]])


def term_dk(term, xa, xb):
    """Analytic ∂K_t/∂(l_df, l_cf, ratio[, var_t, l_t]) as a list of (2Na, 2Nb) matrices (zeros for
    a parameter the kind does not use)."""
    xa, xb = np.asarray(xa, dtype=np.float64), np.asarray(xb, dtype=np.float64)
    sa, sb = (xa[:, 1:], xb[:, 1:]) if is_st(term) else (xa, xb)
    f, df, g, dg = _spatial_parts(sa, sb, term["l_df"], term["l_cf"])
    rho = term["ratio"]
    zero = np.zeros_like(f)
    kind = O.kind_code(term["kind"])
    if kind == O.KIND_DIVFREE:
        ks, d = f, [df, zero, zero]
    elif kind == O.KIND_CURLFREE:
        ks, d = g, [zero, dg, zero]
    elif kind == O.KIND_MIXED:
        ks, d = rho * f + (1.0 - rho) * g, [rho * df, (1.0 - rho) * dg, f - g]
    else:
        raise ValueError("sum_ref differentiates the df, cf and mixed kinds")
    if not is_st(term):
        return [_blocks(a) for a in d]
    dt2 = np.square(xa[:, 0][:, None] - xb[:, 0][None, :])
    e = np.exp(-0.5 * dt2 / term["l_t"] ** 2)
    ct = term["var_t"] * e
    out = [_blocks(ct * a) for a in d]
    out.append(_blocks(e * ks))
    out.append(_blocks(ct * dt2 / term["l_t"] ** 3 * ks))
    return out


def grad_matrices(terms, weights, xa, xb):
    """∂K_sum/∂θ for θ in the library's order without the noise: per term K_t (the weight), then
    w_t·∂K_t/∂(the term's own parameters)."""
    out = []
    for t, w in zip(terms, weights):
        out.append(term_k(t, xa, xb))
        out += [w * d for d in term_dk(t, xa, xb)]
    return out


def lml_grad(terms, weights, x, y, noise):
    """(LML, gradient) with the noise entry last."""
    K = ky(terms, weights, x, noise)
    val, L, alpha = O.lml_from_K(K, y)
    Ki = sla.cho_solve((L, True), np.eye(K.shape[0]))
    M = np.outer(alpha, alpha) - Ki
    g = [0.5 * np.einsum("ij,ji->", M, dK) for dK in grad_matrices(terms, weights, x, x)]
    g.append(0.5 * np.trace(M))
    return float(val), np.array(g)


def kernel_grad(terms, weights, xa, xb, dL_dK):
    """Σ dL_dK ⊙ ∂K(xa, xb)/∂θ, the library's order without the noise."""
    return np.array([np.sum(dL_dK * dK) for dK in grad_matrices(terms, weights, xa, xb)])


def param_names(terms):
    names = []
    for t, term in enumerate(terms):
        own = ("l_df", "l_cf", "ratio") + (("var_t", "l_t") if is_st(term) else ())
        names += [f"weight_{t}"] + [f"{n}_{t}" for n in own]
    return tuple(names + ["noise"])
