"""numpy reference for posterior draws of the flow and ensembles advected through them
(gp2d_paths_eval, gp2d_advect_draws, engine.draw_flows / advect_draws): a plain helper module of
tests/test_paths_cpu.py and tests/test_gpu_paths.py, built on tests/advect_ref.py.

Pathwise conditioning (Matheron's rule; Wilson et al. 2020): a posterior draw as a function,
    g_s(x, t) = f_s(x, t) + K((x, t), X)·α_s,   α_s = K_y⁻¹(y − f_s(X) − ε_s),
with the prior draw a finite sum over the rows [τ, w1, w2, b, a1, a2] of the draw's feature table,
    f_s(x, t) = Σ_j (a1_j, a2_j)·sin(w1_j·x1 + w2_j·x2 + τ_j·t + b_j).
K_y = Σ_t w_t·K_t(X, X) + noise·I from the oracle's kernels (sum_ref.ky) and α_s from
np.linalg.solve on it.  DrawFlow is an advect_ref.Flow with the feature sum added to velocity() and
its gradient Σ_j a_j w_jᵀ cos θ_j to gradient(), so advect_ref.advect integrates a draw as it
integrates the mean flow and yields its umax and fmax.  Observations, eps and α are [u…, v…] in the
order of the training points given (the caller's; a device fit's Morton order is the device's
business).
"""
import dataclasses

import numpy as np

import advect_ref as A
import sum_ref as S


def phase(rows, p, t):
    """θ (M, F) of the rows (F, 6) at the positions p (M, 2) and time(s) t (scalar or (M,))."""
    p = np.asarray(p, dtype=np.float64).reshape(-1, 2)
    tt = np.broadcast_to(np.asarray(t, dtype=np.float64).reshape(-1, 1), (p.shape[0], 1))
    return p[:, :1] * rows[:, 1] + p[:, 1:] * rows[:, 2] + tt * rows[:, 0] + rows[:, 3]


def prior(rows, p, t=0.0):
    """f_s (M, 2) at the positions p and time(s) t."""
    return np.sin(phase(rows, p, t)) @ rows[:, 4:6]


def prior_gradient(rows, p, t=0.0):
    """∇f_s (M, 2, 2), [a][b] = ∂f_a/∂x_b."""
    c = np.cos(phase(rows, p, t))
    return np.einsum("mf,fa,fb->mab", c, rows[:, 4:6], rows[:, 1:3])


@dataclasses.dataclass
class DrawFlow(A.Flow):
    """One posterior draw: advect_ref.Flow's update term with the draw's α, plus its features."""
    rows: np.ndarray = None

    def velocity(self, p, t):
        return super().velocity(p, t) + prior(self.rows, p, t)

    def gradient(self, p, t):
        return super().gradient(p, t) + prior_gradient(self.rows, p, t)


def prior_at_training(rows, x):
    """f_s(X) as an observation vector [u…, v…]: rows (t, x1, x2) are evaluated at their own time."""
    x = np.asarray(x, dtype=np.float64)
    f = prior(rows, x[:, -2:], x[:, 0] if x.shape[1] == 3 else 0.0)
    return np.concatenate([f[:, 0], f[:, 1]])


def draw_alphas(terms, weights, x, y, noise, table, eps):
    """α_s (S, 2N) of every draw of the table (S, F, 6) with the noise draws eps (S, 2N)."""
    Ky = S.ky(list(terms), list(weights), np.asarray(x, dtype=np.float64), noise)
    R = np.stack([np.asarray(y).reshape(-1) - prior_at_training(table[s], x) - eps[s] for s in range(table.shape[0])])
    return np.linalg.solve(Ky, R.T).T


def draw_flows(terms, weights, x, y, noise, table, eps):
    """The DrawFlow of every draw."""
    al = draw_alphas(terms, weights, x, y, noise, table, eps)
    return [DrawFlow(tuple(terms), tuple(weights), np.asarray(x, dtype=np.float64), al[s], None, table[s])
            for s in range(table.shape[0])]


def velocity_rows(flows, p, t=0.0):
    """(S, 2M): each draw's velocity at p as [u(M), v(M)] — FlowDraws.velocity's layout."""
    out = []
    for f in flows:
        u = f.velocity(p, t)
        out.append(np.concatenate([u[:, 0], u[:, 1]]))
    return np.stack(out)
