"""numpy reference for particles advected through the fitted flow (gp2d_advect, engine.advect): a
plain helper module of tests/test_advect_cpu.py and tests/test_gpu_advect.py.

Conventions (the library's).  Points are (x1, x2), components (f1, f2) = the first
and second half of the observation vector, and dx1/dt = s·f1, dx2/dt = s·f2 (s = vel_scale).  The
augmented system is
    dx/dt = s·μ(x, t),   dF/dt = s·∇μ(x, t)·F,   F(t0) = I,
μ(x, t) = K(x, X)·α (+ h(x)ᵀβ̂ for a trend fit) the posterior mean velocity and ∇μ its 2 × 2 gradient
in grad_ref's component order c = 2a + b (a the field component, b the direction), so that
F[a][b] = ∂x_a(t)/∂x_b(t0).  A linear trend u = β0 + β2·ξ + β3·η, v = β1 + β4·ξ + β5·η in
ξ = (x1 − c1)/scale, η = (x2 − c2)/scale adds (β2, β3; β4, β5)/scale to ∇μ.  For the spatio-temporal
product the training rows are (t, x1, x2) and the mean is evaluated at the stage's time; the purely
spatial kernels ignore t.  Classical RK4, stage for stage: step n starts at t_n = t0 + n·dt (formed
from n), the stage times are t_n, t_n + dt/2, t_n + dt/2, t_n + dt, and
    k_i = (s·μ, s·∇μ·F) at the stage state,   state += dt/6·(k1 + 2·k2 + 2·k3 + k4).
dt may be negative.  The kernel blocks come from oracle.vector_kernel / oracle.vector_st_kernel and
the gradient's cross-covariance from grad_ref.cross; a kernel is a list of sum_ref-style terms
(dicts kind, l_df, l_cf, ratio[, var_t, l_t]) with weights, K = Σ_t w_t·K_t.

eps > 0 perturbs every evaluation: each entry of μ gets eps·max|μ|·ξ and each entry of ∇μ gets
eps·max|∇μ|·ξ with ξ uniform on [−1, 1] from a generator seeded with `seed` (the maxima over the
particles of that evaluation) — a model of an implementation whose evaluations differ from this one
by a relative eps, which is how the GPU tests size their gates.
"""
import dataclasses
import functools

import numpy as np

import grad_ref as G
from oracle import gp2d_oracle as O

L_DF, L_CF, NOISE = 5.0, 4.0, 0.01


@functools.lru_cache(maxsize=None)
def tracks(n, sd=0.05):
    """test_gpu_fields.tracks (that module needs a GPU to import): n points on [0, 45] × [0, 60] with
    f1 = sin(x2/7), f2 = cos(x1/9) plus noise of standard deviation sd."""
    rng = np.random.default_rng(n)
    x = np.stack([rng.uniform(0, 45, n), rng.uniform(0, 60, n)], 1)
    y = np.concatenate([np.sin(x[:, 1] / 7), np.cos(x[:, 0] / 9)]) + sd * rng.normal(0, 1, 2 * n)
    return x, y


def seeds(x, m=300, seed=1):
    """m start points on [−5, 50] × [−5, 65], the first five on training points (test_gpu_fields.targets)."""
    rng = np.random.default_rng(seed)
    g = np.stack([rng.uniform(-5, 50, m), rng.uniform(-5, 65, m)], 1)
    k = min(5, x.shape[0]) if m > 5 else 0
    g[:k] = x[:k, -2:]
    return g


def term(kind, ratio, l_df=L_DF, l_cf=L_CF, **st):
    return dict(kind=kind, l_df=l_df, l_cf=l_cf, ratio=ratio, **st)


@dataclasses.dataclass
class Flow:
    """The posterior mean flow of a fit: the kernel's terms and weights, the training points (rows
    (x1, x2) or (t, x1, x2)), α = [α_u; α_v] without padding, and the trend (None, or a dict with beta
    (2 or 6 coefficients), centre, scale)."""
    terms: tuple
    weights: tuple
    x: np.ndarray
    alpha: np.ndarray
    trend: dict = None

    @property
    def st(self):
        return "var_t" in self.terms[0]

    def _points(self, p, t):
        p = np.asarray(p, dtype=np.float64).reshape(-1, 2)
        return np.column_stack([np.full(p.shape[0], float(t)), p]) if self.st else p

    def velocity(self, p, t):
        """μ at the positions p (M, 2) and time t: (M, 2)."""
        g = self._points(p, t)
        m = g.shape[0]
        mu = np.zeros(2 * m)
        for tm, w in zip(self.terms, self.weights):
            kw = dict(kind=tm["kind"], l_df=tm["l_df"], l_cf=tm["l_cf"], ratio=tm["ratio"])
            K = O.vector_st_kernel(g, self.x, var_t=tm["var_t"], l_t=tm["l_t"], **kw) if self.st else \
                O.vector_kernel(g, self.x, **kw)
            mu += w * (K @ self.alpha)
        u = np.stack([mu[:m], mu[m:]], 1)
        if self.trend is not None:
            b, c, s = np.asarray(self.trend["beta"]), self.trend["centre"], self.trend["scale"]
            u = u + b[:2]
            if b.size == 6:
                xi, eta = (g[:, -2] - c[0]) / s, (g[:, -1] - c[1]) / s
                u = u + np.stack([b[2] * xi + b[3] * eta, b[4] * xi + b[5] * eta], 1)
        return u

    def gradient(self, p, t):
        """∇μ at the positions p and time t: (M, 2, 2), [a][b] = ∂μ_a/∂x_b."""
        g = self._points(p, t)
        out = np.zeros((g.shape[0], 4))
        for tm, w in zip(self.terms, self.weights):
            C = G.cross(self.x, g, tm["kind"], tm["l_df"], tm["l_cf"], tm["ratio"], tm.get("var_t"), tm.get("l_t"))
            out += w * np.einsum("nmc,n->mc", C, self.alpha)
        if self.trend is not None and np.size(self.trend["beta"]) == 6:
            out = out + np.asarray(self.trend["beta"])[2:6] / self.trend["scale"]
        return out.reshape(-1, 2, 2)


def oracle_flow(n, kind, ratio):
    """The flow of oracle.OracleFit on tracks(n) (noise 0.01, l_df 5, l_cf 4)."""
    x, y = tracks(n)
    fit = O.OracleFit(x, y, kind, L_DF, L_CF, ratio, NOISE)
    return Flow((term(kind, ratio),), (1.0,), x, fit.alpha)


@dataclasses.dataclass
class Run:
    path: np.ndarray      # (nsteps + 1, M, 2): the positions after every step, [0] = x0
    tangent: np.ndarray   # (nsteps + 1, M, 2, 2) or None
    fmax: float           # max ‖F‖₂ over the steps and particles (1 without the tangent)
    umax: float           # max |μ| over every evaluation

    def records(self, save_every):
        """The step numbers gp2d_advect records: 0, save_every, 2·save_every, …, and nsteps."""
        n = self.path.shape[0] - 1
        idx = list(range(0, n, save_every)) + [n]
        return np.array(sorted(set(idx)))


def advect(flow, x0, t0, dt, nsteps, vel_scale=1.0, tangent=True, eps=0.0, seed=0):
    """RK4 of the augmented system from x0 (M, 2) at t0: a Run with every step's state."""
    x = np.array(x0, dtype=np.float64).reshape(-1, 2)
    m = x.shape[0]
    F = np.broadcast_to(np.eye(2), (m, 2, 2)).copy()
    rng = np.random.default_rng(seed)
    umax = 0.0
    s = float(vel_scale)

    def rhs(xs, Fs, ts):
        nonlocal umax
        u = flow.velocity(xs, ts)
        if u.size:
            umax = max(umax, float(np.max(np.abs(u))))
        if eps:
            u = u + eps * np.max(np.abs(u)) * rng.uniform(-1, 1, u.shape)
        if not tangent:
            return s * u, None
        g = flow.gradient(xs, ts)
        if eps:
            g = g + eps * np.max(np.abs(g)) * rng.uniform(-1, 1, g.shape)
        return s * u, s * (g @ Fs)

    def step(a, ka, h):
        return a if ka is None else a + h * ka

    path, tang = [x.copy()], [F.copy()]
    for n in range(nsteps):
        tn = t0 + n * dt
        k1x, k1F = rhs(x, F, tn)
        k2x, k2F = rhs(x + 0.5 * dt * k1x, step(F, k1F, 0.5 * dt), tn + 0.5 * dt)
        k3x, k3F = rhs(x + 0.5 * dt * k2x, step(F, k2F, 0.5 * dt), tn + 0.5 * dt)
        k4x, k4F = rhs(x + dt * k3x, step(F, k3F, dt), tn + dt)
        x = x + dt / 6.0 * (k1x + 2.0 * k2x + 2.0 * k3x + k4x)
        if tangent:
            F = F + dt / 6.0 * (k1F + 2.0 * k2F + 2.0 * k3F + k4F)
        path.append(x.copy())
        tang.append(F.copy())
    tang = np.stack(tang) if tangent else None
    fmax = float(np.max(np.linalg.norm(tang, 2, axis=(-2, -1)))) if tangent and m else 1.0
    return Run(np.stack(path), tang, fmax, umax)


def ftle(F, duration):
    """ln λ_max(FᵀF) / (2·|duration|) from numpy's symmetric eigensolver (the check of engine.ftle)."""
    C = np.swapaxes(F, -1, -2) @ F
    return np.log(np.linalg.eigvalsh(C)[..., -1]) / (2.0 * abs(duration))
