"""Host side of the posterior flow draws (engine.draw_flows): the random Fourier
feature table of the prior draws and the observation-noise draws, from seeded CPU generators.

A prior draw of the velocity is a finite sum, family-agnostic on the device,
    f_s(x, t) = Σ_j (a1_j, a2_j)·sin(w1_j·x1 + w2_j·x2 + τ_j·t + b_j),
one table row [τ, w1, w2, b, a1, a2] per feature.  For every term of the kernel (one unless
'vector_sum') and every part it has (div-free, curl-free; a mixed kind has both unless its ratio
makes one vanish) n_features rows:
    (w1, w2) ~ N(0, I/ℓ_part²),  τ ~ N(0, 1/ℓ_t²) ('vector_st', else 0),  b ~ U[0, 2π),  g ~ N(0, 1),
    amp = g·sqrt(2c / n_features),  c = w_term · w_part · var_t,
    div-free: (a1, a2) = amp·(−w2, w1)       curl-free: (a1, a2) = amp·(w1, w2)
with w_part = ratio | 1 − ratio | 1 and var_t = 1 for the purely spatial family.  The div-free form
is the curl of a stream function with covariance c·exp(−r²/2ℓ²), the curl-free form the gradient of
a potential with the same covariance: E[f f′ᵀ] = ½ Σ_j a′_j a′_jᵀ cos(ω_j·d + τ_j·Δt) → the kernel's
2 × 2 blocks with their 1/ℓ² prefactor (tests/test_paths_cpu.py proves it against the oracle).

Every draw has its own rows: the covariance of f_s is then exactly K in expectation and the
ensemble has exactly the posterior mean and covariance (g_s is affine in (f_s, ε_s)); one feature
set shared by the draws would bias the ensemble covariance by O(1/√F).  Draw s is generated from
numpy's PCG64 seeded with (s, seed): the same seed gives the same bits on any machine, and draw s
does not depend on how many draws are made.  numpy only — no device, no native library.
"""
from __future__ import annotations

import math

import numpy as np

FEATURE_WIDTH = 6   # τ, w1, w2, b, a1, a2
_EPS_STREAM = 0x657073   # the noise draws' own generator stream


def kernel_parts(kernel) -> list:
    """The parts of a KernelSpec a prior draw is built from: dicts part ('df' | 'cf'), length, c (the
    stream function's or potential's variance: sum weight · part weight · var_t), l_t (None for the
    purely spatial family) — in the order of the table's blocks of n_features rows."""
    if kernel.family == "vector_sum":
        terms, weights = kernel._sum_terms(), [float(w) for w in kernel.weights]
    elif kernel.family in ("vector2d", "vector_st"):
        terms, weights = (kernel,), [1.0]
    else:
        raise ValueError("posterior flow draws need a div-free, curl-free or mixed vector kernel "
                         f"(family {kernel.family!r} has no velocity draw)")
    parts = []
    for tm, w in zip(terms, weights):
        kind = {1: "df", 2: "cf", 3: "mixed", 0: "scalar"}.get(tm.kind, tm.kind)
        if kind not in ("df", "cf", "mixed"):
            raise ValueError("posterior flow draws need a div-free, curl-free or mixed vector kernel "
                             "(the scalar kind has no velocity draw)")
        st = tm.family == "vector_st"
        var_t, l_t = (float(tm.var_t), float(tm.l_t)) if st else (1.0, None)
        w_df = {"df": 1.0, "cf": 0.0, "mixed": float(tm.ratio)}[kind]
        w_cf = {"df": 0.0, "cf": 1.0, "mixed": 1.0 - float(tm.ratio)}[kind]
        for part, wp, length in (("df", w_df, float(tm.l_df)), ("cf", w_cf, float(tm.l_cf))):
            if wp != 0.0:
                parts.append(dict(part=part, length=length, c=w * wp * var_t, l_t=l_t))
    return parts


def feature_count(kernel, n_features: int) -> int:
    """F_tot = n_features × (the parts present over all terms)."""
    return int(n_features) * len(kernel_parts(kernel))


def feature_table(kernel, n_draws: int, n_features: int = 1024, seed: int = 0) -> np.ndarray:
    """The (S, F_tot, 6) FP64 feature table of S prior draws, rows [τ, w1, w2, b, a1, a2] (the module
    docstring).  A negative c (a negative sum weight) has no prior draw: ValueError."""
    S, F = int(n_draws), int(n_features)
    if S < 1:
        raise ValueError("n_draws must be at least 1")
    if F < 1:
        raise ValueError("n_features must be at least 1")
    parts = kernel_parts(kernel)
    if any(p["c"] < 0.0 for p in parts):
        raise ValueError("a kernel term with a negative weight has no prior draw")
    table = np.zeros((S, F * len(parts), FEATURE_WIDTH))
    for s in range(S):
        rng = np.random.default_rng([s, int(seed)])
        for i, p in enumerate(parts):
            rows = table[s, i * F:(i + 1) * F]
            w = rng.standard_normal((F, 2)) / p["length"]
            tau = rng.standard_normal(F) / p["l_t"] if p["l_t"] is not None else np.zeros(F)
            b = rng.uniform(0.0, 2.0 * math.pi, F)
            amp = rng.standard_normal(F) * math.sqrt(2.0 * p["c"] / F)
            rows[:, 0] = tau
            rows[:, 1:3] = w
            rows[:, 3] = b
            if p["part"] == "df":
                rows[:, 4], rows[:, 5] = -amp * w[:, 1], amp * w[:, 0]
            else:
                rows[:, 4], rows[:, 5] = amp * w[:, 0], amp * w[:, 1]
    return table


def noise_draws(n_draws: int, n_obs: int, variance: float, seed: int = 0) -> np.ndarray:
    """ε (S, n_obs) ~ N(0, variance·I) in the caller's observation order, draw s from PCG64 seeded
    with (s, seed) on a stream of its own."""
    sd = math.sqrt(float(variance))
    return np.stack([sd * np.random.default_rng([s, int(seed), _EPS_STREAM]).standard_normal(int(n_obs))
                     for s in range(int(n_draws))])

