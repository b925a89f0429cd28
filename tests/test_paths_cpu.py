"""The mathematics of the posterior flow draws, on the host: the random Fourier
feature table of gp2d.paths against the oracle's kernels, the ensemble moments of the pathwise
draws against the oracle's posterior (on the numpy reference tests/paths_ref.py), reproducibility of
the seeded table, and the host-side refusals of the two entry points, which run before any device
work and so need no device.

Gates.  Every statistical gate is 6 standard errors with the standard error estimated from the
sample under test, nothing is tuned to what the code gives:
  a. K̂ = ½ Σ_j a′_j a′_jᵀ cos(ω_j·d + τ_j·Δt) is, per part, a mean of F i.i.d. terms; its standard
     error is the terms' own spread / √F (summed in quadrature over the parts).
  b. the ensemble mean of S draws lies within 6·sqrt(v̂/S) of the posterior mean, the ensemble
     variance v̂ within 6·sqrt((m̂4 − v̂²)/S) of the posterior variance, m̂4 the sample's own fourth
     central moment (no Gaussian assumption: a draw of 64 features is only approximately Gaussian).
With 5 kernels × 7 separations × 3 entries and 8 mean and 8 variance checks, a 6-σ gate fails by
chance with probability < 1e-6; the seeds are fixed, so a pass is reproducible.
"""
import ctypes
import math
import types

import numpy as np
import pytest

import advect_ref as A
import paths_ref as PR
import sum_ref as SR
from gp2d import paths as P
from oracle import gp2d_oracle as O

NSIG = 6.0


def spec(family="vector2d", **kw):
    """A KernelSpec look-alike: gp2d.paths reads attributes only (no native library, no torch)."""
    d = dict(family=family, kind="df", l_df=5.0, l_cf=5.0, ratio=1.0, var_t=1.0, l_t=1.0, terms=(), weights=())
    d.update(kw)
    ns = types.SimpleNamespace(**d)
    ns._sum_terms = lambda: tuple(ns.terms)
    return ns


def as_term(s):
    t = dict(kind=s.kind, l_df=s.l_df, l_cf=s.l_cf, ratio=s.ratio)
    if s.family == "vector_st":
        t.update(var_t=s.var_t, l_t=s.l_t)
    return t


ST_A = spec("vector_st", kind="mixed", l_df=5.0, l_cf=4.0, ratio=0.3, var_t=2.0, l_t=1.5)
CASES = {
    "df": spec(kind="df", l_df=5.0),
    "cf": spec(kind="cf", l_cf=4.0),
    "mixed": spec(kind="mixed", l_df=5.0, l_cf=3.0, ratio=0.35),
    "vector_st": ST_A,
    "sum": spec("vector_sum", terms=(spec(kind="mixed", l_df=6.0, l_cf=2.5, ratio=0.6), spec(kind="df", l_df=1.5)),
                weights=(0.7, 1.8)),
}


def terms_of(ks):
    if ks.family == "vector_sum":
        return [as_term(t) for t in ks.terms], [float(w) for w in ks.weights]
    return [as_term(ks)], [1.0]


def oracle_block(ks, d, dt):
    """The kernel's 2 × 2 block between (0, 0, 0) and (dt, d1, d2)."""
    terms, weights = terms_of(ks)
    st = SR.is_st(terms[0])
    xa = np.array([[0.0, 0.0, 0.0]]) if st else np.array([[0.0, 0.0]])
    xb = np.array([[dt, d[0], d[1]]]) if st else np.array([[d[0], d[1]]])
    return SR.k_sum(terms, weights, xa, xb)   # component-major (2, 2)


# ---------------------------------------------------------------- a. the feature covariance
SEPARATIONS = [(0.0, 0.0), (1.3, -0.7), (4.0, 3.0), (-6.0, 2.0), (0.0, 9.0), (0.4, 0.0), (-2.0, -2.5)]


@pytest.mark.parametrize("name", list(CASES))
def test_feature_covariance_is_the_kernel(name):
    """One draw of 2^16 features per part: the expectation of f f′ᵀ over (b, g) is
    ½ Σ_j a′_j a′_jᵀ cos(ω_j·d + τ_j·Δt), a′ the amplitude without g, and equals the oracle's block
    (1/ℓ² prefactor, ratio, sum weights, var_t and the temporal factor included) within 6 standard
    errors; the table's (a1, a2) is g·a′ with g ~ N(0, 1) and b ~ U[0, 2π) (their first two moments,
    same gate)."""
    ks, F = CASES[name], 1 << 16
    parts = P.kernel_parts(ks)
    table = P.feature_table(ks, 1, F, seed=11)
    assert table.shape == (1, F * len(parts), 6) and table.dtype == np.float64
    assert P.feature_count(ks, F) == F * len(parts)
    st = ks.family == "vector_st"
    worst = 0.0
    blocks = []
    for i, p in enumerate(parts):
        rows = table[0, i * F:(i + 1) * F]
        tau, w, b, a = rows[:, 0], rows[:, 1:3], rows[:, 3], rows[:, 4:6]
        dirs = np.stack([-w[:, 1], w[:, 0]], 1) if p["part"] == "df" else w
        ap = math.sqrt(2.0 * p["c"] / F) * dirs                 # a′: the amplitude without g
        g = np.einsum("fa,fa->f", a, ap) / np.einsum("fa,fa->f", ap, ap)
        assert np.allclose(a, g[:, None] * ap, rtol=1e-12, atol=0.0)   # parallel: the part's form
        assert abs(g.mean()) < NSIG / math.sqrt(F) and abs(g.var() - 1.0) < NSIG * math.sqrt(2.0 / F)
        assert abs(b.mean() - math.pi) < NSIG * (2 * math.pi / math.sqrt(12)) / math.sqrt(F)
        assert 0.0 <= b.min() and b.max() < 2 * math.pi
        assert abs(w.var() * p["length"] ** 2 - 1.0) < NSIG * math.sqrt(2.0 / (2 * F))
        assert (np.all(tau == 0.0) if not st else abs(tau.var() * p["l_t"] ** 2 - 1.0) < NSIG * math.sqrt(2.0 / F))
        blocks.append((tau, w, ap))
    for d in SEPARATIONS:
        for dt in ((0.0, 0.8) if st else (0.0,)):
            est, var = np.zeros((2, 2)), np.zeros((2, 2))
            for tau, w, ap in blocks:
                # X_j = F·½·a′_j a′_jᵀ cos(…): the part's estimate is their mean
                X = 0.5 * F * np.einsum("fa,fb,f->fab", ap, ap, np.cos(w @ np.array(d) + tau * dt))
                est += X.mean(0)
                var += X.var(0, ddof=1) / F
            want = oracle_block(ks, d, dt)
            z = np.abs(est - want) / np.sqrt(var + 1e-300)
            worst = max(worst, float(z.max()))
            assert np.all(np.abs(est - want) <= NSIG * np.sqrt(var)), (name, d, dt, est, want, np.sqrt(var))
    print(f"{name}: worst deviation {worst:.2f} standard errors (gate {NSIG})")


# ---------------------------------------------------------------- b. the ensemble moments
def test_ensemble_has_the_posterior_moments():
    """S = 4000 reference draws, each with its own 64 features per part, on 40 training points and 4
    targets (one on a training point, one outside the data): ensemble mean and variance of g_s at
    the targets against oracle.OracleFit's posterior (mixed kernel, ratio 0.35)."""
    n, S, F = 40, 4000, 64
    ks = spec(kind="mixed", l_df=A.L_DF, l_cf=A.L_CF, ratio=0.35)
    x, y = A.tracks(n)
    xg = np.array([x[0], [20.0, 30.0], [33.3, 11.1], [-3.0, 62.0]])
    table = P.feature_table(ks, S, F, seed=3)
    eps = P.noise_draws(S, 2 * n, A.NOISE, seed=3)
    terms, weights = terms_of(ks)
    alphas = PR.draw_alphas(terms, weights, x, y, A.NOISE, table, eps)
    Ks = O.vector_kernel(xg, x, kind="mixed", l_df=A.L_DF, l_cf=A.L_CF, ratio=0.35)
    G = np.stack([np.concatenate(PR.prior(table[s], xg).T) for s in range(S)]) + alphas @ Ks.T   # (S, 2m)
    mu, var = O.OracleFit(x, y, "mixed", A.L_DF, A.L_CF, 0.35, A.NOISE).predict(xg)
    m1 = G.mean(0)
    c = G - m1
    v = (c ** 2).sum(0) / (S - 1)
    m4 = (c ** 4).mean(0)
    se_mean, se_var = np.sqrt(v / S), np.sqrt((m4 - v ** 2) / S)
    zm, zv = np.abs(m1 - mu) / se_mean, np.abs(v - var) / se_var
    print(f"ensemble of {S}: mean within {zm.max():.2f} and variance within {zv.max():.2f} standard errors (gate {NSIG}); "
          f"posterior sd {np.sqrt(var).min():.3f}..{np.sqrt(var).max():.3f}")
    assert np.all(zm <= NSIG) and np.all(zv <= NSIG), (zm, zv)
    # the gates have teeth: the noise draws left out shrink the variance on the training point
    G0 = np.stack([np.concatenate(PR.prior(table[s], xg).T) for s in range(S)]) + \
        PR.draw_alphas(terms, weights, x, y, A.NOISE, table, 0.0 * eps) @ Ks.T
    v0 = G0.var(0, ddof=1)
    assert np.max(np.abs(v0 - var) / se_var) > 2 * NSIG


# ---------------------------------------------------------------- c. reproducibility
def test_seeded_table_is_reproducible():
    """The same seed gives the same bits; another seed and another draw differ; draw s does not depend
    on how many draws are made; the noise draws likewise, on a stream of their own."""
    ks = CASES["sum"]
    t1, t2 = P.feature_table(ks, 3, 50, seed=5), P.feature_table(ks, 3, 50, seed=5)
    assert t1.shape == (3, 150, 6) and np.array_equal(t1.view(np.int64), t2.view(np.int64))
    assert not np.array_equal(t1, P.feature_table(ks, 3, 50, seed=6))
    assert not np.array_equal(t1[0], t1[1])
    assert np.array_equal(P.feature_table(ks, 5, 50, seed=5)[:3], t1)
    e1 = P.noise_draws(3, 20, 0.04, seed=5)
    assert e1.shape == (3, 20) and np.array_equal(e1, P.noise_draws(4, 20, 0.04, seed=5)[:3])
    assert not np.array_equal(e1[0], e1[1]) and abs(e1.std() - 0.2) < 0.1
    assert not np.array_equal(e1[0], P.feature_table(CASES["df"], 1, 20, seed=5)[0, :, 1])   # not the table's stream
    # known bits: PCG64 seeded with (s, seed) — the table does not change under a refactoring
    ref = np.random.default_rng([1, 5])
    assert np.array_equal(t1[1, :50, 1:3], ref.standard_normal((50, 2)) / 6.0)


def test_parts_and_refusals_of_the_table():
    assert [p["part"] for p in P.kernel_parts(CASES["mixed"])] == ["df", "cf"]
    assert [(p["part"], p["length"]) for p in P.kernel_parts(CASES["sum"])] == [("df", 6.0), ("cf", 2.5), ("df", 1.5)]
    assert [round(p["c"], 12) for p in P.kernel_parts(CASES["sum"])] == [0.42, 0.28, 1.8]
    assert [round(p["c"], 12) for p in P.kernel_parts(ST_A)] == [0.6, 1.4] and P.kernel_parts(ST_A)[0]["l_t"] == 1.5
    assert len(P.kernel_parts(spec(kind="mixed", ratio=1.0))) == 1   # a vanishing part is absent
    with pytest.raises(ValueError, match="scalar kind"):
        P.kernel_parts(spec(kind="scalar"))
    with pytest.raises(ValueError, match="'ard'"):
        P.kernel_parts(spec("ard"))
    with pytest.raises(ValueError, match="n_draws"):
        P.feature_table(CASES["df"], 0)
    with pytest.raises(ValueError, match="negative weight"):
        P.feature_table(spec("vector_sum", terms=(spec(),), weights=(-1.0,)), 1, 4)


# ---------------------------------------------------------------- the reference's own consistency
def test_reference_gradient_is_the_derivative_of_its_velocity():
    """paths_ref.DrawFlow.gradient against central differences of its velocity (what fmax rests on)."""
    x, y = A.tracks(30)
    ks = spec(kind="mixed", l_df=A.L_DF, l_cf=A.L_CF, ratio=0.35)
    terms, weights = terms_of(ks)
    table = P.feature_table(ks, 1, 16, seed=2)
    flow = PR.draw_flows(terms, weights, x, y, A.NOISE, table, P.noise_draws(1, 60, A.NOISE, seed=2))[0]
    p, h = A.seeds(x, 20, seed=3), 1e-5
    g = flow.gradient(p, 0.0)
    for b in range(2):
        e = np.zeros(2)
        e[b] = h
        fd = (flow.velocity(p + e, 0.0) - flow.velocity(p - e, 0.0)) / (2 * h)
        assert np.max(np.abs(fd - g[:, :, b])) < 1e-8 * max(1.0, np.max(np.abs(g)))


# ---------------------------------------------------------------- the entry points' host checks
def _lib():
    from gp2d import _native as N
    return N, N.lib()


def test_entry_points_are_exported_within_abi_11():
    N, L = _lib()
    for s in ("gp2d_paths_eval", "gp2d_advect_draws"):
        assert s in N.EXPORTS and hasattr(L, s), s
    assert L.gp2d_abi_version() == 11


def test_host_checks_refuse_before_any_device_work():
    """Every refusal names its parameter; the calls return before a device is touched (this test
    runs without one), with dangling-looking but never dereferenced pointers."""
    N, L = _lib()
    buf = (ctypes.c_double * 8)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    k = N.vector_kernel_desc(N.KIND_DIVFREE, 5.0, 5.0, 1.0)
    kb = ctypes.byref(k)

    def draws(alpha=p, n=128, xtr=p, ntr=1, ntr_pad=64, kern=kb, feat=p, nfeat=1, ndraws=1, x0=p, m=1, per=0, t0=0.0,
              dt=0.5, nsteps=1, save_every=1, s=1.0, path=p):
        return L.gp2d_advect_draws(alpha, n, xtr, ntr, ntr_pad, kern, feat, nfeat, ndraws, x0, m, per, t0, dt, nsteps,
                                   save_every, s, path, None)

    def evalv(alpha=p, n=128, xtr=p, ntr=1, ntr_pad=64, kern=kb, feat=p, nfeat=1, ndraws=1, xg=p, m=1, dim=2, t=0.0,
              vel=p):
        return L.gp2d_paths_eval(alpha, n, xtr, ntr, ntr_pad, kern, feat, nfeat, ndraws, xg, m, dim, t, vel, None)

    def refused(rc, word):
        msg = L.gp2d_last_error().decode(errors="replace")
        assert rc != 0 and word in msg, (rc, msg)

    scalar = N.vector_kernel_desc(N.KIND_SCALAR, 5.0, 5.0, 1.0)
    ard = N.ard_kernel_desc([1.0], [[3.0, 4.0]])
    for call, who in ((draws, "advect_draws"), (evalv, "paths_eval")):
        refused(call(nfeat=-1), f"{who}: nfeat")
        refused(call(ndraws=0), f"{who}: ndraws must be >= 1")
        refused(call(ndraws=65536), f"{who}: ndraws must be <= 65535")
        refused(call(feat=None), f"{who}: feat is NULL")
        refused(call(kern=ctypes.byref(scalar)), f"{who}: k must be")
        refused(call(kern=ctypes.byref(ard)), f"{who}: k must be")
        refused(call(n=64), f"{who}: n must equal")
        refused(call(ntr=65), f"{who}: ntr must be")
    refused(draws(per=2), "x0_per_draw")
    refused(draws(dt=0.0), "dt must be")
    refused(draws(save_every=0), "save_every")
    refused(draws(nsteps=-1), "nsteps")
    refused(draws(x0=None), "x0 is NULL")
    refused(draws(kern=None), "k is invalid")
    refused(evalv(kern=None), "alpha and k")
    refused(evalv(alpha=None), "alpha and k")
    refused(evalv(dim=3), "dim must be 2")
    refused(evalv(alpha=None, kern=None, dim=4), "dim must be 2 (x1, x2) or 3")
    refused(evalv(t=float("nan")), "t must be finite")
    # m = 0: nothing to do, no launch, also without a device
    assert draws(m=0) == 0 and evalv(m=0) == 0 and evalv(alpha=None, kern=None, m=0, dim=3) == 0
