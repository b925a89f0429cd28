"""Divergence and vorticity of the fitted velocity field, with variance (gp2d_predict_field,
engine.predict_field, Krig.predict_fields), against the numpy reference tests/field_ref.py.

Tolerances: cross-covariance entries 1e-13 relative to the matrix max-norm (the gate of
test_gpu_st.test_st_assemble); posterior mean / variance 1e-10 relative normwise (the gate of
test_gpu_st.test_st_fit_predict_vs_oracle for the same fit sizes; the reference's own `inv` and
`chol` recipes differ by ≤ 3.1e-14 on these inputs and the smallest posterior variance is 2.7 % of
the prior, so the gate hides nothing); sharded and whole predictions bit-identical.
"""
import dataclasses
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
if not torch.cuda.is_available():  # pragma: no cover
    pytest.skip("no HIP device", allow_module_level=True)

import field_ref as F  # noqa: E402
from gp2d import data as D  # noqa: E402
from gp2d import engine as E  # noqa: E402
from gp2d.krig import Krig  # noqa: E402
from oracle import gp2d_oracle as O  # noqa: E402

L_DF, L_CF, NOISE = 5.0, 4.0, 0.01
# (kind, ratio, the fields it carries)
CASES = [("df", 1.0, ("vorticity",)), ("cf", 0.0, ("divergence",)), ("mixed", 0.35, F.FIELDS)]
CASE_FIELDS = [(k, r, f) for k, r, fs in CASES for f in fs]


def rel(a, b):
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    return float(np.max(np.abs(a - b)) / max(np.max(np.abs(b)), 1e-300))


def spec(kind, ratio):
    return E.KernelSpec(kind=kind, l_df=L_DF, l_cf=L_CF, ratio=ratio)


@functools.lru_cache(maxsize=None)
def tracks(n, sd=0.05):
    rng = np.random.default_rng(n)
    x = np.stack([rng.uniform(0, 45, n), rng.uniform(0, 60, n)], 1)
    y = np.concatenate([np.sin(x[:, 1] / 7), np.cos(x[:, 0] / 9)]) + sd * rng.normal(0, 1, 2 * n)
    return x, y


def targets(x, m=700, seed=1):
    """m points on [−5, 50] × [−5, 65], the first five on training points (d = 0)."""
    rng = np.random.default_rng(seed)
    g = np.stack([rng.uniform(-5, 50, m), rng.uniform(-5, 65, m)], 1)
    k = min(5, x.shape[0]) if m > 5 else 0
    g[:k] = x[:k]
    return g


@functools.lru_cache(maxsize=None)
def oracle_fit(n, kind, ratio):
    x, y = tracks(n)
    return O.OracleFit(x, y, kind, L_DF, L_CF, ratio, NOISE)


@functools.lru_cache(maxsize=None)
def reference(n, kind, ratio, field):
    """(mean, var, prior) of `field` at targets(tracks(n)) from the oracle's Cholesky fit."""
    x, _ = tracks(n)
    fit = oracle_fit(n, kind, ratio)
    mo, vo = F.fit_predict_field(fit.L, fit.alpha, x, targets(x), field, kind, L_DF, L_CF, ratio)
    return mo, vo, F.prior_var(field, kind, L_DF, L_CF, ratio)


def check_posterior(gp, n, kind, ratio, field, chunk=256):
    x, _ = tracks(n)
    mo, vo, prior = reference(n, kind, ratio, field)
    mu, var = E.predict_field(gp, targets(x), field, chunk=chunk)
    assert mu.shape == var.shape == (700,)
    mu, var = mu.cpu().numpy(), var.cpu().numpy()
    em, ev = rel(mu, mo), rel(var, vo)
    print(f"{kind} {field} N={n}: mean rel {em:.2e}, var rel {ev:.2e}, min var/prior {var.min() / prior:.3f}")
    assert em < 1e-10 and ev < 1e-10, (kind, field, em, ev)
    assert var.min() >= 0.0 and var.max() <= prior * (1 + 1e-12)
    assert gp.kernel.field_prior_var(field) == pytest.approx(prior, rel=1e-15)


# ---- 4. the cross-covariance alone --------------------------------------------------------
@pytest.mark.parametrize("kind,ratio,field", CASE_FIELDS)
@pytest.mark.parametrize("na,m", [(1, 1), (37, 100), (130, 64)])
def test_field_cross_covariance(kind, ratio, field, na, m):
    """With W = I and α = e_k the predicted mean is row k of the assembled matrix and the variance
    is prior − the column's sum of squares: every row of the buffer — the padded ones, which must
    be exact zeros, included — against field_ref.cross.  (1, 1): a single point; (37, 100): ragged
    tiles; (130, 64): na_pad = 192, the second component's rows start past a 64-point tile."""
    rng = np.random.default_rng(na + 7 * m)
    xa = np.stack([rng.uniform(0, 45, na), rng.uniform(0, 60, na)], 1)
    g = targets(xa, m, seed=na)
    dev = torch.device("cuda")
    npad = E.padded_points(na)
    n = 2 * npad
    assert n % 128 == 0 and npad == {1: 64, 37: 64, 130: 192}[na]
    ks = spec(kind, ratio)
    X = torch.as_tensor(xa, device=dev)
    eye = torch.eye(n, dtype=torch.float64, device=dev)
    C = np.empty((n, m))
    var = None
    for k in range(n):
        gp = E.GPFit(kernel=ks, noise=NOISE, x=X, n_train=na, n_pad=npad, W=eye, alpha=eye[k].contiguous(), device=dev)
        mu, v = E.predict_field(gp, g, field, compute_var=(k == 0))
        C[k] = mu.cpu().numpy()
        var = v if k == 0 else var
    ref = F.cross(xa, g, field, kind, L_DF, L_CF, ratio)
    valid = np.r_[0:na, npad:npad + na]
    assert rel(C[valid], ref) < 1e-13
    pad = np.setdiff1d(np.arange(n), valid)
    assert not C[pad].any()
    prior = F.prior_var(field, kind, L_DF, L_CF, ratio)
    assert rel(var.cpu().numpy(), prior - np.sum(ref * ref, 0)) < 1e-13


# ---- 5. posterior against the reference ---------------------------------------------------
@pytest.mark.parametrize("kind,ratio,fields", CASES)
@pytest.mark.parametrize("n", [130, 300, 1000])
def test_field_posterior_vs_reference(kind, ratio, fields, n):
    x, y = tracks(n)
    gp = E.fit(spec(kind, ratio), x, y, NOISE)
    for field in fields:
        check_posterior(gp, n, kind, ratio, field)   # chunk = 256: three chunks, the last ragged


# ---- 6. a fit of the int8 engine gives the same fields -------------------------------------
def test_field_from_ozaki_fit():
    """The ozaki fit keeps x, α and W in Morton order; predict_field uses them as they are."""
    x, y = tracks(300)
    gp = E.fit(spec("mixed", 0.35), x, y, NOISE, variance="ozaki")
    assert gp.perm is not None and gp.W is not None
    for field in F.FIELDS:
        check_posterior(gp, 300, "mixed", 0.35, field)


# ---- 7. exact zeros ------------------------------------------------------------------------
def test_field_exact_zeros():
    x, y = tracks(130)
    g = targets(x)
    zero = torch.zeros(700, dtype=torch.float64, device="cuda")
    for kind, ratio, field in [("df", 1.0, "divergence"), ("cf", 0.0, "vorticity"),
                               ("mixed", 1.0, "divergence")]:   # the last through the general path
        gp = E.fit(spec(kind, ratio), x, y, NOISE)
        junk = [torch.full((700,), float("nan"), dtype=torch.float64, device="cuda") for _ in range(2)]
        del junk                               # the outputs are written over what the allocator hands back
        mu, var = E.predict_field(gp, g, field, chunk=256)
        assert torch.equal(mu, zero) and torch.equal(var, zero), (kind, field)
        assert gp.kernel.field_prior_var(field) == 0.0
        mu, var = E.predict_field(gp, g, field, compute_var=False)
        assert var is None and torch.equal(mu, zero)


# ---- 8. sharding ---------------------------------------------------------------------------
def test_field_sharded_is_bit_identical():
    x, y = tracks(300)
    g = targets(x, 300)
    gp = E.fit(spec("mixed", 0.35), x, y, NOISE)
    for field in F.FIELDS:
        mu, var = (t.cpu().numpy() for t in E.predict_field(gp, g, field, chunk=1024))
        parts = []
        for r in range(2):
            lo, hi = D.shard_range(300, 2, r)
            parts.append([t.cpu().numpy() for t in E.predict_field(gp, g[lo:hi], field, chunk=128)])
        assert np.array_equal(mu, np.concatenate([p[0] for p in parts]))
        assert np.array_equal(var, np.concatenate([p[1] for p in parts]))


# ---- 9. spatio-temporal product ------------------------------------------------------------
def st_tracks(n, seed):
    """The (T, Y, X) tracks of test_gpu_st.py: observations [v; u]."""
    rng = np.random.default_rng(seed)
    X = np.stack([rng.uniform(0, 6, n), rng.uniform(0, 45, n), rng.uniform(0, 60, n)], 1)
    v = np.cos(X[:, 2] / 9) + 0.1 * X[:, 0] + rng.normal(0, 0.05, n)
    u = np.sin(X[:, 1] / 7) - 0.05 * X[:, 0] + rng.normal(0, 0.05, n)
    return X, np.concatenate([v, u])


def test_field_spatio_temporal():
    import scipy.linalg as sla
    X, y = st_tracks(300, seed=300)
    rng = np.random.default_rng(1)
    G = np.stack([rng.uniform(-1, 7, 700), rng.uniform(-5, 50, 700), rng.uniform(-5, 65, 700)], 1)
    G[:5] = X[:5]
    assert G[:, 0].min() < 0 and G[:, 0].max() > 6          # times outside the tracks' [0, 6]
    kw = dict(kind="mixed", l_df=L_DF, l_cf=L_CF, ratio=0.35, var_t=2.0, l_t=1.5)
    K = O.vector_st_kernel(X, X, **kw)
    K[np.diag_indices_from(K)] += NOISE
    Lo = np.linalg.cholesky(K)
    alpha = sla.cho_solve((Lo, True), y)
    ks = E.KernelSpec(family="vector_st", **kw)
    gp = E.fit(ks, X, y, NOISE)
    for field in F.FIELDS:
        mo, vo = F.fit_predict_field(Lo, alpha, X, G, field, "mixed", L_DF, L_CF, 0.35, var_t=2.0, l_t=1.5)
        prior = F.prior_var(field, "mixed", L_DF, L_CF, 0.35, var_t=2.0)
        mu, var = (t.cpu().numpy() for t in E.predict_field(gp, G, field, chunk=256))
        em, ev = rel(mu, mo), rel(var, vo)
        print(f"st {field}: mean rel {em:.2e}, var rel {ev:.2e}")
        assert em < 1e-10 and ev < 1e-10, (field, em, ev)
        assert var.min() >= 0.0 and var.max() <= prior * (1 + 1e-12)
        assert ks.field_prior_var(field) == pytest.approx(prior, rel=1e-15)


# ---- 10. the Krig surface and the sign convention ------------------------------------------
def test_krig_predict_fields_grid():
    """The centred difference of the velocity grid carries its own truncation error dx²/6·|f‴|:
    for the observed u = sin(y/7), v = cos(x/9) that is 0.25/6/49 = 8.5e-4 and 0.25/6/81 = 5.1e-4
    of the two terms of ζ, below the 1e-3 only where the posterior mean follows them closely —
    structure on the kernel's own scale ℓ = 5 has |f‴/f′| up to 3/ℓ², six times more.  So this test
    fits 1000 noise-free observations, and its 12 × 9 grid lies where both terms of ζ have one
    sign (ζ ≈ −0.23), away from the zero crossings where a sign comparison means nothing."""
    x, y = tracks(1000, sd=0.0)
    kr = Krig(kernel="df", l_df=5.0, noise=NOISE).fit(x, y)
    gx, gy = 10.0 + 0.5 * np.arange(12), 40.0 + 0.5 * np.arange(9)
    out = kr.predict_fields_grid(gx, gy)
    assert set(out) == set(E.FIELDS)
    XX, YY = np.meshgrid(gx, gy)
    pts = np.stack([XX.reshape(-1), YY.reshape(-1)], 1)
    for name in E.FIELDS:
        mu, var = out[name]
        assert mu.shape == var.shape == (9, 12)
        dm, dv = E.predict_field(kr.gp, pts, name)
        assert np.array_equal(mu, dm.cpu().numpy().reshape(9, 12))
        assert np.array_equal(var, dv.cpu().numpy().reshape(9, 12))
    flat = kr.predict_fields(pts, fields=("vorticity",))
    assert set(flat) == {"vorticity"} and np.array_equal(flat["vorticity"][0].reshape(9, 12), out["vorticity"][0])
    # ζ = ∂v/∂x − ∂u/∂y for points (x, y) and components (u, v): a centred difference of the
    # predicted velocity grid (dx = 0.5) pins the sign; its own truncation error is the 1e-3
    uf, vf, _, _ = kr.predict_grid(gx, gy)
    fd = (vf[1:-1, 2:] - vf[1:-1, :-2]) / 1.0 - (uf[2:, 1:-1] - uf[:-2, 1:-1]) / 1.0
    zeta = out["vorticity"][0][1:-1, 1:-1]
    print(f"vorticity vs centred difference: rel {rel(zeta, fd):.2e}")
    assert rel(zeta, fd) < 1e-3
    assert np.array_equal(np.sign(zeta), np.sign(fd))


# ---- 11. what has no derived field ---------------------------------------------------------
def test_predict_field_refuses_scalar_ard_and_planes_only_fits():
    x, y = tracks(130)
    gp = E.fit(spec("df", 1.0), x, y, NOISE)
    g = targets(x, 10)
    with pytest.raises(ValueError, match="vector kernel"):
        E.predict_field(dataclasses.replace(gp, kernel=E.KernelSpec(kind="scalar")), g, "vorticity")
    ard = E.KernelSpec(family="ard", variances=(1.0,), lengthscales=((5.0, 5.0),))
    with pytest.raises(ValueError, match="vector kernel"):
        E.predict_field(dataclasses.replace(gp, kernel=ard), g, "divergence")
    with pytest.raises(ValueError, match="W"):
        E.predict_field(dataclasses.replace(gp, W=None, n_mat=gp.n), g, "vorticity")
    with pytest.raises(ValueError, match="field must be one of"):
        E.predict_field(gp, g, "strain")
    sc = Krig(kernel="scalar", l_df=5.0, noise=NOISE).fit(x, y)
    with pytest.raises(ValueError, match="vector kernel"):
        sc.predict_fields(g)
