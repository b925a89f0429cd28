"""A background flow estimated with the fit (trend='constant' | 'linear') on the device against
tests/trend_ref.py.

Training sets: 100 points (pad 128, n = 256: padded rows live) and 130 points (pad 192, n = 384);
70 targets with chunk = 64 (two chunks, the last ragged), the first three on observations (the
smallest variances).  Data: tests/test_gpu_sum.py's generator plus a background flow of order 1 m/s
with a linear shear (trend_ref.data), so β̂ is far from zero.  Kernels: plain mixed vector2d, its
spatio-temporal product, and the two-term sum.

Tolerances, each the gate of the test it extends: β̂, α′, A⁻¹ and the posterior mean / variance 1e-10
of the largest entry (test_gpu_parity, test_gpu_fields, test_gpu_sum); the term means plus the
trend 1e-12 of the largest entry (test_gpu_sum); REML 1e-10 relative and its gradient 1e-6 of the
largest entry (test_gpu_lml); far from the data 1e-6 absolute on the mean (K* ≈ e⁻⁵⁰ there).
"""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
if not torch.cuda.is_available():  # pragma: no cover
    pytest.skip("no HIP device", allow_module_level=True)

import krig  # noqa: E402
import trend_ref as T  # noqa: E402
from gp2d import _native as N  # noqa: E402
from gp2d import engine as E  # noqa: E402
from gp2d import hyper as H  # noqa: E402

DEV = torch.device("cuda")
NOISE = T.NOISE
CHUNK = 64
CASES = tuple(T.CASES)
NAMES = ("constant", "linear")


def rel(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return float(np.max(np.abs(a - b)) / max(np.max(np.abs(b)), 1e-300))


def host(t):
    return t.cpu().numpy()


def term_spec(t):
    if T.S.is_st(t):
        return E.KernelSpec(family="vector_st", **t)
    return E.KernelSpec(**t)


def spec_of(case):
    terms, weights = T.CASES[case]
    if case == "sum":
        return E.KernelSpec(family="vector_sum", terms=tuple(term_spec(t) for t in terms), weights=tuple(weights))
    return term_spec(terms[0])


@functools.lru_cache(maxsize=None)
def fit(case, n, order):
    x, y, _ = T.case_data(case, n)
    return E.fit(spec_of(case), np.array(x), np.array(y), noise=NOISE, device=DEV, trend=NAMES[order])


@functools.lru_cache(maxsize=None)
def plain_fit(case, n):
    x, y, _ = T.case_data(case, n)
    return E.fit(spec_of(case), np.array(x), np.array(y), noise=NOISE, device=DEV)


def unpad(v, gp):
    """The valid entries [u…, v…] of a padded component-major vector, and the padded ones."""
    a = host(v).reshape(2, gp.n_pad)
    return a[:, :gp.n_train].reshape(-1), a[:, gp.n_train:]


ALL = [pytest.param(c, n, o, id=f"{c}-{n}-{NAMES[o]}") for c in CASES for n in T.SIZES for o in (0, 1)]


# ---------------------------------------------------------------- 1. the fit
@pytest.mark.parametrize("case,n,order", ALL)
def test_fit_matches_reference(case, n, order):
    gp, r = fit(case, n, order), T.ref(case, n, order)
    assert (gp.n_pad, gp.n) == {100: (128, 256), 130: (192, 384)}[n]
    t = gp.extra["trend"]
    assert t["order"] == order and t["centre"] == tuple(r.centre) and t["scale"] == r.scale
    c = E.trend_coefficients(gp)
    alpha, pad = unpad(gp.alpha, gp)
    block = host(t["block"])
    rhs = block[N.TREND_RHS:].reshape(gp.n, N.TREND_RHS_LD)
    B0 = np.concatenate([rhs[:n, 1:1 + r.q], rhs[gp.n_pad:gp.n_pad + n, 1:1 + r.q]])
    e = dict(beta=rel(c["beta"], r.beta), alpha=rel(alpha, r.alpha), Ainv=rel(c["cov"], r.Ainv), B0=rel(B0, r.B0),
             logdet=abs(c["logdet"] - np.linalg.slogdet(r.A)[1]))
    print(f"{case} N={n} {NAMES[order]}: {e}; beta {c['beta']}")
    assert all(v <= 1e-10 for v in e.values()), e
    assert not pad.any() and np.array_equal(rhs[:, 0], host(gp.alpha))       # right-hand side 0 is α′
    assert not rhs[:, 1 + r.q:].any() and block[N.TREND_STATUS] == 0.0
    assert np.array_equal(c["cov"], c["cov"].T)
    # the physical reading
    assert np.array_equal(c["mean_flow"], c["beta"][:2])
    assert np.array_equal(c["gradient"], c["beta"][2:] / t["scale"] if order else np.zeros(4))
    assert np.all(np.abs(c["mean_flow"] - [0.8, -0.5]) < 0.5)   # the generator's background flow, roughly


# ---------------------------------------------------------------- 2. predict
@pytest.mark.parametrize("case,n,order", ALL)
def test_predict_matches_reference(case, n, order):
    _, _, xg = T.case_data(case, n)
    gp, r = fit(case, n, order), T.ref(case, n, order)
    mo, vo = r.predict(xg)
    pred = E.Predictor(gp, CHUNK)
    for mode, want in (("latent", vo), ("gpy", vo + NOISE), ("sklearn", np.maximum(vo + NOISE, 0.0))):
        mu, var = E.predict(gp, xg, var_mode=mode, chunk=CHUNK)
        em, ev = rel(host(mu), mo), rel(host(var), want)
        print(f"{case} N={n} {NAMES[order]} {mode}: mean {em:.2e}, var {ev:.2e}; min var / max {vo.min() / vo.max():.2e}")
        assert em <= 1e-10 and ev <= 1e-10, (mode, em, ev)
        m2, v2 = E.predict(gp, xg, var_mode=mode, chunk=128)       # one chunk instead of two
        assert torch.equal(mu, m2) and torch.equal(var, v2), mode
        m3, v3 = pred(xg, var_mode=mode)                            # a reused workspace
        assert torch.equal(mu, m3) and torch.equal(var, v3), mode
    mu, none = E.predict(gp, xg, compute_var=False, chunk=CHUNK)
    assert none is None and torch.equal(mu, E.predict(gp, xg, chunk=CHUNK)[0])
    # a workspace made for a zero-mean fit is not handed to a trend fit, or the reverse
    assert not E.Predictor(plain_fit(case, n), CHUNK).fits(gp) and not pred.fits(plain_fit(case, n))
    assert pred.fits(fit(case, n, order)) and not pred.fits(fit(case, n, 1 - order))


# ---------------------------------------------------------------- 3. derived fields
@pytest.mark.parametrize("case,n,order", ALL)
def test_fields_match_reference(case, n, order):
    _, _, xg = T.case_data(case, n)
    gp, r = fit(case, n, order), T.ref(case, n, order)
    for field in E.FIELDS:
        mu, var = E.predict_field(gp, xg, field)
        mo, vo = r.predict_field(xg, field)
        em, ev = rel(host(mu), mo), rel(host(var), vo)
        print(f"{case} N={n} {NAMES[order]} {field}: mean {em:.2e}, var {ev:.2e}")
        assert em <= 1e-10 and ev <= 1e-10, (field, em, ev)
        if order == 0:
            # no divergence or vorticity in a constant: the mean is the GP part's field alone (cᵀα′),
            # and the variance still carries rᵀA⁻¹r with r = −B0ᵀc*
            C = T.S.Fit.field_cross(r, xg, field)
            assert rel(host(mu), C.T @ r.alpha) <= 1e-10
            V = T.sla.solve_triangular(r.L, C, lower=True)
            gp_only = T.S.Fit.field_prior(r, field) - np.einsum("ij,ij->j", V, V)
            R = r.B0.T @ C
            want = np.einsum("ij,ij->j", R, r.Ainv @ R)
            corr = host(var) - gp_only
            print(f"    order 0 {field}: rᵀA⁻¹r up to {want.max():.2e} of a variance up to {vo.max():.2e}")
            assert want.max() > 0.0 and np.max(np.abs(corr - want)) <= 1e-10 * vo.max(), field


@pytest.mark.parametrize("order", [0, 1])
def test_a_field_that_vanishes_by_kind_keeps_the_trends_own(order):
    """A div-free kernel has no divergence: the plain predict answers exact zeros without a launch,
    the trend predict takes the general path with K* = 0 and leaves the trend's divergence
    (β2 + β5)/s with the variance h_δᵀA⁻¹h_δ — the same at every target."""
    n = 130
    x, y, xg = T.case_data("vector2d", n)
    term = dict(kind="df", l_df=8.0, l_cf=1.0, ratio=1.0)
    gp = E.fit(term_spec(term), np.array(x), np.array(y), noise=NOISE, device=DEV, trend=NAMES[order])
    r = T.Fit([term], [1.0], x, y, NOISE, order)
    assert gp.kernel.field_prior_var("divergence") == 0.0
    mu, var = E.predict_field(gp, xg, "divergence")
    mo, vo = r.predict_field(xg, "divergence")
    if order == 0:
        assert not mu.any() and not var.any() and not mo.any() and np.max(np.abs(vo)) == 0.0
    else:
        c = E.trend_coefficients(gp)
        print(f"df kernel, linear trend: divergence {float(mu[0]):.6f} ± {float(var[0]) ** 0.5:.6f}; "
              f"mean {rel(host(mu), mo):.2e}, var {rel(host(var), vo):.2e}")
        assert rel(host(mu), mo) <= 1e-10 and rel(host(var), vo) <= 1e-10
        assert np.allclose(host(mu), (c["beta"][2] + c["beta"][5]) / c["scale"], rtol=1e-12, atol=0.0)
        assert float(var.min()) > 0.0 and rel(host(var), np.full(70, float(var[0]))) <= 1e-12
    zeta, zvar = E.predict_field(gp, xg, "vorticity")
    zo, wo = r.predict_field(xg, "vorticity")
    assert rel(host(zeta), zo) <= 1e-10 and rel(host(zvar), wo) <= 1e-10


def test_term_posteriors_and_the_trend_add_up():
    for n in T.SIZES:
        for order in (0, 1):
            _, _, xg = T.case_data("sum", n)
            gp, r = fit("sum", n, order), T.ref("sum", n, order)
            mu, _ = E.predict(gp, xg, chunk=CHUNK)
            c = E.trend_coefficients(gp)
            total = T.basis(xg, order, c["centre"], c["scale"]).T @ c["beta"]
            for t in range(2):
                mt, vt = E.predict(gp, xg, chunk=CHUNK, term=t)
                mo, vo = r.predict(xg, term=t)
                em, ev = rel(host(mt), mo), rel(host(vt), vo)
                print(f"N={n} {NAMES[order]} term {t}: mean {em:.2e}, var {ev:.2e}")
                assert em <= 1e-10 and ev <= 1e-10, (t, em, ev)
                total = total + host(mt)
                for field in E.FIELDS:
                    ft, wt = E.predict_field(gp, xg, field, term=t)
                    fo, wo = r.predict_field(xg, field, term=t)
                    assert rel(host(ft), fo) <= 1e-10 and rel(host(wt), wo) <= 1e-10, (t, field)
            err = rel(total, host(mu))
            print(f"N={n} {NAMES[order]}: Σ term means + hᵀβ̂ vs the whole {err:.2e}")
            assert err <= 1e-12
            with pytest.raises(ValueError, match="latent"):
                E.predict(gp, xg, var_mode="gpy", term=0)


# ---------------------------------------------------------------- 4. shift invariance
@pytest.mark.parametrize("case,n,order", ALL)
def test_shift_invariance_on_the_device(case, n, order):
    x, y, xg = T.case_data(case, n)
    gp, r = fit(case, n, order), T.ref(case, n, order)
    gamma = np.array([0.7, -1.3, 0.4, -0.2, 0.9, 0.5])[:r.q]
    moved = E.fit(spec_of(case), np.array(x), y + r.H.T @ gamma, noise=NOISE, device=DEV, trend=NAMES[order])
    b0, b1 = E.trend_coefficients(gp)["beta"], E.trend_coefficients(moved)["beta"]
    v0, v1 = E.predict(gp, xg, chunk=CHUNK)[1], E.predict(moved, xg, chunk=CHUNK)[1]
    e = dict(beta=rel(b1 - gamma, b0), alpha=rel(host(moved.alpha), host(gp.alpha)), var=rel(host(v1), host(v0)))
    print(f"{case} N={n} {NAMES[order]}: {e}")
    assert all(v <= 1e-10 for v in e.values()), e
    assert torch.equal(v0, v1)   # the variance never sees y


# ---------------------------------------------------------------- 5. far from the data
@pytest.mark.parametrize("order", [0, 1])
@pytest.mark.parametrize("case", CASES)
def test_far_from_the_data_the_trend_is_what_is_left(case, order):
    n = 130
    x, _, xg = T.case_data(case, n)
    far = np.array(xg[:8])
    far[:, -2:] = [[60 + 80, 45 + 80], [-80, -80], [60 + 80, -80], [-80, 45 + 80], [30, 45 + 80], [30, -80],
                   [60 + 80, 22], [-80, 22]]           # 10 ℓ outside the hull (ℓ = 8)
    gp, r = fit(case, n, order), T.ref(case, n, order)
    mu, var = E.predict(gp, far, chunk=CHUNK)
    m0, v0 = E.predict(plain_fit(case, n), far, chunk=CHUNK)
    prior = gp.kernel.kdiag()
    em = float(np.max(np.abs(host(mu) - r.trend_at(far))))
    e0 = float(np.max(np.abs(host(m0))))
    ev = rel(host(var) - prior, r.trend_var(far))
    print(f"{case} {NAMES[order]}: |mean − hᵀβ̂| {em:.2e}, zero-mean |mean| {e0:.2e}, var − prior vs hᵀA⁻¹h {ev:.2e}; "
          f"hᵀA⁻¹h / prior up to {r.trend_var(far).max() / prior:.2f}")
    assert em <= 1e-6 and e0 <= 1e-6 and ev <= 1e-10
    assert np.max(np.abs(r.trend_at(far))) > 0.3 and float(var.min()) > prior
    assert rel(host(v0), np.full(16, prior)) <= 1e-12


# ---------------------------------------------------------------- 6. the restricted likelihood
@pytest.mark.parametrize("case,n,order", ALL)
def test_reml_and_gradient(case, n, order):
    gp, r = fit(case, n, order), T.ref(case, n, order)
    val, g = E.log_marginal_likelihood(gp, eval_gradient=True)
    oval, og = r.reml(), r.reml_grad(case != "sum")
    names = E.param_names(gp.kernel)
    assert g.shape == (len(names),) == og.shape
    print(f"{case} N={n} {NAMES[order]}: REML {val:.6f} err {abs(val - oval):.2e} of {1e-10 * abs(oval):.2e}; "
          f"grad rel {rel(g, og):.2e}\n  {dict(zip(names, g))}")
    assert abs(val - oval) <= 1e-10 * abs(oval), (val, oval)
    assert rel(g, og) <= 1e-6, (g, og)
    assert E.log_marginal_likelihood(gp) == val
    assert np.array_equal(g, E.log_marginal_likelihood(gp, eval_gradient=True)[1])
    # not the zero-mean likelihood of the same data
    assert abs(val - E.log_marginal_likelihood(plain_fit(case, n))) > 1.0


def test_optimize_with_a_trend_does_not_decrease_the_reml():
    x, y, _ = T.case_data("vector2d", 100)
    spec = spec_of("vector2d")
    start = E.log_marginal_likelihood(fit("vector2d", 100, 1))
    res = H.optimize(spec, np.array(x), np.array(y), NOISE, device=DEV, maxiter=4, trend="linear")
    print(f"REML {start:.4f} -> {res.lml:.4f} in {res.nfev} evaluations: {H.get_params(res.kernel, res.noise)}")
    assert res.lml >= start - 1e-9 * abs(start)
    again = E.fit(res.kernel, np.array(x), np.array(y), noise=res.noise, device=DEV, trend="linear")
    assert E.log_marginal_likelihood(again) == pytest.approx(res.lml, rel=1e-12)
    vals, grads = H.sweep(spec, np.array(x), np.array(y), [dict(), dict(l_df=6.0)], noise=NOISE, device=DEV,
                          eval_gradient=True, trend="linear")
    v0, g0 = E.log_marginal_likelihood(fit("vector2d", 100, 1), eval_gradient=True)
    assert vals[0] == v0 and np.array_equal(grads[0], g0) and vals[1] != v0
    c2 = H.sweep(spec, np.array(x), np.array(y), [dict(), dict(l_df=6.0)], noise=NOISE, device=DEV,
                 eval_gradient=True, concurrent=2, trend="linear")
    assert np.array_equal(c2[0], vals) and np.array_equal(c2[1], grads)


# ---------------------------------------------------------------- 7. trend=None is today's path
@pytest.mark.parametrize("case", CASES)
def test_trend_none_is_bit_identical_to_no_keyword(case):
    n = 130
    x, y, xg = T.case_data(case, n)
    a = plain_fit(case, n)
    b = E.fit(spec_of(case), np.array(x), np.array(y), noise=NOISE, device=DEV, trend=None)
    assert "trend" not in a.extra and "trend" not in b.extra
    assert torch.equal(a.W, b.W) and torch.equal(a.alpha, b.alpha)
    for f in (lambda g: E.predict(g, xg, chunk=CHUNK), lambda g: E.predict(g, xg, var_mode="gpy", chunk=128),
              lambda g: E.predict_field(g, xg, "vorticity"), lambda g: E.predict_field(g, xg, "divergence")):
        (ma, va), (mb, vb) = f(a), f(b)
        assert torch.equal(ma, mb) and torch.equal(va, vb)
    va, ga = E.log_marginal_likelihood(a, eval_gradient=True)
    vb, gb = E.log_marginal_likelihood(b, eval_gradient=True)
    assert va == vb and np.array_equal(ga, gb)
    k0 = krig.Krig(spec_of(case), noise=NOISE).fit(np.array(x), np.array(y))
    k1 = krig.Krig(spec_of(case), noise=NOISE, trend=None).fit(np.array(x), np.array(y))
    assert all(np.array_equal(p, q) for p, q in zip(k0.predict(xg), k1.predict(xg)))
    # and a trend fit is not the zero-mean fit
    assert not torch.equal(fit(case, n, 0).alpha, a.alpha)


# ---------------------------------------------------------------- 8. the drop-in object
@pytest.mark.parametrize("with_factor", [False, True])
@pytest.mark.parametrize("case", CASES)
def test_krig_save_load_round_trip(tmp_path, case, with_factor):
    n = 100
    x, y, xg = T.case_data(case, n)
    k = krig.Krig(spec_of(case), noise=NOISE, trend="linear", chunk=CHUNK).fit(np.array(x), np.array(y))
    assert torch.equal(k.gp.alpha, fit(case, n, 1).alpha)
    m0, v0 = k.predict(xg)
    f0 = k.predict_fields(xg)
    path = str(tmp_path / "model.npz")
    k.save(path, with_factor=with_factor)
    z = np.load(path)
    assert str(z["trend"]) == "linear" and ("W" in z.files) == with_factor
    k2 = krig.Krig.load(path)
    assert k2.trend == "linear" and k2.gp.extra["trend"]["order"] == 1
    m2, v2 = k2.predict(xg)
    assert np.array_equal(m0, m2) and np.array_equal(v0, v2)
    f2 = k2.predict_fields(xg)
    assert all(np.array_equal(f0[f][i], f2[f][i]) for f in E.FIELDS for i in (0, 1))
    assert k2.log_likelihood() == k.log_likelihood()
    c0, c2 = k.trend_coefficients(), k2.trend_coefficients()
    assert np.array_equal(c0["beta"], c2["beta"]) and np.array_equal(c0["cov"], c2["cov"])
    if case != "vector_st":   # a grid of (x, y) points
        uf, vf, uvar, vvar = k2.predict_grid(np.linspace(0, 60, 7), np.linspace(0, 45, 5))
        assert uf.shape == (5, 7) and float(uvar.min()) >= 0.0
        fields = k2.predict_fields_grid(np.linspace(0, 60, 7), np.linspace(0, 45, 5))
        assert fields["vorticity"][0].shape == (5, 7)
    # a file without the trend's order loads as the zero-mean model it was
    plain = krig.Krig(spec_of(case), noise=NOISE).fit(np.array(x), np.array(y))
    plain.save(path)
    assert "trend" not in np.load(path).files
    k3 = krig.Krig.load(path)
    assert k3.trend is None and "trend" not in k3.gp.extra
    assert np.array_equal(k3.predict(xg)[0], plain.predict(xg)[0])


def test_laser_and_kriging_take_the_keyword(tmp_path):
    from gp2d import data as D
    x, y, _ = T.case_data("vector2d", 130)
    u, v = y[:130], y[130:]
    out0 = krig.laser(x[:, 0], x[:, 1], u, v, l_df=8, l_cf=8, rate=0.6, dx=5.0)
    out1 = krig.laser(x[:, 0], x[:, 1], u, v, l_df=8, l_cf=8, rate=0.6, dx=5.0, trend="linear")
    keep, _ = D.split_indices(130, 3)
    k = krig.Krig("mixed", l_df=8, l_cf=8, ratio=0.6, noise=NOISE, trend="linear")
    k.fit(x[keep], np.concatenate([u[keep], v[keep]]))
    uf, vf, uvar, vvar = k.predict_grid(out1[0], out1[1])
    assert np.array_equal(uf, out1[2]) and np.array_equal(vf, out1[3]) and np.array_equal(uvar, out1[8])
    assert out1[2].shape == out0[2].shape and not np.array_equal(out0[2], out1[2])
    tracks = krig.Tracks.synthetic(n_time=24, n_drifters=40)
    out = str(tmp_path / "model")
    m = krig.kriging(0, 24, sample_step=-2, skip=2, output=out, kernelType=2, tracks=tracks, trend="constant",
                     hyper=dict(var_t=1.5, l_t=4.0))["_divFree"]
    assert m.trend == "constant" and m.trend_coefficients()["beta"].shape == (2,)
    f = np.load(out + ".npz")
    back = krig.Krig.load(out + "_divFree.npz")
    assert back.trend == "constant"
    assert all(np.array_equal(a, b) for a, b in zip(m.predict(f["Xt"][:50]), back.predict(f["Xt"][:50])))
    with pytest.raises(ValueError, match="trend"):
        krig.kriging(0, 24, sample_step=-2, skip=2, output=out, kernelType=1, tracks=tracks, trend="constant")


# ---------------------------------------------------------------- 9. a basis that is not identifiable
def test_linear_trend_on_collinear_points_is_a_linalg_error():
    rng = np.random.default_rng(7)
    a = np.sort(rng.uniform(0, 60, 40))
    x = np.stack([a, 3.0 + 0.5 * a], 1)
    y = np.concatenate([0.8 + 0.01 * a, -0.5 + 0.004 * a]) + rng.normal(0, 0.05, 80)
    spec = spec_of("vector2d")
    with pytest.raises(np.linalg.LinAlgError, match="collinear"):
        E.fit(spec, x, y, noise=NOISE, device=DEV, trend="linear")
    gp = E.fit(spec, x, y, noise=NOISE, device=DEV, trend="linear", check=False)   # deferred: a status word
    with pytest.raises(np.linalg.LinAlgError, match="collinear"):
        gp.check()
    assert float(gp.extra["trend"]["block"][N.TREND_STATUS]) > 0
    torch.cuda.synchronize()
    # two distinct points: fewer than three
    with pytest.raises(np.linalg.LinAlgError):
        E.fit(spec, x[:2], np.concatenate([y[:2], y[40:42]]), noise=NOISE, device=DEV, trend="linear")
    # the constant is identifiable on the same points, and the device still answers
    c = E.trend_coefficients(E.fit(spec, x, y, noise=NOISE, device=DEV, trend="constant"))
    assert np.all(np.isfinite(c["beta"])) and c["beta"].shape == (2,)
    vals, _ = H.sweep(spec, x, y, [dict()], noise=NOISE, device=DEV, trend="linear")
    assert vals[0] == -np.inf


# ---------------------------------------------------------------- 10. refusals
def test_entries_without_a_trend_form_refuse_a_trend_fit():
    x, y, xg = (np.array(a) for a in T.case_data("vector2d", 100))
    gp = fit("vector2d", 100, 1)
    spec = gp.kernel
    job = (spec, x, y, NOISE, xg)
    for f in (lambda: E.predict_gradient(gp, xg), lambda: E.predict_cov(gp, xg),
              lambda: E.sample_posterior(gp, xg, 2), lambda: E.cv_points(gp),
              lambda: E.cv_groups(gp, np.arange(100) % 5),
              lambda: E.fit(spec, x, y, NOISE, device=DEV, variance="ozaki", trend="linear"),
              lambda: E.fit_batch([job[:4]], device=DEV, trend="linear"),
              lambda: next(E.krige_jobs([job], variance="f64", device=DEV, trend="linear")),
              lambda: krig.Krig(spec, trend="linear").fit(x, y).predict_cov(xg),
              lambda: krig.Krig(spec, trend="linear").fit(x, y).cross_validate(),
              lambda: krig.Krig(spec, trend="linear").fit(x, y).predict_diagnostics(xg)):
        with pytest.raises(ValueError, match="trend"):
            f()
    # the library refuses what the Python layer would not send
    t = gp.extra["trend"]
    G = E._as_points(xg, 2, DEV)
    out = torch.empty(200, dtype=torch.float64, device=DEV)
    bad = N.trend_desc(2, t["centre"], t["scale"])
    import ctypes
    rc = N.lib().gp2d_predict_trend(*E._f64_fit_args(gp, G, spec.desc()), 0, NOISE, 1, E._ptr(out), E._ptr(out), 64,
                                    E._ptr(out), 1 << 40, E._stream_handle(DEV), ctypes.byref(bad), E._ptr(t["block"]), 1)
    assert rc < 0 and b"order" in N.lib().gp2d_last_error()
