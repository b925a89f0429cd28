"""Sums of vector kernels (GP2D_FAMILY_VECTOR_SUM) on the device against tests/sum_ref.py.

Training sets: 100 points (pad 128, n = 256: padded rows live) and 130 points (pad 192, n = 384);
70 targets with chunk = 64 (two chunks, the last ragged).  Terms: a mesoscale mixed term (ℓ 8 / 8,
ratio 0.6, weight 1) and a submesoscale div-free term (ℓ 2, weight 0.05), noise 0.0025; the
spatio-temporal case carries the same points with a time column and the amplitudes in var_t.

Tolerances, each the gate of the one-term test it extends: assembly 1e-13 of the matrix max-norm
(test_gpu_parity); posterior mean / variance 1e-10 relative to the largest entry (test_gpu_parity,
test_gpu_fields); the term means add up to the whole within 1e-12 of the largest entry (T roundings
of an n-term dot product); LML 1e-10 relative, its gradient 1e-6 and the dense kernel gradient 1e-7
of the largest entry (test_gpu_lml); cross-validation 1e-10 in test_gpu_cv's norms.  A one-term sum
of weight 1 gives the bits of its term.
"""
import ctypes
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
if not torch.cuda.is_available():  # pragma: no cover
    pytest.skip("no HIP device", allow_module_level=True)

import cv_ref as CV  # noqa: E402
import krig  # noqa: E402
import sum_ref as S  # noqa: E402
from gp2d import _native as N  # noqa: E402
from gp2d import engine as E  # noqa: E402

DEV = torch.device("cuda")
NOISE = 0.0025
CHUNK = 64
SIZES = (100, 130)

T2D = (dict(kind="mixed", l_df=8.0, l_cf=8.0, ratio=0.6), dict(kind="df", l_df=2.0, l_cf=1.0, ratio=1.0))
W2D = (1.0, 0.05)
TST = (dict(kind="mixed", l_df=8.0, l_cf=8.0, ratio=0.6, var_t=1.0, l_t=3.0),
       dict(kind="df", l_df=2.0, l_cf=1.0, ratio=1.0, var_t=0.05, l_t=1.0))
WST = (1.0, 1.0)


def rel(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return float(np.max(np.abs(a - b)) / max(np.max(np.abs(b)), 1e-300))


def host(t):
    return t.cpu().numpy()


def term_spec(t):
    if S.is_st(t):
        return E.KernelSpec(family="vector_st", **t)
    return E.KernelSpec(**t)


def sum_spec(terms, weights):
    return E.KernelSpec(family="vector_sum", terms=tuple(term_spec(t) for t in terms), weights=tuple(weights))


def case(st):
    return (TST, WST) if st else (T2D, W2D)


@functools.lru_cache(maxsize=None)
def data(n, st):
    """(x, y, xg): two-scale observations [u…, v…] at n points, 70 targets; shared by the tests, which never modify them."""
    rng = np.random.default_rng(2016 + n)
    x = np.stack([rng.uniform(0, 60, n), rng.uniform(0, 45, n)], 1)
    xg = np.stack([rng.uniform(-3, 63, 70), rng.uniform(-3, 48, 70)], 1)
    xg[:3] = x[:3]                              # targets on observations: the smallest variances
    if st:
        x = np.concatenate([rng.uniform(0, 6, (n, 1)), x], 1)
        xg = np.concatenate([rng.uniform(-1, 7, (70, 1)), xg], 1)
        xg[:3] = x[:3]
    a, b = x[:, -2], x[:, -1]
    y = np.concatenate([np.sin(b / 7) + 0.2 * np.sin(a / 1.5), np.cos(a / 9) + 0.2 * np.cos(b / 1.5)])
    y = y + rng.normal(0, 0.05, 2 * n)
    return x, y, xg


@functools.lru_cache(maxsize=None)
def ref(n, st):
    x, y, _ = data(n, st)
    return S.Fit(*case(st), x, y, NOISE)


@functools.lru_cache(maxsize=None)
def fit(n, st):
    x, y, _ = data(n, st)
    return E.fit(sum_spec(*case(st)), np.array(x), np.array(y), noise=NOISE, device=DEV)


# ---------------------------------------------------------------- 1. one-term bit identity
SENTINEL = -7.0


def raw_assemble(spec, x, sym):
    """gp2d_assemble(x, x) into a sentinel-filled padded matrix: what the call leaves unwritten
    keeps the sentinel, so equal tensors also wrote the same elements."""
    X = E._as_points(np.array(x), spec.input_dim, DEV)
    na, nap = X.shape[0], E.padded_points(X.shape[0])
    out = torch.full((2 * nap, 2 * nap), SENTINEL, dtype=torch.float64, device=DEV)
    desc = spec.desc()
    N.check(N.lib().gp2d_assemble(E._ptr(X), na, nap, E._ptr(X), na, nap, ctypes.byref(desc), NOISE, sym,
                                  E._ptr(out), out.shape[1], E._stream_handle(DEV)), "gp2d_assemble")
    return out


def raw_assemble_cols(spec, x, c0, ncols):
    X = E._as_points(np.array(x), spec.input_dim, DEV)
    na, nap = X.shape[0], E.padded_points(X.shape[0])
    out = torch.full((2 * nap, 2 * nap), SENTINEL, dtype=torch.float64, device=DEV)
    desc = spec.desc()
    N.check(N.lib().gp2d_assemble_cols(E._ptr(X), na, nap, ctypes.byref(desc), NOISE, E._ptr(out), out.shape[1],
                                       c0, ncols, E._stream_handle(DEV)), "gp2d_assemble_cols")
    return out


@pytest.mark.parametrize("st", [False, True])
@pytest.mark.parametrize("n", SIZES)
def test_one_term_sum_of_weight_one_is_its_term_to_the_bit(n, st):
    x, y, xg = data(n, st)
    plain = term_spec(case(st)[0][0])
    one = sum_spec(case(st)[0][:1], (1.0,))
    nap = E.padded_points(n)
    for sym in (0, 1, 2):
        a, b = raw_assemble(plain, x, sym), raw_assemble(one, x, sym)
        assert torch.equal(a, b), (sym, int((a != b).sum()))
        written = int((a != SENTINEL).sum())
        assert written == (4 * nap * nap if sym < 2 else nap * (2 * nap + 1)), (sym, written)
    for c0, ncols in ((0, 64), (nap + 64, 64), (nap, nap)):
        a, b = raw_assemble_cols(plain, x, c0, ncols), raw_assemble_cols(one, x, c0, ncols)
        assert torch.equal(a, b), (c0, ncols)
        assert torch.equal(a[:, c0:c0 + ncols], raw_assemble(one, x, 1)[:, c0:c0 + ncols])
        assert int((a != SENTINEL).sum()) == 2 * nap * ncols
    ga = E.fit(plain, np.array(x), np.array(y), noise=NOISE, device=DEV)
    gb = E.fit(one, np.array(x), np.array(y), noise=NOISE, device=DEV)
    assert torch.equal(ga.W, gb.W) and torch.equal(ga.alpha, gb.alpha)
    for mode in ("latent", "gpy"):
        ma, va = E.predict(ga, xg, var_mode=mode, chunk=CHUNK)
        mb, vb = E.predict(gb, xg, var_mode=mode, chunk=CHUNK)
        assert torch.equal(ma, mb) and torch.equal(va, vb), mode
    assert one.kdiag() == plain.kdiag()


# ---------------------------------------------------------------- 2. two-term assembly
@pytest.mark.parametrize("st", [False, True])
@pytest.mark.parametrize("n", SIZES)
def test_two_term_assembly_matches_reference(n, st):
    x, _, xg = data(n, st)
    terms, weights = case(st)
    spec = sum_spec(terms, weights)
    Ky = host(E.assemble(spec, x, diag_add=NOISE))
    want = S.ky(terms, weights, x, NOISE)
    e1 = float(np.max(np.abs(Ky - want)) / np.max(np.abs(want)))
    Ks = host(E.assemble(spec, xg, x))
    want = S.k_sum(terms, weights, xg, x)
    e2 = float(np.max(np.abs(Ks - want)) / np.max(np.abs(want)))
    print(f"N={n} st={st}: K_y {e1:.2e}, K* {e2:.2e} of max|K|")
    assert e1 <= 1e-13 and e2 <= 1e-13, (e1, e2)
    # the lower-triangle mode holds the same values where it writes
    low = raw_assemble(spec, x, 2)
    full = raw_assemble(spec, x, 1)
    mask = low != SENTINEL
    assert torch.equal(low[mask], full[mask])
    assert torch.equal(mask, torch.ones(mask.shape, device=DEV).tril().bool())


def test_identical_terms_split_the_single_kernel():
    x, _, xg = data(130, False)
    t = T2D[0]
    split = sum_spec((t, t), (0.25, 0.75))
    for xa, xb, add in ((x, None, NOISE), (xg, x, 0.0)):
        got = host(E.assemble(split, xa, xb, diag_add=add))
        want = host(E.assemble(term_spec(t), xa, xb, diag_add=add))
        err = float(np.max(np.abs(got - want)) / np.max(np.abs(want)))
        print(f"0.25·K + 0.75·K vs K: {err:.2e}")
        assert err <= 1e-13


# ---------------------------------------------------------------- 3. fit and predict
@pytest.mark.parametrize("st", [False, True])
@pytest.mark.parametrize("n", SIZES)
def test_fit_predict_matches_reference(n, st):
    _, _, xg = data(n, st)
    gp, r = fit(n, st), ref(n, st)
    assert (gp.n_pad, gp.n) == {100: (128, 256), 130: (192, 384)}[n]
    mu, var = E.predict(gp, xg, chunk=CHUNK)
    mo, vo = r.predict(xg)
    em, ev = rel(host(mu), mo), rel(host(var), vo)
    print(f"N={n} st={st}: mean {em:.2e}, var {ev:.2e}; min var / prior {vo.min() / vo.max():.2e}")
    assert em < 1e-10 and ev < 1e-10, (em, ev)
    _, vn = E.predict(gp, xg, var_mode="gpy", chunk=CHUNK)
    assert rel(host(vn), vo + NOISE) < 1e-10


# ---------------------------------------------------------------- 4. per-term predicts
@pytest.mark.parametrize("st", [False, True])
@pytest.mark.parametrize("n", SIZES)
def test_term_posteriors(n, st):
    _, _, xg = data(n, st)
    gp, r = fit(n, st), ref(n, st)
    mu, _ = E.predict(gp, xg, chunk=CHUNK)
    total = torch.zeros_like(mu)
    for t in range(2):
        mt, vt = E.predict(gp, xg, chunk=CHUNK, term=t)
        mo, vo = r.predict(xg, term=t)
        em, ev = rel(host(mt), mo), rel(host(vt), vo)
        print(f"N={n} st={st} term {t}: mean {em:.2e}, var {ev:.2e}")
        assert em < 1e-10 and ev < 1e-10, (t, em, ev)
        prior = gp.kernel.term(t).kdiag()
        assert float(vt.min()) >= 0.0 and float(vt.max()) <= prior * (1 + 1e-12)
        total += mt
    err = float((total - mu).abs().max() / mu.abs().max())
    print(f"N={n} st={st}: Σ term means vs the whole {err:.2e}")
    assert err <= 1e-12
    for mode in ("gpy", "sklearn", "noisy", "clipped"):
        with pytest.raises(ValueError, match="latent"):
            E.predict(gp, xg, var_mode=mode, term=0)
    with pytest.raises(ValueError, match="term must be"):
        E.predict(gp, xg, term=2)
    plain = E.fit(term_spec(case(st)[0][0]), np.array(data(n, st)[0]), np.array(data(n, st)[1]), noise=NOISE, device=DEV)
    with pytest.raises(ValueError, match="kernel sum"):
        E.predict(plain, xg, term=0)


# ---------------------------------------------------------------- 5. fields
@pytest.mark.parametrize("st", [False, True])
def test_fields_whole_and_per_term(st):
    n = 130
    _, _, xg = data(n, st)
    terms = list(case(st)[0]) + [dict(case(st)[0][1], kind="cf", l_cf=3.0, ratio=0.0)]   # vorticity and divergence in
    weights = list(case(st)[1]) + [0.02 if not st else 1.0]                               # more than one term
    x, y, _ = data(n, st)
    gp = E.fit(sum_spec(terms, weights), np.array(x), np.array(y), noise=NOISE, device=DEV)
    r = S.Fit(terms, weights, x, y, NOISE)
    for field in E.FIELDS:
        for term in (None, 0, 1, 2):
            mu, var = E.predict_field(gp, xg, field, term=term)
            mo, vo = r.predict_field(xg, field, term=term)
            prior = r.field_prior(field, term)
            spec = gp.kernel if term is None else gp.kernel.term(term)
            assert spec.field_prior_var(field) == pytest.approx(prior, rel=1e-15, abs=1e-300)
            if prior == 0.0:      # the field vanishes in every term of this predict: exact zeros
                assert not mu.any() and not var.any(), (field, term)
                continue
            em, ev = rel(host(mu), mo), rel(host(var), vo)
            print(f"st={st} {field} term={term}: mean {em:.2e}, var {ev:.2e}")
            assert em < 1e-10 and ev < 1e-10, (field, term, em, ev)
            assert float(var.min()) >= 0.0 and float(var.max()) <= prior * (1 + 1e-12)


def test_sum_of_divfree_terms_has_no_divergence():
    x, y, xg = data(100, False)
    spec = sum_spec((dict(kind="df", l_df=8.0, l_cf=1.0, ratio=1.0), T2D[1]), (1.0, 0.05))
    gp = E.fit(spec, np.array(x), np.array(y), noise=NOISE, device=DEV)
    mu, var = E.predict_field(gp, xg, "divergence")
    assert mu.shape == var.shape == (70,) and not mu.any() and not var.any()
    assert spec.field_prior_var("divergence") == 0.0 and spec.field_prior_var("vorticity") > 0.0
    zeta, zvar = E.predict_field(gp, xg, "vorticity")
    assert zeta.any() and float(zvar.min()) >= 0.0


# ---------------------------------------------------------------- 6. gradients
@pytest.mark.parametrize("st", [False, True])
@pytest.mark.parametrize("n", SIZES)
def test_lml_and_gradient(n, st):
    x, y, _ = data(n, st)
    terms, weights = case(st)
    gp = fit(n, st)
    val, g = E.log_marginal_likelihood(gp, eval_gradient=True)
    oval, og = S.lml_grad(terms, weights, x, y, NOISE)
    names = E.param_names(gp.kernel)
    assert names == S.param_names(terms) and g.shape == (len(names),)
    print(f"N={n} st={st}: lml err {abs(val - oval):.2e} of {1e-10 * abs(oval):.2e}; grad rel {rel(g, og):.2e}\n"
          f"  {dict(zip(names, g))}")
    assert abs(val - oval) <= 1e-10 * abs(oval), (val, oval)
    assert rel(g, og) < 1e-6, (g, og)
    assert not g[[names.index("l_cf_1"), names.index("ratio_1")]].any()    # a df term uses neither
    _, g2 = E.log_marginal_likelihood(gp, eval_gradient=True)
    assert np.array_equal(g, g2)


@pytest.mark.parametrize("st", [False, True])
def test_kernel_grad_with_a_dense_weight(st):
    x, _, xg = data(130, st)
    terms, weights = case(st)
    spec = sum_spec(terms, weights)
    rng = np.random.default_rng(3)
    for xa, xb in ((x, None), (x[:37], xg)):
        nb = (xa if xb is None else xb).shape[0]
        G = rng.normal(0, 1, (2 * xa.shape[0], 2 * nb))
        got = E.kernel_grad(spec, xa, G, xb, device=DEV)
        want = S.kernel_grad(terms, weights, xa, xa if xb is None else xb, G)
        assert got.shape == (len(E.param_names(spec)) - 1,)
        print(f"st={st} {xa.shape[0]}×{nb}: kernel_grad rel {rel(got, want):.2e}")
        assert rel(got, want) < 1e-7, (got, want)
        assert np.array_equal(got, E.kernel_grad(spec, xa, G, xb, device=DEV))


# ---------------------------------------------------------------- 7. cross-validation
@pytest.mark.parametrize("st", [False, True])
def test_cv_points_on_a_sum_fit(st):
    n = 130
    _, y, _ = data(n, st)
    gp, r = fit(n, st), ref(n, st)
    Li = np.linalg.inv(r.L)
    P = Li.T @ Li
    alpha = P @ y
    mean, var, cuv, lpd = np.empty(2 * n), np.empty(2 * n), np.empty(n), np.empty(n)
    chi2 = 0.0
    for i in range(n):
        idx = CV.components([i], n, 2)
        m, c, lpd[i] = CV.closed_group(P, alpha, y, idx)
        mean[idx], var[idx], cuv[i] = m, np.diag(c), c[0, 1]
        chi2 += float(alpha[idx] @ (c @ alpha[idx]))
    want = CV.scores(y - mean, lpd.sum(), chi2, n, n, 2)
    got = E.cv_points(gp)
    ymax = float(np.max(np.abs(y)))
    v = var.reshape(2, n)
    e = dict(mean=float(np.max(np.abs(host(got["mean"]) - mean)) / ymax),
             var=float(np.max(np.abs(host(got["var"]) - var) / var)),
             cuv=float(np.max(np.abs(host(got["cuv"]) - cuv) / np.sqrt(v[0] * v[1]))),
             lpd=float(np.max(np.abs(host(got["lpd"]) - lpd) / np.maximum(1.0, np.abs(lpd)))))
    for k, w in want.items():
        e[k] = abs(got[k] - w) / max(1.0, abs(w))
    print(f"cv_points on a sum fit st={st}: {e}")
    assert all(x < 1e-10 for x in e.values()), e


def test_cv_groups_fit_batch_and_sweep_take_sums():
    """The entries that never look at the kernel, and the layers that only pass it on."""
    from gp2d import hyper as H
    n = 130
    x, y, _ = data(n, False)
    gp, r = fit(n, False), ref(n, False)
    labels = np.arange(n) % 5
    got = E.cv_groups(gp, labels)
    Li = np.linalg.inv(r.L)
    P = Li.T @ Li
    alpha = P @ y
    for g in range(5):
        idx = CV.components(np.flatnonzero(labels == g), n, 2)
        m, c, lpd = CV.closed_group(P, alpha, y, idx)
        assert rel(host(got["mean"])[idx], m) < 1e-10 and rel(host(got["var"])[idx], np.diag(c)) < 1e-10
        assert abs(float(got["lpd"][g]) - lpd) < 1e-10 * max(1.0, abs(lpd))
    # a batched fit gives each problem the lone fit's bits
    other = sum_spec(T2D, (0.5, 0.1))
    a, b = E.fit_batch([(gp.kernel, np.array(x), np.array(y), NOISE), (other, np.array(x), np.array(y), 0.01)],
                       device=DEV)
    assert torch.equal(a.W, gp.W) and torch.equal(a.alpha, gp.alpha)
    lone = E.fit(other, np.array(x), np.array(y), noise=0.01, device=DEV)
    assert torch.equal(b.W, lone.W) and torch.equal(b.alpha, lone.alpha)
    # a sweep over per-term settings is the fits one by one
    settings = [dict(l_df_1=2.0, weight_1=0.05), dict(l_df_1=3.0, weight_1=0.1, noise=0.01)]
    vals, grads = H.sweep(gp.kernel, np.array(x), np.array(y), settings, noise=NOISE, device=DEV, eval_gradient=True)
    v0, g0 = E.log_marginal_likelihood(gp, eval_gradient=True)
    assert vals[0] == v0 and np.array_equal(grads[0], g0)
    k1, nz1 = H.set_params(gp.kernel, dict(H.get_params(gp.kernel, NOISE), **settings[1]))
    v1, g1 = E.log_marginal_likelihood(E.fit(k1, np.array(x), np.array(y), noise=nz1, device=DEV), eval_gradient=True)
    assert vals[1] == v1 and np.array_equal(grads[1], g1)


# ---------------------------------------------------------------- 8. the drop-in path
@functools.lru_cache(maxsize=None)
def synthetic_tracks():
    return krig.Tracks.synthetic(n_time=24, n_drifters=40)


@pytest.mark.parametrize("kernel_type,hyper,family", [
    (2, dict(l_df=[8.0, 2.0], var_t=[1.0, 0.05], l_t=[4.0, 1.0]), "vector_st"),
    (4, dict(l_df=[8.0, 2.0], l_cf=[8.0, 3.0], ratio=[0.6, 0.5], variance=[1.0, 0.05], temporal=False), "vector2d"),
])
def test_kriging_two_kernels_save_load_restarts(tmp_path, capsys, kernel_type, hyper, family):
    out = str(tmp_path / "model")
    tag = {2: "_divFree", 4: "_combined"}[kernel_type]
    models = krig.kriging(0, 24, sample_step=-2, skip=2, nKernels=2, output=out, kernelType=kernel_type,
                          tracks=synthetic_tracks(), hyper=hyper)
    k = models[tag]
    s = k.spec
    assert s.family == "vector_sum" and len(s.terms) == 2 and {t.family for t in s.terms} == {family}
    assert [t.l_df for t in s.terms] == [8.0, 2.0]
    assert s.weights == ((1.0, 1.0) if family == "vector_st" else (1.0, 0.05))
    assert k.param_array.shape == (len(E.param_names(s)),) and k.param_array[-1] == k.noise
    f = np.load(out + ".npz")
    pts = f["Xt"][:50] if family == "vector_st" else f["Xt"][:50, 1:3]
    m0, v0 = k.predict(pts)
    k2 = krig.Krig.load(out + tag + ".npz")
    assert k2.spec == s
    m2, v2 = k2.predict(pts)
    assert np.array_equal(m2, m0) and np.array_equal(v2, v0)
    # the terms' contributions add up, and come with their own (latent) error bars
    mt = [k2.predict(pts, term=t) for t in range(2)]
    assert rel(mt[0][0] + mt[1][0], m0) < 1e-12
    assert all(float(v.min()) >= 0.0 for _, v in mt)
    fields = k2.predict_fields(pts, term=1)
    assert set(fields) == set(E.FIELDS) and fields["vorticity"][0].shape == (50,)
    start = k2.log_likelihood()
    res = krig.runRestarts(out + tag, nres=2)
    printed = capsys.readouterr().out
    for t in range(2):
        assert f"l_df_{t} = " in printed and f"weight_{t} = " in printed
    print(f"kernelType {kernel_type}: LML {start:.6f} -> {res.lml:.6f} in {res.nfev} evaluations of the best run")
    assert res.lml >= start - 1e-9 * abs(start), (res.lml, start)
    k3 = krig.Krig.load(out + tag + ".npz")
    assert k3.spec.family == "vector_sum" and k3.log_likelihood() == pytest.approx(res.lml, rel=1e-10)


def test_kriging_one_kernel_is_the_plain_model(tmp_path):
    out = str(tmp_path / "model")
    k = krig.kriging(0, 24, sample_step=-2, skip=2, nKernels=1, output=out, kernelType=2, tracks=synthetic_tracks(),
                     hyper=dict(var_t=1.5, l_t=4.0))["_divFree"]
    assert k.spec.family == "vector_st" and k.spec.terms == ()
    z = np.load(out + "_divFree.npz")
    assert str(z["family"]) == "vector_st" and not [n for n in z.files if n.startswith("sum_")]
    f = np.load(out + ".npz")
    plain = krig.Krig(E.KernelSpec(family="vector_st", kind="df", l_df=5.0, l_cf=5.0, ratio=1.0, var_t=1.5, l_t=4.0),
                      noise=0.0025, var_mode="gpy").fit(f["Xo"], f["obs"][:, 0])
    pts = f["Xt"][:50]
    m0, v0 = plain.predict(pts)
    m1, v1 = krig.Krig.load(out + "_divFree.npz").predict(pts)
    assert np.array_equal(m0, m1) and np.array_equal(v0, v1)


# ---------------------------------------------------------------- 9. refusals
def test_entries_without_a_sum_form_refuse_one():
    x, y, xg = data(100, False)
    gp = fit(100, False)
    spec = gp.kernel
    with pytest.raises(ValueError, match="kernel sum"):
        E.predict_gradient(gp, xg)
    with pytest.raises(ValueError, match="kernel sum"):
        E.predict_cov(gp, xg)
    with pytest.raises(ValueError, match="variance='f64'"):
        E.fit(spec, np.array(x), np.array(y), noise=NOISE, device=DEV, variance="ozaki")
    with pytest.raises(ValueError, match="variance='f64'"):
        krig.Krig(spec, variance="ozaki")
    with pytest.raises(ValueError, match="variance='f64'"):
        next(E.krige_jobs([(spec, np.array(x), np.array(y), NOISE, xg)]))
    # the library itself refuses too, whatever the Python layer does
    desc = spec.desc()
    G = E._as_points(xg, 2, DEV)
    mean = torch.empty((70, 4), dtype=torch.float64, device=DEV)
    rc = N.lib().gp2d_predict_grad(*E._f64_fit_args(gp, G, desc), 0, E._ptr(mean), None, 64, E._ptr(mean), 1 << 40,
                                   E._stream_handle(DEV))
    assert rc < 0 and b"sum" in N.lib().gp2d_last_error()
