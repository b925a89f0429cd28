"""The leave-one-out objective and its exact gradient on the device (gp2d_loo_grad, engine.loo_device /
loo_log_likelihood, hyper's objective="loo", Krig.optimize(objective=)) against the numpy closed
forms of tests/loo_ref.py, which tests/test_loo_cpu.py pins to brute-force refits and their central
differences.

Gates.  Value: 1e-10 relative, as for the LML.  Gradient: the project's `rel` norm (largest deviation
over largest entry) below 1e-10 against the analytic reference, applied twice — to the whole vector
and to the kernel-parameter sub-vector without the noise entry, which is 10³ to 10⁵ times the others
and would hide them.  Two independent float64 routes to K_y⁻¹ on the CPU agree within 1e-13 on both
at N ≤ 300, so the gate carries a margin of 10³; parity stays at N ≤ 300 (at N = 1000 the df
gradient's cancellation is 10⁶ and the device is untested there).

Measured on an MI355X (value, whole, kernel): see the table of DESIGN.md §3.12.

Shapes: N = 40 (n = 128: one GEMM tile, one point tile), 100 (n = 256: u and v in different tiles),
130 (np = 192, n = 384: the v block starts in the middle of a 128 tile), 300 (n = 640), 128 (no
padded point) and 65 (63 padded points).
"""
import ctypes
import dataclasses
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
if not torch.cuda.is_available():  # pragma: no cover
    pytest.skip("no HIP device", allow_module_level=True)

import cv_ref as C  # noqa: E402
import loo_ref as R  # noqa: E402
import sum_ref as S  # noqa: E402
from gp2d import _native as N  # noqa: E402
from gp2d import engine as E  # noqa: E402
from gp2d import hyper as H  # noqa: E402
from gp2d import krig  # noqa: E402
from test_gpu_lml import _sample  # noqa: E402

GATE = 1e-10
DEV = torch.device("cuda")


def term_spec(t):
    if S.is_st(t):
        return E.KernelSpec(family="vector_st", **t)
    return E.KernelSpec(**t)


@functools.lru_cache(maxsize=None)
def case(name, n):
    """(KernelSpec, x, y, reference value, reference gradient) of a named kernel at cv_ref's shared
    settings and seeded data; computed once, read-only."""
    if name == "ard":
        x, y = R.data(n, bd=1)
        spec = E.KernelSpec(family="ard", variances=C.ARD_VARIANCES, lengthscales=C.ARD_LENGTHSCALES)
        val, g = R.ard_value_grad(x, y, C.ARD_VARIANCES, C.ARD_LENGTHSCALES, C.NOISE)
    elif name == "sum":
        x, y = R.data(n)
        spec = E.KernelSpec(family="vector_sum", terms=tuple(term_spec(t) for t in R.SUM_TERMS),
                            weights=tuple(R.SUM_WEIGHTS))
        val, g = R.loo_value_grad(R.SUM_TERMS, R.SUM_WEIGHTS, x, y, C.NOISE)
    else:
        st = name == "st"
        t = R.term("mixed" if st else name, st=st)
        x, y = R.data(n, dim=3 if st else 2)
        spec = term_spec(t)
        val, g = R.loo_value_grad_single(t, x, y, C.NOISE)
    for a in (x, y, g):
        a.setflags(write=False)
    return spec, x, y, val, g


@functools.lru_cache(maxsize=None)
def fit(name, n, variance="f64"):
    spec, x, y = case(name, n)[:3]
    return E.fit(spec, np.array(x), np.array(y), noise=C.NOISE, device=DEV, variance=variance)


def check_parity(what, val, g, rval, rg):
    e = dict(value=abs(val - rval) / max(1.0, abs(rval)), whole=R.rel(g, rg), kernel=R.rel(g[:-1], rg[:-1]))
    print(f"{what}: {e}")
    assert e["value"] < GATE and e["whole"] < GATE and e["kernel"] < GATE, (what, e, g, rg)


PARITY = [(k, n) for n in (40, 100, 130, 300) for k in ("df", "cf", "mixed")]
PARITY += [("st", 100), ("sum", 130), ("ard", 70), ("ard", 200)]
PARITY += [("mixed", 128), ("mixed", 65)]   # N = ntr_pad (no padded point) and N = ntr_pad − 63


@pytest.mark.parametrize("name,n", PARITY)
def test_value_and_gradient_match_reference(name, n):
    spec, _, _, rval, rg = case(name, n)
    gp = fit(name, n)
    val, g = E.loo_log_likelihood(gp, eval_gradient=True)
    assert g.shape == (len(E.param_names(spec)),) == rg.shape
    check_parity(f"loo {name} N={n}", val, g, rval, rg)
    assert E.loo_log_likelihood(gp) == val            # the value-only form: the same bits
    if name == "df":                                  # natural units, param_names order
        names = E.param_names(spec)
        assert names == ("l_df", "l_cf", "ratio", "noise")
        assert g[1] == 0.0 and g[2] == 0.0 and g[0] != 0.0 and g[3] != 0.0


def test_ozaki_morton_fit_agrees():
    """A Morton-ordered fit (the ozaki engine's) and the unordered FP64 fit of the same data: the
    objective does not depend on the order."""
    spec, _, _, rval, rg = case("mixed", 130)
    gp = fit("mixed", 130, "ozaki")
    assert gp.perm is not None and not torch.equal(gp.perm, torch.arange(130, device=DEV))
    val, g = E.loo_log_likelihood(gp, eval_gradient=True)
    check_parity("loo mixed N=130 ozaki (Morton order)", val, g, rval, rg)
    v0, g0 = E.loo_log_likelihood(fit("mixed", 130), eval_gradient=True)
    check_parity("loo ordered vs unordered", val, g, v0, g0)


@pytest.mark.parametrize("name,n", [("mixed", 130), ("ard", 200), ("st", 100)])
def test_value_is_cv_points_sum(name, n):
    gp = fit(name, n)
    val = E.loo_log_likelihood(gp)
    ref = E.cv_points(gp)["mean_lpd"] * n
    assert abs(val - ref) <= 1e-12 * abs(ref), (val, ref)


def c_loo(gp, W, wld, work_fill=None, grad=True):
    """The C entry itself: (value, grad, info) tensors after a synchronise."""
    L = N.lib()
    desc = gp.kernel.desc()
    ng = int(L.gp2d_lml_grad_count(ctypes.byref(desc)))
    out = torch.full((1,), -7.0, dtype=torch.float64, device=DEV)
    g = torch.full((ng,), -7.0, dtype=torch.float64, device=DEV)
    info = torch.full((1,), -7, dtype=torch.int32, device=DEV)
    wb = int(L.gp2d_loo_grad_workspace(gp.n))
    work = torch.empty(wb // 8, dtype=torch.float64, device=DEV)
    if work_fill is not None:
        work.fill_(work_fill)
    N.check(L.gp2d_loo_grad(E._ptr(W), gp.n, wld, E._ptr(gp.alpha), E._ptr(gp.y), E._ptr(gp.x), gp.n_train,
                            gp.n_pad, ctypes.byref(desc), E._ptr(out), E._ptr(g) if grad else None,
                            E._ptr(info), E._ptr(work), wb, E._stream_handle(DEV)), "gp2d_loo_grad")
    torch.cuda.synchronize()
    return out, g, info


@pytest.mark.parametrize("name,n", [("mixed", 130), ("mixed", 300), ("ard", 70)])
def test_c_entry_embedded_w_and_dirty_workspace(name, n):
    """W inside a wider buffer (wld = n + 64, NaN in the slack) and a workspace pre-filled with NaN
    give the bits of a plain call, as does a repeat: nothing above the stored triangles, in a row's
    slack or in a padded slot is read."""
    gp = fit(name, n)
    nn = gp.n
    a = c_loo(gp, gp.W, gp.W.stride(0), work_fill=0.0)
    b = c_loo(gp, gp.W, gp.W.stride(0), work_fill=float("nan"))
    wide = torch.full((nn, nn + 64), float("nan"), dtype=torch.float64, device=DEV)
    wide[:, :nn] = gp.W
    c = c_loo(gp, wide, nn + 64, work_fill=float("nan"))
    d = c_loo(gp, gp.W, gp.W.stride(0))
    for other in (b, c, d):
        for x, y in zip(a, other):
            assert torch.equal(x, y)
    assert int(a[2].item()) == 0 and bool(torch.isfinite(a[1]).all())
    v = c_loo(gp, gp.W, gp.W.stride(0), work_fill=float("nan"), grad=False)
    assert torch.equal(v[0], a[0]) and bool((v[1] == -7.0).all())      # grad_dev = NULL: value only
    val, g = E.loo_log_likelihood(gp, eval_gradient=True)
    assert val == float(a[0].item()) and np.array_equal(g, a[1].cpu().numpy())


def test_bad_fit_is_reported_not_rooted():
    """A factor whose K_y⁻¹ has a non-positive diagonal block: the info word names the first such
    point, the value is NaN, and the Python entry raises LinAlgError."""
    gp = fit("mixed", 40)
    W = gp.W.clone()
    W[:, 5] = 0.0            # column 5 of W: P_uu of point 5 = 0
    out, _, info = c_loo(gp, W, W.stride(0))
    assert int(info.item()) == 6 and bool(torch.isnan(out).all())
    broken = dataclasses.replace(gp, W=W)
    with pytest.raises(np.linalg.LinAlgError, match="point 5"):
        E.loo_log_likelihood(broken)
    assert bool(torch.isnan(E.loo_device(broken)[0]).all())


def test_refusals():
    spec, x, y = case("mixed", 40)[:3]
    gp = fit("mixed", 40)
    with pytest.raises(ValueError, match="observations"):
        E.loo_log_likelihood(dataclasses.replace(gp, y=None))
    with pytest.raises(ValueError, match="no factor W"):
        E.loo_device(dataclasses.replace(gp, W=None, n_mat=gp.n))
    tr = E.fit(spec, np.array(x), np.array(y), noise=C.NOISE, device=DEV, trend="constant")
    for fn in (E.loo_log_likelihood, E.loo_device):
        with pytest.raises(ValueError, match="trend"):
            fn(tr)


def test_lml_grad_keeps_the_parents_bits(golden):
    """gp2d_lml_grad on the same fits: the bits recorded with the library as it was before
    LooWeights joined the pair loop's policies (tests/golden/lml_grad_parent_bits.npz)."""
    g = golden("lml_grad_parent_bits.npz")
    for name, n in (("df", 130), ("cf", 130), ("mixed", 130), ("mixed", 300), ("st", 100), ("sum", 130), ("ard", 70)):
        val, grad = E.log_marginal_likelihood(fit(name, n), eval_gradient=True)
        assert np.array_equal(grad, g[f"{name}_{n}_grad"]), (name, n)
        assert val == float(g[f"{name}_{n}_lml"]), (name, n)


# ---------------------------------------------------------------------------- hyper, Krig
@functools.lru_cache(maxsize=None)
def optimum_problem():
    x, y = _sample(250, "df", 6.0, 6.0, 1.0, 0.01, seed=21)
    return x, y


def test_optimize_loo_matches_reference_optimum():
    """L-BFGS-B on the device objective reaches the optimum Nelder–Mead finds on loo_ref's value
    (test_gpu_lml.test_optimize_matches_oracle_optimum's problem and tolerances).  The LML optimum
    of the same data is l_df = 6.2890, noise = 0.0099977 against the LOO optimum's 6.5514, 0.010022:
    the assertions fail if the objective switch is ignored."""
    from scipy.optimize import minimize
    x, y = optimum_problem()
    res = H.optimize(E.KernelSpec(kind="df", l_df=3.0), x, y, 0.05, objective="loo")
    assert res.success, res.message
    assert res.objective == "loo"

    def f(z):
        t = R.term("df", l_df=float(np.exp(z[0])))
        return -R.value_from_K(S.ky([t], [1.0], x, float(np.exp(z[1]))), y, 2)

    ref = minimize(f, np.log([3.0, 0.05]), method="Nelder-Mead", options=dict(xatol=1e-10, fatol=1e-12,
                                                                               maxiter=4000))
    print("loo optimum", np.exp(ref.x), -ref.fun, "device", res.kernel.l_df, res.noise, res.value, "lml", res.lml)
    assert abs(res.value - (-ref.fun)) < 1e-6 * abs(ref.fun)
    assert abs(res.kernel.l_df - np.exp(ref.x[0])) < 1e-3 * np.exp(ref.x[0])
    assert abs(res.noise - np.exp(ref.x[1])) < 1e-3 * np.exp(ref.x[1])
    gp = E.fit(res.kernel, x, y, res.noise)
    val, g = E.loo_log_likelihood(gp, eval_gradient=True)
    assert abs(g[0] * res.kernel.l_df) < 1e-2 and abs(g[3] * res.noise) < 1e-2
    assert val == pytest.approx(res.value, rel=1e-12)
    assert res.lml == E.log_marginal_likelihood(gp) and res.lml != res.value   # .lml stays the LML


def test_optimize_restarts_ranks_by_value():
    x, y = _sample(100, "mixed", 5.0, 3.0, 0.7, 0.01, seed=22)
    ks = E.KernelSpec(kind="mixed", l_df=4.0, l_cf=4.0, ratio=0.5)
    start = E.loo_log_likelihood(E.fit(ks, x, y, 0.02))
    res = H.optimize_restarts(ks, x, y, 0.02, num_restarts=3, seed=1, objective="loo")
    assert len(res.runs) == 3 and res.objective == "loo"
    assert res.value == max(r[1] for r in res.runs) and res.value > start
    for p, v in res.runs:   # each run lists the maximised objective, not the LML
        k, nz = H.set_params(ks, p)
        gp = E.fit(k, x, y, nz)
        assert E.loo_log_likelihood(gp) == pytest.approx(v, rel=1e-10)
    best = E.fit(res.kernel, x, y, res.noise)
    assert E.log_marginal_likelihood(best) == pytest.approx(res.lml, rel=1e-12)
    # the default objective's result carries the new fields too
    lml = H.optimize(ks, x, y, 0.02, fix=("ratio", "noise"))
    assert lml.objective == "lml" and lml.value == lml.lml


def test_sweep_loo_same_numbers_through_every_schedule():
    spec, x, y = case("df", 130)[:3]
    x, y = np.array(x), np.array(y)
    settings = [dict(l_df=l, noise=nz) for l in (3.0, 5.0) for nz in (0.0025, 0.01)] + [dict(noise=-50.0)]
    ref_v, ref_g = [], []
    for s in settings[:-1]:
        gp = E.fit(E.KernelSpec(kind="df", l_df=s["l_df"], l_cf=spec.l_cf, ratio=1.0), x, y, s["noise"], device=DEV)
        v, g = E.loo_log_likelihood(gp, eval_gradient=True)
        ref_v.append(v)
        ref_g.append(g)
    for kw in (dict(concurrent=1, batch=1), dict(concurrent=2, batch=1), dict(batch=2)):
        vals, grads = H.sweep(spec, x, y, settings, noise=C.NOISE, eval_gradient=True, objective="loo", **kw)
        assert vals[-1] == -np.inf, kw
        assert np.array_equal(vals[:-1], ref_v) and np.array_equal(grads[:-1], np.array(ref_g)), kw
    lml = H.sweep(spec, x, y, settings[:2], noise=C.NOISE, concurrent=1, batch=1)[0]
    assert not np.array_equal(lml, ref_v[:2])   # and the default is still the LML
    assert lml[0] == E.log_marginal_likelihood(E.fit(E.KernelSpec(kind="df", l_df=3.0, l_cf=spec.l_cf, ratio=1.0),
                                                     x, y, 0.0025, device=DEV))


def test_sweep_lgo_equals_cv_groups():
    spec, x, y = case("mixed", 100)[:3]
    x, y = np.array(x), np.array(y)
    labels = np.random.default_rng(5).integers(-1, 9, 100)
    settings = [dict(l_df=4.0), dict(l_df=6.0, noise=0.01)]
    vals, grads = H.sweep(spec, x, y, settings, noise=C.NOISE, objective="lgo", labels=labels)
    assert grads is None
    for s, v in zip(settings, vals):
        k, nz = H.set_params(spec, dict(H.get_params(spec, C.NOISE), **s))
        lpd = E.cv_groups(E.fit(k, x, y, nz, device=DEV), labels)["lpd"]
        assert v == float(lpd.sum().item())


def test_krig_optimize_loo_refits_at_the_optimum():
    x, y = _sample(150, "df", 6.0, 6.0, 1.0, 0.01, seed=23)
    k = krig.Krig("df", l_df=3.0, noise=0.05).fit(x, y)
    before = k.loo_log_likelihood()
    res = k.optimize(objective="loo")
    assert res.objective == "loo" and res.value > before
    assert k.loo_log_likelihood() == pytest.approx(res.value, rel=1e-12)
    assert k.log_likelihood() == pytest.approx(res.lml, rel=1e-12)
    assert k.param_array[0] == pytest.approx(res.kernel.l_df, rel=1e-12)
    r2 = k.optimize_restarts(num_restarts=2, objective="loo")
    assert r2.value >= res.value - 1e-6 * abs(res.value)
