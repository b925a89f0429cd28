"""A background flow estimated with the fit (trend='constant' | 'linear'), without a device: the
numpy reference tests/trend_ref.py against an independent route and against central differences of
its own restricted likelihood, the new host entries of include/gp2d.h (sizes, argument checks) and
the Python layer's refusals.

Shapes: tests/test_gpu_trend.py's — 100 and 130 training points, 70 targets — and its kernels.
Tolerances: the two routes 1e-12 of the largest entry (both are a few roundings of a system whose
condition is ~1e3: K_y = K + 0.0025·I with kernel amplitudes ~0.02); shift invariance 1e-10 of the
largest entry, the device test's gate; the gradient 1e-7 of its largest entry against the 4-point
central difference (the stencil and gate of tests/test_sum_cpu.py); host sizes exact.
"""
import ctypes
import os
import re

import numpy as np
import pytest

import trend_ref as T
from conftest import ROOT

CASES = tuple(T.CASES)


def rel(a, b):
    return float(np.max(np.abs(np.asarray(a) - np.asarray(b))) / max(np.max(np.abs(b)), 1e-300))


# ---------------------------------------------------------------- the reference
@pytest.mark.parametrize("order", [0, 1])
@pytest.mark.parametrize("n", T.SIZES)
@pytest.mark.parametrize("case", CASES)
def test_reference_routes_agree(case, n, order):
    _, _, xg = T.case_data(case, n)
    a, b = T.ref(case, n, order), T.ref(case, n, order, "augmented")
    e = dict(beta=rel(a.beta, b.beta), alpha=rel(a.alpha, b.alpha), Ainv=rel(a.Ainv, b.Ainv), B0=rel(a.B0, b.B0),
             reml=abs(a.reml() - b.reml()) / abs(b.reml()))
    (ma, va), (mb, vb) = a.predict(xg), b.predict(xg)
    e.update(mean=rel(ma, mb), var=rel(va, vb))
    for field in ("divergence", "vorticity"):
        (fa, wa), (fb, wb) = a.predict_field(xg, field), b.predict_field(xg, field)
        e[field] = max(rel(fa, fb), rel(wa, wb))
    print(f"{case} N={n} order={order}: cond(A) {np.linalg.cond(a.A):.1f}; {e}")
    assert np.linalg.cond(a.A) < 100.0
    assert np.max(np.abs(a.beta)) > 0.3          # the background flow is far from zero
    assert all(v <= 1e-12 for v in e.values()), e
    assert np.max(np.abs(a.H @ a.alpha)) <= 1e-10 * np.max(np.abs(a.alpha)) * a.H.shape[1]   # H·α′ = 0


@pytest.mark.parametrize("order", [0, 1])
@pytest.mark.parametrize("n", T.SIZES)
@pytest.mark.parametrize("case", CASES)
def test_reference_shift_invariance(case, n, order):
    """y + Hᵀγ moves β̂ by γ and leaves α′ and the variances alone."""
    x, y, xg = T.case_data(case, n)
    terms, weights = T.CASES[case]
    base = T.ref(case, n, order)
    gamma = np.array([0.7, -1.3, 0.4, -0.2, 0.9, 0.5])[:base.q]
    moved = T.Fit(terms, weights, x, y + base.H.T @ gamma, T.NOISE, order)
    e = dict(beta=rel(moved.beta - gamma, base.beta), alpha=rel(moved.alpha, base.alpha),
             var=rel(moved.predict(xg)[1], base.predict(xg)[1]),
             mean=rel(moved.predict(xg)[0] - T.basis(xg, order, base.centre, base.scale).T @ gamma,
                      base.predict(xg)[0]))
    print(f"{case} N={n} order={order}: {e}")
    assert all(v <= 1e-10 for v in e.values()), e


@pytest.mark.parametrize("order", [0, 1])
@pytest.mark.parametrize("case", CASES)
def test_reference_gradient_is_the_derivative_of_its_reml(case, order):
    n = 100
    x, y, _ = T.case_data(case, n)
    terms, weights = T.CASES[case]
    plain = case != "sum"
    f0 = T.ref(case, n, order)
    g = f0.reml_grad(plain)
    names = T.S.param_names(terms)
    if plain:
        names = tuple(nm for nm in names if not nm.startswith("weight_"))
    assert g.shape == (len(names),)

    def at(name, value):
        ts, ws, nz = [dict(t) for t in terms], list(weights), T.NOISE
        if name == "noise":
            nz = value
        else:
            b, t = name.rsplit("_", 1)
            if b == "weight":
                ws[int(t)] = value
            else:
                ts[int(t)][b] = value
        return T.reml(ts, ws, x, y, nz, order, f0.centre, f0.scale)

    fd = np.zeros_like(g)
    for i, name in enumerate(names):
        if name == "noise":
            v, b = T.NOISE, "noise"
        else:
            b, t = name.rsplit("_", 1)
            v = weights[int(t)] if b == "weight" else terms[int(t)][b]
            used = {"df": ("l_df",), "cf": ("l_cf",), "mixed": ("l_df", "l_cf", "ratio")}[terms[int(t)]["kind"]] \
                + (("var_t", "l_t") if T.S.is_st(terms[int(t)]) else ())
            if b != "weight" and b not in used:
                assert g[i] == 0.0, name
                continue
        h = 1e-3 * (1.0 if b == "ratio" else abs(v))
        f = [at(name, v + s * h) for s in (-2, -1, 1, 2)]
        fd[i] = (f[0] - 8 * f[1] + 8 * f[2] - f[3]) / (12 * h)
    err = rel(g, fd)
    print(f"{case} order={order}: REML gradient vs central difference {err:.2e}\n  {dict(zip(names, g))}")
    assert err < 1e-7, (err, g, fd)


def test_reml_differs_from_the_plain_likelihood_by_its_terms():
    """With β̂ fixed at 0 the formulas are the zero-mean ones: REML − LML(y − Hᵀβ̂) = −½ log|A| + ½ q log 2π."""
    f = T.ref("vector2d", 100, 1)
    plain = T.S.lml(f.terms, f.weights, f.x, f.y - f.H.T @ f.beta, T.NOISE)
    want = plain - 0.5 * np.linalg.slogdet(f.A)[1] + 0.5 * f.q * np.log(2 * np.pi)
    assert f.reml() == pytest.approx(want, rel=1e-12)


# ---------------------------------------------------------------- the header and the binding
NEW = ("gp2d_trend_coefficients", "gp2d_trend_block_doubles", "gp2d_trend_workspace", "gp2d_trend_fit",
       "gp2d_predict_trend_workspace", "gp2d_predict_trend", "gp2d_predict_field_trend", "gp2d_lml_trend",
       "gp2d_lml_grad_trend_workspace", "gp2d_lml_grad_trend")


def _header():
    return open(os.path.join(ROOT, "include", "gp2d.h")).read()


def _prototypes():
    txt = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    out = {}
    for name, params in re.findall(r"\b(gp2d_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", txt):
        out[name] = [re.findall(r"[A-Za-z_]\w*", p)[-1] for p in params.split(",") if p.strip() != "void"]
    return out


def test_new_symbols_are_exported_and_match_the_header():
    from gp2d import _native as N
    L = N.lib()
    protos = _prototypes()
    for s in NEW:
        assert s in N.EXPORTS and hasattr(L, s) and s in protos, s
        assert len(protos[s]) == len(N._SIGS[s][1]), s
    assert L.gp2d_abi_version() == 11
    # the trend predicts take their plain entries' arguments, then (trend, block, with_basis)
    for plain, trend in (("gp2d_predict", "gp2d_predict_trend"), ("gp2d_predict_field", "gp2d_predict_field_trend")):
        want = [("wld" if p == "ldw" else p) for p in protos[plain]] + ["trend", "block", "with_basis"]
        assert protos[trend] == want
        assert N._SIGS[trend][1][:len(protos[plain])] == N._SIGS[plain][1]
    # the descriptor: order, centre[2], scale
    m = re.search(r"typedef struct gp2d_trend \{(.*?)\} gp2d_trend_t;", re.sub(r"/\*.*?\*/", "", _header(), flags=re.S),
                  flags=re.S)
    fields = re.findall(r"(int32_t|double)\s+(\w+)(\[\d+\])?;", m.group(1))
    assert fields == [("int32_t", "order", ""), ("double", "centre", "[2]"), ("double", "scale", "")]
    assert [f[0] for f in N.TrendDesc._fields_] == ["order", "centre", "scale"] and ctypes.sizeof(N.TrendDesc) == 32
    assert N.TREND_ORDERS == {"constant": 0, "linear": 1}
    assert L.gp2d_trend_coefficients(0) == 2 and L.gp2d_trend_coefficients(1) == 6
    assert L.gp2d_trend_coefficients(2) < 0 and L.gp2d_trend_coefficients(-1) < 0
    # no entry's existing signature moved
    assert protos["gp2d_predict"][2] == "ldw" and len(protos["gp2d_predict"]) == 19


def test_workspace_queries_obey_their_arithmetic():
    from gp2d import _native as N
    L = N.lib()
    for n in (128, 256, 384, 8192):
        assert L.gp2d_trend_block_doubles(n) == N.TREND_RHS + N.TREND_RHS_LD * n == 48 + 8 * n
        seg = n // 128
        for order in (0, 1):
            # Y and Z tables (8 doubles per row) and one table per 128-row segment, plus one
            assert L.gp2d_trend_workspace(n, order) == 8 * 8 * n * (3 + seg)
            q = L.gp2d_trend_coefficients(order)
            for chunk, bd in ((64, 2), (128, 1), (8192, 2), (100, 2)):
                ncols = -(-bd * (-(-chunk // 64) * 64) // 128) * 128
                plain = L.gp2d_predict_workspace(n, chunk, bd)
                assert plain == 8 * ncols * (n + 2 * (seg + 1))
                # q more sets of mean partials than the plain predict
                assert L.gp2d_predict_trend_workspace(n, chunk, bd, order) == plain + q * 8 * (seg + 1) * ncols
        assert L.gp2d_lml_grad_trend_workspace(n) == L.gp2d_lml_grad_workspace(n)
    assert L.gp2d_trend_block_doubles(0) == 48 and L.gp2d_trend_workspace(0, 1) == 0
    assert (N.TREND_BETA, N.TREND_AINV, N.TREND_AINV_LD, N.TREND_LOGDET, N.TREND_STATUS) == (0, 8, 6, 44, 45)


# Valid host arguments per entry, by the header's parameter names (n = 256: 100 points padded to
# 128); pointers are never dereferenced — every call below is refused on the host.
_BASE = dict(n=256, wld=256, ntr=100, ntr_pad=128, dim=2, m=10, chunk=128, var_mode=0, noise=0.0025, compute_var=1,
             field=1, nobs=200, work_bytes=1 << 40, with_basis=1)


def _call(name, trend=(1, (30.0, 22.0), 30.0), kernel=None, ptr=64, **over):
    from gp2d import _native as N
    L = N.lib()
    vals = dict(_BASE, **over)
    keep, args = [], []
    for p, t in zip(_prototypes()[name], N._SIGS[name][1]):
        if p in over and over[p] is None:
            args.append(None)
        elif p == "stream":
            args.append(None)
        elif t is N._TP:
            if trend is None:
                args.append(None)
            else:
                keep.append(N.trend_desc(*trend))
                args.append(ctypes.byref(keep[-1]))
        elif t is N._KP:
            keep.append(kernel if kernel is not None else N.vector_kernel_desc(N.KIND_MIXED, 8.0, 8.0, 0.6))
            args.append(ctypes.byref(keep[-1]))
        elif t is ctypes.c_void_p:
            args.append(ctypes.c_void_p(int(over.get(p, ptr))))
        elif t is ctypes.c_double:
            args.append(float(vals.get(p, 0.0)))
        else:
            args.append(int(vals.get(p, 0)))
    rc = getattr(L, name)(*args)
    return rc, L.gp2d_last_error().decode()


TREND_ENTRIES = ("gp2d_trend_fit", "gp2d_predict_trend", "gp2d_predict_field_trend", "gp2d_lml_trend",
                 "gp2d_lml_grad_trend")
_BLOCK = {"gp2d_trend_fit": "block_out"}


@pytest.mark.parametrize("name", TREND_ENTRIES)
def test_trend_descriptor_checks_fire_in_every_entry(name):
    block = _BLOCK.get(name, "block")
    bad = [(dict(trend=None), "trend is NULL"),
           (dict(trend=(2, (0.0, 0.0), 1.0)), "order must be 0"),
           (dict(trend=(-1, (0.0, 0.0), 1.0)), "order must be 0"),
           (dict(trend=(1, (0.0, 0.0), 0.0)), "scale must be finite and > 0"),
           (dict(trend=(1, (0.0, 0.0), -2.0)), "scale must be finite and > 0"),
           (dict(trend=(0, (0.0, 0.0), float("inf"))), "scale must be finite and > 0"),
           (dict(trend=(0, (0.0, 0.0), float("nan"))), "scale must be finite and > 0"),
           (dict(trend=(1, (float("nan"), 0.0), 1.0)), "centre must be finite"),
           ({block: None}, "block is NULL"),
           ({block: 72}, "block must be 64-byte aligned")]
    entry = name[len("gp2d_"):]
    for kw, text in bad:
        rc, msg = _call(name, **kw)
        assert rc < 0 and text in msg and msg.startswith(entry + ":"), (name, kw, rc, msg)


def test_trend_entries_check_their_other_arguments():
    from gp2d import _native as N
    ard = N.ard_kernel_desc([1.0], [[5.0, 5.0]])
    L = N.lib()
    cases = [
        ("gp2d_trend_fit", dict(n=200, wld=200), "n must be a positive multiple of 128"),
        ("gp2d_trend_fit", dict(ntr_pad=64), "n must equal 2 × ntr_pad"),
        ("gp2d_trend_fit", dict(ntr=0), "bad point count"),
        ("gp2d_trend_fit", dict(ntr=129), "bad point count"),
        ("gp2d_trend_fit", dict(dim=4), "dim must be 2 or 3"),
        ("gp2d_trend_fit", dict(wld=255), "wld must be >= n"),
        ("gp2d_trend_fit", dict(work_bytes=L.gp2d_trend_workspace(256, 1) - 1), "workspace too small"),
        ("gp2d_trend_fit", dict(work=None), "workspace too small"),
        ("gp2d_trend_fit", dict(y=None), "NULL argument"),
        ("gp2d_predict_trend", dict(wld=255), "wld must be >= n and even"),
        ("gp2d_predict_trend", dict(wld=257), "wld must be >= n and even"),
        ("gp2d_predict_trend", dict(W=8), "16-byte aligned"),
        ("gp2d_predict_trend", dict(chunk=100), "chunk must be a positive multiple of 64"),
        ("gp2d_predict_trend", dict(var_mode=3), "bad var_mode"),
        ("gp2d_predict_trend", dict(kernel=ard), "vector kernel"),
        ("gp2d_predict_trend", dict(work_bytes=L.gp2d_predict_trend_workspace(256, 128, 2, 1) - 1),
         "workspace too small"),
        # a plain predict's workspace is too small for the q + 1 sets of partials
        ("gp2d_predict_trend", dict(work_bytes=L.gp2d_predict_workspace(256, 128, 2)), "workspace too small"),
        ("gp2d_predict_field_trend", dict(wld=257), "wld must be >= n and even"),
        ("gp2d_predict_field_trend", dict(W=8), "16-byte aligned"),
        ("gp2d_predict_field_trend", dict(field=3), "field must be"),
        ("gp2d_predict_field_trend", dict(chunk=64), "chunk must be a positive multiple of 128"),
        ("gp2d_predict_field_trend", dict(work_bytes=L.gp2d_predict_trend_workspace(256, 128, 1, 1) - 1),
         "workspace too small"),
        ("gp2d_lml_trend", dict(wld=255), "wld must be >= n"),
        ("gp2d_lml_trend", dict(nobs=257), "bad sizes"),
        ("gp2d_lml_trend", dict(lml_dev=None), "NULL argument"),
        ("gp2d_lml_grad_trend", dict(wld=257), "wld must be >= n and even"),
        ("gp2d_lml_grad_trend", dict(W=8), "16-byte aligned"),
        ("gp2d_lml_grad_trend", dict(kernel=ard, n=128), "vector kernel"),
        ("gp2d_lml_grad_trend", dict(work_bytes=L.gp2d_lml_grad_trend_workspace(256) - 1), "workspace too small"),
    ]
    for name, kw, text in cases:
        rc, msg = _call(name, **kw)
        assert rc < 0 and text in msg, (name, kw, rc, msg)
    # m = 0 is an empty predict, not an error, and launches nothing
    assert _call("gp2d_predict_trend", m=0)[0] == 0 and _call("gp2d_predict_field_trend", m=0)[0] == 0


# ---------------------------------------------------------------- the Python layer
def _fake_trend_fit():
    """A GPFit that says it is a trend fit; every entry below must refuse it before touching it."""
    import torch
    from gp2d import engine as E
    spec = E.KernelSpec(kind="mixed", l_df=8.0, l_cf=8.0, ratio=0.6)
    z = torch.zeros(1, dtype=torch.float64)
    gp = E.GPFit(kernel=spec, noise=T.NOISE, x=z, n_train=1, n_pad=64, W=z, alpha=z, device=torch.device("cpu"), y=z)
    gp.extra["trend"] = dict(order=1, name="linear")
    return gp


def test_python_refusals_come_before_a_device_is_required():
    import krig
    from gp2d import distributed as DI
    from gp2d import engine as E
    from gp2d import hyper as H
    x, y, xg = (np.array(a) for a in T.data(100, False))
    spec = E.KernelSpec(kind="mixed", l_df=8.0, l_cf=8.0, ratio=0.6)
    ard = E.KernelSpec(family="ard", variances=(1.0,), lengthscales=((5.0, 5.0),))
    gp = _fake_trend_fit()
    job = (spec, x, y, T.NOISE, xg)
    refused = [
        lambda: E.fit(spec, x, y, T.NOISE, variance="ozaki", trend="linear"),
        lambda: E.fit(ard, x, y[:100], T.NOISE, trend="constant"),
        lambda: E.fit(spec, x, y, T.NOISE, trend="quadratic"),
        lambda: E.fit(spec, x, y, T.NOISE, trend=1),
        lambda: E.fit_batch([job[:4]], trend="linear"),
        lambda: next(E.krige_jobs([job], trend="constant")),
        lambda: next(DI.krige_jobs_sharded([job], trend="constant")),
        lambda: DI.fit_sharded(spec, x, y, T.NOISE, None, trend="linear"),
        lambda: DI.fit_distributed(spec, x, y, T.NOISE, trend="linear"),
        lambda: DI.broadcast_fit(gp, spec, T.NOISE, x, None),
        lambda: E.predict_gradient(gp, xg),
        lambda: E.predict_cov(gp, xg),
        lambda: E.sample_posterior(gp, xg, 2),
        lambda: E.cv_points(gp),
        lambda: E.cv_groups(gp, np.zeros(1, dtype=np.int64)),
        lambda: krig.Krig("mixed", variance="ozaki", trend="linear"),
        lambda: krig.Krig(ard, trend="linear"),
        lambda: krig.Krig("mixed", trend="cubic"),
        lambda: H.Objective(spec, x, y, T.NOISE, ("l_df",), trend="cubic"),
        lambda: H.sweep(spec, x, y, [dict(l_df=5.0)], noise=T.NOISE, trend="cubic"),
        lambda: H.sweep(spec, x, y, [dict(l_df=5.0), dict(l_df=6.0)], noise=T.NOISE, batch=2, trend="linear"),
    ]
    for i, f in enumerate(refused):
        with pytest.raises(ValueError, match="trend"):
            f()
        assert i >= 0
    with pytest.raises(ValueError, match="trend_coefficients needs"):
        E.trend_coefficients(E.GPFit(kernel=spec, noise=0.0, x=None, n_train=0, n_pad=0, W=None, alpha=None,
                                     device=None))
    # trend=None is no trend anywhere
    assert E.trend_order(None) is None and E.trend_order("constant") == 0 and E.trend_order("linear") == 1
    assert krig.Krig("mixed").trend is None and krig.Krig("mixed", trend="linear").trend == "linear"
    # the keyword reaches every layer that is documented to take it
    import inspect
    for fn in (E.fit, E.fit_batch, E.krige_jobs, H.optimize, H.optimize_restarts, H.sweep, H.Objective.__init__,
               krig.Krig.__init__, krig.kriging, krig.laser, DI.fit_sharded, DI.fit_distributed, DI.krige_jobs_sharded):
        assert inspect.signature(fn).parameters["trend"].default is None, fn
    assert E.param_names(spec) == ("l_df", "l_cf", "ratio", "noise")


def test_linear_trend_on_coincident_points_is_a_linalg_error_on_the_host():
    """All points at one place: no scale, and no linear trend — decided before any device work."""
    from gp2d import engine as E
    x = np.tile([[3.0, 4.0]], (5, 1))
    with pytest.raises(np.linalg.LinAlgError, match="collinear"):
        E._trend_basis(x, np.empty((5, 2)), 1)
    assert E._trend_basis(x, np.empty((5, 2)), 0) == ((3.0, 4.0), 1.0)
    c, s = E._trend_basis(np.array(T.data(100, False)[0]), np.empty((100, 2)), 1)
    cr, sr = T.centre_scale(T.data(100, False)[0])
    assert c == tuple(cr) and s == sr
    xst = np.array(T.data(100, True)[0])
    assert E._trend_basis(xst, np.empty((100, 3)), 1)[0] == tuple(T.centre_scale(xst)[0])   # steady in time
    with pytest.raises(ValueError, match="trend"):
        E._trend_basis(np.array([[np.nan, 1.0], [0.0, 1.0]]), np.empty((2, 2)), 0)
