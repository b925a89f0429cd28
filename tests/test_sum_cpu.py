"""Sums of vector kernels (GP2D_FAMILY_VECTOR_SUM) without a device: the reference of
tests/sum_ref.py against central differences of its own LML, the host entries of include/gp2d.h on
a sum's descriptor array, every validation error and refusal, and the Python layers' parameter
packing.

Tolerances: the gradient 1e-7 relative to its largest entry against the 4-point central difference
(the stencil and gate of tests/test_grad_cpu.py); host scalars 1e-15 relative (a handful of fp64
operations).
"""
import ctypes
import math

import numpy as np
import pytest

import sum_ref as S

T2D = [dict(kind="mixed", l_df=8.0, l_cf=8.0, ratio=0.6), dict(kind="df", l_df=2.0, l_cf=1.0, ratio=1.0)]
W2D = [1.0, 0.05]
TST = [dict(kind="mixed", l_df=8.0, l_cf=6.0, ratio=0.6, var_t=1.5, l_t=3.0),
       dict(kind="cf", l_df=1.0, l_cf=2.5, ratio=0.0, var_t=0.05, l_t=1.0)]
WST = [1.0, 1.0]
NOISE = 0.0025


def rel(a, b):
    return float(np.max(np.abs(np.asarray(a) - np.asarray(b))) / max(np.max(np.abs(b)), 1e-300))


def _data(st, n=40, seed=5):
    rng = np.random.default_rng(seed)
    x = rng.uniform(0, 30, (n, 2))
    if st:
        x = np.concatenate([rng.uniform(0, 6, (n, 1)), x], 1)
    a, b = x[:, -2], x[:, -1]
    y = np.concatenate([np.sin(b / 7) + 0.2 * np.sin(a / 1.5), np.cos(a / 9) + 0.2 * np.cos(b / 1.5)])
    return x, y + rng.normal(0, 0.05, 2 * n)


def _used(term):
    own = {"df": ("l_df",), "cf": ("l_cf",), "mixed": ("l_df", "l_cf", "ratio")}[term["kind"]]
    return own + (("var_t", "l_t") if S.is_st(term) else ())


@pytest.mark.parametrize("st", [False, True])
def test_reference_gradient_is_the_derivative_of_its_lml(st):
    terms, weights = (TST, WST) if st else (T2D, W2D)
    x, y = _data(st)
    val, g = S.lml_grad(terms, weights, x, y, NOISE)
    names = S.param_names(terms)
    assert g.shape == (len(names),)
    assert val == pytest.approx(S.lml(terms, weights, x, y, NOISE), rel=1e-14)

    def at(name, value):
        ts, ws, nz = [dict(t) for t in terms], list(weights), NOISE
        if name == "noise":
            nz = value
        else:
            base, t = name.rsplit("_", 1)
            if base == "weight":
                ws[int(t)] = value
            else:
                ts[int(t)][base] = value
        return S.lml(ts, ws, x, y, nz)

    def current(name):
        if name == "noise":
            return NOISE
        base, t = name.rsplit("_", 1)
        return weights[int(t)] if base == "weight" else terms[int(t)][base]

    fd = np.zeros_like(g)
    for i, name in enumerate(names):
        base = name.rsplit("_", 1)[0] if name != "noise" else name
        if base not in ("weight", "noise") and base not in _used(terms[int(name.rsplit("_", 1)[1])]):
            assert g[i] == 0.0, name          # a parameter the kind does not use
            continue
        v = current(name)
        h = 1e-3 * (1.0 if base == "ratio" else abs(v))
        f = [at(name, v + s * h) for s in (-2, -1, 1, 2)]
        fd[i] = (f[0] - 8 * f[1] + 8 * f[2] - f[3]) / (12 * h)
    err = rel(g, fd)
    print(f"st={st}: trace gradient vs central difference of the LML {err:.2e}\n  {dict(zip(names, g))}")
    assert err < 1e-7, (err, g, fd)


def _kinds():
    from gp2d import _native as N
    return {"df": N.KIND_DIVFREE, "cf": N.KIND_CURLFREE, "mixed": N.KIND_MIXED, "scalar": N.KIND_SCALAR}


def _desc(terms, weights):
    from gp2d import _native as N
    ds = []
    for t in terms:
        if S.is_st(t):
            ds.append(N.vector_st_kernel_desc(_kinds()[t["kind"]], t["l_df"], t["l_cf"], t["ratio"], t["var_t"], t["l_t"]))
        else:
            ds.append(N.vector_kernel_desc(_kinds()[t["kind"]], t["l_df"], t["l_cf"], t["ratio"]))
    return N.vector_sum_kernel_desc(ds, weights)


def test_host_entries_on_a_sum():
    from gp2d import _native as N
    import field_ref as F
    L = N.lib()
    assert N.FAMILY_VECTOR_SUM == 3 and N.SUM_MAX_TERMS == 3
    for terms, weights, per in ((T2D, W2D, 4), (TST, WST, 6), (T2D[:1], [0.7], 4), (T2D + T2D[:1], [1.0, 0.05, 0.3], 4)):
        d = _desc(terms, weights)
        assert len(d) == 1 + len(terms) and d[0].family == N.FAMILY_VECTOR_SUM and d[0].nterms == len(terms)
        k = ctypes.byref(d)
        assert L.gp2d_block_dim(k) == 2
        want = sum(w * S.term_diag(t) for t, w in zip(terms, weights))
        assert L.gp2d_kernel_diag(k) == pytest.approx(want, rel=1e-15)
        assert L.gp2d_lml_grad_count(k) == per * len(terms) + 1
        assert L.gp2d_kernel_grad_count(k) == per * len(terms)
        for field, code in (("divergence", N.FIELD_DIVERGENCE), ("vorticity", N.FIELD_VORTICITY)):
            want = sum(w * F.prior_var(field, t["kind"], t["l_df"], t["l_cf"], t["ratio"], t.get("var_t"))
                       for t, w in zip(terms, weights))
            assert L.gp2d_field_prior_var(k, code) == pytest.approx(want, rel=1e-15, abs=1e-300)
    # a one-term sum of weight 1 is its term, to the bit
    one = _desc(T2D[:1], [1.0])
    assert L.gp2d_kernel_diag(ctypes.byref(one)) == L.gp2d_kernel_diag(ctypes.byref(one[1]))
    # a scalar term has no derived field
    sc = _desc([dict(kind="scalar", l_df=3.0, l_cf=3.0, ratio=1.0)], [1.0])
    assert math.isnan(L.gp2d_field_prior_var(ctypes.byref(sc), N.FIELD_VORTICITY))
    assert L.gp2d_lml_grad_workspace(256) == L.gp2d_lml_grad_workspace(256)   # a function of n alone


def test_validation_errors_and_refusals_are_reported():
    """Every error comes from a host check before any device work: the pointers here are never
    dereferenced (the style of test_fields_cpu.test_predict_field_argument_errors_are_reported)."""
    from gp2d import _native as N
    L = N.lib()
    one = ctypes.c_void_p(1)
    big = 1 << 40
    good2 = N.vector_kernel_desc(N.KIND_MIXED, 8.0, 8.0, 0.6)
    goodst = N.vector_st_kernel_desc(N.KIND_DIVFREE, 5.0, 5.0, 1.0, 1.0, 2.0)
    ard = N.ard_kernel_desc([1.0], [[5.0, 5.0]])

    def header(nterms, weights):
        d = (N.KernelDesc * 5)()
        d[0].family = N.FAMILY_VECTOR_SUM
        d[0].nterms = nterms
        for t, w in enumerate(weights):
            d[0].ls[0][t] = w
        return d

    def put(d, t, k):
        ctypes.memmove(ctypes.byref(d[1 + t]), ctypes.byref(k), ctypes.sizeof(N.KernelDesc))

    def assemble(d):
        return L.gp2d_assemble(one, 10, 64, one, 10, 64, ctypes.byref(d), 0.0, 0, one, 128, None)

    cases = []
    for nterms in (0, 4, -1):
        cases.append((header(nterms, [1.0, 1.0, 1.0]), b"nterms must be 1..3"))
    d = header(2, [1.0, 1.0]); put(d, 0, good2); put(d, 1, goodst)
    cases.append((d, b"all VECTOR2D or all VECTOR_ST"))
    d = header(2, [1.0, 1.0]); put(d, 0, good2); d[2].family = N.FAMILY_VECTOR_SUM; d[2].nterms = 1
    cases.append((d, b"must not be a sum"))
    d = header(2, [1.0, 1.0]); put(d, 0, good2); put(d, 1, ard)
    cases.append((d, b"ARD terms"))
    for w in (0.0, -0.5, float("nan")):
        d = header(2, [1.0, w]); put(d, 0, good2); put(d, 1, good2)
        cases.append((d, b"weight must be > 0"))
    d = header(2, [1.0, 1.0]); put(d, 0, good2); put(d, 1, N.vector_kernel_desc(N.KIND_DIVFREE, -1.0))
    cases.append((d, b"term 1 is invalid: l_df must be > 0"))
    d = header(1, [1.0]); put(d, 0, N.vector_st_kernel_desc(N.KIND_DIVFREE, 5.0, 5.0, 1.0, 0.0, 2.0))
    cases.append((d, b"term 0 is invalid: spatio-temporal"))
    for d, msg in cases:
        assert assemble(d) < 0 and msg in L.gp2d_last_error(), (msg, L.gp2d_last_error())
        assert L.gp2d_lml_grad_count(ctypes.byref(d)) < 0 and msg in L.gp2d_last_error()
        assert L.gp2d_assemble_cols(one, 10, 64, ctypes.byref(d), 0.0, one, 128, 0, 64, None) < 0
        assert msg in L.gp2d_last_error()
        assert L.gp2d_predict(one, 128, 128, one, one, 10, 64, one, 5, ctypes.byref(d), 0, 0.0, 1, one, one, 64, one,
                              big, None) < 0 and msg in L.gp2d_last_error()
        assert L.gp2d_kernel_grad(one, 5, one, 5, ctypes.byref(d), one, 10, one, one, big, None) < 0
        assert msg in L.gp2d_last_error()
        assert math.isnan(L.gp2d_field_prior_var(ctypes.byref(d), N.FIELD_VORTICITY))

    # a valid sum: the entries without a sum form refuse it by name, before anything else
    s = header(2, [1.0, 0.05]); put(s, 0, good2); put(s, 1, N.vector_kernel_desc(N.KIND_DIVFREE, 2.0))
    k = ctypes.byref(s)
    out16 = (ctypes.c_double * 16)()
    nmod = ctypes.c_int(0)
    refused = {
        "gp2d_grad_prior_cov": lambda: L.gp2d_grad_prior_cov(k, out16),
        "gp2d_predict_grad": lambda: L.gp2d_predict_grad(one, 256, 256, one, one, 100, 128, one, 10, k, 1, one, one, 64,
                                                         one, big, None),
        "gp2d_predict_cov": lambda: L.gp2d_predict_cov(one, 256, 256, one, one, 100, 128, one, 10, k, 0.0, one, one,
                                                       128, one, big, None),
        "gp2d_ozaki_prepare": lambda: L.gp2d_ozaki_prepare(one, 256, 256, k, 0, 0, one, one, ctypes.byref(nmod), None),
        "gp2d_ozaki_prepare_async": lambda: L.gp2d_ozaki_prepare_async(one, 256, 256, k, 0.0025, 0, 0, one, one,
                                                                       ctypes.byref(nmod), None),
        "gp2d_ozaki_prepare_packed": lambda: L.gp2d_ozaki_prepare_packed(one, 256, k, 0.0025, 0, 0, one, one,
                                                                         ctypes.byref(nmod), None),
        "gp2d_ozaki_nmod_apriori": lambda: L.gp2d_ozaki_nmod_apriori(256, k, 0.0025, 0, 0),
        "gp2d_ozaki_kstar": lambda: L.gp2d_ozaki_kstar(one, 100, 128, one, 10, k, 10, 0, 256, one, big, None),
        "gp2d_predict_ozaki": lambda: L.gp2d_predict_ozaki(one, one, 10, 0, 256, one, one, 100, 128, one, 10, k, 0, 0.0,
                                                           1, one, one, None, 256, one, big, None),
        "gp2d_predict_ozaki_planes": lambda: L.gp2d_predict_ozaki_planes(one, one, 10, 0, 256, one, one, 100, 128, one,
                                                                         10, k, 0, 0.0, one, 10, 0, one, one, None, 256,
                                                                         one, big, None),
    }
    for name, call in refused.items():
        assert call() < 0, name
        assert b"sum" in L.gp2d_last_error(), (name, L.gp2d_last_error())
    assert all(math.isnan(v) for v in out16)
    # and the field predict refuses a sum with a scalar term
    sc = header(2, [1.0, 1.0]); put(sc, 0, good2); put(sc, 1, N.vector_kernel_desc(N.KIND_SCALAR, 3.0))
    assert L.gp2d_predict_field(one, 256, 256, one, one, 100, 128, one, 10, ctypes.byref(sc), N.FIELD_VORTICITY, 1,
                                one, one, 128, one, big, None) < 0
    assert b"vector kernels only" in L.gp2d_last_error()


def _spec3():
    from gp2d import engine as E
    terms = (E.KernelSpec(kind="mixed", l_df=8.0, l_cf=6.0, ratio=0.6), E.KernelSpec(kind="df", l_df=2.0),
             E.KernelSpec(kind="cf", l_cf=1.2, ratio=0.0))
    return E.KernelSpec(family="vector_sum", terms=terms, weights=(1.0, 0.05, 0.02))


def test_param_names_order_and_length():
    from gp2d import engine as E
    from gp2d import _native as N
    s = _spec3()
    names = E.param_names(s)
    assert names == ("weight_0", "l_df_0", "l_cf_0", "ratio_0", "weight_1", "l_df_1", "l_cf_1", "ratio_1",
                     "weight_2", "l_df_2", "l_cf_2", "ratio_2", "noise")
    assert len(names) == N.lib().gp2d_lml_grad_count(ctypes.byref(s.desc()))
    st = E.KernelSpec(family="vector_sum", weights=(1.0, 1.0),
                      terms=(E.KernelSpec(family="vector_st", kind="df", l_df=5.0, var_t=1.5, l_t=3.0),
                             E.KernelSpec(family="vector_st", kind="df", l_df=1.0, var_t=0.1, l_t=1.0)))
    names = E.param_names(st)
    assert names == ("weight_0", "l_df_0", "l_cf_0", "ratio_0", "var_t_0", "l_t_0",
                     "weight_1", "l_df_1", "l_cf_1", "ratio_1", "var_t_1", "l_t_1", "noise")
    assert names == S.param_names([dict(var_t=1, l_t=1)] * 2)
    assert len(names) == N.lib().gp2d_lml_grad_count(ctypes.byref(st.desc()))
    assert s.is_vector and s.block_dim == 2 and s.input_dim == 2 and st.input_dim == 3
    assert s.kdiag() == pytest.approx(1.0 * (0.6 / 64 + 0.4 / 36) + 0.05 / 4 + 0.02 / 1.44, rel=1e-15)
    t1 = s.term(1)
    assert t1.family == "vector_sum" and t1.terms == (s.terms[1],) and t1.weights == (0.05,)
    assert t1.kdiag() == pytest.approx(0.05 / 4, rel=1e-15)
    with pytest.raises(ValueError, match="term must be"):
        s.term(3)
    with pytest.raises(ValueError, match="sum"):
        s.grad_prior_cov()
    with pytest.raises(ValueError, match="all 'vector2d' or all 'vector_st'"):
        E.KernelSpec(family="vector_sum", terms=(s.terms[0], st.terms[0]), weights=(1.0, 1.0)).desc()
    with pytest.raises(ValueError, match="1..3 terms"):
        E.KernelSpec(family="vector_sum").desc()
    for variance_user in (lambda: E._check_family(s, "ozaki"), lambda: E.fit(s, np.zeros((4, 2)), np.zeros(8), 0.01,
                                                                              variance="ozaki")):
        with pytest.raises(ValueError, match="variance='f64'"):
            variance_user()


def test_hyper_pack_unpack_round_trips_a_three_term_sum():
    from gp2d import engine as E
    from gp2d import hyper as H
    s = _spec3()
    p = H.get_params(s, 0.0025)
    assert tuple(p) == E.param_names(s)
    assert p["weight_1"] == 0.05 and p["l_df_1"] == 2.0 and p["l_cf_2"] == 1.2 and p["noise"] == 0.0025
    k, nz = H.set_params(s, p)
    assert k == s and nz == 0.0025
    # what the optimiser moves: a vector2d term's weight and what its kind uses
    assert H.free_names(s) == ("weight_0", "l_df_0", "l_cf_0", "ratio_0", "weight_1", "l_df_1", "weight_2", "l_cf_2",
                               "noise")
    assert H.free_names(s, fix=("weight_0", "noise")) == ("l_df_0", "l_cf_0", "ratio_0", "weight_1", "l_df_1",
                                                          "weight_2", "l_cf_2")
    # through the free coordinates and back
    names = H.free_names(s)
    z = [H._to_free(n, p[n]) for n in names]
    q = dict(p, **{n: H._from_free(n, zi) for n, zi in zip(names, z)})
    k2, _ = H.set_params(s, q)
    for a, b in zip(H.get_params(k2, 0.0025).values(), p.values()):
        assert a == pytest.approx(b, rel=1e-14)
    assert H._dfree("ratio_0", 0.6) == pytest.approx(0.24) and H._dfree("weight_1", 0.05) == 0.05
    # a spatio-temporal term's amplitude is var_t: its weight is held
    st = E.KernelSpec(family="vector_sum", weights=(1.0, 1.0),
                      terms=(E.KernelSpec(family="vector_st", kind="df", l_df=5.0, var_t=1.5, l_t=3.0),
                             E.KernelSpec(family="vector_st", kind="mixed", l_df=1.0, l_cf=2.0, ratio=0.5, var_t=0.1)))
    assert H.free_names(st) == ("l_df_0", "var_t_0", "l_t_0", "l_df_1", "l_cf_1", "ratio_1", "var_t_1", "l_t_1", "noise")
    k3, _ = H.set_params(st, dict(H.get_params(st, 0.01), var_t_1=0.2, weight_0=1.0))
    assert k3.terms[1].var_t == 0.2 and k3.terms[0] == st.terms[0] and k3.weights == (1.0, 1.0)
