"""Particles advected through the fitted flow on the device (gp2d_advect, engine.advect, Krig.advect,
Krig.ftle_grid) against the numpy reference tests/advect_ref.py.

Gates.  The project's gate for a predicted mean is 1e-10 relative to its largest entry; a
per-evaluation difference of ε = 1e-10·Umax, carried by the flow map, moves a position by at most
    ε·s·Umax·|T|·Fmax                                                   (the position gate),
with Umax = max |μ| and Fmax = max ‖F‖₂ from the reference run.  The tangent gate is measured: 20 ×
the deviation of F that advect_ref shows when every velocity and gradient evaluation is perturbed by
the same relative ε = 1e-10 (seeded) — 20 being the factor between that noise run's position
deviation and the position bound.  Each test prints its gates and what it observed.  The
truncation differences of tests/test_advect_cpu.py are ≥ 1e-6, so a wrong stage weight or stage
time cannot pass.
"""
import dataclasses
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
if not torch.cuda.is_available():  # pragma: no cover
    pytest.skip("no HIP device", allow_module_level=True)

import advect_ref as A  # noqa: E402
import sum_ref as S  # noqa: E402
import trend_ref as T  # noqa: E402
from gp2d import engine as E  # noqa: E402
from gp2d.krig import Krig  # noqa: E402
from oracle import gp2d_oracle as O  # noqa: E402

DEV = torch.device("cuda")
EPS = 1e-10
KINDS = [("df", 1.0), ("cf", 0.0), ("mixed", 0.35)]
N_TR, T_END, NSTEPS = 200, 20.0, 40


def host(t):
    return t.cpu().numpy()


def spec(kind, ratio):
    return E.KernelSpec(kind=kind, l_df=A.L_DF, l_cf=A.L_CF, ratio=ratio)


def bits(a):
    return np.ascontiguousarray(a).view(np.int64)


@dataclasses.dataclass
class Ref:
    run: A.Run
    pos_gate: float
    tan_gate: float


def make_ref(flow, x0, t0, dt, nsteps, s=1.0):
    """The reference run with its two gates (the module docstring)."""
    run = A.advect(flow, x0, t0, dt, nsteps, vel_scale=s)
    noisy = A.advect(flow, x0, t0, dt, nsteps, vel_scale=s, eps=EPS, seed=7)
    pos_gate = EPS * abs(s) * run.umax * abs(dt * nsteps) * run.fmax
    tan_gate = 20.0 * float(np.max(np.abs(noisy.tangent - run.tangent))) if nsteps else 0.0
    return Ref(run, pos_gate, tan_gate)


def check(name, ref, save_every, path, tan, times=None, t0=0.0, dt=None):
    """Every record of a device run against the reference's steps."""
    idx = ref.run.records(save_every)
    path, tan = host(path), host(tan)
    assert path.shape == (len(idx),) + ref.run.path.shape[1:] and tan.shape == (len(idx),) + ref.run.tangent.shape[1:]
    ep = float(np.max(np.abs(path - ref.run.path[idx])))
    et = float(np.max(np.abs(tan - ref.run.tangent[idx])))
    print(f"{name} save_every={save_every}: position diff {ep:.2e} (gate {ref.pos_gate:.2e}), tangent diff {et:.2e} "
          f"(gate {ref.tan_gate:.2e}); Umax {ref.run.umax:.3f}, Fmax {ref.run.fmax:.2f}")
    assert ep <= ref.pos_gate and et <= ref.tan_gate, (name, ep, ref.pos_gate, et, ref.tan_gate)
    if times is not None:
        assert np.array_equal(host(times), t0 + idx * dt)


# ---------------------------------------------------------------- the shared fits and references
@functools.lru_cache(maxsize=None)
def starts():
    return A.seeds(A.tracks(N_TR)[0])


@functools.lru_cache(maxsize=None)
def gpu_fit(n, kind, ratio, variance="f64"):
    x, y = A.tracks(n)
    return E.fit(spec(kind, ratio), np.array(x), np.array(y), noise=A.NOISE, device=DEV, variance=variance)


@functools.lru_cache(maxsize=None)
def plain_ref(kind, ratio, dt=T_END / NSTEPS):
    return make_ref(A.oracle_flow(N_TR, kind, ratio), starts(), 0.0, dt, NSTEPS)


@functools.lru_cache(maxsize=None)
def df_run(save_every=8, tangent=True):
    """The 300 particles of the div-free fit in one call (the bit-identity tests' baseline)."""
    _, p, f = E.advect(gpu_fit(N_TR, "df", 1.0), starts(), dt=T_END / NSTEPS, nsteps=NSTEPS, save_every=save_every,
                       tangent=tangent)
    return host(p), (None if f is None else host(f))


# ---------------------------------------------------------------- a. plain 2-D flow
@pytest.mark.parametrize("kind,ratio", KINDS)
def test_plain_flow_matches_reference(kind, ratio):
    """df, cf and mixed: every record of path and tangent, with save_every 8 and 7 (which does not
    divide 40: the last record sits at step 40).  Two start points 1e4 away from the data, where
    every exp underflows: their velocity is exactly 0 and every record equals x0 bit for bit."""
    gp, ref = gpu_fit(N_TR, kind, ratio), plain_ref(kind, ratio)
    far = np.array([[1e4, 30.0], [20.0, -1e4]])
    x0 = np.concatenate([starts(), far])
    for save_every in (8, 7):
        t, p, f = E.advect(gp, x0, t0=0.0, dt=T_END / NSTEPS, nsteps=NSTEPS, save_every=save_every, tangent=True)
        check(kind, ref, save_every, p[:, :300], f[:, :300], t, 0.0, T_END / NSTEPS)
        p, f = host(p), host(f)
        assert np.array_equal(bits(p[:, 300:]), bits(np.broadcast_to(far, p[:, 300:].shape)))
        assert np.array_equal(f[:, 300:], np.broadcast_to(np.eye(2), f[:, 300:].shape))


# ---------------------------------------------------------------- b. backward in time
def test_negative_dt():
    ref = plain_ref("mixed", 0.35, -T_END / NSTEPS)
    t, p, f = E.advect(gpu_fit(N_TR, "mixed", 0.35), starts(), t0=0.0, dt=-T_END / NSTEPS, nsteps=NSTEPS, save_every=8,
                       tangent=True)
    check("mixed dt<0", ref, 8, p, f, t, 0.0, -T_END / NSTEPS)
    fwd = plain_ref("mixed", 0.35).run.path[-1]
    assert np.max(np.abs(host(p)[-1] - fwd)) > 1.0   # not the forward run


# ---------------------------------------------------------------- c. the spatio-temporal product
ST = dict(kind="mixed", l_df=5.0, l_cf=4.0, ratio=0.3, var_t=2.0, l_t=1.5)


def st_tracks(n, seed=5):
    """test_gpu_st.st_tracks: rows (t, x1, x2), a flow that drifts in time."""
    rng = np.random.default_rng(seed)
    X = np.stack([rng.uniform(0, 6, n), rng.uniform(0, 45, n), rng.uniform(0, 60, n)], 1)
    f1 = np.cos(X[:, 2] / 9) + 0.1 * X[:, 0] + rng.normal(0, 0.05, n)
    f2 = np.sin(X[:, 1] / 7) - 0.05 * X[:, 0] + rng.normal(0, 0.05, n)
    return X, np.concatenate([f1, f2])


def test_spatio_temporal_flow():
    """A (t, x1, x2) fit of 150 points with var_t = 2, l_t = 1.5; t0 = 1 inside the data's time span
    and h = 0.375 = l_t/4, eight steps: the mean changes by its own size over the run, so half-step
    stage times that are wrong cannot pass."""
    X, y = st_tracks(150)
    K = O.vector_st_kernel(X, X, **ST)
    K[np.diag_indices_from(K)] += A.NOISE
    flow = A.Flow((ST,), (1.0,), X, np.linalg.solve(K, y))
    x0 = A.seeds(X, 120, seed=2)
    t0, dt, nsteps, s = 1.0, 0.375, 8, 2.0
    ref = make_ref(flow, x0, t0, dt, nsteps, s)
    gp = E.fit(E.KernelSpec(family="vector_st", **ST), X, y, noise=A.NOISE, device=DEV)
    t, p, f = E.advect(gp, x0, t0=t0, dt=dt, nsteps=nsteps, save_every=3, vel_scale=s, tangent=True)
    check("vector_st", ref, 3, p, f, t, t0, dt)
    # what the stage times are worth here: the same run with the mean frozen at each step's start
    frozen = A.Flow((ST,), (1.0,), X, flow.alpha)
    frozen._points = lambda q, tt: A.Flow._points(flow, q, np.floor((tt - t0) / dt + 1e-9) * dt + t0)
    wrong = A.advect(frozen, x0, t0, dt, nsteps, vel_scale=s).path[-1]
    assert np.max(np.abs(wrong - ref.run.path[-1])) > 1e3 * ref.pos_gate


# ---------------------------------------------------------------- d. bit identity
def test_bits_do_not_depend_on_the_call():
    """The 300 particles in one call, in two calls of 150, in reversed order and one alone give the
    same bits per particle; the final record does not depend on save_every; the path does not
    depend on whether the tangent is integrated."""
    gp, x0 = gpu_fit(N_TR, "df", 1.0), starts()
    kw = dict(dt=T_END / NSTEPS, nsteps=NSTEPS, save_every=8, tangent=True)
    p, f = df_run()
    halves = [E.advect(gp, x0[a:a + 150], **kw) for a in (0, 150)]
    assert np.array_equal(bits(np.concatenate([host(h[1]) for h in halves], 1)), bits(p))
    assert np.array_equal(bits(np.concatenate([host(h[2]) for h in halves], 1)), bits(f))
    _, pr, fr = E.advect(gp, x0[::-1].copy(), **kw)
    assert np.array_equal(bits(host(pr)[:, ::-1]), bits(p)) and np.array_equal(bits(host(fr)[:, ::-1]), bits(f))
    for j in (0, 77, 299):
        _, p1, f1 = E.advect(gp, x0[j:j + 1], **kw)
        assert np.array_equal(bits(host(p1)[:, 0]), bits(p[:, j])) and np.array_equal(bits(host(f1)[:, 0]), bits(f[:, j]))
    pe, fe = df_run(NSTEPS)
    assert pe.shape == (2, 300, 2)
    assert np.array_equal(bits(pe[-1]), bits(p[-1])) and np.array_equal(bits(fe[-1]), bits(f[-1]))
    p7, f7 = df_run(7)
    assert np.array_equal(bits(p7[-1]), bits(p[-1])) and np.array_equal(bits(f7[-1]), bits(f[-1]))
    pn, fn = df_run(8, False)
    assert fn is None and np.array_equal(bits(pn), bits(p))
    assert np.array_equal(bits(df_run(None, False)[0][-1]), bits(p[-1]))   # save_every=None: the end only


# ---------------------------------------------------------------- e. smallest shapes
@pytest.mark.parametrize("ntr,m", [(1, 1), (1, 65), (65, 1), (65, 65), (65, 257)])
def test_smallest_shapes(ntr, m):
    """ntr = 1; ntr = 65 (ntr_pad 128, a partial tile, the second slice's first point); m = 1, 65, 257
    (a partial wave, more than one workgroup with the last one partial)."""
    x, y = A.tracks(ntr)
    fit = O.OracleFit(x, y, "mixed", A.L_DF, A.L_CF, 0.35, A.NOISE)
    flow = A.Flow((A.term("mixed", 0.35),), (1.0,), x, fit.alpha)
    x0 = A.seeds(x, m, seed=m) if m > 5 else x[:1] + 0.5
    ref = make_ref(flow, x0, 0.0, 0.5, 8)
    gp = gpu_fit(ntr, "mixed", 0.35)
    assert gp.n_pad == {1: 64, 65: 128}[ntr]
    t, p, f = E.advect(gp, x0, dt=0.5, nsteps=8, save_every=3, tangent=True)
    check(f"ntr={ntr} m={m}", ref, 3, p, f, t, 0.0, 0.5)
    assert ref.run.umax > 0 and np.max(np.abs(ref.run.path[-1] - x0)) > 0


@pytest.mark.parametrize("tangent", [True, False])
def test_no_steps(tangent):
    """nsteps = 0: record 0 alone, x0 bit for bit and F = I; dt is not needed."""
    x0 = starts()[:70]
    t, p, f = E.advect(gpu_fit(N_TR, "df", 1.0), x0, t0=3.0, dt=0.0, nsteps=0, save_every=5, tangent=tangent)
    assert host(t).tolist() == [3.0] and np.array_equal(bits(host(p)), bits(x0[None]))
    assert (f is None) if not tangent else np.array_equal(host(f), np.broadcast_to(np.eye(2), (1, 70, 2, 2)))
    t, p, _ = E.advect(gpu_fit(N_TR, "df", 1.0), np.empty((0, 2)), dt=0.5, nsteps=4, save_every=2)
    assert p.shape == (3, 0, 2) and host(t).tolist() == [0.0, 1.0, 2.0]


# ---------------------------------------------------------------- f. a kernel sum and trend fits
def term_spec(t):
    return E.KernelSpec(family="vector_st", **t) if S.is_st(t) else E.KernelSpec(**t)


@pytest.mark.parametrize("case,trend", [("sum", None), ("sum", "constant"), ("sum", "linear"),
                                        ("vector_st", "linear")])
def test_sum_and_trend_fits(case, trend):
    """A two-term vector_sum fit, zero-mean and with a constant or linear trend, and a linear trend
    on the spatio-temporal product.  The reference takes α′ and β̂ from the device fit and evaluates
    Σ_t w_t·K_t·α′ + h(x)ᵀβ̂ in numpy: the advect kernel is what is under test.  A linear trend's
    constant gradient must show in F."""
    terms, weights = T.CASES[case]
    x, y, _ = T.case_data(case, 100)
    ks = E.KernelSpec(family="vector_sum", terms=tuple(term_spec(t) for t in terms), weights=tuple(weights)) \
        if case == "sum" else term_spec(terms[0])
    gp = E.fit(ks, np.array(x), np.array(y), noise=T.NOISE, device=DEV, trend=trend)
    alpha = host(gp.alpha).reshape(2, gp.n_pad)[:, :gp.n_train].reshape(-1)
    tr = None
    if trend is not None:
        c = E.trend_coefficients(gp)
        tr = dict(beta=c["beta"], centre=c["centre"], scale=c["scale"])
        assert np.max(np.abs(c["beta"])) > 0.1   # the data's background flow
    flow = A.Flow(tuple(terms), tuple(weights), x, alpha, tr)
    x0 = A.seeds(x, 90, seed=4)
    t0, dt, nsteps, s = 1.0, 0.5, 12, 1.5
    ref = make_ref(flow, x0, t0, dt, nsteps, s)
    t, p, f = E.advect(gp, x0, t0=t0, dt=dt, nsteps=nsteps, save_every=5, vel_scale=s, tangent=True)
    check(f"{case} trend={trend}", ref, 5, p, f, t, t0, dt)
    if trend == "linear":   # the same flow without the trend's gradient in ∇μ is far outside the gate
        bare = A.Flow(tuple(terms), tuple(weights), x, alpha, tr)
        grad = bare.gradient
        bare.gradient = lambda q, tt: grad(q, tt) - (np.asarray(tr["beta"])[2:6] / tr["scale"]).reshape(2, 2)
        other = A.advect(bare, x0, t0, dt, nsteps, vel_scale=s).tangent[-1]
        assert np.max(np.abs(other - host(f)[-1])) > 1e3 * ref.tan_gate
    if trend is not None:   # and the trend moves the particles
        assert np.max(np.abs(A.advect(dataclasses.replace(flow, trend=None), x0, t0, dt, nsteps, vel_scale=s,
                                      tangent=False).path[-1] - host(p)[-1])) > 1.0


# ---------------------------------------------------------------- g. either variance engine, no W
def test_ozaki_fit_and_fit_without_w():
    """A variance='ozaki' fit of 256 points (Morton-ordered: gp.perm is a permutation, α and x share
    it) and the FP64 fit of the same data both agree with the reference; a fit object that kept no
    W (a job stream's receiving rank) advects to the same bits."""
    n = 256
    x, _ = A.tracks(n)
    x0 = A.seeds(x, 130, seed=9)
    ref = make_ref(A.oracle_flow(n, "df", 1.0), x0, 0.0, 0.5, 16)
    kw = dict(dt=0.5, nsteps=16, save_every=16, tangent=True)
    for variance in ("ozaki", "f64"):
        gp = gpu_fit(n, "df", 1.0, variance)
        if variance == "ozaki":
            perm = host(gp.perm)
            assert sorted(perm.tolist()) == list(range(n)) and not np.array_equal(perm, np.arange(n))
        t, p, f = E.advect(gp, x0, **kw)
        check(variance, ref, 16, p, f)
        bare = dataclasses.replace(gp, W=None, n_mat=gp.n)
        _, pb, fb = E.advect(bare, x0, **kw)
        assert np.array_equal(bits(host(pb)), bits(host(p))) and np.array_equal(bits(host(fb)), bits(host(f)))


# ---------------------------------------------------------------- h. a NaN start position
@pytest.mark.parametrize("bad", [(np.nan, np.nan), (np.nan, 12.0), (np.inf, 12.0)])
def test_non_finite_start(bad):
    """Every record of a non-finite start is NaN (its tangent after the identity of record 0); every
    other particle keeps the bits of the run without it."""
    p, f = df_run()
    x0 = starts().copy()
    j = 70   # inside the second wave of its workgroup
    x0[j] = bad
    _, q, g = E.advect(gpu_fit(N_TR, "df", 1.0), x0, dt=T_END / NSTEPS, nsteps=NSTEPS, save_every=8, tangent=True)
    q, g = host(q), host(g)
    assert np.isnan(q[:, j]).all() and np.isnan(g[1:, j]).all() and np.array_equal(g[0, j], np.eye(2))
    keep = np.arange(300) != j
    assert np.array_equal(bits(q[:, keep]), bits(p[:, keep])) and np.array_equal(bits(g[:, keep]), bits(f[:, keep]))


# ---------------------------------------------------------------- i. the Krig surface
def test_krig_advect_and_ftle_grid():
    """Krig.advect returns numpy arrays; Krig.ftle_grid seeds meshgrid(x, y) as predict_grid does and
    returns [y.size, x.size], equal to engine.ftle of engine.advect's tangent at the same seeds."""
    xt, yt = A.tracks(N_TR)
    k = Krig("df", l_df=A.L_DF, noise=A.NOISE, device=DEV).fit(xt, yt)
    gx, gy = np.linspace(0, 45, 17), np.linspace(5, 55, 13)
    X, Y = np.meshgrid(gx, gy)
    pts = np.stack([X.reshape(-1), Y.reshape(-1)], 1)
    t, p, f = k.advect(pts, t0=0.0, dt=0.5, nsteps=10, save_every=4, tangent=True)
    assert all(isinstance(a, np.ndarray) for a in (t, p, f))
    assert t.tolist() == [0.0, 2.0, 4.0, 5.0] and p.shape == (4, 221, 2) and f.shape == (4, 221, 2, 2)
    assert k.advect(pts, dt=0.5, nsteps=10)[2] is None
    field = k.ftle_grid(gx, gy, 0.0, 5.0, 10)
    assert field.shape == (13, 17)
    _, _, tan = E.advect(k.gp, pts, dt=0.5, nsteps=10, tangent=True)
    want = host(E.ftle(tan[-1], 5.0)).reshape(13, 17)
    assert np.array_equal(bits(field), bits(want))
    # row y, column x (the CPU's log and sqrt may round differently from the device's)
    assert abs(field[3, 5] - float(E.ftle(torch.as_tensor(f[-1, 3 * 17 + 5]), 5.0))) < 1e-14
    assert np.max(np.abs(field - field[:, ::-1])) > 1e-3 and np.max(np.abs(field - field[::-1])) > 1e-3
    assert np.max(np.abs(field - A.ftle(f[-1], 5.0).reshape(13, 17))) < 1e-12   # numpy's eigensolver
    back = k.ftle_grid(gx, gy, 5.0, -5.0, 10)
    assert back.shape == (13, 17) and np.isfinite(back).all() and not np.array_equal(back, field)


def test_kernels_without_a_velocity_are_refused():
    x, y = A.tracks(N_TR)
    gp = gpu_fit(N_TR, "df", 1.0)
    with pytest.raises(ValueError, match="advection needs"):
        E.advect(dataclasses.replace(gp, kernel=E.KernelSpec(kind="scalar", l_df=5.0)), starts(), dt=0.5, nsteps=2)
    with pytest.raises(ValueError, match="advection needs"):
        E.advect(dataclasses.replace(gp, kernel=E.KernelSpec(family="ard", variances=(1.0,), lengthscales=((3.0, 4.0),))),
                 starts(), dt=0.5, nsteps=2)
    with pytest.raises(ValueError, match="dt and nsteps"):
        E.advect(gp, starts())
