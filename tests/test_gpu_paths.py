"""Posterior draws of the flow and ensembles advected through them on the device (gp2d_paths_eval,
gp2d_advect_draws, engine.draw_flows / advect_draws / path_spread, Krig.advect_ensemble) against
the numpy reference tests/paths_ref.py.  Feature tables and noise draws are passed in, so the device
and the reference see the same numbers; the statistics of the draws are tests/test_paths_cpu.py's.

Gates.  Velocities and α: the project's gate for a predicted mean, 1e-10 relative to the largest
entry.  Positions: tests/test_gpu_advect.py's gate ε·s·Umax·|T|·Fmax with ε = 1e-10 and Umax, Fmax
from the reference run of that draw (tangent on).  Each test prints its gates and what it observed.
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

import advect_ref as A  # noqa: E402
import paths_ref as PR  # noqa: E402
from gp2d import _native as N  # noqa: E402
from gp2d import engine as E  # noqa: E402
from gp2d import paths as P  # noqa: E402
from gp2d.krig import Krig  # noqa: E402

DEV = torch.device("cuda")
EPS = 1e-10
ST = dict(kind="mixed", l_df=5.0, l_cf=4.0, ratio=0.3, var_t=2.0, l_t=1.5)
SUM_TERMS = (A.term("mixed", 0.6, l_df=6.0, l_cf=2.5), A.term("df", 1.0, l_df=2.0))
SUM_WEIGHTS = (0.7, 1.8)


def host(t):
    return t.cpu().numpy()


def bits(a):
    return np.ascontiguousarray(a).view(np.int64)


def st_tracks(n, seed=5):
    """test_gpu_advect.st_tracks: rows (t, x1, x2), a flow that drifts in time."""
    rng = np.random.default_rng(seed)
    X = np.stack([rng.uniform(0, 6, n), rng.uniform(0, 45, n), rng.uniform(0, 60, n)], 1)
    f1 = np.cos(X[:, 2] / 9) + 0.1 * X[:, 0] + rng.normal(0, 0.05, n)
    f2 = np.sin(X[:, 1] / 7) - 0.05 * X[:, 0] + rng.normal(0, 0.05, n)
    return X, np.concatenate([f1, f2])


@dataclasses.dataclass
class Case:
    gp: object
    terms: tuple
    weights: tuple
    x: np.ndarray
    y: np.ndarray
    table: np.ndarray
    eps: np.ndarray
    draws: object      # engine.FlowDraws from (table, eps)
    flows: list        # the reference's DrawFlow per draw

    def alpha_input_order(self):
        """draws.alpha as (S, 2·n_train) in the caller's order (an ozaki fit is Morton-sorted)."""
        gp = self.gp
        a = host(self.draws.alpha).reshape(-1, 2, gp.n_pad)[:, :, :gp.n_train]
        if gp.perm is not None:
            out = np.empty_like(a)
            out[:, :, host(gp.perm)] = a
            a = out
        return a.reshape(a.shape[0], -1)


def kernel_case(name):
    if name in ("df", "cf", "mixed"):
        ratio = {"df": 1.0, "cf": 0.0, "mixed": 0.35}[name]
        return E.KernelSpec(kind=name, l_df=A.L_DF, l_cf=A.L_CF, ratio=ratio), (A.term(name, ratio),), (1.0,)
    if name == "vector_st":
        return E.KernelSpec(family="vector_st", **ST), (ST,), (1.0,)
    if name == "sum":
        return E.KernelSpec(family="vector_sum", terms=tuple(E.KernelSpec(**t) for t in SUM_TERMS),
                            weights=SUM_WEIGHTS), SUM_TERMS, SUM_WEIGHTS
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def case(name, n=120, S=3, F=40, variance="f64"):
    ks, terms, weights = kernel_case(name)
    x, y = st_tracks(n) if name == "vector_st" else A.tracks(n)
    gp = E.fit(ks, np.array(x), np.array(y), noise=A.NOISE, device=DEV, variance=variance)
    table = P.feature_table(ks, S, F, seed=n + F)
    eps = P.noise_draws(S, 2 * n, A.NOISE, seed=n + F)
    draws = E.draw_flows(gp, S, features=table, eps=eps)
    flows = PR.draw_flows(terms, weights, x, y, A.NOISE, table, eps)
    return Case(gp, terms, weights, x, y, table, eps, draws, flows)


def rel(a, b):
    return float(np.max(np.abs(a - b)) / np.max(np.abs(b)))


@functools.lru_cache(maxsize=None)
def ref_run(name, s, m, t0, dt, nsteps, vel=1.0, **kw):
    c = case(name, **kw)
    x0 = A.seeds(c.x, m, seed=4) if m > 5 else c.x[:m, -2:] + 0.5
    return x0, A.advect(c.flows[s], x0, t0, dt, nsteps, vel_scale=vel, tangent=True)


def check_paths(label, paths, name, m, t0, dt, nsteps, save_every, vel=1.0, **kw):
    """Every record of every draw against the reference run of that draw."""
    paths = host(paths)
    for s in range(paths.shape[1]):
        x0, run = ref_run(name, s, m, t0, dt, nsteps, vel, **kw)
        idx = run.records(save_every)
        assert paths.shape == (len(idx), paths.shape[1], m, 2)
        gate = EPS * abs(vel) * run.umax * abs(dt * nsteps) * run.fmax
        err = float(np.max(np.abs(paths[:, s] - run.path[idx])))
        print(f"{label} draw {s}: position diff {err:.2e} (gate {gate:.2e}); Umax {run.umax:.3f}, Fmax {run.fmax:.2f}")
        assert err <= gate, (label, s, err, gate)
        assert np.max(np.abs(run.path[-1] - x0)) > 0 and run.umax > 0


# ---------------------------------------------------------------- a. velocity and α
@pytest.mark.parametrize("name,kw", [("df", {}), ("cf", {}), ("mixed", {}), ("vector_st", {}), ("sum", {}),
                                     ("df", dict(n=256, variance="ozaki"))])
def test_velocity_and_alpha_match_reference(name, kw):
    """FlowDraws.velocity at 70 points (five on training points) and draws.alpha against the
    reference, 1e-10 relative to the largest entry; an ozaki fit holds W and is served, its Morton
    permutation applied to eps and to the training order.  The table passes through unchanged."""
    c = case(name, **kw)
    if kw:
        perm = host(c.gp.perm)
        assert sorted(perm.tolist()) == list(range(256)) and not np.array_equal(perm, np.arange(256))
    xg = A.seeds(c.x, 70, seed=3)
    t = 1.7 if name == "vector_st" else 0.0
    got = host(c.draws.velocity(xg, t))
    want = PR.velocity_rows(c.flows, xg, t)
    al, al_ref = c.alpha_input_order(), np.stack([f.alpha for f in c.flows])
    ev, ea = rel(got, want), rel(al, al_ref)
    print(f"{name} {kw}: velocity rel diff {ev:.2e}, alpha rel diff {ea:.2e} (gate {EPS:.0e}); "
          f"max|v| {np.max(np.abs(want)):.3f}, max|alpha| {np.max(np.abs(al_ref)):.3f}")
    assert got.shape == (3, 140) and ev <= EPS and ea <= EPS
    assert np.array_equal(bits(host(c.draws.features)), bits(c.table))
    # the draws differ from each other and from the mean flow by far more than the gate
    assert np.max(np.abs(want[0] - want[1])) > 1e-3 * np.max(np.abs(want))
    pad = host(c.draws.alpha).reshape(3, 2, c.gp.n_pad)[:, :, c.gp.n_train:]
    assert np.all(pad == 0.0)


def test_seeded_draws():
    """Without features and eps the host generators are used: the same seed gives the same bits, and
    α is the reference's for paths.feature_table / paths.noise_draws of that seed."""
    c = case("mixed")
    d1, d2 = E.draw_flows(c.gp, 2, n_features=24, seed=9), E.draw_flows(c.gp, 2, n_features=24, seed=9)
    assert d1.features.shape == (2, 48, 6) and np.array_equal(bits(host(d1.alpha)), bits(host(d2.alpha)))
    table, eps = P.feature_table(c.gp.kernel, 2, 24, seed=9), P.noise_draws(2, 240, A.NOISE, seed=9)
    assert np.array_equal(bits(host(d1.features)), bits(table))
    want = PR.draw_alphas(c.terms, c.weights, c.x, c.y, A.NOISE, table, eps)
    got = host(d1.alpha).reshape(2, 2, c.gp.n_pad)[:, :, :120].reshape(2, -1)
    assert rel(got, want) <= EPS
    assert not np.array_equal(host(E.draw_flows(c.gp, 2, n_features=24, seed=10).alpha), host(d1.alpha))


# ---------------------------------------------------------------- b. trajectories
@pytest.mark.parametrize("name", ["df", "mixed", "vector_st", "sum"])
def test_trajectories_match_reference(name):
    """40 particles, 3 draws, 8 steps of 0.5 with a record every 3 (the last record at step 8)."""
    c = case(name)
    t0, dt, nsteps, se, s = 1.0, 0.5, 8, 3, 1.5
    x0, _ = ref_run(name, 0, 40, t0, dt, nsteps, s)
    t, p = E.advect_draws(c.draws, x0, t0=t0, dt=dt, nsteps=nsteps, save_every=se, vel_scale=s)
    assert host(t).tolist() == [1.0, 2.5, 4.0, 5.0]
    check_paths(name, p, name, 40, t0, dt, nsteps, se, s)


def test_negative_dt():
    c = case("mixed")
    x0, fwd = ref_run("mixed", 0, 40, 0.0, 0.5, 8)
    t, p = E.advect_draws(c.draws, x0, dt=-0.5, nsteps=8, save_every=8)
    assert host(t).tolist() == [0.0, -4.0]
    check_paths("mixed dt<0", p, "mixed", 40, 0.0, -0.5, 8, 8)
    assert np.max(np.abs(host(p)[-1, 0] - fwd.path[-1])) > 0.5   # not the forward run


# ---------------------------------------------------------------- c. the limit cases
def test_zero_features_and_zero_noise_give_the_mean_flow():
    """eps = 0 and a zero feature table: every drawn flow is the posterior mean flow, and
    advect_draws equals engine.advect of the same fit within the position gate (Umax, Fmax from the
    reference run of the mean flow)."""
    c = case("mixed")
    draws = E.draw_flows(c.gp, 2, features=np.zeros((2, 64, 6)), eps=np.zeros((2, 240)))
    x0 = A.seeds(c.x, 70, seed=4)
    run = A.advect(A.oracle_flow(120, "mixed", 0.35), x0, 0.0, 0.5, 8)
    gate = EPS * run.umax * 4.0 * run.fmax
    _, p = E.advect_draws(draws, x0, dt=0.5, nsteps=8, save_every=3)
    _, q, _ = E.advect(c.gp, x0, dt=0.5, nsteps=8, save_every=3)
    err = float(np.max(np.abs(host(p) - host(q)[:, None])))
    print(f"zero table: diff to engine.advect {err:.2e} (gate {gate:.2e})")
    assert err <= gate and rel(host(draws.alpha), host(c.gp.alpha)[None].repeat(2, 0)) <= EPS


def test_no_features_is_the_predicted_mean():
    """nfeat = 0 and a caller's α (the fit's own): gp2d_paths_eval is predict's mean."""
    c = case("mixed")
    gp = c.gp
    xg = A.seeds(c.x, 65, seed=6)
    G = torch.as_tensor(xg, device=DEV)
    vel = torch.empty((1, 130), dtype=torch.float64, device=DEV)
    desc = gp.kernel.desc()
    rc = N.lib().gp2d_paths_eval(E._ptr(gp.alpha), gp.n, E._ptr(gp.x), gp.n_train, gp.n_pad, ctypes.byref(desc), None, 0,
                                 1, E._ptr(G), 65, 2, 0.0, E._ptr(vel), E._stream_handle(DEV))
    assert rc == 0
    mu, _ = E.predict(gp, xg, compute_var=False)
    assert rel(host(vel)[0], host(mu)) <= EPS


# ---------------------------------------------------------------- d. smallest shapes
@pytest.mark.parametrize("ntr,m,S,F", [(1, 1, 1, 1), (1, 64, 3, 63), (63, 65, 1, 64), (63, 1, 3, 65), (65, 64, 1, 255),
                                       (65, 65, 3, 256), (65, 1, 1, 257), (63, 64, 3, 257), (1, 65, 3, 255),
                                       (65, 65, 1, 63), (63, 65, 3, 1)])
def test_smallest_shapes(ntr, m, S, F):
    """n_train 1, 63, 65 (a partial tile; the second slice's first point), m 1, 64, 65 (a partial
    wave; a second workgroup), 1 and 3 draws, and feature counts at the edges of the 64-feature tile
    and of the four-slice trip (1, 63, 64, 65, 255, 256, 257; a div-free kernel has one part).  Four
    steps, records at 0, 3 and 4; the velocity at the start points too."""
    kw = dict(n=ntr, S=S, F=F)
    c = case("df", **kw)
    assert c.draws.features.shape == (S, F, 6) and c.gp.n_pad == {1: 64, 63: 64, 65: 128}[ntr]
    x0, _ = ref_run("df", 0, m, 0.0, 0.5, 4, **kw)
    assert rel(host(c.draws.velocity(x0)), PR.velocity_rows(c.flows, x0)) <= EPS
    _, p = E.advect_draws(c.draws, x0, dt=0.5, nsteps=4, save_every=3)
    check_paths(f"ntr={ntr} m={m} S={S} F={F}", p, "df", m, 0.0, 0.5, 4, 3, **kw)


def test_no_steps_and_no_particles():
    c = case("df")
    x0 = A.seeds(c.x, 70, seed=4)
    t, p = E.advect_draws(c.draws, x0, t0=3.0, dt=0.0, nsteps=0, save_every=5)
    assert host(t).tolist() == [3.0] and np.array_equal(bits(host(p)), bits(np.broadcast_to(x0, (1, 3, 70, 2))))
    t, p = E.advect_draws(c.draws, np.empty((0, 2)), dt=0.5, nsteps=4, save_every=2)
    assert p.shape == (3, 3, 0, 2) and host(t).tolist() == [0.0, 1.0, 2.0]


# ---------------------------------------------------------------- e. bit identity
def test_bits_do_not_depend_on_the_call():
    """A draw advected alone equals the same draw advected as one of three, for any split of x0 and
    any save_every; x0_per_draw = 1 with equal rows equals x0_per_draw = 0; velocity likewise."""
    c = case("mixed")
    x0 = A.seeds(c.x, 70, seed=4)
    kw = dict(dt=0.5, nsteps=8)
    _, p = E.advect_draws(c.draws, x0, save_every=3, **kw)
    p = host(p)
    v = host(c.draws.velocity(x0))
    for s in range(3):
        one = E.FlowDraws(c.gp, c.draws.alpha[s:s + 1].contiguous(), c.draws.features[s:s + 1].contiguous())
        parts = [host(E.advect_draws(one, x0[a:b], save_every=3, **kw)[1]) for a, b in ((0, 1), (1, 30), (30, 70))]
        assert np.array_equal(bits(np.concatenate(parts, 2)[:, 0]), bits(p[:, s]))
        for se in (8, 5, 1):
            end = host(E.advect_draws(one, x0[::-1].copy(), save_every=se, **kw)[1])[-1, 0, ::-1]
            assert np.array_equal(bits(end), bits(p[-1, s]))
        assert np.array_equal(bits(host(one.velocity(x0[20:]))[0].reshape(2, -1)), bits(v[s].reshape(2, -1)[:, 20:]))
    _, q = E.advect_draws(c.draws, np.broadcast_to(x0, (3, 70, 2)).copy(), save_every=3, **kw)
    assert np.array_equal(bits(host(q)), bits(p))
    # a start set of its own per draw is that draw's: draw 1 from shifted starts, the others unchanged
    x3 = np.broadcast_to(x0, (3, 70, 2)).copy()
    x3[1] += 0.25
    _, q = E.advect_draws(c.draws, x3, save_every=3, **kw)
    q = host(q)
    assert np.array_equal(bits(q[:, [0, 2]]), bits(p[:, [0, 2]]))
    assert np.array_equal(bits(q[0, 1]), bits(x3[1])) and np.all(np.abs(q[-1, 1] - p[-1, 1]).max(-1) > 0)


# ---------------------------------------------------------------- f. non-finite starts
@pytest.mark.parametrize("bad", [(np.nan, np.nan), (np.nan, 12.0), (np.inf, 12.0)])
def test_non_finite_start(bad):
    """A non-finite start gives NaN for that (draw, particle) only; path_spread leaves it out and
    counts what is left."""
    c = case("mixed")
    x0 = A.seeds(c.x, 70, seed=4)
    kw = dict(dt=0.5, nsteps=8, save_every=3)
    p = host(E.advect_draws(c.draws, x0, **kw)[1])
    x3 = np.broadcast_to(x0, (3, 70, 2)).copy()
    x3[1, 66] = bad   # the second workgroup's partial wave
    _, q = E.advect_draws(c.draws, x3, **kw)
    mean, cov, cnt = (host(a) for a in E.path_spread(q))
    q = host(q)
    assert np.isnan(q[:, 1, 66]).all()
    keep = np.ones((3, 70), dtype=bool)
    keep[1, 66] = False
    assert np.array_equal(bits(q[:, keep]), bits(p[:, keep]))
    assert cnt.shape == (4, 70) and np.all(cnt[:, 66] == 2) and np.all(np.delete(cnt, 66, 1) == 3)
    assert np.isfinite(mean).all() and np.isfinite(cov).all()
    assert np.allclose(mean[:, 66], p[:, [0, 2], 66].mean(1), rtol=1e-14, atol=0)
    d = p[:, [0, 2], 66] - mean[:, None, 66]
    # 1/(2 − 1); d = p − mean carries a relative rounding error of 2^-52·|p|/|d|
    assert np.allclose(cov[:, 66], np.einsum("rsa,rsb->rab", d, d), rtol=1e-8, atol=1e-300)
    # a shared non-finite start: NaN in every draw, nothing left to average
    x1 = x0.copy()
    x1[5] = bad
    _, q = E.advect_draws(c.draws, x1, **kw)
    mean, cov, cnt = (host(a) for a in E.path_spread(q))
    assert np.isnan(host(q)[:, :, 5]).all() and np.all(cnt[:, 5] == 0) and np.isnan(mean[:, 5]).all()
    assert np.array_equal(bits(np.delete(host(q), 5, 2)), bits(np.delete(p, 5, 2)))


def test_path_spread_is_the_unbiased_sample_covariance():
    rng = np.random.default_rng(0)
    z = rng.normal(size=(3, 7, 5, 2))
    mean, cov, cnt = E.path_spread(torch.as_tensor(z, device=DEV))
    assert np.allclose(host(mean), z.mean(1), rtol=1e-14) and np.all(host(cnt) == 7)
    want = np.stack([[np.cov(z[r, :, j].T, ddof=1) for j in range(5)] for r in range(3)])
    assert np.allclose(host(cov), want, rtol=1e-12)
    one = E.path_spread(torch.as_tensor(z[:, :1]))   # one draw: no covariance; any device
    assert np.isnan(host(one[1])).all() and np.array_equal(host(one[0]), z[:, 0])


# ---------------------------------------------------------------- g. refusals
def test_fits_that_cannot_serve_are_refused():
    c = case("mixed")
    gp = c.gp
    tr = E.fit(gp.kernel, np.array(c.x), np.array(c.y), noise=A.NOISE, device=DEV, trend="constant")
    with pytest.raises(ValueError, match=r"trend"):
        E.draw_flows(tr, 2)
    with pytest.raises(ValueError, match="posterior flow draws need"):
        E.draw_flows(dataclasses.replace(gp, kernel=E.KernelSpec(kind="scalar", l_df=5.0)), 2)
    with pytest.raises(ValueError, match="posterior flow draws need"):
        E.draw_flows(dataclasses.replace(gp, kernel=E.KernelSpec(family="ard", variances=(1.0,),
                                                                 lengthscales=((3.0, 4.0),))), 2)
    with pytest.raises(ValueError, match="factor W"):
        E.draw_flows(dataclasses.replace(gp, W=None, n_mat=gp.n), 2)
    with pytest.raises(ValueError, match="observations y"):
        E.draw_flows(dataclasses.replace(gp, y=None), 2)
    with pytest.raises(ValueError, match="n_draws"):
        E.draw_flows(gp, 0)
    with pytest.raises(ValueError, match="features must have shape"):
        E.draw_flows(gp, 2, features=np.zeros((3, 8, 6)))
    with pytest.raises(ValueError, match="eps must have shape"):
        E.draw_flows(gp, 2, eps=np.zeros((2, 7)))
    with pytest.raises(ValueError, match="dt and nsteps"):
        E.advect_draws(c.draws, A.seeds(c.x, 5))
    with pytest.raises(ValueError, match="x0 must be"):
        E.advect_draws(c.draws, np.zeros((2, 5, 2)), dt=0.5, nsteps=2)


def test_entry_point_refusals_leave_the_output_untouched():
    """nfeat < 0, ndraws = 0, NULL feat with nfeat > 0, the scalar kind and the ARD family, each by
    its message and before any launch: the pre-filled output keeps its bits."""
    c = case("mixed")
    gp, d, L = c.gp, c.draws, N.lib()
    x0 = torch.as_tensor(A.seeds(c.x, 70, seed=4), device=DEV)
    out = torch.full((2, 3, 70, 2), 7.0, dtype=torch.float64, device=DEV)
    vel = torch.full((3, 140), 7.0, dtype=torch.float64, device=DEV)
    ok = dict(k=gp.kernel.desc(), feat=E._ptr(d.features), nfeat=d.features.shape[1], ndraws=3)
    scalar = E.KernelSpec(kind="scalar", l_df=5.0).desc()
    ard = E.KernelSpec(family="ard", variances=(1.0,), lengthscales=((3.0, 4.0),)).desc()
    for change, word in ((dict(nfeat=-1), "nfeat must be >= 0"), (dict(ndraws=0), "ndraws must be >= 1"),
                         (dict(feat=None), "feat is NULL"), (dict(k=scalar), "KIND_SCALAR"), (dict(k=ard), "ARD")):
        a = {**ok, **change}
        fit = (E._ptr(d.alpha), gp.n, E._ptr(gp.x), gp.n_train, gp.n_pad, ctypes.byref(a["k"]), a["feat"], a["nfeat"],
               a["ndraws"])
        rc = L.gp2d_advect_draws(*fit, E._ptr(x0), 70, 0, 0.0, 0.5, 4, 4, 1.0, E._ptr(out), E._stream_handle(DEV))
        assert rc != 0 and "advect_draws" in L.gp2d_last_error().decode() and word in L.gp2d_last_error().decode()
        rc = L.gp2d_paths_eval(*fit, E._ptr(x0), 70, 2, 0.0, E._ptr(vel), E._stream_handle(DEV))
        assert rc != 0 and "paths_eval" in L.gp2d_last_error().decode() and word in L.gp2d_last_error().decode()
    torch.cuda.synchronize()
    assert torch.all(out == 7.0) and torch.all(vel == 7.0)


# ---------------------------------------------------------------- h. the Krig surface
def test_krig_advect_ensemble():
    """One call: the shapes, numpy arrays, and at record 0 a spread of exactly zero around the shared
    start; later records have spread, and the ensemble mean is not the path through the mean flow."""
    xt, yt = A.tracks(120)
    k = Krig("df", l_df=A.L_DF, noise=A.NOISE, device=DEV).fit(xt, yt)
    x0 = A.seeds(xt, 30, seed=4)
    t, paths, mean, cov, cnt = k.advect_ensemble(x0, 8, dt=0.5, nsteps=8, save_every=4, n_features=64, seed=1)
    assert all(isinstance(a, np.ndarray) for a in (t, paths, mean, cov, cnt))
    assert t.tolist() == [0.0, 2.0, 4.0] and paths.shape == (3, 8, 30, 2)
    assert mean.shape == (3, 30, 2) and cov.shape == (3, 30, 2, 2) and cnt.shape == (3, 30) and np.all(cnt == 8)
    assert np.array_equal(bits(mean[0]), bits(x0)) and np.all(cov[0] == 0.0)
    assert np.all(cov[-1][:, 0, 0] > 0) and np.all(cov[-1][:, 1, 1] > 0)
    assert np.allclose(cov[-1][:, 0, 1], cov[-1][:, 1, 0], rtol=1e-12, atol=0)
    d = k.draw_flows(2, n_features=16, seed=1)
    assert isinstance(d, E.FlowDraws) and d.alpha.shape == (2, k.gp.n) and d.features.shape == (2, 16, 6)
