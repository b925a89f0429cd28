"""Cross-validation without refitting on the device (gp2d_cv_points, gp2d_cv_groups, engine.cv_points
/ cv_groups, Krig.cross_validate, krig.crossValidate) against the numpy closed forms of
tests/cv_ref.py, which tests/test_cv_cpu.py pins to brute-force refits.

Tolerance: the project's 1e-10 parity gate in every norm — mean: error / max|y|; var: elementwise
relative (it is bounded below by the noise); cuv: error / √(var_u·var_v); lpd and the host scores:
|Δ| / max(1, |ref|).  Shapes are the smallest at which the indexing can go wrong (one and three
256-row segments, padded points, u and v in different column blocks, a Morton order, groups below,
at and above a 128-wide block, several factor batches).
"""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
if not torch.cuda.is_available():  # pragma: no cover
    pytest.skip("no HIP device", allow_module_level=True)

import cv_ref as R  # noqa: E402
from gp2d import _native as N  # noqa: E402
from gp2d import engine as E  # noqa: E402
from gp2d import krig as K  # noqa: E402
from oracle import gp2d_oracle as O  # noqa: E402

GATE = 1e-10
DEV = torch.device("cuda")
SCORES = ("rmse_u", "rmse_v", "mean_lpd", "msll_chi2")
SPECS = {
    "vector2d": E.KernelSpec(kind="mixed", l_df=R.L_DF, l_cf=R.L_CF, ratio=R.RATIO),
    "ard": E.KernelSpec(family="ard", variances=R.ARD_VARIANCES, lengthscales=R.ARD_LENGTHSCALES),
    "vector_st": E.KernelSpec(family="vector_st", kind="mixed", l_df=R.L_DF, l_cf=R.L_CF, ratio=R.RATIO,
                              var_t=R.VAR_T, l_t=R.L_T),
}


@functools.lru_cache(maxsize=None)
def fit(family, n, variance="f64"):
    x, y = (np.array(a) for a in R.problem(family, n)[:2])   # writable copies of the read-only reference
    return E.fit(SPECS[family], x, y, noise=R.NOISE, device=DEV, variance=variance)


def host(t):
    return t.cpu().numpy()


def errors(got, ref, ymax, bd, n):
    """The issue's norms of a result dict against the reference's; NaNs must coincide."""
    gm, gv = host(got["mean"]), host(got["var"])
    assert np.array_equal(np.isnan(gm), np.isnan(ref["mean"])) and np.array_equal(np.isnan(gv), np.isnan(ref["var"]))
    e = dict(mean=float(np.nanmax(np.abs(gm - ref["mean"])) / ymax),
             var=float(np.nanmax(np.abs(gv - ref["var"]) / ref["var"])),
             resid=float(np.nanmax(np.abs(host(got["resid"]) - ref["resid"])) / ymax),
             lpd=float(np.max(np.abs(host(got["lpd"]) - ref["lpd"]) / np.maximum(1.0, np.abs(ref["lpd"])))))
    if ref.get("cuv") is not None:
        v = ref["var"].reshape(bd, n)
        e["cuv"] = float(np.max(np.abs(host(got["cuv"]) - ref["cuv"]) / np.sqrt(v[0] * v[1])))
    for k in SCORES:
        e[k] = abs(got[k] - ref[k]) / max(1.0, abs(ref[k]))
    return e


def check(got, ref, family, n, what):
    _, y, _, bd = R.problem(family, n)[:4]
    e = errors(got, ref, float(np.max(np.abs(y))), bd, n)
    print(f"{what}: {e}")
    assert all(v < GATE for v in e.values()), (what, e)
    return e


# ---------------------------------------------------------------------------- points
@pytest.mark.parametrize("family,n,variance", [
    ("vector2d", 100, "f64"),     # Np = 128, n = 256: one row segment, 28 padded points
    ("vector2d", 300, "f64"),     # Np = 320, n = 640: three segments, v columns from the middle of segment 1
    ("vector2d", 300, "ozaki"),   # Np = 384, n = 768: Morton order, outputs in the caller's order
    ("ard", 200, "f64"),          # bd = 1, two terms
    ("vector_st", 100, "f64"),    # dim 3: the entry never sees the kernel
])
def test_points_match_closed_forms(family, n, variance):
    gp = fit(family, n, variance)
    bd = gp.kernel.block_dim
    if variance == "ozaki":
        assert gp.perm is not None and not torch.equal(gp.perm, torch.arange(n, device=DEV))
        assert (gp.n_pad, gp.n) == (384, 768)
    got = E.cv_points(gp)
    assert got["mean"].shape == got["var"].shape == (bd * n,) and got["lpd"].shape == (n,)
    assert (got["cuv"] is None) == (bd == 1)
    for k in ("mean", "var", "lpd", "resid"):
        assert bool(torch.isfinite(got[k]).all()), k
    check(got, R.cv_points(family, n), family, n, f"cv_points {family} N={n} {variance}")
    if bd == 1:
        assert got["rmse_v"] == 0.0


def test_points_ozaki_equals_f64():
    a, b = E.cv_points(fit("vector2d", 300, "f64")), E.cv_points(fit("vector2d", 300, "ozaki"))
    ref = {k: (host(v) if isinstance(v, torch.Tensor) else v) for k, v in a.items()}
    check(b, ref, "vector2d", 300, "cv_points ozaki vs f64")


def test_points_latent_and_repeat():
    gp = fit("vector2d", 100)
    a, b, c = E.cv_points(gp), E.cv_points(gp), E.cv_points(gp, latent=True)
    for k in ("mean", "var", "cuv", "lpd", "resid"):
        assert torch.equal(a[k], b[k]), k
    assert all(a[k] == b[k] for k in SCORES)
    assert torch.equal(c["var"], a["var"] - R.NOISE) and torch.equal(c["mean"], a["mean"])


def c_points(gp, W, ldw, with_cuv):
    L = N.lib()
    bd, ntr, npad, n = gp.kernel.block_dim, gp.n_train, gp.n_pad, gp.n
    out = [torch.full((k,), -7.0, dtype=torch.float64, device=DEV) for k in (bd * ntr, bd * ntr, ntr, ntr, 4)]
    wb = int(L.gp2d_cv_points_workspace(n))
    work = torch.empty(wb // 8, dtype=torch.float64, device=DEV)
    N.check(L.gp2d_cv_points(E._ptr(W), n, ldw, E._ptr(gp.alpha), E._ptr(gp.y), ntr, npad, bd, None, E._ptr(out[0]),
                             E._ptr(out[1]), E._ptr(out[2]) if with_cuv else None, E._ptr(out[3]), E._ptr(out[4]),
                             E._ptr(work), wb, E._stream_handle(DEV)), "gp2d_cv_points")
    torch.cuda.synchronize()
    return out


def test_points_c_entry_embedded_w():
    """W inside a wider buffer (ldw = n + 64, NaN in the slack) and cuv = NULL: the same bits."""
    gp = fit("vector2d", 300)
    n = gp.n
    wide = torch.full((n, n + 64), float("nan"), dtype=torch.float64, device=DEV)
    wide[:, :n] = gp.W
    a = c_points(gp, gp.W, gp.W.stride(0), True)
    b = c_points(gp, wide, n + 64, False)
    for i in (0, 1, 3, 4):
        assert torch.equal(a[i], b[i]), i
    assert bool((b[2] == -7.0).all())            # cuv = NULL: untouched
    assert bool(torch.isfinite(a[2]).all())
    ref = E.cv_points(gp)                        # the engine's call (fit order = input order here)
    assert torch.equal(a[0], ref["mean"]) and torch.equal(a[2], ref["cuv"])


# ---------------------------------------------------------------------------- groups
GROUP_SIZES = {7: 1, 1000: 5, 42: 64, 3: 65, 99991: 165}   # non-dense ids; q = 2, 10, 128, 130, 330: q_pad = 384


@functools.lru_cache(maxsize=None)
def group_labels(n=300):
    """Randomly interleaved labels of GROUP_SIZES; point 0 is the singleton, point n − 1 is in the
    group of 5."""
    rng = np.random.default_rng(11)
    lab = rng.permutation(np.concatenate([np.full(c, i) for i, c in GROUP_SIZES.items()])).astype(np.int64)
    for pos, want in ((0, 7), (n - 1, 1000)):
        j = int(np.flatnonzero(lab == want)[0 if pos else -1])
        lab[pos], lab[j] = lab[j], lab[pos]
    assert lab.size == n and lab[0] == 7 and lab[n - 1] == 1000
    assert all(int(np.sum(lab == i)) == c for i, c in GROUP_SIZES.items())
    lab.setflags(write=False)
    return lab


@pytest.mark.parametrize("variance", ["f64", "ozaki"])
def test_groups_match_closed_forms(variance):
    n = 300
    gp = fit("vector2d", n, variance)
    lab = group_labels()
    got = E.cv_groups(gp, lab)
    assert np.array_equal(got["labels"], np.array(sorted(GROUP_SIZES)))
    check(got, R.cv_groups("vector2d", n, lab), "vector2d", n, f"cv_groups {variance}")
    again = E.cv_groups(gp, torch.tensor(lab))   # repeat calls: the same bits
    for k in ("mean", "var", "lpd", "resid"):
        assert torch.equal(got[k], again[k]), k
    # ten points of the largest group in no group: NaN, and out of the scores
    lab2 = lab.copy()
    out = np.flatnonzero(lab == 99991)[:10]
    lab2[out] = -1 - np.arange(10)
    got2 = E.cv_groups(gp, lab2)
    m = host(got2["mean"]).reshape(2, n)
    assert np.all(np.isnan(m[:, out])) and int(np.isnan(m).sum()) == 20
    check(got2, R.cv_groups("vector2d", n, lab2), "vector2d", n, f"cv_groups {variance}, ten points out")


def test_groups_latent():
    gp = fit("vector2d", 300)
    a, b = E.cv_groups(gp, group_labels()), E.cv_groups(gp, group_labels(), latent=True)
    assert torch.equal(b["var"], a["var"] - R.NOISE) and torch.equal(b["lpd"], a["lpd"])


@pytest.mark.parametrize("variance", ["f64", "ozaki"])
def test_singleton_groups_equal_points(variance):
    """300 groups of one point (five factor batches of 64) against cv_points."""
    n = 300
    gp = fit("vector2d", n, variance)
    g, p = E.cv_groups(gp, np.arange(n) * 3 + 1), E.cv_points(gp)
    ref = {k: (host(v) if isinstance(v, torch.Tensor) else v) for k, v in p.items()}
    ref["cuv"] = None
    check(g, ref, "vector2d", n, f"singleton groups vs cv_points {variance}")
    check(g, R.cv_groups("vector2d", n, np.arange(n)), "vector2d", n, f"singleton groups vs closed forms {variance}")


def test_gram_block_is_symmetric_with_identity_padding():
    n = 300
    gp = fit("vector2d", n)
    lab = group_labels()
    _, _, _, info, ids, nheld, work, qpad = E._cv_groups_run(gp, lab)
    assert qpad == 384 and nheld == n and not bool(info.any())
    g = int(np.flatnonzero(ids == 3)[0])                      # the group of 65 points: q = 130
    q = 130
    B = host(work[g * qpad * qpad:(g + 1) * qpad * qpad].view(qpad, qpad))
    assert np.array_equal(B, B.T)
    pad = np.eye(qpad)
    assert np.array_equal(B[q:, :], pad[q:, :]) and np.array_equal(B[:, q:], pad[:, q:])
    P = R.problem("vector2d", n)[4]
    idx = R.components(np.flatnonzero(lab == 3), n, 2)
    ref = P[np.ix_(idx, idx)]
    assert np.max(np.abs(B[:q, :q] - ref)) / np.max(np.abs(ref)) < GATE


def hand_fit(n_train, w):
    """A GPFit with W = w·I, α = 0, y = 0 (no factorisation)."""
    npad = E.padded_points(n_train)
    n = 2 * npad
    W = torch.zeros((n, n), dtype=torch.float64, device=DEV)
    W.diagonal().fill_(float(w))
    z = torch.zeros(n, dtype=torch.float64, device=DEV)
    return E.GPFit(kernel=SPECS["vector2d"], noise=R.NOISE, x=torch.zeros((n_train, 2), dtype=torch.float64, device=DEV),
                   n_train=n_train, n_pad=npad, W=W, alpha=z, device=DEV, y=z.clone())


def test_group_over_the_cap_and_bad_fits_raise():
    gp = hand_fit(576, 2.0)
    lab = np.full(576, -1)
    lab[:513] = 12345                                          # 513 points, bd = 2: 1026 components
    with pytest.raises(ValueError, match="group 12345"):
        E.cv_groups(gp, lab)
    lab[512] = -1                                              # 512 points: exactly the cap, q_pad = 1024
    got = E.cv_groups(gp, lab)                                 # P = 4·I: var = 1/4, mean = y = 0
    v = host(got["var"]).reshape(2, 576)
    assert np.all(v[:, :512] == 0.25) and np.all(np.isnan(v[:, 512:]))
    assert host(got["lpd"])[0] == pytest.approx(0.5 * 1024 * np.log(4.0) - 512 * R.LOG_2PI, rel=1e-13)
    with pytest.raises(ValueError, match="integers"):
        E.cv_groups(gp, np.zeros(575, dtype=np.int64))
    with pytest.raises(np.linalg.LinAlgError, match="group 5"):
        E.cv_groups(hand_fit(64, 0.0), np.full(64, 5))         # P_GG = 0: not positive definite
    planes_only = hand_fit(64, 1.0)
    planes_only.W = None
    with pytest.raises(ValueError, match="no factor W"):
        E.cv_points(planes_only)
    no_obs = hand_fit(64, 1.0)
    no_obs.y = None
    with pytest.raises(ValueError, match="no observations"):
        E.cv_groups(no_obs, np.zeros(64, dtype=np.int64))


# ---------------------------------------------------------------------------- the krig surface
def test_krig_cross_validate_and_module_function(tmp_path):
    n = 100
    x, y = (np.array(a) for a in R.problem("vector2d", n)[:2])
    k = K.Krig("mixed", l_df=R.L_DF, l_cf=R.L_CF, ratio=R.RATIO, noise=R.NOISE, device=DEV).fit(x, y)
    res = k.cross_validate()
    assert res["mean"].shape == res["var"].shape == res["resid"].shape == (2 * n, 1)
    assert res["cuv"].shape == (n, 1) and res["lpd"].shape == (n,)
    ref = R.cv_points("vector2d", n)
    assert np.max(np.abs(res["mean"][:, 0] - ref["mean"])) / np.max(np.abs(y)) < GATE
    assert abs(res["mean_lpd"] - ref["mean_lpd"]) / max(1.0, abs(ref["mean_lpd"])) < GATE
    lab = np.arange(n) // 9
    resg = k.cross_validate(groups=lab)
    refg = R.cv_groups("vector2d", n, lab)
    assert np.array_equal(resg["labels"], refg["labels"]) and resg["lpd"].shape == refg["lpd"].shape
    assert np.max(np.abs(resg["lpd"] - refg["lpd"]) / np.maximum(1.0, np.abs(refg["lpd"]))) < GATE

    # a saved window of drifter tracks, scored per fix and per drifter without a refit
    tracks = K.Tracks.synthetic(n_time=24, n_drifters=8, seed=5)
    out = str(tmp_path / "win")
    hyper = dict(l_df=R.L_DF, l_cf=R.L_CF, ratio=R.RATIO, noise=R.NOISE, temporal=False)
    K.kriging(0, 24, sample_step=3, skip=1, kernelType=4, output=out, tracks=tracks, hyper=hyper, device=DEV)
    f = np.load(out + ".npz")
    X, obs, drifter = f["Xo"][:, 1:3], f["obs"][:, 0], f["drifter"].reshape(-1)
    nw = X.shape[0]
    assert drifter.shape == (nw,) and set(drifter.tolist()) == set(range(8))
    Ky = O.vector_kernel(X, X, kind="mixed", l_df=R.L_DF, l_cf=R.L_CF, ratio=R.RATIO) + R.NOISE * np.eye(2 * nw)
    Li = np.linalg.inv(np.linalg.cholesky(Ky))
    P = Li.T @ Li
    alpha = P @ obs
    by_d = K.crossValidate(out, by="drifter", device=DEV)["_combined"]
    assert np.array_equal(by_d["labels"], np.arange(8))
    for g in range(8):
        idx = R.components(np.flatnonzero(drifter == g), nw, 2)
        m, c, lpd = R.closed_group(P, alpha, obs, idx)
        assert np.max(np.abs(by_d["mean"][idx, 0] - m)) / np.max(np.abs(obs)) < GATE
        assert np.max(np.abs(by_d["var"][idx, 0] - np.diag(c)) / np.diag(c)) < GATE
        assert abs(by_d["lpd"][g] - lpd) / max(1.0, abs(lpd)) < GATE
    by_p = K.crossValidate(out, by="point", device=DEV)["_combined"]
    assert by_p["lpd"].shape == (nw,) and np.isfinite(by_p["mean_lpd"])
    saved = np.load(out + "_cv.npz")
    assert str(saved["by"]) == "point" and float(saved["combined_mean_lpd"]) == by_p["mean_lpd"]
    with pytest.raises(ValueError, match="by must be"):
        K.crossValidate(out, by="window")
