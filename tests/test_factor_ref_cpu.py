"""The references and inputs of tests/test_gpu_factor_hard.py, proven on the host before any kernel
is judged by them: the matrices factor in LAPACK, in longdouble and in the float64 emulation of the
project's algorithm; the backward errors are the ones the design table states; the extended-precision
helper's `info` is LAPACK's on planted failures."""
import numpy as np
import pytest
import scipy.linalg.lapack as lapack

import factor_ref as F
from oracle import gp2d_oracle as O

if not F.have_longdouble():  # pragma: no cover
    pytest.skip("np.longdouble is no wider than float64 on this host", allow_module_level=True)

# ρ/(n·u) of the blocked inverse-panel Cholesky as first simulated (float64, nb = 128); another
# LAPACK build or summation order moves it, so it is held within a factor of two
TABLE = {"G1": 0.035, "G2": 0.438, "G3": 1.411, "G4": 3.050, "GR": 0.009, "P": 0.009}
PLANTS = [0, 1, 31, 32, 63, 64, 127, 128, 129, 200, 383]


def lapack_chol(K):
    L, info = lapack.dpotrf(K, lower=1, clean=1)
    return L, int(info)


@pytest.fixture(scope="module")
def factors():
    """(LAPACK's L, the yardstick's L) per matrix, infos asserted zero."""
    out = {}
    for name in F.NAMES:
        K = F.matrix(name)
        Ll, il = lapack_chol(K)
        Lb, ib = F.blocked_chol(K)
        assert (il, ib) == (0, 0), name
        out[name] = (Ll, Lb)
    return out


def test_gram_restates_the_oracle_kernel():
    npts, ell, noise = F.GRAM["G3"]
    x = F.gram_points(npts)
    K = O.vector_kernel(x, x, "df", l_df=ell) + noise * np.eye(2 * npts)
    G = F.matrix("G3")
    assert G.shape == (384, 384) and np.array_equal(G, G.T)
    # the two write the same entry with another association of the same few factors
    assert np.max(np.abs(G - K)) <= 8 * F.U * np.max(np.abs(K))
    assert F.matrix("G4").shape == (640, 640)


def test_benign_and_graded_are_as_stated():
    Pm, GR = F.matrix("P"), F.matrix("GR")
    ev = np.linalg.eigvalsh(Pm)
    assert 0.5 <= ev[0] and ev[-1] <= 4.5
    d = np.sqrt(np.diag(GR) / np.diag(Pm))
    assert 1e-8 <= d.min() and d.max() <= 1.0 and d.max() / d.min() > 1e7
    assert np.allclose(GR, d[:, None] * Pm * d[None, :], rtol=1e-14, atol=0.0)
    assert np.array_equal(F.spd(128, 7), _spd_of_the_suite(128, 7))


def _spd_of_the_suite(n, seed):   # test_gpu_parity._spd, which needs a device to import
    rng = np.random.default_rng(seed)
    A = rng.normal(size=(n, n))
    return A @ A.T / n + np.eye(n) * 0.5


@pytest.mark.parametrize("name", F.NAMES)
def test_every_reference_factors_every_matrix(name, factors):
    K = F.matrix(name)
    n = K.shape[0]
    Ll, Lb = factors[name]
    Lx, ix = F.chol_ld(K)
    assert ix == 0
    rl, rb, rx = F.rho(K, Ll), F.rho(K, Lb), F.rho(K, Lx)
    assert rl <= 0.1 * n * F.U, rl / (n * F.U)            # the largest measured: 0.045
    assert TABLE[name] / 2 <= rb / (n * F.U) <= TABLE[name] * 2, rb / (n * F.U)
    assert rx <= n * 2.0 ** -63                           # the extended factor is an extended factor
    # and LAPACK's factor is the extended one rounded, up to the conditioning of its own columns
    assert np.max(np.abs(Ll - Lx.astype(np.float64))) <= 1e-4 * np.max(np.abs(Ll))


@pytest.mark.parametrize("name", ["G3", "GR"])
def test_inverse_references(name, factors):
    """tri_inv_ld inverts (L·W − I at the extended precision's level); the yardstick's and dtrtri's φ
    on LAPACK's factor are a modest multiple of u: φ is a componentwise relative measure."""
    L = factors[name][0]
    ref = F.InverseRef(L)
    n = L.shape[0]
    resid = np.abs(np.asarray(L, dtype=F.LD) @ ref.W - np.eye(n, dtype=F.LD))
    scale = np.abs(L).astype(F.LD) @ np.abs(ref.W)
    assert not resid[~ref.low].any()
    assert float(np.max(resid[ref.low] / scale[ref.low])) <= n * 2.0 ** -63
    Wt, info = lapack.dtrtri(L, lower=1)
    assert info == 0
    assert ref.phi(Wt) <= n * F.U and ref.phi(F.blocked_inv(L)) <= 16 * n * F.U
    assert ref.phi(ref.W.astype(np.float64)) <= F.U      # rounding the reference itself


def test_trtri_pairs_are_pinned():
    """(left block, right block, right blocks) per level, the left part g blocks wide."""
    assert [F.trtri_pairs(3, g) for g in (1, 2)] == [[(0, 1, 1)], [(0, 2, 1)]]
    assert [F.trtri_pairs(5, g) for g in (1, 2, 4)] == [[(0, 1, 1), (2, 3, 1)], [(0, 2, 2)], [(0, 4, 1)]]
    assert [F.trtri_pairs(9, g) for g in (1, 2, 4, 8)] == [
        [(0, 1, 1), (2, 3, 1), (4, 5, 1), (6, 7, 1)], [(0, 2, 2), (4, 6, 2)], [(0, 4, 4)], [(0, 8, 1)]]
    for nbk in range(1, 20):   # every off-diagonal block is written exactly once
        seen = np.zeros((nbk, nbk), dtype=int)
        g = 1
        while g < nbk:
            for ls, rs, rn in F.trtri_pairs(nbk, g):
                assert rs == ls + g and 1 <= rn <= g and rs + rn <= nbk
                seen[rs:rs + rn, ls:ls + g] += 1
            g *= 2
        assert np.array_equal(seen, np.tril(np.ones((nbk, nbk), dtype=int), -1))


def test_solve_bound_holds_for_a_float64_solve():
    W = F.blocked_inv(F.blocked_chol(F.matrix("G3"))[0])
    y = np.random.default_rng(5).normal(size=384)
    alpha, b = F.solve_ref(W, y)
    got = W.T @ (W @ y)
    assert np.all(np.abs(got - alpha) <= b) and np.all(b > 0)


@pytest.mark.parametrize("j", PLANTS)
def test_planted_pivot_info_is_lapacks(j):
    K = F.plant(F.matrix("P"), j)
    assert lapack_chol(K)[1] == j + 1
    assert F.chol_ld(K)[1] == j + 1
    assert F.blocked_chol(K)[1] == j + 1


def test_two_plants_report_the_first():
    K = F.plant(F.matrix("P"), 140, 300)
    assert lapack_chol(K)[1] == 141 and F.chol_ld(K)[1] == 141 and F.blocked_chol(K)[1] == 141
    assert lapack_chol(F.plant(F.matrix("P"), 300))[1] == 301   # the second is a failure of its own


def test_nan_reference_is_the_helper_not_scipy():
    """The installed LAPACK returns info 0 on a NaN entry (its pivot test lets NaN through), so for
    NaN inputs the reference is chol_ld's `not (d > 0)` — netlib's rule — and not scipy: a NaN on
    the diagonal fails its own pivot, one at (i, j), i > j, of the lower triangle reaches row i
    only and fails pivot i."""
    for (i, j), want in {(200, 200): 201, (70, 3): 71, (300, 10): 301, (129, 128): 130}.items():
        K = np.array(F.matrix("P"))
        K[i, j] = np.nan
        assert F.chol_ld(K)[1] == want
    K = np.array(F.matrix("P"))
    K[200, 200] = np.nan
    assert lapack_chol(K)[1] in (0, 201)   # 0 here; a netlib-conforming build gives 201
