"""Cross-validation without refitting, host side: the numpy reference's closed forms against brute-
force refits, and the C ABI's exports, workspace queries and argument checks (no HIP device).

Gate of the first test: 1e-10 in the norms of tests/test_gpu_cv.py.  The two numpy routes disagree
by ≤ 5.1e-13 (mean, covariance) and 2.6e-12 (lpd) at these settings, so the gate is the reference's
own behaviour with two orders of margin.
"""
import ctypes

import numpy as np
import pytest

import cv_ref as R

GATE = 1e-10


def random_groups(n, count, seed):
    """`count` disjoint random groups of 1..12 points."""
    rng = np.random.default_rng(seed)
    perm = rng.permutation(n)
    sizes = rng.integers(1, 13, count)
    cuts = np.concatenate([[0], np.cumsum(sizes)])
    return [np.sort(perm[cuts[g]:cuts[g + 1]]) for g in range(count)]


@pytest.mark.parametrize("n", [100, 300])
def test_closed_forms_equal_bruteforce_refits(n):
    _, y, K, bd, P, alpha = R.problem("vector2d", n)
    cases = [np.array([i]) for i in range(0, n, 7)] + random_groups(n, 7, seed=n)
    ymax = np.max(np.abs(y))
    worst = dict(mean=0.0, cov=0.0, lpd=0.0)
    for G in cases:
        idx = R.components(G, n, bd)
        m0, c0, l0 = R.refit_without(K, y, idx)
        m1, c1, l1 = R.closed_group(P, alpha, y, idx)
        worst["mean"] = max(worst["mean"], float(np.max(np.abs(m1 - m0)) / ymax))
        worst["cov"] = max(worst["cov"], float(np.max(np.abs(c1 - c0)) / np.max(np.abs(c0))))
        worst["lpd"] = max(worst["lpd"], abs(l1 - l0) / max(1.0, abs(l0)))
    print(f"N = {n}: closed form vs refit {worst}")
    assert worst["mean"] < GATE and worst["cov"] < GATE and worst["lpd"] < GATE, worst


def test_point_results_are_singleton_groups():
    """The reference's own consistency: cv_points equals cv_groups with one point per group."""
    n = 100
    a = R.cv_points("vector2d", n)
    b = R.cv_groups("vector2d", n, np.arange(n))
    for k in ("mean", "var", "lpd"):
        assert np.array_equal(a[k], b[k]), k
    for k in ("rmse_u", "rmse_v", "mean_lpd", "msll_chi2"):
        assert a[k] == pytest.approx(b[k], rel=1e-14), k


def test_cv_symbols_are_exported():
    from gp2d import _native as N
    L = N.lib()
    for s in ("gp2d_cv_points_workspace", "gp2d_cv_points", "gp2d_cv_groups_workspace", "gp2d_cv_groups"):
        assert s in N.EXPORTS and hasattr(L, s), s
    assert N.CV_MAX_Q == 1024
    from gp2d import engine as E
    from gp2d.krig import Krig
    import krig
    assert callable(E.cv_points) and callable(E.cv_groups) and callable(Krig.cross_validate)
    assert callable(krig.crossValidate)


def test_cv_workspace_queries():
    from gp2d import _native as N
    L = N.lib()
    assert L.gp2d_cv_points_workspace(0) == 0 and L.gp2d_cv_points_workspace(-128) == 0
    assert L.gp2d_cv_points_workspace(100) == 0                    # not a multiple of the point tile
    assert L.gp2d_cv_points_workspace(640) == 8 * 3 * 3 * 640       # three 256-row segments
    assert L.gp2d_cv_groups_workspace(0, 128, 1) == 0
    assert L.gp2d_cv_groups_workspace(640, 100, 1) == 0            # q_pad not a multiple of 128
    assert L.gp2d_cv_groups_workspace(640, 1152, 1) == 0           # q_pad over the cap
    assert L.gp2d_cv_groups_workspace(640, 128, 0) == 0
    one = L.gp2d_cv_groups_workspace(640, 384, 1)
    assert one >= 8 * (2 * 384 * 384 + 384 * 640)                  # Gram + factor blocks + the panel
    assert L.gp2d_cv_groups_workspace(640, 384, 5) > one


def test_cv_argument_errors_are_reported():
    from gp2d import _native as N
    L = N.lib()
    one = ctypes.c_void_p(1)   # never dereferenced: the argument checks fail first
    big = 1 << 40

    def points(n=256, ldw=256, ntr=100, npad=128, bd=2, cuv=None, wb=big):
        return L.gp2d_cv_points(one, n, ldw, one, one, ntr, npad, bd, None, one, one, cuv, one, one, one, wb, None)

    def err():
        return L.gp2d_last_error()

    assert points(bd=3) < 0 and b"bd must be 1 or 2" in err()
    assert points(bd=0) < 0 and b"bd must be 1 or 2" in err()
    assert points(n=384) < 0 and b"bd" in err() and b"npad" in err()          # n ≠ bd·npad
    assert points(ldw=128) < 0 and b"ldw" in err()
    assert points(ntr=0) < 0 and b"ntr" in err()
    assert points(ntr=129) < 0 and b"ntr" in err()
    assert points(wb=L.gp2d_cv_points_workspace(256) - 1) < 0 and b"workspace" in err()
    assert points(n=128, ldw=128, bd=1, cuv=one) < 0 and b"cuv" in err()      # no cross term for one component

    gs = (ctypes.c_int64 * 3)(0, 5, 12)

    def groups(n=256, ldw=256, ntr=100, npad=128, bd=2, gstart=gs, ng=2, wb=big):
        return L.gp2d_cv_groups(one, n, ldw, one, one, ntr, npad, bd, gstart, one, ng, None, one, one, one, one,
                                one, wb, None)

    assert groups(bd=4) < 0 and b"bd must be 1 or 2" in err()
    assert groups(n=512) < 0 and b"npad" in err()
    assert groups(ng=0) < 0 and b"no groups" in err()
    assert groups(wb=L.gp2d_cv_groups_workspace(256, 128, 1) - 1) < 0 and b"workspace" in err()
    over = (ctypes.c_int64 * 3)(0, 5, 5 + 513)                                 # 513 points, bd = 2: q = 1026
    rc = groups(n=2048, ldw=2048, ntr=1000, npad=1024, gstart=over)
    assert rc < 0 and b"group 1" in err() and b"1026" in err() and b"GP2D_CV_MAX_Q" in err()
    down = (ctypes.c_int64 * 3)(0, 5, 3)
    assert groups(gstart=down) < 0 and b"gstart" in err()
