"""Host references for the FP64 factor (numpy and scipy only): the test matrices at real conditioning,
an extended-precision Cholesky and triangular inverse, a float64 emulation of the project's own
blocked algorithm (the yardstick) and the error measures of tests/test_gpu_factor_hard.py.

test_factor_ref_cpu.py proves all of this against LAPACK and the oracle before a kernel is judged
by it.  Nothing here is the code under test.

Matrices (n, condition number): G1 (384, 2e3), G2 (384, 2e7), G3 (384, 6e9), G4 (640, 5e10) are
div-free Gram matrices [[uu, uv], [uv, vv]] + noise·I on uniform points; P (384, 9) is the benign
A·Aᵀ/n + 0.5·I of the older tests; GR (384, 1e16) is P graded by D = 10^(−8·U), D·P·D.
"""
import functools

import numpy as np
import scipy.linalg.lapack as lapack

NB = 128
U = 2.0 ** -53
LD = np.longdouble

GRAM = {"G1": (192, 3.0, 1e-2 / 9), "G2": (192, 3.0, 1e-6 / 9), "G3": (192, 6.0, 1e-8 / 36),
        "G4": (320, 4.0, 1e-9 / 16)}
NAMES = ("G1", "G2", "G3", "G4", "GR", "P")


def have_longdouble():
    """The references need an extended type (x87's 80 bits or wider)."""
    return bool(np.finfo(LD).eps <= 2.0 ** -63)


def require_longdouble():
    if not have_longdouble():
        import pytest
        pytest.skip("np.longdouble is no wider than float64 on this host")
    assert np.finfo(LD).eps <= 2.0 ** -63


def gram_points(npts):
    return np.random.default_rng(1).uniform(0, 20, (npts, 2))


def gram(npts, ell, noise):
    x = gram_points(npts)
    dx = x[:, 0][:, None] - x[:, 0][None, :]
    dy = x[:, 1][:, None] - x[:, 1][None, :]
    e = np.exp(-(dx * dx + dy * dy) / (2 * ell ** 2))
    uu = (1 / ell ** 2 - dy * dy / ell ** 4) * e
    vv = (1 / ell ** 2 - dx * dx / ell ** 4) * e
    uv = dx * dy / ell ** 4 * e
    return np.block([[uu, uv], [uv, vv]]) + noise * np.eye(2 * npts)


@functools.lru_cache(maxsize=None)
def _benign_and_graded():
    rng = np.random.default_rng(3)
    A = rng.normal(size=(384, 384))
    Pm = A @ A.T / 384 + 0.5 * np.eye(384)
    D = 10.0 ** (-8 * rng.uniform(size=384))
    return Pm, D[:, None] * Pm * D[None, :]


@functools.lru_cache(maxsize=None)
def _matrix(name):
    if name in GRAM:
        K = gram(*GRAM[name])
    else:
        K = _benign_and_graded()[0 if name == "P" else 1]
    K = np.ascontiguousarray(K)
    K.setflags(write=False)
    return K


def matrix(name):
    """The named test matrix, float64, full symmetric storage (read-only: copy before planting)."""
    return _matrix(name)


def spd(n, seed):
    """The suite's benign matrix (test_gpu_parity._spd), restated so that this module needs no torch."""
    A = np.random.default_rng(seed).normal(size=(n, n))
    return A @ A.T / n + np.eye(n) * 0.5


# ------------------------------------------------------------------ extended-precision reference
def chol_ld(K):
    """Column Cholesky of K's lower triangle in np.longdouble.  Returns (L, info): info is the
    1-based order of the first pivot d with `not (d > 0)` (netlib's rule: a NaN pivot fails), 0 if
    none; on failure the columns before it are final and the rest of L is zero."""
    require_longdouble()
    K = np.asarray(K, dtype=LD)
    n = K.shape[0]
    L = np.zeros((n, n), dtype=LD)
    for j in range(n):
        row = L[j, :j]
        d = K[j, j] - row @ row
        if not (d > 0):
            return L, j + 1
        r = np.sqrt(d)
        L[j, j] = r
        if j + 1 < n:
            L[j + 1:, j] = (K[j + 1:, j] - L[j + 1:, :j] @ row) / r
    return L, 0


def tri_inv_ld(L):
    """W = L⁻¹ of a lower-triangular L by forward substitution in np.longdouble (row i of L·W = I)."""
    require_longdouble()
    L = np.tril(np.asarray(L, dtype=LD))
    n = L.shape[0]
    W = np.zeros((n, n), dtype=LD)
    for i in range(n):
        r = -(L[i, :i] @ W[:i, :])
        r[i] += 1
        W[i, :] = r / L[i, i]
    return W


# ------------------------------------------------------------------------------- the yardstick
def trtri_pairs(nbk, g):
    """The pairs (left block, right block, right blocks) of level g of the recursive-doubling
    inverse over nbk blocks, the left part g blocks wide: the rule of trtri_level_pairs
    (csrc/factor_host.hpp) — the full pairs, then one ragged pair when more than g blocks trail."""
    full = nbk // (2 * g)
    rem = nbk - full * 2 * g
    out = [(s * 2 * g, s * 2 * g + g, g) for s in range(full)]
    if rem > g:
        out.append((full * 2 * g, full * 2 * g + g, rem - g))
    return out


def blocked_chol(K, nb=NB):
    """float64 emulation of the project's algorithm: per 128-block column, factor the diagonal block
    (LAPACK), invert it, L_ik = A_ik·W_kkᵀ below it, then the SYRK update of the trailing matrix.
    Returns (L, info) with LAPACK's info as a global order."""
    A = np.array(K, dtype=np.float64)
    n = A.shape[0]
    assert n % nb == 0
    for k in range(0, n, nb):
        e = k + nb
        Lkk, info = lapack.dpotrf(A[k:e, k:e], lower=1, clean=1)
        if info != 0:
            return np.tril(A), k + int(info)
        Wkk, ti = lapack.dtrtri(Lkk, lower=1)
        assert ti == 0
        A[k:e, k:e] = Lkk
        if e < n:
            A[e:, k:e] = A[e:, k:e] @ Wkk.T
            A[e:, e:] -= A[e:, k:e] @ A[e:, k:e].T
    return np.tril(A), 0


def blocked_inv(L, nb=NB):
    """float64 emulation of the recursive-doubling inverse: W_kk = L_kk⁻¹ (LAPACK), then per level g
    and pair: T = L[R, left]·W[left, left], W[R, left] = −W[R, R]·T."""
    L = np.asarray(L, dtype=np.float64)
    n = L.shape[0]
    assert n % nb == 0
    nbk = n // nb
    W = np.zeros_like(L)
    for k in range(0, n, nb):
        W[k:k + nb, k:k + nb], ti = lapack.dtrtri(np.tril(L[k:k + nb, k:k + nb]), lower=1)
        assert ti == 0
    g = 1
    while g < nbk:
        for ls, rs, rn in trtri_pairs(nbk, g):
            left = slice(ls * nb, (ls + g) * nb)
            R = slice(rs * nb, (rs + rn) * nb)
            T = L[R, left] @ W[left, left]
            W[R, left] = -(W[R, R] @ T)
        g *= 2
    return W


# ----------------------------------------------------------------------------------- measures
def rho(K, L):
    """max |K − L·Lᵀ|ᵢⱼ / √(kᵢᵢ·kⱼⱼ), in longdouble."""
    require_longdouble()
    Kl = np.asarray(K, dtype=LD)
    Ll = np.tril(np.asarray(L, dtype=LD))
    s = np.sqrt(np.diag(Kl))
    return float(np.max(np.abs(Kl - Ll @ Ll.T) / (s[:, None] * s[None, :])))


class InverseRef:
    """W_ld = the longdouble inverse of the float64 L given, and φ's denominator |W_ld|·|L|·|W_ld|:
    computed once per L, shared by every inverse that is judged on that L."""

    def __init__(self, L):
        require_longdouble()
        self.L = np.tril(np.asarray(L, dtype=np.float64))
        self.W = tri_inv_ld(self.L)
        aW = np.abs(self.W)
        self.den = aW @ np.abs(self.L).astype(LD) @ aW
        self.low = np.tril(np.ones(self.L.shape, dtype=bool))

    def phi(self, W):
        """max over i ≥ j of |W − W_ld|ᵢⱼ / (|W_ld|·|L|·|W_ld|)ᵢⱼ."""
        err = np.abs(np.asarray(W, dtype=LD) - self.W)
        return float(np.max(err[self.low] / self.den[self.low]))


def solve_ref(W, y):
    """(α = Wᵀ(W·y) in longdouble, the per-component bound b = 2(n+1)u·|Wᵀ|·(|W|·|y|)) for the
    float64 W given: two dot products of length ≤ n each, in any order of summation."""
    require_longdouble()
    Wl = np.tril(np.asarray(W, dtype=LD))
    yl = np.asarray(y, dtype=LD)
    n = yl.shape[0]
    alpha = Wl.T @ (Wl @ yl)
    b = 2 * (n + 1) * LD(U) * (np.abs(Wl).T @ (np.abs(Wl) @ np.abs(yl)))
    return alpha, b


# --------------------------------------------------------------------------- planted failures
def plant(K, *js):
    """A copy of the SPD K whose pivot j (0-based; each of js, which ascend) is −0.25: K[j, j] =
    L[j, :j]·L[j, :j] − 0.25 with L the factor of the unmodified K, so no rounding decides the
    outcome.  The columns before the first plant are K's own, so its pivot is exactly that; a later
    plant only has to stay the later one."""
    K = np.array(K, dtype=np.float64)
    L = np.linalg.cholesky(K)
    for j in js:
        K[j, j] = L[j, :j] @ L[j, :j] - 0.25
    return K
