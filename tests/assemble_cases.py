"""Checks of the raw assembly ABI (gp2d_assemble, gp2d_assemble_cols) shared by test_gpu_parity.py
and test_gpu_st.py: what the calls write into a NaN-filled padded buffer, entry by entry."""
import ctypes

import numpy as np
import torch

from gp2d import _native as N
from gp2d import engine as E

DIAG_ADD = 0.0025
# 64-aligned column ranges (c0, ncols) inside one component, by padded point count
COL_RANGES = {128: [(0, 64), (64, 64), (0, 128), (128, 128), (192, 64)], 64: [(0, 64), (64, 64)]}


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr())


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def raw_assemble(ks, xa, xb, symmetric, diag_add=0.0):
    """gp2d_assemble into a NaN-filled bd·na_pad × bd·nb_pad buffer (xb None: xa itself, the
    symmetric modes' requirement); the whole buffer as an array."""
    A = torch.tensor(np.ascontiguousarray(xa), dtype=torch.float64, device="cuda")
    B = A if xb is None else torch.tensor(np.ascontiguousarray(xb), dtype=torch.float64, device="cuda")
    na, nb = A.shape[0], B.shape[0]
    nap, nbp = E.padded_points(na), E.padded_points(nb)
    bd = ks.block_dim
    out = torch.full((bd * nap, bd * nbp), float("nan"), dtype=torch.float64, device="cuda")
    desc = ks.desc()
    N.check(N.lib().gp2d_assemble(_ptr(A), na, nap, _ptr(B), nb, nbp, ctypes.byref(desc), float(diag_add),
                                  int(symmetric), _ptr(out), out.shape[1], _stream()), "gp2d_assemble")
    return out.cpu().numpy()


def padded_mask(n, n_pad, bd):
    """True at the bd·n_pad indices that belong to padded points (component-major)."""
    return np.tile(np.arange(n_pad) >= n, bd)


def check_whole_buffer(ks, xa, xb):
    """symmetric = 0 on (xa, xb) and symmetric = 1 on xa: every entry of the padded buffer is
    written; padded rows and columns are exact zeros, in the symmetric mode with an exact 1.0 on
    their diagonal; DIAG_ADD sits on the valid diagonal and nowhere else.  Returns the valid part
    of the symmetric = 0 buffer (bd·na × bd·nb) for a comparison with an oracle."""
    bd = ks.block_dim
    na, nb = xa.shape[0], xb.shape[0]
    nap, nbp = E.padded_points(na), E.padded_points(nb)
    K = raw_assemble(ks, xa, xb, 0)
    assert K.shape == (bd * nap, bd * nbp) and not np.any(np.isnan(K))
    pr, pc = padded_mask(na, nap, bd), padded_mask(nb, nbp, bd)
    assert np.all(K[pr, :] == 0.0) and np.all(K[:, pc] == 0.0)

    S = raw_assemble(ks, xa, None, 1, DIAG_ADD)
    assert S.shape == (bd * nap, bd * nap) and not np.any(np.isnan(S))
    expect = np.zeros_like(S)
    expect[np.flatnonzero(pr), np.flatnonzero(pr)] = 1.0
    touched = pr[:, None] | pr[None, :]
    assert np.array_equal(S[touched], expect[touched])
    # off the diagonal the symmetric mode is the plain one, bit for bit; on the valid diagonal it
    # adds DIAG_ADD, which the compiler may fuse into the value's last multiply: one rounding of
    # the value less, i.e. within 2 spacings of the sum
    P = raw_assemble(ks, xa, xa, 0)
    off = ~np.eye(S.shape[0], dtype=bool)
    assert np.array_equal(S[off], P[off])
    d = np.flatnonzero(~pr)
    want = P[d, d] + DIAG_ADD
    assert np.all(np.abs(S[d, d] - want) <= 2 * np.spacing(want))
    return K[~pr][:, ~pc]


def check_cols_alone(ks, x):
    """gp2d_assemble_cols into a NaN-filled n × n buffer, for each column range of COL_RANGES: the
    written columns are gp2d_assemble(symmetric = 1)'s bit for bit over all n rows (padded identity
    rows included) and every other entry is still NaN."""
    npts = x.shape[0]
    npad = E.padded_points(npts)
    n = 2 * npad
    full = raw_assemble(ks, x, None, 1, DIAG_ADD)
    X = torch.tensor(np.ascontiguousarray(x), dtype=torch.float64, device="cuda")
    desc = ks.desc()
    for c0, ncols in COL_RANGES[npad]:
        out = torch.full((n, n), float("nan"), dtype=torch.float64, device="cuda")
        N.check(N.lib().gp2d_assemble_cols(_ptr(X), npts, npad, ctypes.byref(desc), DIAG_ADD, _ptr(out), n, c0,
                                           ncols, _stream()), "gp2d_assemble_cols")
        out = out.cpu().numpy()
        assert np.array_equal(out[:, c0:c0 + ncols], full[:, c0:c0 + ncols]), (c0, ncols)
        rest = np.ones(n, dtype=bool)
        rest[c0:c0 + ncols] = False
        assert np.all(np.isnan(out[:, rest])), (c0, ncols)
