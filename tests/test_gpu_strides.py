"""The leading-dimension contract of include/gp2d.h on the device: every entry that takes a leading
dimension runs once on contiguous operands (ld = row length, a fresh 256-byte aligned allocation,
what the rest of the suite passes) and once on the same operands embedded in sentinel-filled
buffers at the weakest alignment and smallest slack its rule allows (tests/stride_cases.py).

Every comparison is exact: each output of the embedded run equals the contiguous run's bit for bit
(info words, moduli counts and residue planes included), and no word of an embedded buffer outside
the operand has changed.  The contiguous results are pinned to the oracle and to LAPACK by the
other GPU tests; these extend that pinning to the strided form without a tolerance.  gp2d_gemm is
checked against exact integer arithmetic instead.  Inputs are embedded too: a read of a row's
slack or of a guard row brings a NaN into the output.

Shapes are the smallest at which each structure appears: n = 384 (three 128-blocks, a ragged
inverse recursion), three problems of n = 256 for the batched factor, the predict cases of
tests/predict_cases.py (three chunks with a ragged tail), n = 512 for the int8 preparation (the
three-product layout), 130 points padded to 192 for the assembly, n = 1024 (two super-blocks) for
the distributed factor."""
import ctypes
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
if not torch.cuda.is_available():  # pragma: no cover
    pytest.skip("no HIP device", allow_module_level=True)

import predict_cases as PC  # noqa: E402
import stride_cases as SC  # noqa: E402
from gp2d import _native as N  # noqa: E402
from gp2d import engine as E  # noqa: E402
from test_gpu_cv import fit as cv_fit, group_labels  # noqa: E402
from test_gpu_parity import _spd  # noqa: E402

L = N.lib()
DEV = torch.device("cuda")
NB = 128


def P(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def S():
    return ctypes.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)


def zeros(*shape, dtype=torch.float64):
    return torch.zeros(shape, dtype=dtype, device=DEV)


def workspace(nbytes):
    """A zeroed workspace of at least nbytes: both runs start from the same bytes."""
    return zeros(nbytes // 8 + 2)


def run_both(mat, even, call):
    """call(ptr, ld) -> outputs, on a contiguous copy of `mat` and on an embedded one: the outputs
    and the matrices afterwards (in-place entries) are the same bits, the slack is intact.
    Returns (the contiguous matrix after the call, its outputs)."""
    c = mat.clone().contiguous()
    assert c.data_ptr() % 256 == 0 and c.stride(0) == c.shape[1]
    out_c = call(P(c), c.stride(0))
    e = SC.embed(mat, even)
    out_e = call(e.ptr, e.ld)
    torch.cuda.synchronize()
    e.assert_slack_intact()
    assert SC.same_bits(e.view, c), "the matrix after the call differs"
    assert len(out_c) == len(out_e)
    for i, (a, b) in enumerate(zip(out_c, out_e)):
        assert SC.same_bits(a, b), f"output {i} differs"
        if a.dtype == torch.float64:
            assert bool(torch.isfinite(a).all()), f"output {i} of the contiguous run is not finite"
    return c, out_c


# ------------------------------------------------------------------------------------ factor
NF = 384


@functools.lru_cache(maxsize=None)
def spd():
    return torch.tensor(_spd(NF, NF), device=DEV)


def potrf(ptr, ld, n=NF):
    dinv, info = zeros(n // NB, NB, NB), torch.full((1,), 7, dtype=torch.int32, device=DEV)
    N.check(L.gp2d_potrf(ptr, n, ld, P(dinv), P(info), None, 0, S()), "gp2d_potrf")
    return dinv, info


@functools.lru_cache(maxsize=None)
def factored():
    """(L, dinv) of spd() from the contiguous gp2d_potrf."""
    A = spd().clone()
    dinv, info = potrf(P(A), NF)
    assert int(info.item()) == 0
    return A, dinv


@functools.lru_cache(maxsize=None)
def inverse():
    """W = L⁻¹ of spd() from the contiguous gp2d_potrf_inv."""
    A = spd().clone()
    potrf_inv(P(A), NF)
    torch.cuda.synchronize()
    return A


def potrf_inv(ptr, ld):
    wb = int(L.gp2d_potrf_inv_workspace(NF))
    dinv, info, work = zeros(NF // NB, NB, NB), torch.full((1,), 7, dtype=torch.int32, device=DEV), workspace(wb)
    N.check(L.gp2d_potrf_inv(ptr, NF, ld, P(dinv), P(info), P(work), wb, S()), "gp2d_potrf_inv")
    return dinv, info


def test_potrf():
    A, (dinv, info) = run_both(spd(), True, potrf)
    assert int(info.item()) == 0 and not bool(torch.triu(A, 1).any())


@pytest.mark.parametrize("with_dinv", [True, False])
def test_trtri(with_dinv):
    Lf, dinv = factored()
    wb = int(L.gp2d_trtri_workspace(NF))

    def call(ptr, ld):
        N.check(L.gp2d_trtri(ptr, NF, ld, P(dinv) if with_dinv else None, P(workspace(wb)), wb, S()), "gp2d_trtri")
        return ()
    W, _ = run_both(Lf, True, call)
    assert not SC.same_bits(W, Lf)


def test_potrf_inv():
    W, (dinv, info) = run_both(spd(), True, potrf_inv)
    assert int(info.item()) == 0 and SC.same_bits(W, inverse())


def test_potrs_inv():
    y = torch.tensor(np.random.default_rng(1).normal(size=NF), device=DEV)
    wb = int(L.gp2d_potrs_workspace(NF))

    def call(ptr, ld):
        alpha = zeros(NF)
        N.check(L.gp2d_potrs_inv(ptr, NF, ld, P(y), P(alpha), P(workspace(wb)), wb, S()), "gp2d_potrs_inv")
        return (alpha,)
    run_both(inverse(), False, call)


def test_zero_upper():
    full = torch.tensor(np.random.default_rng(2).normal(size=(NF, NF)), device=DEV)

    def call(ptr, ld):
        N.check(L.gp2d_zero_upper(ptr, NF, ld, S()), "gp2d_zero_upper")
        return ()
    Z, _ = run_both(full, True, call)
    blocks = torch.kron(torch.eye(NF // NB, device=DEV), torch.ones(NB, NB, device=DEV)).bool()
    keep = blocks | torch.tril(torch.ones(NF, NF, device=DEV)).bool()   # diagonal blocks are left whole
    assert torch.equal(Z, torch.where(keep, full, torch.zeros_like(full)))


def test_pack_lower_and_unpack():
    W = inverse()
    npk = int(L.gp2d_pack_lower_doubles(NF))

    def pack(ptr, ld):
        packed = zeros(npk)
        N.check(L.gp2d_pack_lower(ptr, NF, ld, P(packed), 0, S()), "gp2d_pack_lower")
        return (packed,)
    _, (packed,) = run_both(W, True, pack)
    # unpack into an embedded sentinel block: row block rb receives columns [0, 128·(rb + 1)) only
    e = SC.embed(W, True, fill=False)
    N.check(L.gp2d_pack_lower(e.ptr, NF, e.ld, P(packed), 1, S()), "gp2d_pack_lower(unpack)")
    torch.cuda.synchronize()
    e.assert_slack_intact()
    r, c = torch.meshgrid(torch.arange(NF, device=DEV), torch.arange(NF, device=DEV), indexing="ij")
    kept = c < (r // NB + 1) * NB
    assert torch.equal(e.view[kept], W[kept])
    assert bool(SC.is_sentinel(e.view)[~kept].all())


def test_transpose():
    A = torch.tensor(np.random.default_rng(3).normal(size=(NF, NF)), device=DEV)

    def call(ptr, ld):
        At = zeros(NF, NF)
        N.check(L.gp2d_transpose(ptr, NF, ld, P(At), S()), "gp2d_transpose")
        return (At,)
    _, (At,) = run_both(A, False, call)
    assert torch.equal(At, A.T)


def test_potrf_trtri_batched():
    """nprob = 3 problems of n = 256 with lda = n + 4 and a problem stride above n·lda, inside one
    sentinel buffer, against the same problems contiguous (lda = n, sA = n²)."""
    n, B = 256, 3
    mats = torch.stack([torch.tensor(_spd(n, 10 + b) + b * np.eye(n), device=DEV) for b in range(B)])
    wb = int(L.gp2d_trtri_batched_workspace(n, B))

    def run(ptr, lda, sA):
        dinv, info = zeros(B, n // NB, NB, NB), torch.full((B,), 7, dtype=torch.int32, device=DEV)
        N.check(L.gp2d_potrf_batched(ptr, n, lda, sA, B, P(dinv), P(info), S()), "gp2d_potrf_batched")
        torch.cuda.synchronize()
        return dinv, info

    def invert(ptr, lda, sA, dinv):
        N.check(L.gp2d_trtri_batched(ptr, n, lda, sA, B, P(dinv), P(workspace(wb)), wb, S()), "gp2d_trtri_batched")
        torch.cuda.synchronize()

    C = mats.clone()
    lda = n + 4
    sA = n * lda + 4 * 37                      # even, above n·lda, no multiple of 128 bytes
    base = n * lda + 2                         # guard of one whole problem; 16-byte, not 32-byte aligned
    buf = SC.sentinel_buffer((base + B * sA + n * lda,), DEV)
    idx = (base + torch.arange(B, device=DEV)[:, None, None] * sA + torch.arange(n, device=DEV)[None, :, None] * lda
           + torch.arange(n, device=DEV)[None, None, :])
    buf[idx] = mats
    mask = torch.ones(buf.shape, dtype=torch.bool, device=DEV)
    mask[idx.reshape(-1)] = False
    ptr = ctypes.c_void_p(buf.data_ptr() + 8 * base)
    assert ptr.value % 32 == 16

    dc, ic = run(P(C), n, n * n)
    de, ie = run(ptr, lda, sA)
    assert ic.tolist() == [0] * B and torch.equal(ic, ie) and SC.same_bits(dc, de)
    assert SC.same_bits(buf[idx], C) and bool(SC.is_sentinel(buf)[mask].all())
    Lc = C.clone()
    invert(P(C), n, n * n, dc)
    invert(ptr, lda, sA, de)
    assert SC.same_bits(buf[idx], C) and bool(SC.is_sentinel(buf)[mask].all())
    assert not SC.same_bits(C, Lc) and bool(torch.isfinite(C).all())


# ------------------------------------------------------------------------------ FP64 predicts
def fit_args(gp, wptr, ldw, G, m, desc):
    return (wptr, gp.n, ldw, P(gp.alpha), P(gp.x), gp.n_train, gp.n_pad, P(G), m, ctypes.byref(desc))


def targets(m):
    return torch.as_tensor(PC.targets()[:m].copy(), device=DEV)


@pytest.mark.parametrize("case", ["df", "ard"])
def test_predict(case):
    gp, G, desc = PC.fit(case), targets(PC.M), PC.fit(case).kernel.desc()
    bd = gp.kernel.block_dim
    wb = int(L.gp2d_predict_workspace(gp.n, PC.CHUNK, bd))

    def call(ptr, ld):
        mean, var = zeros(bd * PC.M), zeros(bd * PC.M)
        N.check(L.gp2d_predict(*fit_args(gp, ptr, ld, G, PC.M, desc), N.VAR_LATENT, float(gp.noise), 1, P(mean),
                               P(var), PC.CHUNK, P(workspace(wb)), wb, S()), "gp2d_predict")
        return mean, var
    run_both(gp.W, True, call)


def test_predict_field():
    gp, G = PC.fit("vorticity"), targets(PC.M)
    desc = gp.kernel.desc()
    wb = int(L.gp2d_predict_field_workspace(gp.n, PC.CHUNK))

    def call(ptr, ld):
        mean, var = zeros(PC.M), zeros(PC.M)
        N.check(L.gp2d_predict_field(*fit_args(gp, ptr, ld, G, PC.M, desc), N.FIELD_VORTICITY, 1, P(mean), P(var),
                                     PC.CHUNK, P(workspace(wb)), wb, S()), "gp2d_predict_field")
        return mean, var
    run_both(gp.W, True, call)


def test_predict_grad_with_covariance():
    gp, G = PC.fit("vorticity"), targets(PC.M)
    desc = gp.kernel.desc()
    wb = int(L.gp2d_predict_grad_workspace(gp.n, PC.CHUNK))

    def call(ptr, ld):
        mean, cov = zeros(PC.M, 4), zeros(PC.M, 16)
        N.check(L.gp2d_predict_grad(*fit_args(gp, ptr, ld, G, PC.M, desc), 1, P(mean), P(cov), PC.CHUNK,
                                    P(workspace(wb)), wb, S()), "gp2d_predict_grad")
        return mean, cov
    run_both(gp.W, True, call)


def test_predict_cov_embedded_w_and_output():
    gp, m = PC.fit("cov"), PC.COV_M
    G, desc = targets(m), gp.kernel.desc()
    q = 2 * E.padded_points(m)
    wb = int(L.gp2d_predict_cov_workspace(gp.n, m))
    out = []   # the embedded outputs of the two runs: the second one's slack is checked below

    def call(ptr, ld):
        mean = zeros(2 * m)
        # the contiguous run (the first) writes a contiguous covariance, the embedded run an
        # embedded one with an odd ldc > q
        cov = SC.embed(zeros(q, q), False, fill=False) if out else None
        dst = zeros(q, q) if cov is None else cov.view
        N.check(L.gp2d_predict_cov(*fit_args(gp, ptr, ld, G, m, desc), 0.0, P(mean), ctypes.c_void_p(dst.data_ptr()),
                                   dst.stride(0), P(workspace(wb)), wb, S()), "gp2d_predict_cov")
        out.append(cov)
        torch.cuda.synchronize()
        return mean, dst.contiguous()
    run_both(gp.W, True, call)
    assert out[0] is None and out[1].ld > q and out[1].ld % 2 == 1
    out[1].assert_slack_intact()


# ------------------------------------------------------------------------------------- Ozaki
@functools.lru_cache(maxsize=None)
def ozaki_fit():
    x, y = PC.tracks(200)
    gp = E.fit(E.KernelSpec(kind="mixed", l_df=5.0, l_cf=4.0, ratio=0.3), x, y, noise=0.0025)
    assert (gp.n_pad, gp.n) == (256, 512)
    return gp


@pytest.mark.parametrize("entry", ["prepare", "prepare_async"])
def test_ozaki_prepare(entry):
    gp = ozaki_fit()
    n, desc = gp.n, gp.kernel.desc()
    nbytes = int(L.gp2d_ozaki_wres_bytes(n))

    def call(ptr, ld):
        wres, rowscale, nmod = zeros(nbytes, dtype=torch.uint8), zeros(n), ctypes.c_int(0)
        if entry == "prepare":
            rc = L.gp2d_ozaki_prepare(ptr, n, ld, ctypes.byref(desc), 0, 0, P(wres), P(rowscale), ctypes.byref(nmod), S())
        else:
            rc = L.gp2d_ozaki_prepare_async(ptr, n, ld, ctypes.byref(desc), float(gp.noise), 0, 0, P(wres),
                                            P(rowscale), ctypes.byref(nmod), S())
        N.check(rc, "gp2d_ozaki_" + entry)
        return wres, rowscale, torch.tensor([nmod.value])
    _, (wres, _, nmod) = run_both(gp.W, True, call)
    assert 0 < int(nmod) <= int(L.gp2d_ozaki_nmod(n)) and bool(wres[:int(nmod) * n * n].any())


def test_ozaki_guard():
    gp = ozaki_fit()
    wb = int(L.gp2d_ozaki_guard_workspace(gp.n))

    def call(ptr, ld):
        stats = zeros(2)
        N.check(L.gp2d_ozaki_guard(ptr, gp.n, ld, gp.n_train, gp.n_pad, float(gp.noise), P(stats), P(workspace(wb)),
                                   wb, S()), "gp2d_ozaki_guard")
        return (stats,)
    _, (stats,) = run_both(gp.W, False, call)
    assert float(stats[0]) > 0.0 and float(stats[1]) > 0.0


# ------------------------------------------------------- likelihood and cross-validation
def test_lml():
    gp = PC.fit("vorticity")

    def call(ptr, ld):
        out = zeros(1)
        N.check(L.gp2d_lml(ptr, gp.n, ld, P(gp.alpha), P(gp.y), 2 * gp.n_train, P(out), S()), "gp2d_lml")
        return (out,)
    run_both(gp.W, False, call)


@pytest.mark.parametrize("case", ["vorticity", "ard"])   # vector2d mixed, ARD
def test_lml_grad(case):
    gp = PC.fit(case)
    desc = gp.kernel.desc()
    ng, wb = int(L.gp2d_lml_grad_count(ctypes.byref(desc))), int(L.gp2d_lml_grad_workspace(gp.n))

    def call(ptr, ld):
        g = zeros(ng)
        N.check(L.gp2d_lml_grad(ptr, gp.n, ld, P(gp.alpha), P(gp.x), gp.n_train, gp.n_pad, ctypes.byref(desc), P(g),
                                P(workspace(wb)), wb, S()), "gp2d_lml_grad")
        return (g,)
    _, (g,) = run_both(gp.W, True, call)
    assert bool(g.abs().min() > 0)


def test_kernel_grad_odd_ld():
    """dL_dK is the reference's unpadded layout: 2·37 rows of 2·100 columns, embedded with an odd
    leading dimension and a base that is only 8-byte aligned."""
    na, nb = 37, 100
    desc = PC.fit("vorticity").kernel.desc()
    rng = np.random.default_rng(4)
    xa, xb = (torch.tensor(rng.uniform(0, 30, (k, 2)), device=DEV) for k in (na, nb))
    G = torch.tensor(rng.normal(size=(2 * na, 2 * nb)), device=DEV)
    ng, wb = int(L.gp2d_kernel_grad_count(ctypes.byref(desc))), int(L.gp2d_kernel_grad_workspace(na, nb))

    def call(ptr, ld):
        g = zeros(ng)
        N.check(L.gp2d_kernel_grad(P(xa), na, P(xb), nb, ctypes.byref(desc), ptr, ld, P(g), P(workspace(wb)), wb,
                                   S()), "gp2d_kernel_grad")
        return (g,)
    _, (g,) = run_both(G, False, call)
    assert bool(g.abs().min() > 0)


def test_cv_groups():
    """The group labels of test_gpu_cv.py (groups below, at and above a 128-wide block)."""
    gp = cv_fit("vector2d", 300)
    assert gp.perm is None
    bd, ntr, npad, n = gp.kernel.block_dim, gp.n_train, gp.n_pad, gp.n
    lab = np.asarray(group_labels())
    order = np.argsort(lab, kind="stable")
    ids, counts = np.unique(lab, return_counts=True)
    ng = int(ids.size)
    gstart = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    qpad = (bd * int(counts.max()) + NB - 1) // NB * NB
    gidx = torch.as_tensor(order.astype(np.int64), device=DEV)
    wb = int(L.gp2d_cv_groups_workspace(n, qpad, ng))

    def call(ptr, ld):
        mean, var, lpd = zeros(bd * ntr), zeros(bd * ntr), zeros(ng)
        info = torch.full((ng,), 7, dtype=torch.int32, device=DEV)
        N.check(L.gp2d_cv_groups(ptr, n, ld, P(gp.alpha), P(gp.y), ntr, npad, bd, gstart.ctypes.data_as(ctypes.c_void_p),
                                 P(gidx), ng, None, P(mean), P(var), P(lpd), P(info), P(workspace(wb)), wb, S()),
                "gp2d_cv_groups")
        return mean, var, lpd, info
    _, (_, _, _, info) = run_both(gp.W, False, call)
    assert not bool(info.any())


# ---------------------------------------------------------------------------------- assembly
ASM_SPECS = {
    "vector2d": E.KernelSpec(kind="mixed", l_df=5.0, l_cf=4.0, ratio=0.3),
    "vector_st": E.KernelSpec(family="vector_st", kind="mixed", l_df=5.0, l_cf=4.0, ratio=0.3, var_t=1.5, l_t=2.0),
    "ard": E.KernelSpec(family="ard", variances=(1.3, 0.4), lengthscales=((2.0, 3.0), (7.0, 5.0))),
}
ASM_N, ASM_PAD = 130, 192


def asm_points(ks, n, seed):
    return torch.tensor(np.random.default_rng(seed).uniform(0, 30, (n, ks.input_dim)), device=DEV)


# symmetric = 2 (the lower block triangle) exists for the vector families only
@pytest.mark.parametrize("family,symmetric", [(f, sym) for f in ASM_SPECS for sym in (0, 1, 2)
                                              if sym < 2 or ASM_SPECS[f].is_vector])
def test_assemble(family, symmetric):
    ks = ASM_SPECS[family]
    desc, bd = ks.desc(), ks.block_dim
    xa = asm_points(ks, ASM_N, 5)
    # the cross-covariance against another point set (70 points padded to 128); K_y on xa itself
    xb, nb, nbp = (asm_points(ks, 70, 6), 70, 128) if symmetric == 0 else (xa, ASM_N, ASM_PAD)
    rows, cols = bd * ASM_PAD, bd * nbp

    def call(ptr, ld):
        N.check(L.gp2d_assemble(P(xa), ASM_N, ASM_PAD, P(xb), nb, nbp, ctypes.byref(desc), 0.01 if symmetric else 0.0,
                                symmetric, ptr, ld, S()), "gp2d_assemble")
        return ()
    # both outputs start as sentinel: what symmetric = 2 leaves unwritten compares as sentinel
    K, _ = run_both(SC.sentinel_buffer((rows, cols), DEV), False, call)
    upper = torch.triu(torch.ones(rows, cols, device=DEV), 1).bool()
    unwritten = SC.is_sentinel(K)
    if symmetric == 2:
        assert bool(unwritten[upper].all()) and not bool(unwritten[~upper].any())
    else:
        assert not bool(unwritten.any())
    assert bool(torch.isfinite(K[~unwritten]).all())


def test_assemble_cols():
    ks = ASM_SPECS["vector2d"]
    desc, x, n = ks.desc(), asm_points(ks, ASM_N, 5), 2 * ASM_PAD
    c0, ncols = 64, 64

    def call(ptr, ld):
        N.check(L.gp2d_assemble_cols(P(x), ASM_N, ASM_PAD, ctypes.byref(desc), 0.01, ptr, ld, c0, ncols, S()),
                "gp2d_assemble_cols")
        return ()
    K, _ = run_both(SC.sentinel_buffer((n, n), DEV), False, call)
    unwritten = SC.is_sentinel(K)
    assert not bool(unwritten[:, c0:c0 + ncols].any())
    assert bool(unwritten[:, :c0].all()) and bool(unwritten[:, c0 + ncols:].all())


# -------------------------------------------------------------------------- distributed factor
def test_dfact_one_rank():
    """One process, P = 1, n = 1024 (two super-blocks): the whole step sequence, then α's pieces."""
    n = 1024
    SB = int(L.gp2d_dfact_sb())
    nsb = n // SB
    Ky = torch.tensor(_spd(n, n), device=DEV)
    y = torch.tensor(np.random.default_rng(7).normal(size=n), device=DEV)
    wb, pd = int(L.gp2d_dfact_workspace(n)), int(L.gp2d_dfact_panel_doubles(n))
    ab = int(L.gp2d_dfact_alpha_workspace(n, nsb))

    def call(ptr, ld):
        panels = [zeros(pd) for _ in range(2)]
        info, work = torch.zeros(1, dtype=torch.int32, device=DEV), workspace(wb)

        def factor(s):
            N.check(L.gp2d_dfact_panel(ptr, n, ld, s, P(panels[s % 2]), P(info), P(work), wb, S()), "gp2d_dfact_panel")
        factor(0)
        for s in range(nsb):
            N.check(L.gp2d_dfact_update(ptr, n, ld, s, P(panels[s % 2]), 1, 0, s + 1, nsb, S()), "gp2d_dfact_update")
            if s + 1 < nsb:
                factor(s + 1)
            N.check(L.gp2d_dfact_invstep(ptr, n, ld, s, P(panels[s % 2]), 1, 0, P(work), wb, S()), "gp2d_dfact_invstep")
        zp, z, alpha = zeros(nsb, n), zeros(n), zeros(nsb, SB)
        N.check(L.gp2d_dfact_zpart(ptr, n, ld, 0, 1, nsb, P(y), P(zp), S()), "gp2d_dfact_zpart")
        N.check(L.gp2d_dfact_zsum(P(zp), nsb, n, P(z), S()), "gp2d_dfact_zsum")
        N.check(L.gp2d_dfact_alpha_blocks(ptr, n, ld, 0, 1, nsb, P(z), P(alpha), P(workspace(ab)), ab, S()),
                "gp2d_dfact_alpha_blocks")
        return info, zp, alpha
    W, (info, _, alpha) = run_both(Ky, True, call)
    assert int(info.item()) == 0
    # the sequence factored and inverted K_y (the multi-rank tests pin the bits to gp2d_potrf + gp2d_trtri)
    ref = np.linalg.solve(Ky.cpu().numpy(), y.cpu().numpy())
    assert np.max(np.abs(alpha.reshape(-1).cpu().numpy() - ref)) / np.max(np.abs(ref)) < 1e-11


# -------------------------------------------------------- dense product, exact arithmetic
@pytest.mark.parametrize("beta", [0.5, 0.0])
@pytest.mark.parametrize("transb", [0, 1])
def test_gemm_exact_integers(transb, beta):
    """C = −2·A·op(B) + beta·C on small integers: every product and partial sum is an integer far
    below 2^53 and C is even, so FP64 is exact and the result must equal int64 arithmetic — any
    mis-addressed element is an integer error.  lda, ldb, ldc differ, all three operands are
    embedded; with beta = 0 the C block starts as NaN, which shows that C is not read."""
    m, n, k = 256, 128, 48
    rng = np.random.default_rng(8 + transb)
    A = rng.integers(-8, 9, (m, k))
    B = rng.integers(-8, 9, (n, k) if transb else (k, n))
    C = 2 * rng.integers(-4, 5, (m, n))
    want = -2 * (A @ (B.T if transb else B)) + (C // 2 if beta else 0)
    assert want.dtype == np.int64
    dev = lambda a: torch.tensor(a.astype(np.float64), device=DEV)  # noqa: E731
    eA = SC.embed(dev(A), True)
    eB = SC.embed(dev(B), True, extra=4 if transb else 0)
    eC = SC.embed(dev(C), False, fill=bool(beta))
    assert len({eA.ld, eB.ld, eC.ld}) == 3 and eC.ld % 2 == 1
    N.check(L.gp2d_gemm(transb, m, n, k, -2.0, eA.ptr, eA.ld, eB.ptr, eB.ld, beta, eC.ptr, eC.ld, S()), "gp2d_gemm")
    torch.cuda.synchronize()
    for e in (eA, eB, eC):
        e.assert_slack_intact()
    assert torch.equal(eA.view, dev(A)) and torch.equal(eB.view, dev(B))
    got = eC.view.cpu().numpy()
    assert np.array_equal(got, want.astype(np.float64))
