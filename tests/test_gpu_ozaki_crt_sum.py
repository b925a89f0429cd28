"""The three block products of the int8 variance are summed in the CRT pass.

P1 = S·c, P2 = W_L·(a − c) and P3 = W_R·(b − c) leave the GEMM side by side, each reduced mod m on
its own, and the CRT pass forms the residue of V_u as P1 ⊕ P2 and that of V_v as P1 (u-observation
rows) or P1 ⊕ P3 (v-observation rows), r₁ ⊕ r₂ = min(s, s − m) with s = r₁ + r₂ in unsigned 32-bit
arithmetic.  Before (and still where the K* planes are made ahead and belong to the caller, so
that P3 has no room of its own), the GEMM epilogue of P2 and P3 added P1's stored residue to its
accumulator ahead of the one reduction.  Both are the class of the sum mod m in [0, m), so every
output bit stays: the CPU test checks ⊕ and the number the CRT turns it into for every modulus of
the table and every pair of residues; the GPU tests compare the predict against the four-product form
(gp2d_ozaki_set_three_products(0)), which keeps one finished residue per element, with
np.array_equal at the smallest shapes where each new path exists.
"""
import numpy as np
import pytest

MODULI = [256, 255, 253, 251, 247, 241, 239, 233, 229, 227, 223, 217, 211, 199, 197, 193, 191, 181, 179, 173]


# ---------------------------------------------------------------- CPU: ⊕ and the CRT's cl
def _mod_u32(v, m):
    """ozaki_mod_u32 (csrc/ozaki.hpp) on uint32 bit patterns, in integers: the GEMM epilogue's reduction."""
    v = v.astype(np.int64)
    c20 = (1 << 20) % m
    y = v - (v >> 20) * ((1 << 20) - c20)
    assert y.min() >= 0 and y.max() < 1 << 21
    magic = ((1 << 29) + m - 1) // m
    q = ((8 * y) * magic) >> 32
    r = y - q * m
    assert np.array_equal(r, np.mod(v, m))
    return r


def test_residue_sum_every_modulus_every_pair():
    rng = np.random.default_rng(11)
    for m in MODULI:
        r1, r2 = (a.ravel().astype(np.uint32) for a in np.meshgrid(np.arange(m), np.arange(m), indexing="ij"))
        s = r1 + r2                                   # uint32: no wrap, s ≤ 510
        got = np.minimum(s, s - np.uint32(m))         # s − m wraps above s exactly when s < m
        assert got.dtype == np.uint32
        want = (r1.astype(np.int64) + r2.astype(np.int64)) % m
        assert np.array_equal(got.astype(np.int64), want), m
        # ⊕ 0 leaves a residue as it is (the u-observation rows of V_v, which have no P3)
        z = np.arange(m, dtype=np.uint32)
        assert np.array_equal(np.minimum(z, z - np.uint32(m)), z), m

        # cl, the number the CRT multiplies by h_l and t_l.  Before: the epilogue of the second product
        # reduced (its biased accumulator + the first product's stored residue) once.  Now: each
        # accumulator is reduced alone and the CRT adds the residues.  A biased accumulator is any
        # uint32 the GEMM can leave: bias − K·2^14 ≤ v ≤ bias + K·2^14 with bias = m·⌈K·2^14 / m⌉;
        # take K = 65536·2 − 256, the largest the predict admits, and the extremes with random values.
        K = 2 * 65536 - 256
        bias = ((K << 14) + m - 1) // m * m
        acc = rng.integers(bias - (K << 14), bias + (K << 14) + 1, r1.size, dtype=np.int64)
        acc[:4] = (bias - (K << 14), bias + (K << 14), bias, bias + m - 1)
        assert acc.min() >= 0 and acc.max() + 255 < 1 << 32
        prior = r1.astype(np.int64)                   # every residue of the first product …
        second = _mod_u32(acc.astype(np.uint32), m)   # … against a second product's own residue
        cl_before = _mod_u32((acc + prior).astype(np.uint32), m).astype(np.float64)
        s2 = prior.astype(np.uint32) + second.astype(np.uint32)
        cl_now = np.minimum(s2, s2 - np.uint32(m)).astype(np.float64)
        assert np.array_equal(cl_before, cl_now), m
        assert cl_now.min() >= 0 and cl_now.max() <= m - 1


# ---------------------------------------------------------------- GPU: bit identity against the four-product form
@pytest.fixture(scope="module")
def E():
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():  # pragma: no cover
        pytest.skip("no HIP device")
    from gp2d import engine
    return engine


def tracks(n, seed):
    rng = np.random.default_rng(seed)
    x = np.stack([rng.uniform(0, 60, n), rng.uniform(0, 45, n)], 1)
    y = np.concatenate([np.sin(x[:, 1] / 7), np.cos(x[:, 0] / 9)]) + rng.normal(0, 0.05, 2 * n)
    return x, y


def grid(m, seed):
    rng = np.random.default_rng(seed)
    return np.stack([rng.uniform(-5, 65, m), rng.uniform(-5, 50, m)], 1)


def predict_with(E, gp, xg, chunk, three, skip=1):
    """(mean, variance) under the given switch settings; both switches back on afterwards."""
    L = E.N.lib()
    try:
        L.gp2d_ozaki_set_three_products(three)
        L.gp2d_ozaki_set_skip(skip)
        return tuple(t.cpu().numpy() for t in E.predict(gp, xg, chunk=chunk))
    finally:
        L.gp2d_ozaki_set_three_products(1)
        L.gp2d_ozaki_set_skip(1)


def kernel_spec(E, kind):
    return E.KernelSpec(kind=kind, l_df=5.0, l_cf=6.5, ratio=0.5 if kind == "mixed" else 1.0)


_FITS = {}


def fit_of(E, ntr, kind):
    """One fit per (N_train, kernel), shared by the grid sizes."""
    if (ntr, kind) not in _FITS:
        x, y = tracks(ntr, ntr + 3)
        _FITS[ntr, kind] = E.fit(kernel_spec(E, kind), x, y, noise=0.0025, variance="ozaki")
    return _FITS[ntr, kind]


@pytest.mark.gpu
@pytest.mark.parametrize("ntr", [256, 512, 500])   # n = 512: P3 is a single row block and the CRT's second pass
@pytest.mark.parametrize("kind", ["df", "mixed"])  # has no rows; n = 1024: one full segment (500: padded identity
@pytest.mark.parametrize("m", [300, 700])          # rows in both halves).  Chunk 256: ragged last chunk, several chunks
def test_summed_in_crt_bit_identical_to_four_products(E, ntr, kind, m):
    gp = fit_of(E, ntr, kind)
    assert gp.n_pad % 256 == 0 and gp.n == 2 * gp.n_pad and "ozaki" in gp.extra
    xg = grid(m, m + 1)
    m3, v3 = predict_with(E, gp, xg, 256, 1)
    m4, v4 = predict_with(E, gp, xg, 256, 0)
    assert np.array_equal(m3, m4) and np.array_equal(v3, v4)
    assert np.all(np.isfinite(v3)) and np.all(v3 > 0)


@pytest.mark.gpu
def test_summed_in_crt_segment_straddles_the_row_halves(E):
    """N_pad = 768: n = 1536 is a segment and a half, and the second 512-row pass of the first segment
    has u-observation rows (no P3) in its lower lanes and v-observation rows in its upper ones."""
    x, y = tracks(768, 5)
    xg = grid(520, 6)
    gp = E.fit(kernel_spec(E, "df"), x, y, noise=0.0025, variance="ozaki")
    assert gp.n_pad == 768
    m3, v3 = predict_with(E, gp, xg, 384, 1)
    m4, v4 = predict_with(E, gp, xg, 384, 0)
    assert np.array_equal(m3, m4) and np.array_equal(v3, v4)
    assert np.all(np.isfinite(v3)) and np.all(v3 > 0)


@pytest.mark.gpu
def test_summed_in_crt_split_residues(E):
    """wbits 56, kbits 50: the W residues come from the split form and the K* differences are formed
    from the residues (KS_DIFF_R)."""
    x, y = tracks(512, 91)
    xg = grid(300, 92)
    gp = E.fit(kernel_spec(E, "df"), x, y, noise=1e-4, variance="ozaki", guard=False)
    E.ozaki_prepare(gp, wbits=56, kbits=50)
    m3, v3 = predict_with(E, gp, xg, 256, 1)
    m4, v4 = predict_with(E, gp, xg, 256, 0)
    assert np.array_equal(m3, m4) and np.array_equal(v3, v4)
    assert np.all(np.isfinite(v3))


@pytest.mark.gpu
def test_summed_in_crt_thirteen_moduli(E):
    """A moduli count that is no multiple of four: the last plane group of the CRT's loads repeats
    plane nmod − 1, now for the three products' planes.  100 bits of operands need 13 moduli."""
    x, y = tracks(512, 17)
    xg = grid(300, 18)
    gp = E.fit(kernel_spec(E, "df"), x, y, noise=0.0025, variance="ozaki", guard=False)
    counts = {}
    for wbits, kbits in ((50, 50), (53, 47), (51, 49), (52, 48), (50, 48), (52, 50)):
        E.ozaki_prepare(gp, wbits=wbits, kbits=kbits)
        counts[wbits, kbits] = gp.extra["ozaki"][2]
        if counts[wbits, kbits] == 13:
            break
    print("moduli per (wbits, kbits):", counts)
    assert gp.extra["ozaki"][2] == 13, counts
    m3, v3 = predict_with(E, gp, xg, 256, 1)
    m4, v4 = predict_with(E, gp, xg, 256, 0)
    assert np.array_equal(m3, m4) and np.array_equal(v3, v4)
    assert np.all(np.isfinite(v3)) and np.all(v3 > 0)


@pytest.mark.gpu
def test_summed_in_crt_with_zero_slabs(E):
    """A grid block far from every observation (empty slab lists, as in
    test_zero_slab_skip_far_grid_and_planes): skipping on and off, three products and four agree."""
    rng = np.random.default_rng(43)
    x, y = tracks(512, 44)
    near = np.stack([rng.uniform(0, 60, 400), rng.uniform(0, 45, 400)], 1)
    far = np.stack([rng.uniform(900, 960, 300), rng.uniform(900, 945, 300)], 1)
    xg = np.concatenate([near, far])
    ks = E.KernelSpec(kind="df", l_df=5.0)
    gp = E.fit(ks, x, y, noise=0.0025, variance="ozaki")
    ref = predict_with(E, gp, xg, 512, 0, skip=0)
    for three, skip in ((1, 1), (1, 0)):
        mu, var = predict_with(E, gp, xg, 512, three, skip)
        assert np.array_equal(mu, ref[0]) and np.array_equal(var, ref[1]), (three, skip)
    M = xg.shape[0]
    kss = float(E.N.lib().gp2d_kernel_diag(__import__("ctypes").byref(ks.desc())))
    far_idx = np.concatenate([np.arange(400, M), M + np.arange(400, M)])
    assert np.all(ref[1][far_idx] == kss) and np.all(ref[0][far_idx] == 0.0)   # the far block was skipped whole


@pytest.mark.gpu
def test_summed_in_crt_planes_made_ahead(E):
    x, y = tracks(512, 61)
    xg = grid(700, 62)
    ks = kernel_spec(E, "df")
    planes = E.kstar_planes(ks, x, xg, 0.0025, chunk=256)
    gp = E.fit(ks, x, y, noise=0.0025, variance="ozaki")
    assert gp.n == 1024
    pr = E.Predictor(gp, 256)
    mp, vp = (t.cpu().numpy() for t in pr(xg, planes=planes))
    mi, vi = (t.cpu().numpy() for t in pr(xg))
    assert np.array_equal(mp, mi) and np.array_equal(vp, vi)
    m4, v4 = predict_with(E, gp, xg, 256, 0)
    assert np.array_equal(mi, m4) and np.array_equal(vi, v4)
