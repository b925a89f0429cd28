"""The int8 variance product from three block products instead of four.

K*'s (v,u) block equals its (u,v) block c, so with S = W_L + W_R
    V_u = S·c + W_L·(a − c),    V_v = S·c + W_R·(b − c)
replace V_u = W_L·a + W_R·c, V_v = W_L·c + W_R·b.  The engine works on residues mod m and
residues add mod m, so every output bit must be the four-product one: the GPU tests compare
gp2d_ozaki_set_three_products(1) against (0) with np.array_equal; the CPU test checks the residue
identity itself in NumPy for every modulus of the table.
"""
import numpy as np
import pytest

MODULI = [256, 255, 253, 251, 247, 241, 239, 233, 229, 227, 223, 217, 211, 199, 197, 193, 191, 181, 179, 173]


# ---------------------------------------------------------------- CPU: the residue identity
def _centred(x, m):
    """The centred residue the engine stores: in [−m/2, m/2], as an int8 byte (±128 only for m = 256,
    where both are the byte 0x80)."""
    r = np.mod(x, m)
    r = np.where(r > m // 2, r - m, r)
    return r.astype(np.int64)


def test_three_product_residue_identity_every_modulus():
    rng = np.random.default_rng(7)
    rows, k, cols = 24, 40, 16
    for m in MODULI:
        lo, hi = -(m // 2), (m - 1) // 2   # centred residues; for m = 256: −128 … 127
        wl = rng.integers(lo, hi + 1, (rows, k))
        wr = rng.integers(lo, hi + 1, (rows, k))
        a, b, c = (rng.integers(lo, hi + 1, (cols, k)) for _ in range(3))
        # force the extremes into every operand
        wl[0, :2], wr[0, :2] = (lo, hi), (lo, hi)
        wl[1, :2], wr[1, :2] = (lo, hi), (hi, lo)
        a[0, :2], c[0, :2], b[0, :2] = (lo, hi), (hi, lo), (lo, hi)
        # S: centred((r_L + r_R) mod m) fits int8, as do the centred residues of a − c and b − c
        s = _centred(wl + wr, m)
        ac, bc = _centred(a - c, m), _centred(b - c, m)
        for t in (s, ac, bc):
            if m == 256:   # 128 ≡ −128: the byte 0x80 stands for both
                assert t.min() >= -127 and t.max() <= 128
            else:
                assert np.abs(t).max() <= m // 2 <= 127
        # the engine's bytes: int8 two's complement (for m = 256 the residue 128 is stored as −128)
        s8, ac8, bc8 = (t.astype(np.int8).astype(np.int64) for t in (s, ac, bc))
        p1 = s8 @ c.T
        vu3 = np.mod(np.mod(p1, m) + np.mod(wl @ ac8.T, m), m)
        vv3 = np.mod(np.mod(p1, m) + np.mod(wr @ bc8.T, m), m)
        vu4 = np.mod(wl @ a.T + wr @ c.T, m)
        vv4 = np.mod(wl @ c.T + wr @ b.T, m)
        assert np.array_equal(vu3, vu4), m
        assert np.array_equal(vv3, vv4), m


# ---------------------------------------------------------------- GPU: bit identity, on against off
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


def rel(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return float(np.max(np.abs(a - b)) / max(np.max(np.abs(b)), 1e-300))


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


@pytest.mark.gpu
@pytest.mark.parametrize("ntr", [256, 512, 500])   # n = 512: one top and one bottom row block; n = 1024: two of
@pytest.mark.parametrize("kind", ["df", "mixed"])  # each (500: padded identity rows in both halves)
@pytest.mark.parametrize("m", [300, 700])          # chunk 256: a ragged last chunk, more than one chunk
def test_three_products_bit_identical_to_four(E, ntr, kind, m):
    x, y = tracks(ntr, ntr + 1)
    xg = grid(m, m)
    gp = E.fit(kernel_spec(E, kind), x, y, noise=0.0025, variance="ozaki")
    assert gp.n_pad % 256 == 0 and "ozaki" in gp.extra
    m3, v3 = predict_with(E, gp, xg, 256, 1)
    m4, v4 = predict_with(E, gp, xg, 256, 0)
    assert np.array_equal(m3, m4) and np.array_equal(v3, v4)
    assert np.all(np.isfinite(v3)) and np.all(v3 > 0)


@pytest.mark.gpu
@pytest.mark.parametrize("wbits,kbits", [(53, 47), (56, 50)])
def test_three_products_split_residues_bit_identical(E, wbits, kbits):
    """Noise 1e-4 with W above 50 bits: the W residues (and S's) come from the split form; at 50 K*
    bits the stored differences are formed from the residues instead of the integers."""
    x, y = tracks(512, 91)
    xg = grid(300, 92)
    gp = E.fit(kernel_spec(E, "df"), x, y, noise=1e-4, variance="ozaki", guard=False)
    E.ozaki_prepare(gp, wbits=wbits, kbits=kbits)
    m3, v3 = predict_with(E, gp, xg, 256, 1)
    m4, v4 = predict_with(E, gp, xg, 256, 0)
    assert np.array_equal(m3, m4) and np.array_equal(v3, v4)
    assert np.all(np.isfinite(v3))


@pytest.mark.gpu
def test_three_products_with_zero_slabs(E):
    """The far-grid layout of test_zero_slab_skip_far_grid_and_planes (a grid block far from every
    observation: empty slab lists) at N_pad = 768: skip on/off × three products on/off agree bit for bit."""
    rng = np.random.default_rng(41)
    n = 768
    x = np.stack([rng.uniform(0, 60, n), rng.uniform(0, 45, n)], 1)
    y = np.concatenate([np.sin(x[:, 1] / 7), np.cos(x[:, 0] / 9)]) + rng.normal(0, 0.05, 2 * n)
    near = np.stack([rng.uniform(0, 60, 900), rng.uniform(0, 45, 900)], 1)
    far = np.stack([rng.uniform(900, 960, 700), rng.uniform(900, 945, 700)], 1)
    xg = np.concatenate([near, far])
    ks = E.KernelSpec(kind="df", l_df=5.0)
    gp = E.fit(ks, x, y, noise=0.0025, variance="ozaki")
    assert gp.n_pad == 768
    ref = predict_with(E, gp, xg, 512, 0, skip=0)
    for three, skip in ((1, 1), (1, 0), (0, 1)):
        mu, var = predict_with(E, gp, xg, 512, three, skip)
        assert np.array_equal(mu, ref[0]) and np.array_equal(var, ref[1]), (three, skip)
    M = xg.shape[0]
    kss = float(E.N.lib().gp2d_kernel_diag(__import__("ctypes").byref(ks.desc())))
    far_idx = np.concatenate([np.arange(900, M), M + np.arange(900, M)])
    assert np.all(ref[1][far_idx] == kss) and np.all(ref[0][far_idx] == 0.0)


@pytest.mark.gpu
def test_three_products_planes_ahead_equal_inline(E):
    x, y = tracks(512, 61)
    xg = grid(1300, 62)
    ks = kernel_spec(E, "df")
    planes = E.kstar_planes(ks, x, xg, 0.0025, chunk=512)
    gp = E.fit(ks, x, y, noise=0.0025, variance="ozaki")
    assert gp.n == 1024
    pr = E.Predictor(gp, 512)
    mp, vp = (t.cpu().numpy() for t in pr(xg, planes=planes))
    mi, vi = (t.cpu().numpy() for t in pr(xg))
    assert np.array_equal(mp, mi) and np.array_equal(vp, vi)
    m4, v4 = predict_with(E, gp, xg, 512, 0)
    assert np.array_equal(mi, m4) and np.array_equal(vi, v4)


@pytest.mark.gpu
def test_three_products_fallback_where_npad_is_not_a_multiple_of_256(E):
    """N_pad = 384: a 256-row tile would straddle the u and v observation rows, so the four-product
    path runs whatever the switch says; both settings match the FP64 engine within the gate of
    test_ozaki_vs_f64_engine_and_golden."""
    x, y = tracks(384, 71)
    xg = grid(600, 72)
    ks = kernel_spec(E, "df")
    gp = E.fit(ks, x, y, noise=0.0025, variance="ozaki")
    assert gp.n_pad == 384
    m3, v3 = predict_with(E, gp, xg, 256, 1)
    m4, v4 = predict_with(E, gp, xg, 256, 0)
    assert np.array_equal(m3, m4) and np.array_equal(v3, v4)
    gf = E.fit(ks, x, y, noise=0.0025)
    mf, vf = (t.cpu().numpy() for t in E.predict(gf, xg, chunk=256))
    assert rel(m3, mf) < 1e-10
    assert rel(v3, vf) < 1e-11
    assert np.max(np.abs(v3 - vf) / np.abs(vf)) < 1e-10
