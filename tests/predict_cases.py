"""The four small FP64 predict cases shared by the GPU tests that pin the predict family's ABI:
100 training points (n = 256 for the vector kernels, 128 for the ARD one) and 300 targets, which
at chunk = 128 is the smallest shape with more than one chunk and a ragged tail (128, 128, 44).
Each case is fitted once; raw() calls its entry point through the C ABI in a workspace of exactly
the exported size, followed by a sentinel-filled tail."""
import ctypes
import functools

import numpy as np
import torch

from gp2d import _native as N
from gp2d import engine as E

NTR, M, CHUNK, COV_M = 100, 300, 128, 100
TAIL = 1 << 20          # sentinel bytes after the workspace
SENTINEL = 0xA5
CASES = ("df", "ard", "vorticity", "cov")
CHUNKED = CASES[:3]


def tracks(n, seed=2016):   # test_gpu_parity.tracks
    rng = np.random.default_rng(seed)
    x = np.stack([rng.uniform(0, 60, n), rng.uniform(0, 45, n)], 1)
    u = np.sin(x[:, 1] / 7) + rng.normal(0, 0.05, n)
    v = np.cos(x[:, 0] / 9) + rng.normal(0, 0.05, n)
    return x, np.concatenate([u, v])


def targets(m=M):
    rng = np.random.default_rng(m)
    return np.stack([rng.uniform(-5, 65, m), rng.uniform(-5, 50, m)], 1)


@functools.lru_cache(maxsize=None)
def fit(case, variance="f64"):
    x, y = tracks(NTR)
    if case == "ard":
        ks = E.KernelSpec(family="ard", variances=(1.3,), lengthscales=((6.0, 4.0),))
        return E.fit(ks, x, y[:NTR], noise=0.0025)
    ks = {"df": E.KernelSpec(kind="df", l_df=5.0),
          "vorticity": E.KernelSpec(kind="mixed", l_df=5.0, l_cf=4.0, ratio=0.3),
          "cov": E.KernelSpec(kind="df", l_df=5.0)}[case]
    return E.fit(ks, x, y, noise=0.0025, variance=variance)


def workspace_bytes(case, chunk=CHUNK):
    L, gp = N.lib(), fit(case)
    if case == "cov":
        return int(L.gp2d_predict_cov_workspace(gp.n, COV_M))
    if case == "vorticity":
        return int(L.gp2d_predict_field_workspace(gp.n, chunk))
    return int(L.gp2d_predict_workspace(gp.n, chunk, gp.kernel.block_dim))


def raw(case, chunk=CHUNK, compute_var=True):
    """The case through the C ABI: (mean, var or padded q × q covariance or None, the workspace's
    sentinel tail after the call), device tensors."""
    L, gp = N.lib(), fit(case)
    P = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    dev = gp.device
    s = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    wbytes = workspace_bytes(case, chunk)
    buf = torch.full((wbytes + TAIL,), SENTINEL, dtype=torch.uint8, device=dev)
    desc = gp.kernel.desc()
    m = COV_M if case == "cov" else M
    G = torch.as_tensor(targets()[:m].copy(), device=dev)
    bd = gp.kernel.block_dim
    fit_args = (P(gp.W), gp.n, gp.W.stride(0), P(gp.alpha), P(gp.x), gp.n_train, gp.n_pad, P(G), m, ctypes.byref(desc))
    if case == "cov":
        q = 2 * E.padded_points(m)
        mean = torch.empty(2 * m, dtype=torch.float64, device=dev)
        out = torch.empty((q, q), dtype=torch.float64, device=dev)
        N.check(L.gp2d_predict_cov(*fit_args, 0.0, P(mean), P(out), q, P(buf), wbytes, s), "gp2d_predict_cov")
    elif case == "vorticity":
        mean = torch.empty(m, dtype=torch.float64, device=dev)
        out = torch.empty(m, dtype=torch.float64, device=dev) if compute_var else None
        N.check(L.gp2d_predict_field(*fit_args, N.FIELD_VORTICITY, int(compute_var), P(mean),
                                     None if out is None else P(out), chunk, P(buf), wbytes, s), "gp2d_predict_field")
    else:
        mean = torch.empty(bd * m, dtype=torch.float64, device=dev)
        out = torch.empty(bd * m, dtype=torch.float64, device=dev) if compute_var else None
        N.check(L.gp2d_predict(*fit_args, N.VAR_LATENT, float(gp.noise), int(compute_var), P(mean),
                               None if out is None else P(out), chunk, P(buf), wbytes, s), "gp2d_predict")
    torch.cuda.synchronize(dev)
    return mean, out, buf[wbytes:]


def through_engine(case):
    """The same case through the engine's public entry: (mean, var or the 2m × 2m covariance)."""
    gp = fit(case)
    if case == "cov":
        return E.predict_cov(gp, targets()[:COV_M])
    if case == "vorticity":
        return E.predict_field(gp, targets(), "vorticity", chunk=CHUNK)
    return E.predict(gp, targets(), chunk=CHUNK)
