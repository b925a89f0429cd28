"""Digest the outputs of the FP64 matrix-core path of one build of the library (dev tool): load
libgp2d.so from a given path, run a fixed set of calls on seeded inputs and write the SHA-256 of
every raw output.  Two builds whose digests all agree compute the same bits on this path
(profiles/f64_core_ab.json holds the lists of a parent and a refactored build).
  * gp2d_gemm NN and NT at 128 / 256 / 384, β = 0 and β ≠ 0;
  * a fit (W, α) at N_train = 37, 300, 1000, 4096 — the TRTRI's products, K-split from n = 2048 on;
  * gp2d_predict (FP64 engine), gp2d_predict_grad and gp2d_predict_cov on those fits;
  * gp2d_lml_grad for df, mixed, scalar and ARD at n = 128 / 256 / 384 and at N_train = 4096;
  * a batched factor of 4 problems.
usage: python tools/ab_f64_core.py path/to/libgp2d.so out.json"""
import hashlib
import json
import os
import sys

LIB, OUT = os.path.abspath(sys.argv[1]), sys.argv[2]
os.environ["GP2D_LIB"] = LIB   # read by gp2d._native on import
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "2d-gp_amd")]
import numpy as np  # noqa: E402
import torch  # noqa: E402

from gp2d import data as D  # noqa: E402
from gp2d import engine as E  # noqa: E402

digests = {}


def note(name, *arrays):
    h = hashlib.sha256()
    for a in arrays:
        a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a, dtype=np.float64)
        h.update(np.ascontiguousarray(a).tobytes())
    digests[name] = h.hexdigest()


def problem(n, seed):
    x1, x2, u, v = D.synthetic_tracks(n, seed=seed)
    return np.stack([x1, x2], 1), np.concatenate([u, v]), D.bbox_grid(x1, x2, 24, pad=5.0)[2]


rng = np.random.default_rng(5)
for s in (128, 256, 384):
    A, B, C = (rng.normal(0, 1, (s, s)) for _ in range(3))
    for transb in (False, True):
        tag = f"gemm/{'NT' if transb else 'NN'}/{s}"
        note(tag + "/beta0", E.gemm(A, B, transb=transb))
        note(tag + "/beta", E.gemm(A, B, transb=transb, alpha=-1.25, C=C, beta=0.5))

DF = E.KernelSpec(kind="df", l_df=5.0)
for n in (37, 300, 1000, 4096):
    x, y, xg = problem(n, seed=n)
    gp = E.fit(DF, x, y, 0.0025)
    note(f"fit/{n}/W", gp.W)
    note(f"fit/{n}/alpha", gp.alpha)
    note(f"predict/{n}", *E.predict(gp, xg))
    note(f"predict_grad/{n}", *E.predict_gradient(gp, xg))
    note(f"predict_cov/{n}", *E.predict_cov(gp, xg))
    del gp

SPECS = {"df": DF, "mixed": E.KernelSpec(kind="mixed", l_df=5.0, l_cf=4.0, ratio=0.6),
         "scalar": E.KernelSpec(kind="scalar", l_df=5.0),
         "ard": E.KernelSpec(family="ard", variances=(1.0, 0.3), lengthscales=((6.0, 8.0, 3.0), (20.0, 25.0, 9.0)))}
for name, spec in SPECS.items():
    sizes = (128, 256, 384, 4096) if spec.block_dim == 1 else (64, 65, 129, 4096)   # n = 128, 256, 384, then the headline
    for n in sizes:
        if name == "ard":
            r = np.random.default_rng(n)
            x = np.stack([r.uniform(0, 6, n), r.uniform(0, 45, n), r.uniform(0, 60, n)], 1)
            y = np.sin(x[:, 1] / 7) + 0.1 * x[:, 0] + r.normal(0, 0.05, n)
        else:
            x, y, _ = problem(n, seed=100 + n)
        gp = E.fit(spec, x, y, 0.01)
        val, grad = E.log_marginal_likelihood(gp, eval_gradient=True)
        note(f"lml_grad/{name}/{n}", [val], grad)
        del gp

x, y, _ = problem(300, seed=7)
fits = E.fit_batch([(E.KernelSpec(kind="df", l_df=l), x, y, 0.0025) for l in (3.0, 4.0, 5.0, 6.0)])
note("fit_batch/4x300/W", *[g.W for g in fits])
note("fit_batch/4x300/alpha", *[g.alpha for g in fits])

torch.cuda.synchronize()
os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
with open(OUT, "w") as f:
    json.dump(dict(device=torch.cuda.get_device_name(0), digests=digests), f, indent=1)
    f.write("\n")
print(f"{len(digests)} digests -> {OUT}")
