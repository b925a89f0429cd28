"""Time the leave-one-out gradient beside the LML gradient (dev tool): gp2d_loo_grad and
gp2d_lml_grad, the C entries on preallocated buffers, in the same process on the same fit —
N_train = 4096 (n = 8192), mixed kernel, FP64 fit; medians of 20 runs after 3 warm-ups, HIP events
on the stream.  Also the value-only form of gp2d_loo_grad (grad_dev = NULL) and one engine.fit.
By flop count the LOO gradient carries about four times the LML gradient's GEMM work (WᵀW, n³/3,
and B·Bᵀ's lower tiles, n³, against WᵀW alone) plus the n² scale pass and two triangular products.
Writes one JSON document (profiles/loo_timing.json is a run of this tool; DESIGN.md §3.12 quotes it).
usage: python tools/time_loo.py [out.json] [N_train]"""
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "2d-gp_amd")]
import numpy as np  # noqa: E402
import torch  # noqa: E402

from gp2d import _native as N  # noqa: E402
from gp2d import data as D  # noqa: E402
from gp2d import engine as E  # noqa: E402

OUT = sys.argv[1] if len(sys.argv) > 1 else ""
NTR = int(sys.argv[2]) if len(sys.argv) > 2 else 4096
REPS, WARM = 20, 3


def timed(fn):
    for _ in range(WARM):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(REPS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return float(np.median(ms)), [round(t, 4) for t in ms]


x1, x2, u, v = D.synthetic_tracks(NTR, seed=2016)
xt = torch.tensor(np.stack([x1, x2], 1), device="cuda")
yt = torch.tensor(np.concatenate([u, v]), device="cuda")
spec = E.KernelSpec(kind="mixed", l_df=5.0, l_cf=7.0, ratio=0.6)
fit_ms, fit_all = timed(lambda: E.fit(spec, xt, yt, 0.0025))
gp = E.fit(spec, xt, yt, 0.0025)
L, dev = N.lib(), gp.device
n, s = gp.n, E._stream_handle(gp.device)
desc = gp.kernel.desc()
ng = int(L.gp2d_lml_grad_count(ctypes.byref(desc)))
g_lml = torch.empty(ng, dtype=torch.float64, device=dev)
g_loo = torch.empty(ng, dtype=torch.float64, device=dev)
val = torch.empty(1, dtype=torch.float64, device=dev)
info = torch.empty(1, dtype=torch.int32, device=dev)
wb_lml, wb_loo = int(L.gp2d_lml_grad_workspace(n)), int(L.gp2d_loo_grad_workspace(n))
work = E._workspace(max(wb_lml, wb_loo), dev)


def c_lml():
    N.check(L.gp2d_lml_grad(E._ptr(gp.W), n, gp.W.stride(0), E._ptr(gp.alpha), E._ptr(gp.x), gp.n_train, gp.n_pad,
                            ctypes.byref(desc), E._ptr(g_lml), E._ptr(work), wb_lml, s), "gp2d_lml_grad")


def c_loo(grad=True):
    N.check(L.gp2d_loo_grad(E._ptr(gp.W), n, gp.W.stride(0), E._ptr(gp.alpha), E._ptr(gp.y), E._ptr(gp.x),
                            gp.n_train, gp.n_pad, ctypes.byref(desc), E._ptr(val), E._ptr(g_loo) if grad else None,
                            E._ptr(info), E._ptr(work), wb_loo, s), "gp2d_loo_grad")


lml_ms, lml_all = timed(c_lml)
loo_ms, loo_all = timed(c_loo)
val_ms, val_all = timed(lambda: c_loo(False))
assert int(info.item()) == 0 and bool(torch.isfinite(g_loo).all()) and bool(torch.isfinite(g_lml).all())

res = dict(device=torch.cuda.get_device_name(0), n_train=NTR, n=n, kernel="mixed", variance="f64", reps=REPS,
           warm=WARM, fit_ms=round(fit_ms, 4), fit_all_ms=fit_all,
           lml_grad_ms=round(lml_ms, 4), lml_grad_all_ms=lml_all, lml_grad_workspace_bytes=wb_lml,
           loo_grad_ms=round(loo_ms, 4), loo_grad_all_ms=loo_all, loo_grad_workspace_bytes=wb_loo,
           loo_value_ms=round(val_ms, 4), loo_value_all_ms=val_all,
           loo_over_lml=round(loo_ms / lml_ms, 3), loo_over_one_fit=round(loo_ms / fit_ms, 3),
           loo_value=float(val.item()), loo_grad=g_loo.cpu().tolist(), lml_grad=g_lml.cpu().tolist())
print(f"fit {fit_ms:.3f} ms; lml_grad {lml_ms:.3f} ms; loo_grad {loo_ms:.3f} ms ({loo_ms / lml_ms:.2f}x), "
      f"value only {val_ms:.3f} ms", flush=True)
txt = json.dumps(res, indent=1)
if OUT:
    os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
    with open(OUT, "w") as f:
        f.write(txt + "\n")
print(txt)
