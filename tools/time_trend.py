"""Time a trend fit (engine.fit(trend=)) beside the zero-mean one on the headline problem (dev tool):
N_train = 4096, a 256 × 256 grid, chunk 8192, FP64 engine, the mixed kernel; warm, medians of REPS
host-synchronised repetitions (HIP events).  Per case (zero-mean, trend 'constant', trend 'linear'):
the whole fit, the solve after the factor alone (gp2d_potrs_inv or gp2d_trend_fit on the fit's W),
the FP64 predict, the predict without its variance product (K* assembly, the mean pass and the
finalize: what differs between the cases is the mean pass and the finalize) and the likelihood with
its gradient.  By arithmetic the trend adds 2·q/n of the variance GEMM's flops and no extra read of
K*ᵀ, so the trend predict should cost the plain predict plus the difference of the mean passes.
`plain` as the fourth argument measures the zero-mean case only, through the entries every earlier
commit has (for the same numbers from the parent commit).  Writes one JSON document
(profiles/trend_timing.json is a run of this tool; DESIGN.md §3.11 quotes it).
usage: python tools/time_trend.py [out.json] [N_train] [grid] [plain]"""
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
G = int(sys.argv[3]) if len(sys.argv) > 3 else 256
PLAIN_ONLY = len(sys.argv) > 4 and sys.argv[4] == "plain"
REPS, WARM, CHUNK = 10, 3, 8192
NOISE = 0.0025
FLOW = (0.8, -0.5, 0.010, -0.006, 0.004, 0.012)   # background flow (u0, v0) and its shear, added to the tracks


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


def solve_alone(gp, trend):
    """The solve after the factor, on the fit's own W: gp2d_potrs_inv, or gp2d_trend_fit."""
    L, dev, n = N.lib(), gp.device, gp.n
    alpha = torch.empty_like(gp.alpha)
    if trend is None:
        wb = int(L.gp2d_potrs_workspace(n))
        work = E._workspace(wb, dev)
        return lambda: N.check(L.gp2d_potrs_inv(E._ptr(gp.W), n, gp.W.stride(0), E._ptr(gp.y), E._ptr(alpha),
                                                E._ptr(work), wb, E._stream_handle(dev)), "gp2d_potrs_inv")
    t = gp.extra["trend"]
    block = torch.empty_like(t["block"])
    wb = int(L.gp2d_trend_workspace(n, t["order"]))
    work = E._workspace(wb, dev)
    return lambda: N.check(L.gp2d_trend_fit(E._ptr(gp.W), n, gp.W.stride(0), E._ptr(gp.y), E._ptr(gp.x), gp.n_train,
                                            gp.n_pad, gp.x.shape[1], ctypes.byref(t["desc"]), E._ptr(alpha),
                                            E._ptr(block), E._ptr(work), wb, E._stream_handle(dev)), "gp2d_trend_fit")


x1, x2, u, v = D.synthetic_tracks(NTR, seed=2016)
a, b = x1 - x1.mean(), x2 - x2.mean()
u = u + FLOW[0] + FLOW[2] * a + FLOW[3] * b
v = v + FLOW[1] + FLOW[4] * a + FLOW[5] * b
xh, yh = np.stack([x1, x2], 1), np.concatenate([u, v])   # host points: the trend's basis needs no device round trip
xg = torch.tensor(D.bbox_grid(x1, x2, G, pad=5.0)[2], device="cuda")
spec = E.KernelSpec(kind="mixed", l_df=8.0, l_cf=8.0, ratio=0.6)
res = dict(device=torch.cuda.get_device_name(0), n_train=NTR, grid=[G, G], chunk=CHUNK, reps=REPS, warm=WARM,
           noise=NOISE, kernel=dict(kind="mixed", l_df=8.0, l_cf=8.0, ratio=0.6), flow=FLOW, cases=[])
for trend in ((None,) if PLAIN_ONLY else (None, "constant", "linear")):
    kw = {} if trend is None else dict(trend=trend)
    fit_ms, fit_all = timed(lambda: E.fit(spec, xh, yh, NOISE, **kw))
    gp = E.fit(spec, xh, yh, NOISE, **kw)
    solve_ms, solve_all = timed(solve_alone(gp, trend))
    pred = E.Predictor(gp, CHUNK)
    prd, prd_all = timed(lambda: pred(xg))
    mean_only, mean_all = timed(lambda: pred(xg, compute_var=False))
    lml, lml_all = timed(lambda: E.lml_device(gp, eval_gradient=True))
    case = dict(trend=trend, n=gp.n, fit_ms=round(fit_ms, 4), solve_ms=round(solve_ms, 4), predict_f64_ms=round(prd, 4),
                predict_mean_only_ms=round(mean_only, 4), lml_grad_ms=round(lml, 4), fit_all_ms=fit_all,
                solve_all_ms=solve_all, predict_f64_all_ms=prd_all, predict_mean_only_all_ms=mean_all,
                lml_grad_all_ms=lml_all)
    if trend is not None:
        c = E.trend_coefficients(gp)
        case.update(mean_flow=c["mean_flow"].tolist(), gradient=c["gradient"].tolist())
    res["cases"].append(case)
    print(f"trend={trend}: fit {fit_ms:.3f} ms (solve alone {solve_ms:.3f} ms), predict f64 {prd:.3f} ms "
          f"(without the variance product {mean_only:.3f} ms), LML + gradient {lml:.3f} ms", flush=True)
    del gp, pred
txt = json.dumps(res, indent=1)
if OUT:
    os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
    with open(OUT, "w") as f:
        f.write(txt + "\n")
print(txt)
