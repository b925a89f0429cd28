"""Time engine.predict_gradient beside engine.predict (variance 'f64') on the headline problem
(dev tool): N_train = 4096, a 256 × 256 grid, the same targets, a 'df' and a 'mixed' fit; warm,
medians of REPS host-synchronised repetitions (HIP events).  The covariance product is the velocity
predict's GEMM on twice the columns, so 2.0× is what the flop count predicts; the mean-only run
(assemble, mean partials, finalize) shows what the rest costs.  Writes one JSON document
(profiles/grad_timing.json is a run of this tool; DESIGN.md §3.8 quotes it).
usage: python tools/time_grad.py [out.json] [N_train] [grid]"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "2d-gp_amd")]
import numpy as np  # noqa: E402
import torch  # noqa: E402

from gp2d import data as D  # noqa: E402
from gp2d import engine as E  # noqa: E402

OUT = sys.argv[1] if len(sys.argv) > 1 else ""
NTR = int(sys.argv[2]) if len(sys.argv) > 2 else 4096
G = int(sys.argv[3]) if len(sys.argv) > 3 else 256
REPS, WARM, CHUNK = 10, 3, 8192


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
xg = torch.tensor(D.bbox_grid(x1, x2, G, pad=5.0)[2], device="cuda")
res = dict(device=torch.cuda.get_device_name(0), n_train=NTR, grid=[G, G], chunk=CHUNK, reps=REPS, warm=WARM,
           cases=[])
for kind, l_cf, ratio in (("df", 5.0, 1.0), ("mixed", 4.0, 0.35)):
    spec = E.KernelSpec(kind=kind, l_df=5.0, l_cf=l_cf, ratio=ratio)
    gp = E.fit(spec, xt, yt, 0.0025)
    pred = E.Predictor(gp, CHUNK)
    vel, vel_all = timed(lambda: pred(xg))
    vel_mean, _ = timed(lambda: pred(xg, compute_var=False))
    grd, grd_all = timed(lambda: E.predict_gradient(gp, xg, chunk=CHUNK))
    mean_only, _ = timed(lambda: E.predict_gradient(gp, xg, compute_cov=False, chunk=CHUNK))
    res["cases"].append(dict(kind=kind, n=gp.n, predict_f64_ms=round(vel, 4), predict_f64_mean_only_ms=round(vel_mean, 4),
                             predict_gradient_ms=round(grd, 4), predict_gradient_mean_only_ms=round(mean_only, 4),
                             ratio=round(grd / vel, 4),
                             product_ratio=round((grd - mean_only) / (vel - vel_mean), 4),
                             predict_f64_all_ms=vel_all, predict_gradient_all_ms=grd_all))
    print(f"{kind}: predict f64 {vel:.3f} ms (mean only {vel_mean:.3f}), predict_gradient {grd:.3f} ms "
          f"({grd / vel:.3f}×; mean only {mean_only:.3f} ms; products alone "
          f"{(grd - mean_only) / (vel - vel_mean):.3f}×)", flush=True)
txt = json.dumps(res, indent=1)
if OUT:
    os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
    with open(OUT, "w") as f:
        f.write(txt + "\n")
print(txt)
