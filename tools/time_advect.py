"""Time engine.advect beside the route it replaces (dev tool): N_train = 4096, a 'df' fit, 256 × 256
seeds on the data's bounding box, 100 RK4 steps — the fused kernel without and with the tangent, and
the same integration as 400 velocity predicts (a warm engine.Predictor, compute_var=False: K* of a
chunk to memory, a mean pass over it, a finalize, back to Python) combined by torch.  Warm, medians
of REPS host-synchronised repetitions (HIP events); the two routes' final positions are compared.
Writes one JSON document (profiles/advect_timing.json is a run of this tool; DESIGN.md §3.13 quotes
it).
usage: python tools/time_advect.py [out.json] [N_train] [grid] [nsteps]"""
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
NSTEPS = int(sys.argv[4]) if len(sys.argv) > 4 else 100
REPS, WARM, CHUNK = 5, 1, 8192
DT, SAVE_EVERY = 0.1, 10


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
    return float(np.median(ms)), [round(t, 3) for t in ms]


x1, x2, u, v = D.synthetic_tracks(NTR, seed=2016)
xt = torch.tensor(np.stack([x1, x2], 1), device="cuda")
yt = torch.tensor(np.concatenate([u, v]), device="cuda")
x0 = torch.tensor(D.bbox_grid(x1, x2, G, pad=5.0)[2], device="cuda")
m = x0.shape[0]
gp = E.fit(E.KernelSpec(kind="df", l_df=5.0), xt, yt, 0.0025)
pred = E.Predictor(gp, CHUNK)


def velocity(x):
    mu, _ = pred(x, compute_var=False)
    return torch.stack([mu[:m], mu[m:]], 1)


def by_predicts():
    """The parent's route: four predicts per step, the stages combined by torch."""
    x = x0
    for _ in range(NSTEPS):
        k1 = velocity(x)
        k2 = velocity(x + 0.5 * DT * k1)
        k3 = velocity(x + 0.5 * DT * k2)
        k4 = velocity(x + DT * k3)
        x = x + DT / 6.0 * (k1 + 2.0 * k2 + 2.0 * k3 + k4)
    return x


def fused(tangent):
    return E.advect(gp, x0, dt=DT, nsteps=NSTEPS, save_every=SAVE_EVERY, tangent=tangent)


end_fused = fused(False)[1][-1]
diff = float((by_predicts() - end_fused).abs().max())
path_ms, path_all = timed(lambda: fused(False))
tan_ms, tan_all = timed(lambda: fused(True))
pred_ms, pred_all = timed(by_predicts)
pairs = float(m) * NTR * 4 * NSTEPS
res = dict(device=torch.cuda.get_device_name(0), n_train=NTR, seeds=[G, G], nsteps=NSTEPS, dt=DT, save_every=SAVE_EVERY,
           kind="df", chunk=CHUNK, reps=REPS, warm=WARM, pair_evaluations=pairs,
           advect_path_ms=round(path_ms, 3), advect_path_tangent_ms=round(tan_ms, 3),
           predicts_400_ms=round(pred_ms, 3), predicts_over_advect_path=round(pred_ms / path_ms, 3),
           tangent_over_path=round(tan_ms / path_ms, 3),
           pair_evaluations_per_s_path=round(pairs / path_ms * 1e3, 0),
           pair_evaluations_per_s_tangent=round(pairs / tan_ms * 1e3, 0),
           final_position_max_abs_diff=diff,
           advect_path_all_ms=path_all, advect_path_tangent_all_ms=tan_all, predicts_400_all_ms=pred_all)
print(f"advect path {path_ms:.1f} ms, with tangent {tan_ms:.1f} ms ({tan_ms / path_ms:.2f}×); {4 * NSTEPS} predicts "
      f"{pred_ms:.1f} ms ({pred_ms / path_ms:.2f}× the fused path); final positions differ by {diff:.2e}", flush=True)
txt = json.dumps(res, indent=1)
if OUT:
    os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
    with open(OUT, "w") as f:
        f.write(txt + "\n")
print(txt)
