"""Time engine.draw_flows and engine.advect_draws beside engine.advect (dev tool): N_train = 4096, a
'df' fit, S = 64 draws × 1024 particles on the data's bounding box, 100 RK4 steps, one n_features per
invocation (so every configuration runs under a time limit of its own).  The yardstick is
engine.advect of the same fit on S·m = 65,536 particles: the parent's kernel doing the training-point
half of the same work.  Warm, medians of REPS host-synchronised repetitions (HIP events);
draw_flows (host table and noise draws, upload, f_s(X), the two products with W) and advect_draws
are timed separately.  The result is appended to the JSON document's "runs"
(profiles/paths_timing.json is three runs of this tool; DESIGN.md §3.14 quotes it).
usage: python tools/time_paths.py [out.json] [n_features] [N_train] [draws] [particles] [nsteps]"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "2d-gp_amd")]
import numpy as np  # noqa: E402
import torch  # noqa: E402

from gp2d import data as D  # noqa: E402
from gp2d import engine as E  # noqa: E402
from gp2d import paths as P  # noqa: E402

OUT = sys.argv[1] if len(sys.argv) > 1 else ""
NFEAT = int(sys.argv[2]) if len(sys.argv) > 2 else 1024
NTR = int(sys.argv[3]) if len(sys.argv) > 3 else 4096
S = int(sys.argv[4]) if len(sys.argv) > 4 else 64
M = int(sys.argv[5]) if len(sys.argv) > 5 else 1024
NSTEPS = int(sys.argv[6]) if len(sys.argv) > 6 else 100
REPS, WARM = 10, 1
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
g = int(np.ceil(np.sqrt(M)))
x0 = torch.tensor(D.bbox_grid(x1, x2, g, pad=5.0)[2][:M], device="cuda")
gp = E.fit(E.KernelSpec(kind="df", l_df=5.0), xt, yt, 0.0025)
x_all = x0.repeat(S, 1)   # the yardstick's S·m particles

table = P.feature_table(gp.kernel, S, NFEAT, seed=1)
eps = P.noise_draws(S, 2 * NTR, 0.0025, seed=1)
draws = E.draw_flows(gp, S, features=table, eps=eps)
kw = dict(dt=DT, nsteps=NSTEPS, save_every=SAVE_EVERY)
end = E.advect_draws(draws, x0, **kw)[1][-1]
mean_end = E.advect(gp, x0, **kw)[1][-1]
spread = float((end - mean_end[None]).norm(dim=-1).mean())

host_ms, _ = timed(lambda: (P.feature_table(gp.kernel, S, NFEAT, seed=1), P.noise_draws(S, 2 * NTR, 0.0025, seed=1)))
draw_ms, draw_all = timed(lambda: E.draw_flows(gp, S, features=table, eps=eps))
seeded_ms, _ = timed(lambda: E.draw_flows(gp, S, n_features=NFEAT, seed=1))
adv_ms, adv_all = timed(lambda: E.advect_draws(draws, x0, **kw))
mean_ms, mean_all = timed(lambda: E.advect(gp, x_all, **kw))
evals = float(S) * M * 4 * NSTEPS               # velocity evaluations
pairs, feats = evals * NTR, evals * draws.features.shape[1]
pair_ns = mean_ms * 1e6 / pairs                 # one training pair, from the yardstick
feat_ns = (adv_ms - mean_ms) * 1e6 / feats      # one feature, from what the draws add to it
run = dict(n_features=NFEAT, features_per_draw=int(draws.features.shape[1]), draw_flows_ms=round(draw_ms, 3),
           draw_flows_seeded_ms=round(seeded_ms, 3), host_table_and_noise_ms=round(host_ms, 3),
           advect_draws_ms=round(adv_ms, 3), advect_mean_flow_ms=round(mean_ms, 3),
           advect_draws_over_mean_flow=round(adv_ms / mean_ms, 3), pair_evaluation_ns=round(pair_ns, 6),
           feature_evaluation_ns=round(feat_ns, 6), feature_over_pair=round(feat_ns / pair_ns, 3),
           mean_distance_from_mean_flow_path=spread, draw_flows_all_ms=draw_all, advect_draws_all_ms=adv_all,
           advect_mean_flow_all_ms=mean_all)
print(f"n_features {NFEAT}: draw_flows {draw_ms:.1f} ms (seeded, with the host generators {seeded_ms:.1f} ms), advect_draws "
      f"{adv_ms:.1f} ms, engine.advect of {S * M} particles {mean_ms:.1f} ms ({adv_ms / mean_ms:.2f}×); one feature "
      f"{feat_ns / pair_ns:.2f} training pairs", flush=True)
doc = dict(device=torch.cuda.get_device_name(0), n_train=NTR, draws=S, particles=M, nsteps=NSTEPS, dt=DT,
           save_every=SAVE_EVERY, kind="df", reps=REPS, warm=WARM, runs=[])
if OUT and os.path.exists(OUT):
    with open(OUT) as f:
        old = json.load(f)
    if all(old.get(k) == doc[k] for k in doc if k != "runs"):
        doc["runs"] = [r for r in old.get("runs", []) if r.get("n_features") != NFEAT]
doc["runs"] = sorted(doc["runs"] + [run], key=lambda r: r["n_features"])
txt = json.dumps(doc, indent=1)
if OUT:
    os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
    with open(OUT, "w") as f:
        f.write(txt + "\n")
print(txt)
