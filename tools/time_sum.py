"""Time a kernel sum (engine family 'vector_sum') beside the single kernel on the headline problem
(dev tool): N_train = 4096, a 256 × 256 grid, FP64 engine; K_y assembly, fit, FP64 predict and
LML + gradient for the single mixed kernel and for sums of T = 1, 2, 3 mixed terms; warm, medians
of REPS host-synchronised repetitions (HIP events).  Only the K_y assembly, the K* assembly (inside
the predict) and the gradient's pair kernel evaluate the kernel, so only they are expected to grow
with T; the factor and the variance GEMM never see it.  Writes one JSON document
(profiles/sum_timing.json is a run of this tool; DESIGN.md §3.10 quotes it).
usage: python tools/time_sum.py [out.json] [N_train] [grid]"""
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
NOISE = 0.0025
# one term per flow scale: (l_df, l_cf, ratio, weight)
TERMS = ((8.0, 8.0, 0.6, 1.0), (2.0, 3.0, 0.5, 0.05), (1.0, 1.5, 0.5, 0.02))


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


def term(i):
    l_df, l_cf, ratio, _ = TERMS[i]
    return E.KernelSpec(kind="mixed", l_df=l_df, l_cf=l_cf, ratio=ratio)


x1, x2, u, v = D.synthetic_tracks(NTR, seed=2016)
xt = torch.tensor(np.stack([x1, x2], 1), device="cuda")
yt = torch.tensor(np.concatenate([u, v]), device="cuda")
xg = torch.tensor(D.bbox_grid(x1, x2, G, pad=5.0)[2], device="cuda")
res = dict(device=torch.cuda.get_device_name(0), n_train=NTR, grid=[G, G], chunk=CHUNK, reps=REPS, warm=WARM,
           noise=NOISE, terms=[dict(zip(("l_df", "l_cf", "ratio", "weight"), t)) for t in TERMS], cases=[])
specs = [("single", term(0))]
for T in (1, 2, 3):
    specs.append((f"sum_T{T}", E.KernelSpec(family="vector_sum", terms=tuple(term(i) for i in range(T)),
                                             weights=tuple(TERMS[i][3] for i in range(T)))))
dev = torch.device("cuda")
for name, spec in specs:
    st = E._stage_problem(spec, xt, "f64", dev)
    A = torch.empty((st.n, st.n), dtype=torch.float64, device=dev)
    asm, asm_all = timed(lambda: E._assemble_ky(st, NOISE, A, dev))
    fit_ms, fit_all = timed(lambda: E.fit(spec, xt, yt, NOISE))
    gp = E.fit(spec, xt, yt, NOISE)
    pred = E.Predictor(gp, CHUNK)
    prd, prd_all = timed(lambda: pred(xg))
    mean_only, _ = timed(lambda: pred(xg, compute_var=False))     # K* assembly + the mean: no variance GEMM
    lml, lml_all = timed(lambda: E.lml_device(gp, eval_gradient=True))
    res["cases"].append(dict(kernel=name, n=gp.n, assemble_ky_ms=round(asm, 4), fit_ms=round(fit_ms, 4),
                             predict_f64_ms=round(prd, 4), predict_mean_only_ms=round(mean_only, 4),
                             lml_grad_ms=round(lml, 4), assemble_ky_all_ms=asm_all, fit_all_ms=fit_all,
                             predict_f64_all_ms=prd_all, lml_grad_all_ms=lml_all))
    print(f"{name}: assemble K_y {asm:.3f} ms, fit {fit_ms:.3f} ms, predict f64 {prd:.3f} ms "
          f"(mean only {mean_only:.3f} ms), LML + gradient {lml:.3f} ms", flush=True)
    del gp, pred, A
txt = json.dumps(res, indent=1)
if OUT:
    os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
    with open(OUT, "w") as f:
        f.write(txt + "\n")
print(txt)
