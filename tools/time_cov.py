"""Time the joint posterior covariance (dev tool): N_train = 4096, a 64 × 64 target grid (m = 4096,
q = 8192), a 'df' fit; warm, medians of REPS host-synchronised repetitions (HIP events).
  * postcov_kernel alone (the library's timing hook around it): Σ = K(g, g) − VᵀV on lower tiles;
  * beside it, the same Σ from entries the library already had: gp2d_assemble for K(g, g), then
    engine.gemm(Vᵀ, Vᵀ, transb=True, alpha=−1, C=K, beta=1) (the NT kernel, all q × q tiles);
  * the whole engine.predict_cov and engine.sample_posterior(S = 100).
Writes one JSON document (profiles/cov_timing.json is a run of this tool; DESIGN.md §3.7 quotes it).
usage: python tools/time_cov.py [out.json] [N_train] [grid]"""
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
G = int(sys.argv[3]) if len(sys.argv) > 3 else 64
REPS, WARM, NSAMP = 10, 3, 100


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


def rnd(a):
    return [round(t, 4) for t in a]


x1, x2, u, v = D.synthetic_tracks(NTR, seed=2016)
xt = torch.tensor(np.stack([x1, x2], 1), device="cuda")
yt = torch.tensor(np.concatenate([u, v]), device="cuda")
xg = torch.tensor(D.bbox_grid(x1, x2, G, pad=5.0)[2], device="cuda")
m = xg.shape[0]
spec = E.KernelSpec(kind="df", l_df=5.0)
gp = E.fit(spec, xt, yt, 0.0025)
n, q = gp.n, 2 * E.padded_points(m)

# the kernel alone: one hook reading per repetition
for _ in range(WARM):
    E.predict_cov(gp, xg)
E.timing_enable(True)
E.timing_read()
kern, flops = [], 0.0
for _ in range(REPS):
    mean, cov = E.predict_cov(gp, xg)
    ms, cnt, flops = E.timing_read()
    assert cnt == 1
    kern.append(ms)
E.timing_enable(False)
kern_ms = float(np.median(kern))

# the yardstick: V by the dense NN product (not timed), then assemble + NT GEMM with beta = 1
Kst = E.assemble(spec, gp.x, xg)                       # K*ᵀ, n × 2m (n_train = n_pad here)
assert tuple(Kst.shape) == (n, 2 * m) and m % 64 == 0, "the yardstick needs unpadded sizes"
Vt = E.gemm(gp.W, Kst).t().contiguous()                # Vᵀ, 2m × n
asm_ms, _ = timed(lambda: E.assemble(spec, xg))
Kgg = E.assemble(spec, xg)
gemm_ms, _ = timed(lambda: E.gemm(Vt, Vt, transb=True, alpha=-1.0, C=Kgg, beta=1.0))
yard_ms, yard_all = timed(lambda: E.gemm(Vt, Vt, transb=True, alpha=-1.0, C=E.assemble(spec, xg), beta=1.0))
ref = E.gemm(Vt, Vt, transb=True, alpha=-1.0, C=Kgg, beta=1.0)
scale = float(ref.abs().max())
diff = float((ref - cov).abs().max()) / scale
del Kst, Vt, Kgg, ref

whole_ms, whole_all = timed(lambda: E.predict_cov(gp, xg))
info = {}


def draw():
    info.update(E.sample_posterior(gp, xg, NSAMP, seed=1)[1])


samp_ms, samp_all = timed(draw)

res = dict(device=torch.cuda.get_device_name(0), n_train=NTR, grid=[G, G], n=n, q=q, reps=REPS, warm=WARM,
           flop=flops, postcov_kernel_ms=round(kern_ms, 4), postcov_kernel_tflops=round(flops / kern_ms / 1e9, 2),
           postcov_kernel_all_ms=rnd(kern),
           yardstick_ms=round(yard_ms, 4), yardstick_assemble_ms=round(asm_ms, 4), yardstick_gemm_ms=round(gemm_ms, 4),
           yardstick_all_ms=yard_all, kernel_over_yardstick=round(kern_ms / yard_ms, 4),
           max_abs_diff_over_max=diff,
           predict_cov_ms=round(whole_ms, 4), predict_cov_all_ms=whole_all,
           sample_posterior_ms=round(samp_ms, 4), sample_posterior_all_ms=samp_all, samples=NSAMP,
           sample_jitter=info.get("jitter"), sample_tries=info.get("tries"))
print(f"postcov_kernel {kern_ms:.3f} ms ({flops / kern_ms / 1e9:.1f} TF/s); yardstick {yard_ms:.3f} ms "
      f"(assemble {asm_ms:.3f} + gemm {gemm_ms:.3f}); predict_cov {whole_ms:.3f} ms; "
      f"sample_posterior(S={NSAMP}) {samp_ms:.3f} ms; kernel vs yardstick max diff {diff:.2e}", flush=True)
txt = json.dumps(res, indent=1)
if OUT:
    os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
    with open(OUT, "w") as f:
        f.write(txt + "\n")
print(txt)
