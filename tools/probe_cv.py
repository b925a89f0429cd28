"""Time the cross-validation entries at the headline fit (dev tool): N_train = 4096 (n = 8192), a
mixed-kernel fit; medians of 20 runs after 3 warm-ups, HIP events on the stream.
  * gp2d_cv_points (the C entry on preallocated buffers) and its achieved bytes/s against the
    8·n²/2 bytes of W's lower triangle; engine.cv_points (with its host read of the summary);
  * gp2d_cv_groups for 64 groups of 64 points (randomly interleaved labels), and engine.cv_groups;
  * beside them what they replace: one engine.fit of the same size (the same code as before these
    entries existed), times 4096 (one refit per held-out fix) and times 64 (per held-out drifter).
Writes one JSON document (profiles/cv_timing.json is a run of this tool; DESIGN.md §3.9 quotes it).
usage: python tools/probe_cv.py [out.json] [N_train] [variance]"""
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
VARIANCE = sys.argv[3] if len(sys.argv) > 3 else "ozaki"
REPS, WARM, NGROUPS = 20, 3, 64


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
fit_ms, fit_all = timed(lambda: E.fit(spec, xt, yt, 0.0025, variance=VARIANCE))
gp = E.fit(spec, xt, yt, 0.0025, variance=VARIANCE)
L, dev = N.lib(), gp.device
bd, ntr, npad, n = 2, gp.n_train, gp.n_pad, gp.n
s = E._stream_handle(dev)
perm = None if gp.perm is None else E._ptr(gp.perm)


def buf(k, dtype=torch.float64):
    return torch.empty(k, dtype=dtype, device=dev)


# ---- leave one point out
mean, var, cuv, lpd, summ = buf(bd * ntr), buf(bd * ntr), buf(ntr), buf(ntr), buf(4)
wb = int(L.gp2d_cv_points_workspace(n))
work = E._workspace(wb, dev)


def c_points():
    N.check(L.gp2d_cv_points(E._ptr(gp.W), n, n, E._ptr(gp.alpha), E._ptr(gp.y), ntr, npad, bd, perm, E._ptr(mean),
                             E._ptr(var), E._ptr(cuv), E._ptr(lpd), E._ptr(summ), E._ptr(work), wb, s), "cv_points")


pts_ms, pts_all = timed(c_points)
epts_ms, epts_all = timed(lambda: E.cv_points(gp))
tri_bytes = 8.0 * n * n / 2.0
del work

# ---- leave a group out: 64 groups of NTR / 64 points
per = ntr // NGROUPS
labels = np.random.default_rng(5).permutation(np.arange(NGROUPS * per) % NGROUPS)
labels = np.concatenate([labels, np.full(ntr - NGROUPS * per, -1)]).astype(np.int64)
lab_fit = labels if gp.perm is None else labels[gp.perm.cpu().numpy()]   # the fit's point i is input point perm[i]
held = np.flatnonzero(lab_fit >= 0)
order = held[np.argsort(lab_fit[held], kind="stable")]
gstart = (np.arange(NGROUPS + 1) * per).astype(np.int64)
gidx = torch.as_tensor(order.astype(np.int64), device=dev)
qpad = (bd * per + 127) // 128 * 128
lpdg, info = buf(NGROUPS), buf(NGROUPS, torch.int32)
wbg = int(L.gp2d_cv_groups_workspace(n, qpad, NGROUPS))
workg = E._workspace(wbg, dev)


def c_groups():
    N.check(L.gp2d_cv_groups(E._ptr(gp.W), n, n, E._ptr(gp.alpha), E._ptr(gp.y), ntr, npad, bd,
                             gstart.ctypes.data_as(ctypes.c_void_p), E._ptr(gidx), NGROUPS, perm, E._ptr(mean),
                             E._ptr(var), E._ptr(lpdg), E._ptr(info), E._ptr(workg), wbg, s), "cv_groups")


grp_ms, grp_all = timed(c_groups)
assert not bool(info.any())
del workg
egrp_ms, egrp_all = timed(lambda: E.cv_groups(gp, labels))

res = dict(device=torch.cuda.get_device_name(0), n_train=NTR, n=n, variance=VARIANCE, reps=REPS, warm=WARM,
           fit_ms=round(fit_ms, 4), fit_all_ms=fit_all,
           cv_points_ms=round(pts_ms, 4), cv_points_all_ms=pts_all, lower_triangle_bytes=tri_bytes,
           cv_points_gbytes_per_s=round(tri_bytes / pts_ms / 1e6, 1),
           engine_cv_points_ms=round(epts_ms, 4), engine_cv_points_all_ms=epts_all,
           refits_per_point_ms=round(fit_ms * ntr, 1), cv_points_over_one_fit=round(pts_ms / fit_ms, 4),
           groups=NGROUPS, points_per_group=per, q_pad=qpad, cv_groups_workspace_bytes=wbg,
           cv_groups_ms=round(grp_ms, 4), cv_groups_all_ms=grp_all,
           engine_cv_groups_ms=round(egrp_ms, 4), engine_cv_groups_all_ms=egrp_all,
           refits_per_group_ms=round(fit_ms * NGROUPS, 1), cv_groups_over_one_fit=round(grp_ms / fit_ms, 4))
print(f"fit {fit_ms:.3f} ms; cv_points {pts_ms:.3f} ms ({tri_bytes / pts_ms / 1e6:.0f} GB/s of W's lower triangle), "
      f"engine {epts_ms:.3f} ms, vs {ntr} refits {fit_ms * ntr / 1e3:.1f} s; cv_groups {grp_ms:.3f} ms, engine "
      f"{egrp_ms:.3f} ms, vs {NGROUPS} refits {fit_ms * NGROUPS:.1f} ms", flush=True)
txt = json.dumps(res, indent=1)
if OUT:
    os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
    with open(OUT, "w") as f:
        f.write(txt + "\n")
print(txt)
