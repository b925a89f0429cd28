"""Device-resident GP engine: fit (assemble → POTRF → TRTRI → α) and predict.

Host orchestration over the C ABI of libgp2d.so.  torch-ROCm tensors are used
only as device-memory containers and for the current HIP stream; every FLOP runs
in the hand-written HIP kernels.

Reference call sites replaced:
  * GP_laser.laser  GP_laser.py:113-140  (K, +noise·I, inv, Ks, mean, var)
  * GPy GPRegression fit / model.predict  krig.py:411, :543-544
  * sklearn GaussianProcessRegressor fit / predict(return_std)  krig.py:182-194
"""
from __future__ import annotations

import collections
import contextlib
import os
import ctypes
import itertools
import math
import time
from dataclasses import dataclass, field

import numpy as np
import torch

from . import _native as N

NB = 128


def _stream_handle(device) -> ctypes.c_void_p:
    return ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def _ptr(t: torch.Tensor) -> ctypes.c_void_p:
    return ctypes.c_void_p(t.data_ptr())


def _workspace(nbytes: int, device) -> torch.Tensor:
    """Device scratch of at least `nbytes` bytes (the library's *_workspace counts), 8-byte aligned."""
    return torch.empty(nbytes // 8 + 1, dtype=torch.float64, device=device)


def _require_device(device=None) -> torch.device:
    if not torch.cuda.is_available():
        raise N.NativeLibraryError("gp2d needs a HIP device (torch.cuda.is_available() is False); "
                                   "there is no CPU fallback")
    N.lib()
    dev = torch.device(device if device is not None else "cuda")
    warm_streams(dev)
    return dev


_WARM = set()


def warm_streams(device=None):
    """Bind the current (predict) stream and then the library's internal factorisation streams
    to their hardware queues, once per device (gp2d_factor_warm).  HIP binds a stream to a queue
    at its first command; a job stream ran 53.1–53.9 ms per headline job with the predict stream,
    the factor streams and the side streams first used in that order, and 56.4–56.7 ms in the
    other orders measured (tools/probe_first_fit.py, DESIGN.md §6 "bench state").  Every device
    entry point of the engine calls it (through _require_device) before it touches a stream of
    its own; a caller that uses its own side streams before any gp2d call should call it first."""
    dev = torch.device(device if device is not None else "cuda")
    idx = dev.index if dev.index is not None else torch.cuda.current_device()
    if idx in _WARM:
        return
    with torch.cuda.device(idx):
        N.check(N.lib().gp2d_factor_warm(1, ctypes.c_void_p(torch.cuda.current_stream(idx).cuda_stream)),
                "gp2d_factor_warm")
    _WARM.add(idx)


def morton_sort(P: torch.Tensor):
    """(order, P[order]) for device points (N, d), d ∈ {2, 3}: the Z-order (Morton) curve of
    their bounding box (21 bits per coordinate), sorted by a stable device radix sort and
    gathered on the device (gp2d_morton_sort; equal codes keep their input order, so the
    permutation is deterministic).  The ozaki engine orders training and grid points this way so
    that 64 consecutive training points and 256 consecutive grid points are spatially compact:
    K* tiles of far-apart groups are then exactly zero and the int8 GEMMs skip them
    (csrc/ozaki.hpp, ozaki_slab_list_kernel).  Other shapes: (None, P) — no reordering."""
    n, d = P.shape
    if n < 1 or d not in (2, 3):
        return None, P
    P = P.contiguous()
    L = N.lib()
    wb = int(L.gp2d_morton_sort_workspace(n))
    work = torch.empty(wb, dtype=torch.uint8, device=P.device)
    order = torch.empty(n, dtype=torch.int64, device=P.device)
    out = torch.empty_like(P)
    N.check(L.gp2d_morton_sort(_ptr(P), n, d, _ptr(out), _ptr(order), _ptr(work), wb, _stream_handle(P.device)),
            "gp2d_morton_sort")
    return order, out


def morton_order(P: torch.Tensor) -> torch.Tensor:
    """The permutation of morton_sort (sorted point j is P[order[j]])."""
    order, _ = morton_sort(P)
    if order is None:
        raise ValueError("morton_order: points must be (N, 2) or (N, 3) with N ≥ 1")
    return order


def side_stream(device=None) -> torch.cuda.Stream:
    """A stream for work that has to overlap the current (predict) stream — a job's fit, a
    broadcast, concurrent settings.  Taken from torch's HIGH-priority pool: HIP maps streams
    onto at most GPU_MAX_HW_QUEUES hardware queues per priority level (4 on the box), and two
    streams that share a queue run in order, so a side stream on the current stream's queue
    overlaps nothing.  torch's normal-priority pool streams can land there (tools/probe_queues.py (git f1195df):
    pool streams 6 and 10 of 12 did, profiles/r03_queue_aliasing.json); the high-priority pool is
    a different set of queues."""
    return torch.cuda.Stream(device, priority=-1)


def _as_points(x, dim: int, device) -> torch.Tensor:
    if isinstance(x, torch.Tensor):
        t = x.to(device=device, dtype=torch.float64)
    else:
        t = torch.as_tensor(np.ascontiguousarray(np.asarray(x, dtype=np.float64)), device=device)
    return t.reshape(-1, dim).contiguous()


@dataclass
class KernelSpec:
    """Hyperparameters of the covariance function.

    family 'vector2d' (the reference's div-free / curl-free SE kernels):
        kind 'df' | 'cf' | 'mixed' | 'scalar' (divFree 1 | 2 | mixed | 0),
        l_df, l_cf, ratio  (myKernel.py:13-22; GP_laser.py:16 `l_df, l_cf, rate`)
    family 'ard' (the sklearn model of krig.scikit_prior, krig.py:174-180):
        variances (1-2 terms), lengthscales (per term, 1-3 dims)
    family 'vector_st' (SURVEY.md §8f item 2): the spatio-temporal product
        Kt(var_t, l_t) × (the vector2d kernel of `kind`) on (T, Y, X) points — GPy
        `Kt(...) * nonDivK(2, [1, 2], ℓ)` (scratch.py:506-508; Kt myKernel.py:337-363),
        standing in for the reference's missing myKernel2 (krig.py:397-404)
    family 'vector_sum': Σ_t weights[t]·terms[t], 1-3 terms that are all 'vector2d' or all
        'vector_st' (kinds may differ) — the reference's k = k2 + k2 + … (krig.py:405-407), one term
        per flow scale.  FP64 engine only.  term(t) is the one-term sum (w_t, term t): as a
        predict's kernel on the sum's fit it gives the posterior of term t's contribution alone.
    """
    family: str = "vector2d"
    kind: str = "df"
    l_df: float = 5.0
    l_cf: float = 5.0
    ratio: float = 1.0
    variances: tuple = ()
    lengthscales: tuple = ()
    var_t: float = 1.0
    l_t: float = 1.0
    terms: tuple = ()
    weights: tuple = ()

    _KINDS = {"scalar": N.KIND_SCALAR, "df": N.KIND_DIVFREE, "cf": N.KIND_CURLFREE, "mixed": N.KIND_MIXED,
              0: N.KIND_SCALAR, 1: N.KIND_DIVFREE, 2: N.KIND_CURLFREE, 3: N.KIND_MIXED}

    @property
    def is_sum(self) -> bool:
        return self.family == "vector_sum"

    def _sum_terms(self) -> tuple:
        """The terms of a sum, checked: 1..3, one vector family, one weight each."""
        terms, weights = tuple(self.terms), tuple(self.weights)
        if not 1 <= len(terms) <= N.SUM_MAX_TERMS:
            raise ValueError(f"a kernel sum has 1..{N.SUM_MAX_TERMS} terms")
        if len(weights) != len(terms):
            raise ValueError("a kernel sum needs one weight per term")
        fams = {t.family for t in terms}
        if len(fams) != 1 or not fams <= {"vector2d", "vector_st"}:
            raise ValueError("the terms of a kernel sum must be all 'vector2d' or all 'vector_st'")
        return terms

    def term(self, t: int) -> "KernelSpec":
        """The one-term sum (w_t, term t) of a sum: the kernel of term t's posterior (predict(term=t))."""
        terms = self._sum_terms()
        if not 0 <= int(t) < len(terms):
            raise ValueError(f"term must be in 0..{len(terms) - 1}")
        return KernelSpec(family="vector_sum", terms=(terms[int(t)],), weights=(float(self.weights[int(t)]),))

    def desc(self):
        """The library's descriptor: one KernelDesc, or a sum's (KernelDesc * (1 + T)) array; both
        pass by ctypes.byref."""
        if self.family == "vector_sum":
            return N.vector_sum_kernel_desc([t.desc() for t in self._sum_terms()], self.weights)
        if self.family == "vector2d":
            return N.vector_kernel_desc(self._KINDS[self.kind], self.l_df, self.l_cf, self.ratio)
        if self.family == "ard":
            return N.ard_kernel_desc(self.variances, self.lengthscales)
        if self.family == "vector_st":
            return N.vector_st_kernel_desc(self._KINDS[self.kind], self.l_df, self.l_cf, self.ratio, self.var_t,
                                           self.l_t)
        raise ValueError(f"unknown kernel family {self.family!r}")

    @property
    def is_vector(self) -> bool:
        return self.family in ("vector2d", "vector_st", "vector_sum")

    @property
    def block_dim(self) -> int:
        return 2 if self.is_vector else 1

    @property
    def input_dim(self) -> int:
        if self.family == "vector_sum":
            return self._sum_terms()[0].input_dim
        if self.family == "vector2d":
            return 2
        return 3 if self.family == "vector_st" else len(self.lengthscales[0])

    def kdiag(self) -> float:
        return float(N.lib().gp2d_kernel_diag(ctypes.byref(self.desc())))

    def field_prior_var(self, field: str) -> float:
        """Prior variance of a derived field (FIELDS) under this kernel: Var δ = 8·w_cf/ℓ_cf⁴,
        Var ζ = 8·w_df/ℓ_df⁴, times var_t for 'vector_st' (gp2d_field_prior_var); 0 where the
        field vanishes by kind.  ValueError for the scalar kind and the ARD family."""
        return float(N.lib().gp2d_field_prior_var(ctypes.byref(self.desc()), _field_code(self, field)))

    def grad_prior_cov(self) -> np.ndarray:
        """(4, 4) prior covariance of the velocity gradient tensor at one point, components
        GRADIENT_COMPONENTS (gp2d_grad_prior_cov): singular along the divergence for 'df' and along
        the vorticity for 'cf'.  ValueError for the scalar kind and the ARD family."""
        _refuse_sum(self, "grad_prior_cov")
        _require_velocity(self, "the velocity gradient needs a div-free, curl-free or mixed vector kernel "
                                "(the scalar kind and the ARD family have none)")
        out = (ctypes.c_double * 16)()
        N.check(N.lib().gp2d_grad_prior_cov(ctypes.byref(self.desc()), out), "gp2d_grad_prior_cov")
        return np.array(out, dtype=np.float64).reshape(4, 4)


def padded_points(n: int) -> int:
    return int(N.lib().gp2d_padded_points(int(n)))


def assemble(kernel: KernelSpec, xa, xb=None, diag_add: float = 0.0, device=None) -> torch.Tensor:
    """Covariance matrix K(xa, xb) on the device, exactly as the reference lays it out
    ((bd·Na) × (bd·Nb) component-major; no padding in the returned tensor)."""
    dev = _require_device(device)
    d = kernel.input_dim
    bd = kernel.block_dim
    A = _as_points(xa, d, dev)
    sym = xb is None
    B = A if sym else _as_points(xb, d, dev)
    na, nb = A.shape[0], B.shape[0]
    nap, nbp = padded_points(na), padded_points(nb)
    out = torch.empty((bd * nap, bd * nbp), dtype=torch.float64, device=dev)
    desc = kernel.desc()
    N.check(N.lib().gp2d_assemble(_ptr(A), na, nap, _ptr(B), nb, nbp, ctypes.byref(desc), float(diag_add),
                                  int(sym), _ptr(out), out.shape[1], _stream_handle(dev)), "gp2d_assemble")
    if bd == 1:
        return out[:na, :nb]
    idx_r = torch.cat([torch.arange(na, device=dev), nap + torch.arange(na, device=dev)])
    idx_c = torch.cat([torch.arange(nb, device=dev), nbp + torch.arange(nb, device=dev)])
    return out.index_select(0, idx_r).index_select(1, idx_c)


@dataclass
class GPFit:
    """A fitted GP resident in HBM: W = L⁻¹ (n×n), α = K_y⁻¹y, training points."""
    kernel: KernelSpec
    noise: float
    x: torch.Tensor          # (N, dim) device
    n_train: int
    n_pad: int               # padded point count
    W: torch.Tensor          # (n, n) lower-triangular inverse Cholesky factor
    alpha: torch.Tensor      # (n,)
    device: torch.device
    info: int = 0
    extra: dict = field(default_factory=dict)
    y: torch.Tensor = None   # (n,) padded observations (LML)
    perm: torch.Tensor = None  # ozaki engine: x = x_input[perm] (Morton order; α, W follow x)
    pending: tuple = None      # fit(check=False): (pinned status copy, its event, prepare error)
    n_mat: int = 0             # matrix order when W is None (a job stream's receiving rank keeps
    #                            only the INT8 planes, distributed.broadcast_fit)

    def check(self) -> "GPFit":
        """Raise what fit(check=False) deferred: LinAlgError for a non-SPD K_y (waits only
        for the factor's status word, not for later work on the stream), then apply the ozaki
        engine's accuracy guard (apply_guard) with the statistics that travel in the same word.
        Call it before the fit's predict is queued: the guard may re-prepare the planes."""
        if self.pending is not None:
            host, ev, err = self.pending
            self.pending = None
            ev.synchronize()
            try:
                _settle(self, host, err)
            finally:
                _PINNED_STATUS.append(host)
        return _settle_trend(self)

    def record_stream(self, stream) -> "GPFit":
        """Mark the fit's device tensors as in use on `stream` — for a fit made on one stream
        and predicted on another: the caching allocator then keeps their memory until the
        work queued on `stream` when they are freed has finished."""
        oz = self.extra.get("ozaki", ())
        tr = self.extra.get("trend") or {}
        for t in (self.x, self.W, self.alpha, self.y, self.perm, *oz[:2], tr.get("block")):
            if isinstance(t, torch.Tensor) and t.is_cuda:
                t.record_stream(stream)
        return self

    @property
    def n(self) -> int:
        return self.W.shape[0] if self.W is not None else self.n_mat

    def ready_on(self, stream) -> "GPFit":
        """Make `stream` wait for the work the accuracy guard queued in check() (re-prepared
        planes, or W unpacked for the FP64 engine), if any."""
        g = self.extra.get("guard")
        ev = g.pop("event", None) if g else None
        if ev is not None:
            stream.wait_event(ev)
        return self


def _pad_obs(y, n_train: int, n_pad: int, bd: int, device, perm: torch.Tensor | None = None) -> torch.Tensor:
    """The fit's observation vector [u(n_pad), v(n_pad)] with zeros for the padded points, in the
    order of perm (sorted point i is input point perm[i]) — gp2d_obs_pad on the device."""
    if isinstance(y, torch.Tensor):
        yt = y.to(device=device, dtype=torch.float64).reshape(-1)
    else:
        yt = torch.as_tensor(np.asarray(y, dtype=np.float64).reshape(-1), device=device)
    if yt.numel() != bd * n_train:
        raise ValueError(f"observation vector has {yt.numel()} entries, expected {bd * n_train}")
    yt = yt.contiguous()
    out = torch.empty(bd * n_pad, dtype=torch.float64, device=device)
    N.check(N.lib().gp2d_obs_pad(_ptr(yt), n_train, n_pad, bd, None if perm is None else _ptr(perm), _ptr(out),
                                 _stream_handle(device)), "gp2d_obs_pad")
    return out


VARIANCE_ENGINES = ("f64", "ozaki")
ASSEMBLE_LOWER = 2   # gp2d_assemble's symmetric mode: K_y's lower block triangle only

# fit: the two-call gp2d_potrf + gp2d_trtri sequence, or gp2d_potrf_inv (the left half of the
# inverse and the top-level T = L21·W11 issued under the second half of the factorisation).
# Bit-identical results; measured a wash at N = 4096 (the concurrent GEMMs slow the POTRF
# critical path by what they save: 13.5 ms either way), so off by default.
FUSED_INVERSE = False


def fit_layout(kernel: KernelSpec, n_train: int, variance: str = "f64"):
    """(padded point count, matrix order n) of a fit: points padded to 64, n a multiple of
    128 (of 256 for the ozaki engine, whose int8 GEMM tiles are 256 wide)."""
    bd = kernel.block_dim
    npad = padded_points(n_train)
    n = bd * npad
    if n % NB:  # scalar (ARD) family: the matrix order itself must be a multiple of 128
        npad = (npad + NB - 1) // NB * NB
        n = bd * npad
    if variance == "ozaki" and n % 256:
        npad = (npad + 127) // 128 * 128
        n = bd * npad
    return npad, n


# pinned 3-double status slots for fit(check=False) (see status_block), reused after
# GPFit.check(), so the steady state allocates no pinned memory
_PINNED_STATUS: list = []


def status_block(device) -> tuple:
    """A fit's device status word: 3 doubles — [0] holds the LAPACK-style info as an int32 in its
    low bytes (gp2d_potrf writes it there through the returned int32 view), [1:3] the accuracy
    guard's statistics (gp2d_ozaki_guard: min latent variance at the observations, max |W|;
    NaN when the fit ran no guard — apply_guard then keeps the default precision, so a receiving
    rank never acts on stale bytes).  One copy to the host (or one broadcast) carries all of it."""
    st = torch.empty(3, dtype=torch.float64, device=device)
    return st, st.view(torch.int32)[0:1]


def _raise_fit_errors(inf: int, err):
    if inf < 0:   # a status word from the job stream: the fit raised on its owner's host
        if err is not None:
            raise err
        raise RuntimeError("the fit failed on the rank that owned it (see that rank's error)")
    if inf != 0:
        raise np.linalg.LinAlgError(
            f"K_y is not positive definite (leading minor of order {inf}); "
            "increase the noise / jitter (cf. sklearn _gpr.py:350-358)")
    if err is not None:
        raise err


def pending_status(status: torch.Tensor, err=None) -> tuple:
    """A GPFit.pending triple for a device status block (status_block; info < 0: failed on
    another rank): copied to pinned host memory after the work queued so far on the current
    stream, checked by GPFit.check()."""
    host = _PINNED_STATUS.pop() if _PINNED_STATUS else torch.empty(3, dtype=torch.float64, pin_memory=True)
    host.copy_(status, non_blocking=True)
    ev = torch.cuda.Event()
    ev.record(torch.cuda.current_stream(status.device))
    return host, ev, err


# The accuracy the guard holds the int8 variance to: north_star's fp64 posterior gate (1e-10
# relative), elementwise.
GUARD_TARGET = 1e-10
OZAKI_DEFAULT_BITS = (49, 45)   # (W, K*) integer bits: csrc/ozaki.hpp OZ_PW, OZ_PB
OZAKI_MAX_BITS = (60, 50)       # OZ_PW_MAX, OZ_PB_MAX
# fit(guard=None) default; GP2D_GUARD=0 turns the guard off (dev A/Bs only, tools/runs)
GUARD_DEFAULT = os.environ.get("GP2D_GUARD", "1") != "0"


def _guard_stats(W: torch.Tensor, n: int, ntr: int, npad: int, diag_add: float, status: torch.Tensor, dev):
    """gp2d_ozaki_guard into status[1:3] (status_block) on the current stream."""
    L = N.lib()
    wb = int(L.gp2d_ozaki_guard_workspace(n))
    work = torch.empty(wb, dtype=torch.uint8, device=dev)
    N.check(L.gp2d_ozaki_guard(_ptr(W), n, W.stride(0), ntr, npad, float(diag_add),
                               ctypes.c_void_p(status.data_ptr() + 8), _ptr(work), wb, _stream_handle(dev)),
            "gp2d_ozaki_guard")


def apply_guard(gp: GPFit, vmin: float, wmax: float) -> GPFit:
    """The ozaki engine's accuracy guard, once the fit's statistics are on the
    host: the variance's elementwise error grows as the posterior variance falls against kss,
    ≈ A·2^(49 − wbits)·X^1.5 + B·2^(45 − kbits)·X with X = kss / v_min (gp2d_ozaki_error_model;
    v_min: the smallest latent posterior variance at the observations, exact from W).  The cheapest
    W / K* precisions (wbits 49..60, kbits 45..50) that keep the model within GUARD_TARGET are
    taken — the planes re-prepared on the fit's stream when that is more than the defaults — or,
    past them, the fit switches to the FP64 engine.  The decision is in gp.extra['guard']:
    engine, wbits, kbits, vmin_over_kss, wmax, est."""
    g = gp.extra.get("guard")
    if not g or not g.get("pending"):
        return gp
    if math.isnan(vmin):   # the owner's fit ran no guard (status_block's sentinel): default precision
        g.pop("stream", None)
        gp.extra.pop("packed", None)
        g.update(pending=False, engine="ozaki", wbits=OZAKI_DEFAULT_BITS[0], kbits=OZAKI_DEFAULT_BITS[1],
                 vmin_over_kss=None, wmax=None, est=None)
        return gp
    L = N.lib()
    kss = gp.kernel.kdiag()
    wb, kb = ctypes.c_int(0), ctypes.c_int(0)
    ok = int(L.gp2d_ozaki_guard_bits(kss, vmin, GUARD_TARGET, ctypes.byref(wb), ctypes.byref(kb)))
    g.update(pending=False, vmin_over_kss=vmin / kss, wmax=wmax)
    stream = g.pop("stream", None) or torch.cuda.current_stream(gp.device)
    packed = gp.extra.pop("packed", None)
    if ok <= 0:   # beyond the emulation's range (or a non-positive v_min): exact FP64 products
        g.update(engine="f64", wbits=None, kbits=None,
                 est=float(L.gp2d_ozaki_error_model(kss, vmin, OZAKI_MAX_BITS[0], OZAKI_MAX_BITS[1])))
        gp.extra.pop("ozaki", None)
        if gp.W is None:   # a receiving rank kept only the packed payload
            with torch.cuda.stream(stream):
                W = torch.zeros((gp.n, gp.n), dtype=torch.float64, device=gp.device)
                N.check(L.gp2d_pack_lower(_ptr(W), gp.n, gp.n, _ptr(packed), 1, _stream_handle(gp.device)),
                        "gp2d_pack_lower")
                g["event"] = torch.cuda.Event()
                g["event"].record(stream)
            gp.W = W
        return gp
    wbits, kbits = wb.value, kb.value
    g.update(engine="ozaki", wbits=wbits, kbits=kbits, est=float(L.gp2d_ozaki_error_model(kss, vmin, wbits, kbits)))
    if (wbits, kbits) != OZAKI_DEFAULT_BITS:
        with torch.cuda.stream(stream):
            ozaki_prepare(gp, diag_add=g["diag_add"], wbits=wbits, kbits=kbits, packed=packed)
            gp.extra.pop("packed", None)
            g["event"] = torch.cuda.Event()
            g["event"].record(stream)
    return gp


def ozaki_prepare_guarded(gp: GPFit, diag_add: float, guard: bool = True) -> GPFit:
    """The ozaki engine's planes for a fit whose W is already final (a loaded checkpoint, the
    distributed factor): the accuracy guard's statistics read synchronously, then the planes at
    the guard's precision (or none: the FP64 engine) — apply_guard without the deferred path."""
    if not guard:
        return ozaki_prepare(gp, diag_add=float(diag_add))
    status, _ = status_block(gp.device)
    _guard_stats(gp.W, gp.n, gp.n_train, gp.n_pad, diag_add, status, gp.device)
    host = status.cpu()
    _arm_guard(gp, diag_add)
    apply_guard(gp, float(host[1]), float(host[2]))
    if "ozaki" not in gp.extra and gp.extra["guard"]["engine"] == "ozaki":
        ozaki_prepare(gp, diag_add=float(diag_add))
    return gp.ready_on(torch.cuda.current_stream(gp.device))


# ------------------------------------------------------------------ background flow (trend)
TRENDS = (None, "constant", "linear")


def trend_order(trend) -> int | None:
    """The library's order of a trend= argument: None (zero-mean), 'constant' → 0, 'linear' → 1."""
    if trend is None:
        return None
    if trend not in N.TREND_ORDERS:
        raise ValueError(f"trend must be one of {TRENDS}; got {trend!r}")
    return N.TREND_ORDERS[trend]


def refuse_trend(trend, entry: str, hint: str = ""):
    """ValueError for an entry that has no trend form yet (trend: a trend= argument, or a fit)."""
    if isinstance(trend, GPFit):
        trend = trend.extra.get("trend")
    if trend is not None:
        raise ValueError(f"{entry} does not support a background flow (trend=){hint}")


def _check_trend_fit(kernel: "KernelSpec", variance: str, trend) -> int | None:
    """A fit's trend= checked before the device is required."""
    order = trend_order(trend)
    if order is None:
        return None
    if variance == "ozaki":
        raise ValueError("trend= needs the FP64 engine (variance='f64'): the ozaki variance engine has no trend form")
    if not kernel.is_vector:
        raise ValueError("trend= models a background flow (u, v): it needs a vector kernel, not the ARD family")
    return order


def _trend_basis(x, X: torch.Tensor, order: int):
    """(centre, scale) of the trend's basis coordinates: the mean of the training points' two spatial
    coordinates and the largest |coordinate − centre| over both axes — on the host for host points
    (no device round trip), else from the device tensor (one synchronising copy of three numbers)."""
    if isinstance(x, torch.Tensor):
        sp = X[:, -2:]
        c = sp.mean(0)
        c3 = torch.cat([c, (sp - c).abs().max().reshape(1)]).cpu().numpy()
        centre, scale = c3[:2], float(c3[2])
    else:
        sp = np.asarray(x, dtype=np.float64).reshape(-1, X.shape[1])[:, -2:]
        centre = sp.mean(0)
        scale = float(np.abs(sp - centre).max())
    if not (np.all(np.isfinite(centre)) and np.isfinite(scale)):
        raise ValueError("trend=: the training points are not finite")
    if scale == 0.0:   # every point at the centre
        if order == 1:
            raise np.linalg.LinAlgError("trend='linear' needs at least three points that are not collinear "
                                        "(all training points coincide)")
        scale = 1.0
    return (float(centre[0]), float(centre[1])), scale


def _trend_solve(st: "_Staged", W: torch.Tensor, Y: torch.Tensor, alpha: torch.Tensor, x, order: int, dev,
                 basis: tuple | None = None) -> dict:
    """gp2d_trend_fit in place of gp2d_potrs_inv: α′ into alpha and the fit's trend block (β̂, A⁻¹,
    log|A|, status, [α′ | B0]); returns gp.extra['trend'].  basis: a saved (centre, scale) in place
    of the training points' own (Krig.load of a checkpoint with its factor)."""
    L = N.lib()
    centre, scale = _trend_basis(x, st.X, order) if basis is None else basis
    desc = N.trend_desc(order, centre, scale)
    nd = int(L.gp2d_trend_block_doubles(st.n))
    block = torch.empty(nd + 8, dtype=torch.float64, device=dev)
    block = block[(-block.data_ptr() % 64) // 8:][:nd]   # 64-byte aligned: a table row is one aligned piece
    wbytes = int(L.gp2d_trend_workspace(st.n, order))
    work = _workspace(wbytes, dev)
    N.check(L.gp2d_trend_fit(_ptr(W), st.n, W.stride(0), _ptr(Y), _ptr(st.X), st.ntr, st.npad, st.X.shape[1],
                             ctypes.byref(desc), _ptr(alpha), _ptr(block), _ptr(work), wbytes, _stream_handle(dev)),
            "gp2d_trend_fit")
    ev = torch.cuda.Event()   # the status word is read after this, whatever stream is current then
    ev.record(torch.cuda.current_stream(dev))
    return dict(order=order, name=("constant", "linear")[order], centre=centre, scale=scale, desc=desc, block=block,
                q=int(L.gp2d_trend_coefficients(order)), event=ev)


def _settle_trend(gp: "GPFit") -> "GPFit":
    """Raise LinAlgError for a trend whose A = H·K_y⁻¹·Hᵀ was singular (the block's status word; read
    once per fit, after the factor's own status)."""
    t = gp.extra.get("trend")
    if t is not None and not t.get("checked"):
        t["event"].synchronize()
        st = int(t["block"][N.TREND_STATUS].item())
        t["checked"] = True
        if st != 0:
            raise np.linalg.LinAlgError(
                f"the trend's normal matrix H·K_y⁻¹·Hᵀ is singular (pivot {st} of {t['q']}): trend='linear' needs "
                "at least three training points that are not collinear")
    return gp


def trend_coefficients(gp: "GPFit") -> dict:
    """The estimated background flow of a trend fit, on the host: beta (q,) = β̂ and cov (q, q) = A⁻¹ in
    the basis coordinates ξ = (x1 − centre[0])/scale, η = (x2 − centre[1])/scale (u = β0 + β2·ξ + β3·η,
    v = β1 + β4·ξ + β5·η; q = 2 for 'constant'), and the physical reading: mean_flow (u, v) at the
    centre, and gradient = (∂u/∂x1, ∂u/∂x2, ∂v/∂x1, ∂v/∂x2) of the trend (β/scale; zeros for
    'constant'), with order, centre and scale."""
    t = gp.extra.get("trend")
    if t is None:
        raise ValueError("trend_coefficients needs a fit made with trend='constant' or 'linear'")
    gp.check()
    q = t["q"]
    head = t["block"][:N.TREND_RHS].cpu().numpy()
    beta = head[N.TREND_BETA:N.TREND_BETA + q].copy()
    cov = head[N.TREND_AINV:N.TREND_AINV + N.TREND_AINV_LD ** 2].reshape(N.TREND_AINV_LD, -1)[:q, :q].copy()
    grad = beta[2:6] / t["scale"] if q == 6 else np.zeros(4)
    return dict(order=t["name"], centre=np.array(t["centre"]), scale=t["scale"], beta=beta, cov=cov,
                logdet=float(head[N.TREND_LOGDET]), mean_flow=beta[:2].copy(), gradient=grad)


# ------------------------------------------------------------------ the fit's stages
# (shared by fit, fit_batch, distributed.fit_distributed and krig.Krig._restore)
@dataclass
class _Staged:
    """One problem ready for assembly (_stage_problem): the training points in fit order (Morton
    for the ozaki engine, x = x_input[perm]) and the fit's layout."""
    kernel: KernelSpec
    X: torch.Tensor
    ntr: int
    npad: int
    n: int
    perm: torch.Tensor | None


def _refuse_sum(kernel: KernelSpec, entry: str):
    """ValueError for an entry that has no kernel-sum form (the gradient tensor, the joint
    covariance, the int8 engine)."""
    if kernel.is_sum:
        raise ValueError(f"{entry} does not support a kernel sum (family 'vector_sum')")


def _check_family(kernel: KernelSpec, variance: str):
    if variance == "ozaki" and kernel.is_sum:
        raise ValueError("the ozaki variance engine does not support a kernel sum (family 'vector_sum'): "
                         "use variance='f64'")
    if variance == "ozaki" and not kernel.is_vector:
        raise ValueError("the ozaki variance engine supports the vector families only")


def _stage_problem(kernel: KernelSpec, x, variance: str, dev, layout=fit_layout) -> _Staged:
    """Points on the device, the layout ((padded points, matrix order) = layout(kernel, N_train,
    variance)), the ozaki engine's size limit and its Morton order."""
    _check_family(kernel, variance)
    X = _as_points(x, kernel.input_dim, dev)
    ntr = X.shape[0]
    if ntr < 1:
        raise ValueError("need at least one training point")
    npad, n = layout(kernel, ntr, variance)
    if variance == "ozaki" and n >= 131072:
        # the int8 GEMM epilogue's biased sums stay below 2^32 only for K = n < 2^17
        raise ValueError(f"the ozaki variance engine supports n < 131072 (N_train < 65536); got n = {n}: "
                         "use variance='f64'")
    perm = None
    if variance == "ozaki" and ntr > 1:   # Morton order: exact-zero K* slabs cluster (skipped)
        perm, X = morton_sort(X)
    return _Staged(kernel, X, ntr, npad, n, perm)


def _assemble_ky(st: _Staged, diag_add: float, A: torch.Tensor, dev):
    """K_y = K(x, x) + diag_add·I into A (n × n) — for the vector families its lower block
    triangle only (symmetric = 2), all gp2d_potrf reads."""
    N.check(N.lib().gp2d_assemble(_ptr(st.X), st.ntr, st.npad, _ptr(st.X), st.ntr, st.npad,
                                  ctypes.byref(st.kernel.desc()), float(diag_add),
                                  ASSEMBLE_LOWER if st.kernel.is_vector else 1, _ptr(A), st.n, _stream_handle(dev)),
            "gp2d_assemble")


@contextlib.contextmanager
def _factor_join(on: bool):
    """gp2d_factor_join(on) for the factorisations issued inside; the previous mode comes back."""
    prev = N.lib().gp2d_factor_join(1 if on else 0)
    try:
        yield
    finally:
        N.lib().gp2d_factor_join(prev)


def _factor_inverse(A: torch.Tensor, n: int, dinv: torch.Tensor, info: torch.Tensor, dev, join: bool | None = None):
    """A ← W = L⁻¹, L = chol(A): gp2d_potrf then gp2d_trtri, or gp2d_potrf_inv when FUSED_INVERSE.
    join: the gp2d_factor_join mode around the factorisation (None: left as it is)."""
    L = N.lib()
    s = _stream_handle(dev)
    with (contextlib.nullcontext() if join is None else _factor_join(join)):
        if FUSED_INVERSE:   # factor and inverse in one call, the TRTRI GEMMs overlapped with POTRF
            wbytes = int(L.gp2d_potrf_inv_workspace(n))
            work = _workspace(wbytes, dev)
            N.check(L.gp2d_potrf_inv(_ptr(A), n, n, _ptr(dinv), _ptr(info), _ptr(work), wbytes, s),
                    "gp2d_potrf_inv")
            return
        N.check(L.gp2d_potrf(_ptr(A), n, n, _ptr(dinv), _ptr(info), None, 0, s), "gp2d_potrf")
    wbytes = int(L.gp2d_trtri_workspace(n))
    work = _workspace(wbytes, dev)
    N.check(L.gp2d_trtri(_ptr(A), n, n, _ptr(dinv), _ptr(work), wbytes, s), "gp2d_trtri")


def _arm_guard(gp: GPFit, diag_add: float):
    """Arm the accuracy guard of a fit whose statistics are still to come: apply_guard acts on
    exactly these keys, once, on the stream that is current now."""
    gp.extra["guard"] = dict(pending=True, diag_add=float(diag_add), stream=torch.cuda.current_stream(gp.device))


def _make_fit(st: _Staged, noise: float, W: torch.Tensor, alpha: torch.Tensor, Y: torch.Tensor, dev) -> GPFit:
    return GPFit(kernel=st.kernel, noise=float(noise), x=st.X, n_train=st.ntr, n_pad=st.npad, W=W, alpha=alpha,
                 device=dev, y=Y, perm=st.perm)


def _finish_problem(st: _Staged, W: torch.Tensor, y, noise: float, diag_add: float, status: torch.Tensor,
                    guard: bool | None, variance: str, check: bool, dev, pwork: torch.Tensor | None = None,
                    trend: tuple | None = None):
    """Everything of a fit after W = L⁻¹, queued on the current stream: the guard's statistics
    beside info in `status` (status_block), the status copy of a check=False fit (it reads only
    words written before it, so the host later waits for the factor, not for what follows), α, and
    the ozaki engine's planes at the default precision.  pwork: a gp2d_potrs workspace shared by a
    batch's problems.  Returns (fit, the preparation's deferred GP2DError or None); check=False
    leaves both with the copy in fit.pending for GPFit.check()."""
    L = N.lib()
    n = st.n
    guard = (GUARD_DEFAULT if guard is None else guard) and variance == "ozaki"
    if guard:   # the guard's statistics from W, into the status word beside info
        _guard_stats(W, n, st.ntr, st.npad, diag_add, status, dev)
    else:       # "no guard ran": a receiving rank of the job stream keeps the default precision
        status[1:].fill_(float("nan"))
    pend = None if check else pending_status(status)
    Y = _pad_obs(y, st.ntr, st.npad, st.kernel.block_dim, dev, st.perm)
    alpha = torch.empty(n, dtype=torch.float64, device=dev)
    tr = None
    if trend is not None:   # (order, the caller's points): α′ and the trend block in place of α
        tr = _trend_solve(st, W, Y, alpha, trend[1], trend[0], dev)
    else:
        pbytes = int(L.gp2d_potrs_workspace(n))
        if pwork is None:
            pwork = _workspace(pbytes, dev)
        N.check(L.gp2d_potrs_inv(_ptr(W), n, n, _ptr(Y), _ptr(alpha), _ptr(pwork), pbytes, _stream_handle(dev)),
                "gp2d_potrs_inv")
    gp = _make_fit(st, noise, W, alpha, Y, dev)
    if tr is not None:
        gp.extra["trend"] = tr
    gp.extra["status_dev"] = status   # info + guard statistics on the device (the job stream broadcasts it)
    gp.extra["diag_add"] = float(diag_add)   # noise + jitter on K_y's diagonal (cv_points / cv_groups latent=True)
    del pwork
    err = None
    if variance == "ozaki":
        # enqueued before the status is read, with the a-priori moduli count at the default
        # precision: the fit's only host round trip is the status read
        if guard:
            _arm_guard(gp, diag_add)
        try:
            ozaki_prepare(gp, diag_add=float(diag_add))
        except N.GP2DError as e:   # a failed factor (NaN rows) makes prepare fail too: info decides
            err = e
    if pend is not None:
        gp.pending = (pend[0], pend[1], err)
    return gp, err


def _settle(gp: GPFit, host: torch.Tensor, err) -> GPFit:
    """A fit's ending once its status block is on the host: raise what the factor or the
    preparation left, then the accuracy guard."""
    _raise_fit_errors(int(host.view(torch.int32)[0].item()), err)
    return apply_guard(gp, float(host[1]), float(host[2]))


def fit(kernel: KernelSpec, x, y, noise: float, jitter: float = 0.0, device=None, variance: str = "f64",
        check: bool = True, jitchol: int = 0, join: bool | None = None, guard: bool | None = None,
        trend: str | None = None) -> GPFit:
    """K_y = K(x,x) + (noise+jitter)·I → L = chol(K_y) → W = L⁻¹ → α = Wᵀ W y.

    trend = 'constant' | 'linear' (vector kernels, FP64 engine): a background flow estimated with
    the fit (universal kriging) — u = β0 + β2·ξ + β3·η, v = β1 + β4·ξ + β5·η in
    coordinates centred and scaled on the training points.  gp.alpha is then α′ = K_y⁻¹(y − Hᵀβ̂),
    gp.extra['trend'] holds order, centre, scale and the device block (β̂, its covariance, B0), and
    predict, predict_field, Predictor and the likelihood route to their trend forms on their own
    (trend_coefficients reads β̂).  LinAlgError where the basis is not identifiable ('linear' on
    collinear points or fewer than three distinct ones).

    jitchol = k > 0: GPy's jitchol retry (GPy.util.linalg.jitchol, maxtries = k; GPy is not
    installed here, so this follows its published algorithm and is parity-unpinned): if K_y is
    not positive definite, refit with an extra diagonal jitter of mean(diag K_y)·1e-6, ten times
    larger on each further try, up to k tries, then raise LinAlgError.  The jitter that succeeded
    is gp.extra['jitchol'] (0.0 when the first factorisation did).  Implies check=True.

    variance: 'f64'   — predictive variance by the FP64-MFMA contraction;
              'ozaki' — the same contraction emulated exactly on the INT8 matrix cores
                        (Ozaki scheme II, csrc/ozaki.hpp); vector2d family only.
    guard (ozaki): hold the emulated variance to GUARD_TARGET whatever the hyperparameters
    (apply_guard: more W bits, or the FP64 engine); False keeps the default 49 bits.
    Raises numpy.linalg.LinAlgError if K_y is not positive definite (the
    reference's np.linalg.inv / GPy jitchol / sklearn error paths).  check=False returns
    without waiting for the factor (no host sync); the error is raised by GPFit.check().

    join (default: = check): the host waits for the factorisation's chain before it enqueues
    the rest of the fit (gp2d_factor_join), so the current stream holds no wait pending beside
    the chain — a pending wait on some of torch's streams slows the chain by up to 40 %
    (DESIGN.md §6).  It costs nothing when the caller blocks on the result anyway; join=False
    keeps a check=False fit fully asynchronous, join=True blocks one that has nothing to
    overlap (a job stream's first fit).
    """
    if jitchol:
        try:
            gp = fit(kernel, x, y, noise, jitter=jitter, device=device, variance=variance, trend=trend)
            gp.extra["jitchol"] = 0.0
            return gp
        except np.linalg.LinAlgError:
            diag = float(N.lib().gp2d_kernel_diag(ctypes.byref(kernel.desc()))) + noise + jitter
            if not diag > 0.0:
                raise np.linalg.LinAlgError("not pd: non-positive diagonal elements") from None
            jit = diag * 1e-6
            for _ in range(int(jitchol)):
                if not np.isfinite(jit):
                    break
                try:
                    gp = fit(kernel, x, y, noise, jitter=jitter + jit, device=device, variance=variance,
                             trend=trend)
                    gp.extra["jitchol"] = jit
                    return gp
                except np.linalg.LinAlgError:
                    jit *= 10.0
            raise np.linalg.LinAlgError("not positive definite, even with jitter.") from None
    if variance not in VARIANCE_ENGINES:
        raise ValueError(f"variance must be one of {VARIANCE_ENGINES}")
    _check_family(kernel, variance)   # before the device is required, like the check above
    order = _check_trend_fit(kernel, variance, trend)
    dev = _require_device(device)
    st = _stage_problem(kernel, x, variance, dev)
    n, diag_add = st.n, noise + jitter
    A = torch.empty((n, n), dtype=torch.float64, device=dev)
    _assemble_ky(st, diag_add, A, dev)
    dinv = torch.empty((n // NB, NB, NB), dtype=torch.float64, device=dev)
    status, info = status_block(dev)   # gp2d_potrf resets info
    _factor_inverse(A, n, dinv, info, dev, join=check if join is None else join)
    del dinv
    gp, err = _finish_problem(st, A, y, noise, diag_add, status, guard, variance, check, dev,
                              trend=None if order is None else (order, x))
    return gp if not check else _settle_trend(_settle(gp, status.cpu(), err))


def fit_batch(problems, variance: str = "f64", jitter: float = 0.0, device=None, check: bool = True,
              join: bool | None = None, guard: bool | None = None, trend: str | None = None) -> list:
    """Fit several GPs of one size together: `problems` is a sequence of (kernel, x, y, noise)
    whose matrices K_y share the order n (a hyperparameter sweep's settings over one training
    set, or a job stream's next jobs with equal point counts).  Their K_y are factored and
    inverted in ONE chain (gp2d_potrf_batched + gp2d_trtri_batched: every launch carries every
    problem), so the latency-bound diagonal chain of a fit is paid once per
    batch instead of once per fit; each problem's W, α (and INT8 residue planes) are those of
    engine.fit on it alone, bit for bit.  Returns one GPFit per problem (W views into one
    (B, n, n) tensor).  check=True raises LinAlgError for the first non-PD problem (the index
    is in the message); check=False defers it to each GPFit.check().  join, guard as in fit()."""
    if variance not in VARIANCE_ENGINES:
        raise ValueError(f"variance must be one of {VARIANCE_ENGINES}")
    refuse_trend(trend, "fit_batch", ": fit each problem with engine.fit")
    probs = list(problems)
    if not probs:
        return []
    if len(probs) > 64:
        raise ValueError("fit_batch: at most 64 problems per batch")
    dev = _require_device(device)
    L = N.lib()
    s = _stream_handle(dev)
    prep = []
    for kernel, x, y, _ in probs:
        st = _stage_problem(kernel, x, variance, dev)
        ny = y.numel() if isinstance(y, torch.Tensor) else np.asarray(y).size
        if ny != kernel.block_dim * st.ntr:   # every problem's shape is checked before the batch is assembled
            raise ValueError(f"problem {len(prep)}: observation vector has {ny} entries, "
                             f"expected {kernel.block_dim * st.ntr}")
        prep.append(st)
    n = prep[0].n
    if any(st.n != n for st in prep):
        raise ValueError("fit_batch: every problem must have the same matrix order n")
    B = len(prep)
    A = torch.empty((B, n, n), dtype=torch.float64, device=dev)
    for b, st in enumerate(prep):
        _assemble_ky(st, probs[b][3] + jitter, A[b], dev)
    dinv = torch.empty((B, n // NB, NB, NB), dtype=torch.float64, device=dev)
    info = torch.empty(B, dtype=torch.int32, device=dev)   # gp2d_potrf_batched resets them
    with _factor_join(check if join is None else join):
        N.check(L.gp2d_potrf_batched(_ptr(A), n, n, n * n, B, _ptr(dinv), _ptr(info), s), "gp2d_potrf_batched")
    wbytes = int(L.gp2d_trtri_batched_workspace(n, B))
    work = _workspace(wbytes, dev)
    N.check(L.gp2d_trtri_batched(_ptr(A), n, n, n * n, B, _ptr(dinv), _ptr(work), wbytes, s), "gp2d_trtri_batched")
    del work, dinv
    pwork = _workspace(int(L.gp2d_potrs_workspace(n)), dev)
    statuses = torch.empty((B, 3), dtype=torch.float64, device=dev)   # status_block per problem
    fits, errs = [], []
    for b, st in enumerate(prep):
        statuses[b].view(torch.int32)[0:1].copy_(info[b:b + 1])        # a 4-byte device copy
        _, _, y, noise = probs[b]
        gp, err = _finish_problem(st, A[b], y, noise, noise + jitter, statuses[b], guard, variance, check, dev, pwork)
        fits.append(gp)
        errs.append(err)
    del pwork
    if check:
        host = statuses.cpu()
        for b, err in enumerate(errs):
            try:
                _raise_fit_errors(int(host[b].view(torch.int32)[0].item()), err)
            except np.linalg.LinAlgError as e:
                raise np.linalg.LinAlgError(f"problem {b}: {e}") from None
        for b, gp in enumerate(fits):
            apply_guard(gp, float(host[b, 1]), float(host[b, 2]))
    return fits


def ozaki_prepare(gp: GPFit, diag_add: float | None = None, packed: torch.Tensor | None = None,
                  wbits: int = 0, kbits: int = 0) -> GPFit:
    """Residue planes of W for the INT8 variance engine (once per fit).  With `diag_add`
    (the noise + jitter of K_y's diagonal) the moduli count is the a-priori bound and nothing
    synchronises (gp2d_ozaki_prepare_async); without it, the data-driven count of the
    factor's row bounds (one device → host read).  packed: W as the factor broadcast's packed
    lower block triangle (gp2d_ozaki_prepare_packed, needs diag_add) — gp.W may then be None.
    wbits / kbits: integer bits per W row and of K* (0 = the defaults 49 / 45; the accuracy guard's
    choice, apply_guard).  gp.extra['ozaki'] = (residue planes, row scales, moduli count, kbits)."""
    L = N.lib()
    n = gp.n
    desc = gp.kernel.desc()
    # the planes this fit will use: the a-priori count is known before the call (the async and
    # packed preparations use exactly it); the data-driven one only after (the worst case)
    nm = int(L.gp2d_ozaki_nmod_apriori(n, ctypes.byref(desc), float(diag_add), int(wbits), int(kbits))) \
        if diag_add is not None else 0
    wres = torch.empty(nm * n * n if nm > 0 else int(L.gp2d_ozaki_wres_bytes(n)), dtype=torch.int8, device=gp.device)
    rowscale = torch.empty(n, dtype=torch.float64, device=gp.device)
    nmod = ctypes.c_int(0)
    if packed is not None:
        if diag_add is None:
            raise ValueError("ozaki_prepare from the packed factor needs diag_add (the a-priori moduli count)")
        N.check(L.gp2d_ozaki_prepare_packed(_ptr(packed), n, ctypes.byref(desc), float(diag_add), int(wbits),
                                            int(kbits), _ptr(wres), _ptr(rowscale), ctypes.byref(nmod),
                                            _stream_handle(gp.device)), "gp2d_ozaki_prepare_packed")
    elif diag_add is not None:
        N.check(L.gp2d_ozaki_prepare_async(_ptr(gp.W), n, n, ctypes.byref(desc), float(diag_add), int(wbits),
                                           int(kbits), _ptr(wres), _ptr(rowscale), ctypes.byref(nmod),
                                           _stream_handle(gp.device)), "gp2d_ozaki_prepare_async")
    else:
        N.check(L.gp2d_ozaki_prepare(_ptr(gp.W), n, n, ctypes.byref(desc), int(wbits), int(kbits), _ptr(wres),
                                     _ptr(rowscale),
                                     ctypes.byref(nmod), _stream_handle(gp.device)), "gp2d_ozaki_prepare")
    gp.extra["ozaki"] = (wres, rowscale, int(nmod.value), int(kbits))
    if packed is not None:
        gp.extra["packed"] = packed   # kept until the guard has decided (it may need more bits, or W)
    return gp


@dataclass
class KstarPlanes:
    """INT8 residue planes of K*ᵀ for a whole grid (every chunk), generated ahead of the fit:
    they depend on the training points, the grid and the kernel only (not on α), so they can
    run on a side stream while the fit runs (gp2d_ozaki_kstar)."""
    kernel: KernelSpec
    x: torch.Tensor
    m: int
    n: int
    n_pad: int
    chunk: int
    nmod: int
    bres: torch.Tensor
    event: torch.cuda.Event
    xg: torch.Tensor = None     # the grid in plane order (Morton)
    order: torch.Tensor = None  # plane row j ↔ input grid point order[j]


def kstar_planes(kernel: KernelSpec, x, xg, noise: float, jitter: float = 0.0, chunk: int = 8192, stream=None,
                 out: KstarPlanes | None = None, device=None) -> KstarPlanes:
    """Launch the K* residue planes of grid `xg` against training points `x` on `stream`
    (default: the current stream) after the current stream's pending work; returns at once.
    The moduli count is gp2d_ozaki_nmod_apriori's bound for K_y,ii = kdiag + noise + jitter,
    which covers any fit of these hyperparameters.  `out` reuses a previous buffer."""
    if not kernel.is_vector:
        raise ValueError("K* planes are an ozaki-engine feature (vector families)")
    dev = _require_device(device)
    L = N.lib()
    d = kernel.input_dim
    X = _as_points(x, d, dev)
    if X.shape[0] > 1:
        X = morton_sort(X)[1]                     # the order fit() gives the training points
    order, G = morton_sort(_as_points(xg, d, dev))
    ntr, m = X.shape[0], G.shape[0]
    npad, n = fit_layout(kernel, ntr, "ozaki")
    chunk = max(128, (int(chunk) + 127) // 128 * 128)
    desc = kernel.desc()
    nmod = int(L.gp2d_ozaki_nmod_apriori(n, ctypes.byref(desc), float(noise + jitter), 0, 0))
    if nmod <= 0:
        N.check(-1, "gp2d_ozaki_nmod_apriori")
    nbytes = int(L.gp2d_ozaki_kstar_bytes(n, m, chunk, nmod))
    bres = out.bres if (out is not None and out.bres.numel() >= nbytes) else \
        torch.empty(max(nbytes, 1), dtype=torch.int8, device=dev)
    main = torch.cuda.current_stream(dev)
    st = stream if stream is not None else main
    if st is not main:
        st.wait_stream(main)   # the points (and a reused buffer's last reader) are ordered before
    N.check(L.gp2d_ozaki_kstar(_ptr(X), ntr, npad, _ptr(G), m, ctypes.byref(desc), nmod, 0, chunk, _ptr(bres),
                               bres.numel(), ctypes.c_void_p(st.cuda_stream)), "gp2d_ozaki_kstar")
    if st is not main:
        # the caching allocator must not hand these blocks to main-stream work (the fit)
        # while the side stream still reads / writes them
        for t in (X, G, bres):
            t.record_stream(st)
    ev = torch.cuda.Event()
    ev.record(st)
    return KstarPlanes(kernel=kernel, x=X, m=m, n=n, n_pad=npad, chunk=chunk, nmod=nmod, bres=bres, event=ev,
                       xg=G, order=order)


def ozaki_executed_fraction(kernel: KernelSpec, x, xg, noise: float, jitter: float = 0.0, chunk: int = 8192,
                            device=None) -> float:
    """Measurement helper (bench.py): the fraction of the dense int8 GEMM work (W lower-
    triangular, every K slab) the zero-slab skipping executes for this training set and grid —
    read from the K* block flags gp2d_ozaki_kstar stores after each chunk's planes, with the
    slab-list rules of ozaki_slab_list_kernel / igemm_nt_mod_kernel."""
    pl = kstar_planes(kernel, x, xg, noise, jitter, chunk, device=device)
    pl.event.synchronize()
    n, ntb, m, ch = pl.n, pl.n_pad // 64, pl.m, pl.chunk
    planes = pl.nmod * n * 2 * ((ch + 255) // 256 * 256)   # nmod · n · 2·cp_max; the chunk's flags follow
    stride = int(N.lib().gp2d_ozaki_kstar_bytes(n, ch, ch, pl.nmod))   # the bytes of exactly one chunk
    nbi = n // 256
    ke_slabs = 4 * np.arange(1, nbi + 1)          # a_lower: row block bi reads slabs < 4(bi+1)
    executed = dense = 0
    for ci, c0 in enumerate(range(0, m, ch)):
        cp = (min(ch, m - c0) + 255) // 256 * 256
        off = ci * stride + planes
        f = pl.bres[off:off + (cp // 64) * ntb].view(torch.uint8).cpu().numpy().reshape(cp // 256, 4, ntb)
        kept = np.concatenate([f.any(1)] * 2, axis=1)            # (grid tile, slab): u then v blocks
        cum = np.cumsum(kept, axis=1)[:, ke_slabs - 1]           # listed slabs below each row block's end
        run = np.where((cum > 0) & (cum < 3), ke_slabs[None, :], cum)   # 1–2 slabs run dense
        executed += 2 * int(run.sum())                           # u rows and v rows of each tile
        dense += 2 * (cp // 256) * int(ke_slabs.sum())
    return executed / dense if dense else 1.0


_VAR_MODES = {"latent": N.VAR_LATENT, "gpy": N.VAR_NOISY, "noisy": N.VAR_NOISY, "sklearn": N.VAR_CLIPPED,
              "clipped": N.VAR_CLIPPED}


def _f64_fit_args(gp: GPFit, G: torch.Tensor, desc) -> tuple:
    """What gp2d_predict, gp2d_predict_field and gp2d_predict_cov start with: the factor W and its
    row stride, α, the training points, the targets, the kernel."""
    return (_ptr(gp.W), gp.n, gp.W.stride(0), _ptr(gp.alpha), _ptr(gp.x), gp.n_train, gp.n_pad, _ptr(G), G.shape[0],
            ctypes.byref(desc))


class Predictor:
    """Reusable predict workspace for one GPFit (chunked over the grid)."""

    def __init__(self, gp: GPFit, chunk: int = 8192):
        self.gp = gp
        bd = gp.kernel.block_dim
        self.ozaki = "ozaki" in gp.extra
        unit = 128 if (bd == 1 or self.ozaki) else 64
        self.chunk = max(unit, (int(chunk) + unit - 1) // unit * unit)
        self.trend_order = None
        self.wnmod = 0   # the moduli count the ozaki workspace is sized for (grows on demand)
        if self.ozaki:
            self._ozaki_workspace(gp.extra["ozaki"][2])
        else:
            self.trend_order = _trend_of(gp, "order")   # a trend fit's workspace holds q + 1 sets of mean partials
            self.wbytes = int(N.lib().gp2d_predict_workspace(gp.n, self.chunk, bd)) if self.trend_order is None else \
                int(N.lib().gp2d_predict_trend_workspace(gp.n, self.chunk, bd, self.trend_order))
            self.work = _workspace(self.wbytes, gp.device)
        self._grid = None   # (the caller's grid tensor, its version, Morton order, the grid in that order)

    def _ozaki_workspace(self, nmod: int):
        """Size the ozaki workspace for a fit with `nmod` moduli (its layout follows nmod): the
        accuracy guard may give later fits more, and a worst-case buffer would hold 1.5× the bytes
        at n = 32,768 for nothing."""
        if nmod > self.wnmod:
            self.wbytes = int(N.lib().gp2d_predict_ozaki_workspace_nmod(self.gp.n, self.chunk, int(nmod)))
            if self.wbytes <= 0:
                raise N.GP2DError(f"no ozaki workspace for {nmod} moduli at n = {self.gp.n}")
            if self.wnmod:   # a grown workspace: the old one may still be read by queued predicts
                torch.cuda.synchronize(self.gp.device)
            self.work = None
            self.work = _workspace(self.wbytes, self.gp.device)
            self.wnmod = int(nmod)

    def _grid_order(self, xg, G: torch.Tensor, reuse: bool):
        """Morton order of the grid and the grid in that order.  reuse=True (a job stream predicting
        one device grid job after job — the reference's per-window krig.predict on one grid): for the
        same tensor, at the same address and unmodified by version-tracked ops since (its version
        counter), the order of the previous call is reused — the tensor is held, so its memory cannot
        be handed to another grid.  Writes that bypass the version counter (DLPack aliases, raw
        data_ptr kernels) are not seen: callers that modify a grid that way must not ask for reuse."""
        c = self._grid
        st = torch.cuda.current_stream(G.device)
        if reuse and isinstance(xg, torch.Tensor) and c is not None and c[0] is xg and c[1] == xg._version \
                and c[5] == xg.data_ptr() and c[3].shape == G.shape and c[4] == st:   # made on this stream
            return c[2], c[3]
        order, Gs = morton_sort(G)
        self._grid = (xg, xg._version, order, Gs, st, xg.data_ptr()) \
            if reuse and isinstance(xg, torch.Tensor) and xg.is_cuda else None
        return order, Gs

    def fits(self, gp: GPFit) -> bool:
        """True if this workspace serves `gp` as is: same matrix order, engine and block size
        (the FP64 workspace and the chunk rounding depend on the block size)."""
        return (self.gp.n == gp.n and self.ozaki == ("ozaki" in gp.extra)
                and self.gp.kernel.block_dim == gp.kernel.block_dim
                and (self.ozaki or self.trend_order == _trend_of(gp, "order")))

    def __call__(self, xg, var_mode: str = "latent", compute_var: bool = True, out=None,
                 planes: KstarPlanes | None = None, reuse_grid: bool = False, term: int | None = None):
        """planes: K* residue planes of this same grid from kstar_planes() (ozaki engine):
        the variance GEMMs read them and the K* kernel runs mean-only (same results as without).
        reuse_grid: the grid is the one of the previous call, unmodified (_grid_order).
        term: the posterior of term t's contribution alone, from a kernel sum's fit (predict)."""
        gp = self.gp
        L = N.lib()
        d, bd = gp.kernel.input_dim, gp.kernel.block_dim
        G = _as_points(xg, d, gp.device)
        m = G.shape[0]
        if out is None:
            mean = torch.empty(bd * m, dtype=torch.float64, device=gp.device)
            var = torch.empty(bd * m, dtype=torch.float64, device=gp.device)
        else:
            mean, var = out
        desc = _term_kernel(gp, term, var_mode).desc()
        if self.ozaki and "ozaki" in gp.extra:
            wres, rowscale, nmod, kbits = gp.extra["ozaki"]
            self._ozaki_workspace(nmod)
            use_planes = planes is not None and compute_var
            if use_planes and (planes.m != m or planes.n != gp.n or planes.chunk != self.chunk):
                raise ValueError("K* planes were made for another grid, fit layout or chunk size")
            # the variance runs on the grid in Morton order (zero K* tiles cluster and are
            # skipped); every output point is independent of the others, so reordering
            # changes no bits — the epilogue stores each result at its input position
            order, Gs = None, G
            if compute_var and m > 1:
                if use_planes:
                    order, Gs = planes.order, planes.xg
                else:
                    order, Gs = self._grid_order(xg, G, reuse_grid)
            # what both predict calls start and end with: the fit, the points, the mode | outputs, workspace
            fit_args = (_ptr(wres), _ptr(rowscale), nmod, kbits, gp.n, _ptr(gp.alpha), _ptr(gp.x), gp.n_train, gp.n_pad,
                        _ptr(Gs), m, ctypes.byref(desc), _VAR_MODES[var_mode], float(gp.noise))
            out_args = (_ptr(mean), _ptr(var), None if order is None else _ptr(order), self.chunk, _ptr(self.work),
                        self.wbytes)
            rc = -3
            if use_planes:
                s = torch.cuda.current_stream(gp.device)
                s.wait_event(planes.event)
                rc = L.gp2d_predict_ozaki_planes(*fit_args, _ptr(planes.bres), planes.nmod, 0, *out_args,
                                                 ctypes.c_void_p(s.cuda_stream))
                if rc != -3:   # −3: the fit needs more moduli than the planes carry → inline K*
                    N.check(rc, "gp2d_predict_ozaki_planes")
            if rc == -3:
                N.check(L.gp2d_predict_ozaki(*fit_args, int(bool(compute_var)), *out_args, _stream_handle(gp.device)),
                        "gp2d_predict_ozaki")
            return mean, (var if compute_var else None)
        args = (*_f64_fit_args(gp, G, desc), _VAR_MODES[var_mode], float(gp.noise), int(bool(compute_var)), _ptr(mean),
                _ptr(var), self.chunk, _ptr(self.work), self.wbytes, _stream_handle(gp.device))
        tr = gp.extra.get("trend")
        if tr is not None:   # α′ never reaches the plain predict: the trend's terms belong to it
            if self.trend_order != tr["order"]:
                raise ValueError("this Predictor's workspace was made for another trend order")
            N.check(L.gp2d_predict_trend(*args, *_trend_args(tr, term)), "gp2d_predict_trend")
        else:
            N.check(L.gp2d_predict(*args), "gp2d_predict")
        return mean, (var if compute_var else None)


def _trend_of(gp: GPFit, key: str):
    """gp.extra['trend'][key], or None for a zero-mean fit."""
    t = gp.extra.get("trend")
    return None if t is None else t[key]


def _trend_args(tr: dict, term: int | None) -> tuple:
    """What the trend predicts end with: the descriptor, the block, and whether h* is the basis
    (not for one term of a sum, whose mean carries no trend)."""
    return ctypes.byref(tr["desc"]), _ptr(tr["block"]), int(term is None)


def _term_kernel(gp: GPFit, term: int | None, var_mode: str = "latent") -> KernelSpec:
    """The kernel a predict passes to the library: the fit's, or for term=t of a kernel sum's fit
    the one-term sum (w_t, term t).  With y = Σ_t f_t + ε, cov(f_t(g), y) = w_t·K_t(g, X), so the
    fit's W and α with that kernel give term t's posterior mean w_t·K_t*·α and latent variance
    w_t·diag_t − ‖W·w_t·K_t*ᵀ‖²; a term is never observed, so there is no noisy variance."""
    if term is None:
        return gp.kernel
    if not gp.kernel.is_sum:
        raise ValueError("term= needs a fit of a kernel sum (family 'vector_sum')")
    if var_mode != "latent":
        raise ValueError("term= gives the latent variance only (var_mode='latent'): a term is never observed")
    return gp.kernel.term(term)


def predict(gp: GPFit, xg, var_mode: str = "latent", compute_var: bool = True, chunk: int = 8192,
            term: int | None = None):
    """Posterior mean and variance at xg ([u…, v…]).  term=t (a kernel sum's fit): the posterior of
    term t's contribution alone (_term_kernel); the term means add up to the full mean."""
    return _predictor_for(None, gp, chunk)(xg, var_mode=var_mode, compute_var=compute_var, term=term)


FIELDS = ("divergence", "vorticity")
_FIELD_CODES = {"divergence": N.FIELD_DIVERGENCE, "vorticity": N.FIELD_VORTICITY}


def _require_velocity(kernel: KernelSpec, needs: str, gp: GPFit | None = None, entry: str = ""):
    """ValueError(needs) unless the kernel is a div-free, curl-free or mixed vector kernel; for a
    fit, also unless it still has the factor W that `entry` contracts with."""
    kinds = [t.kind for t in kernel._sum_terms()] if kernel.is_sum else [kernel.kind]
    if not kernel.is_vector or any(kernel._KINDS[k] == N.KIND_SCALAR for k in kinds):
        raise ValueError(needs)
    if gp is not None and gp.W is None:
        raise ValueError(f"{entry} needs the fit's factor W = L⁻¹ (this fit keeps only its int8 planes)")


def _field_code(kernel: KernelSpec, field: str, gp: GPFit | None = None) -> int:
    """The library's code of a derived field, or ValueError for a field or kernel without one
    (or, given the fit to predict it from, a fit without W)."""
    if field not in _FIELD_CODES:
        raise ValueError(f"field must be one of {FIELDS}")
    _require_velocity(kernel, "derived fields need a div-free, curl-free or mixed vector kernel "
                              "(the scalar kind and the ARD family have none)", gp, "predict_field")
    return _FIELD_CODES[field]


def predict_field(gp: GPFit, xg, field: str, compute_var: bool = True, chunk: int = 8192,
                  term: int | None = None):
    """Posterior mean and latent variance of a derived scalar field of the fitted velocity, at the
    points xg: (mean, var) device tensors of shape (m,), var None if not asked.

    field: 'divergence' δ = ∂f1/∂x1 + ∂f2/∂x2 or 'vorticity' ζ = ∂f2/∂x1 − ∂f1/∂x2, for points
    (x1, x2) and components (f1, f2) = the first and second half of the observations.  With
    Krig.predict_grid's points (x, y) and components (u, v) these are ∂u/∂x + ∂v/∂y and
    ∂v/∂x − ∂u/∂y; a caller whose points are (Y, X) with observations [v; u] gets −ζ.
    A derivative of a GP is a GP: mean = cᵀα and var = prior − ‖W c‖² with the field's
    cross-covariance c and prior variance (gp2d_predict_field, DESIGN.md "Derived fields").  There is no
    noise or clipping mode: a derived field is never observed.  The divergence of a 'df' fit and
    the vorticity of a 'cf' fit are exact zeros.

    Works for fits of either variance engine — the contraction runs on the FP64 engine from the
    fit's W; gp.x, gp.alpha and gp.W share one point order.  ValueError for the scalar kind, the
    ARD family, and a fit without W (a job stream's receiving rank keeps only the int8 planes).
    term=t (a kernel sum's fit): the field of term t's contribution alone (_term_kernel)."""
    code = _field_code(gp.kernel, field, gp)
    L = N.lib()
    G = _as_points(xg, gp.kernel.input_dim, gp.device)
    m = G.shape[0]
    chunk = max(NB, (int(chunk) + NB - 1) // NB * NB)
    chunk = min(chunk, max(NB, (m + NB - 1) // NB * NB))   # no workspace beyond the points there are
    tr = gp.extra.get("trend")
    wbytes = int(L.gp2d_predict_field_workspace(gp.n, chunk)) if tr is None else \
        int(L.gp2d_predict_trend_workspace(gp.n, chunk, 1, tr["order"]))
    work = _workspace(wbytes, gp.device)
    mean = torch.empty(m, dtype=torch.float64, device=gp.device)
    var = torch.empty(m, dtype=torch.float64, device=gp.device) if compute_var else None
    desc = _term_kernel(gp, term).desc()
    args = (*_f64_fit_args(gp, G, desc), code, int(bool(compute_var)), _ptr(mean), None if var is None else _ptr(var),
            chunk, _ptr(work), wbytes, _stream_handle(gp.device))
    if tr is not None:   # the trend's own divergence / vorticity and its variance correction
        N.check(L.gp2d_predict_field_trend(*args, *_trend_args(tr, term)), "gp2d_predict_field_trend")
    else:
        N.check(L.gp2d_predict_field(*args), "gp2d_predict_field")
    return mean, var


GRADIENT_COMPONENTS = ("du_dx", "du_dy", "dv_dx", "dv_dy")
# the linear diagnostics as aᵀ∇f on (du_dx, du_dy, dv_dx, dv_dy)
_LINEAR_DIAGNOSTICS = {"divergence": (1.0, 0.0, 0.0, 1.0), "vorticity": (0.0, -1.0, 1.0, 0.0),
                       "normal_strain": (1.0, 0.0, 0.0, -1.0), "shear_strain": (0.0, 1.0, 1.0, 0.0)}
# Okubo–Weiss σ_n² + σ_s² − ζ² = (g0 − g3)² + 4·g1·g2 = gᵀAg
_OW_MATRIX = ((1.0, 0.0, 0.0, -1.0), (0.0, 0.0, 2.0, 0.0), (0.0, 2.0, 0.0, 0.0), (-1.0, 0.0, 0.0, 1.0))
DIAGNOSTICS = tuple(_LINEAR_DIAGNOSTICS) + ("okubo_weiss",)


def predict_gradient(gp: GPFit, xg, compute_cov: bool = True, chunk: int = 8192):
    """Posterior mean and covariance of the velocity gradient tensor at the points xg: device
    tensors (mean (m, 4), cov (m, 4, 4)), cov None if not asked.

    Components GRADIENT_COMPONENTS = (∂f1/∂x1, ∂f1/∂x2, ∂f2/∂x1, ∂f2/∂x2) for points (x1, x2) and
    components (f1, f2) = the first and second half of the observations — (∂u/∂x, ∂u/∂y, ∂v/∂x,
    ∂v/∂y) with Krig.predict_grid's conventions; predict_field's caveat for (Y, X) callers stands.
    cov[j] is the joint posterior covariance of the four at point j (exactly symmetric), not
    between points: what flow_diagnostics needs for the variance of every linear diagnostic and
    the moments of the Okubo–Weiss parameter.  One product of the velocity predict's kind on four
    columns per point, the 4 × 4 Gram formed in its epilogue (gp2d_predict_grad).
    No noise or clipping mode: a gradient is never observed.

    Works for fits of either variance engine, like predict_field.  ValueError for the scalar kind,
    the ARD family, a kernel sum, and a fit without W."""
    _refuse_sum(gp.kernel, "predict_gradient")
    refuse_trend(gp, "predict_gradient")
    _require_velocity(gp.kernel, "the velocity gradient needs a div-free, curl-free or mixed vector kernel "
                                 "(the scalar kind and the ARD family have none)", gp, "predict_gradient")
    L = N.lib()
    G = _as_points(xg, gp.kernel.input_dim, gp.device)
    m = G.shape[0]
    chunk = max(64, (int(chunk) + 63) // 64 * 64)
    chunk = min(chunk, max(64, (m + 63) // 64 * 64))   # no workspace beyond the points there are
    wbytes = int(L.gp2d_predict_grad_workspace(gp.n, chunk))
    work = _workspace(wbytes, gp.device)
    mean = torch.empty((m, 4), dtype=torch.float64, device=gp.device)
    cov = torch.empty((m, 4, 4), dtype=torch.float64, device=gp.device) if compute_cov else None
    desc = gp.kernel.desc()
    N.check(L.gp2d_predict_grad(*_f64_fit_args(gp, G, desc), int(bool(compute_cov)), _ptr(mean),
                                None if cov is None else _ptr(cov), chunk, _ptr(work), wbytes,
                                _stream_handle(gp.device)), "gp2d_predict_grad")
    return mean, cov


def flow_diagnostics(mean, cov=None, names=DIAGNOSTICS) -> dict:
    """Kinematic diagnostics of the flow from its gradient tensor: {name: (mean, var)} for
    predict_gradient's (mean (..., 4), cov (..., 4, 4)), torch tensors or numpy arrays alike; var
    is None without cov.

    'divergence' g0 + g3, 'vorticity' g2 − g1, 'normal_strain' g0 − g3 and 'shear_strain' g2 + g1
    are linear: aᵀμ and aᵀΣa.  'okubo_weiss' σ_n² + σ_s² − ζ² = gᵀAg is quadratic; for Gaussian g
    its mean is μᵀAμ + tr(AΣ) (μᵀAμ without cov) and its variance 2·tr(AΣAΣ) + 4·μᵀAΣAμ."""
    is_torch = isinstance(mean, torch.Tensor)

    def const(rows):
        if is_torch:
            return torch.tensor(rows, dtype=mean.dtype, device=mean.device)
        return np.asarray(rows, dtype=np.float64)

    out = {}
    for name in names:
        if name in _LINEAR_DIAGNOSTICS:
            a = const(_LINEAR_DIAGNOSTICS[name])
            out[name] = (mean @ a, None if cov is None else ((cov @ a) * a).sum(-1))
        elif name == "okubo_weiss":
            A = const(_OW_MATRIX)
            Am = mean @ A                                   # A symmetric: (Aμ)ᵀ
            mu = (Am * mean).sum(-1)
            if cov is None:
                out[name] = (mu, None)
                continue
            AS = A @ cov
            tr1 = AS[..., 0, 0] + AS[..., 1, 1] + AS[..., 2, 2] + AS[..., 3, 3]
            tr2 = (AS * AS.swapaxes(-1, -2)).sum((-1, -2))  # tr(AΣAΣ)
            quad = ((cov @ Am[..., None])[..., 0] * Am).sum(-1)
            out[name] = (mu + tr1, 2.0 * tr2 + 4.0 * quad)
        else:
            raise ValueError(f"diagnostic must be one of {DIAGNOSTICS}")
    return out


def advect_records(nsteps: int, save_every: int) -> int:
    """The records an advect call returns: 1 + ⌈nsteps / save_every⌉ (gp2d_advect_records)."""
    r = int(N.lib().gp2d_advect_records(int(nsteps), int(save_every)))
    if r < 0:
        raise ValueError(N.lib().gp2d_last_error().decode(errors="replace"))
    return r


def advect(gp: GPFit, x0, t0: float = 0.0, dt: float = None, nsteps: int = None, save_every: int | None = None,
           vel_scale: float = 1.0, tangent: bool = False):
    """Advect particles through the fitted mean flow: classical RK4 of dx/dt = s·μ(x, t) from the
    start positions x0 (m, 2) at time t0, nsteps steps of size dt (negative: backward in time), with
    s = vel_scale the factor from velocity units to position units per time unit (3.6: m/s → km/h).
    Returns device tensors (times (R,), path (R, m, 2), tangent (R, m, 2, 2) | None): record 0 is the
    start, record r the state after step min(r·save_every, nsteps); save_every=None records the end
    only.  tangent=True integrates the flow map's gradient F[a][b] = ∂x_a(t)/∂x_b(t0) along
    (dF/dt = s·∇μ·F, F(t0) = I; ftle() takes it); without it the gradient terms are not evaluated and
    the path is the same to the bit.

    Points (x1, x2) and components (f1, f2) = the first and second half of the observations:
    dx1/dt = s·f1, dx2/dt = s·f2, so points (Y, X) with observations [v; u] are consistent as they
    stand.  A 'vector_st' fit is evaluated at the stage's time t; the spatial families are steady.
    One fused kernel per record reads only gp.alpha, gp.x and the trend's β̂ (gp2d_advect, DESIGN.md
    §3.13): kernel sums and trend fits are covered, and a fit of either variance engine serves — α
    and x share the fit's order and the start points are the caller's —, also one without W.  A
    particle's results do not depend on the other particles of the call: x0 may be sharded freely.
    ValueError for the scalar kind and the ARD family."""
    _require_velocity(gp.kernel, "advection needs a div-free, curl-free or mixed vector kernel "
                                 "(the scalar kind and the ARD family have no velocity field to follow)")
    if dt is None or nsteps is None:
        raise ValueError("advect needs dt and nsteps")
    nsteps = int(nsteps)
    save_every = max(nsteps, 1) if save_every is None else int(save_every)
    R = advect_records(nsteps, save_every)
    L = N.lib()
    X0 = _as_points(x0, 2, gp.device)
    m = X0.shape[0]
    path = torch.empty((R, m, 2), dtype=torch.float64, device=gp.device)
    tan = torch.empty((R, m, 2, 2), dtype=torch.float64, device=gp.device) if tangent else None
    desc = gp.kernel.desc()
    tr = gp.extra.get("trend")
    targs = (None, None) if tr is None else (ctypes.byref(tr["desc"]), _ptr(tr["block"]))
    N.check(L.gp2d_advect(_ptr(gp.alpha), gp.n, _ptr(gp.x), gp.n_train, gp.n_pad, ctypes.byref(desc), *targs,
                          _ptr(X0), m, float(t0), float(dt), nsteps, save_every, float(vel_scale), _ptr(path),
                          None if tan is None else _ptr(tan), _stream_handle(gp.device)), "gp2d_advect")
    steps = torch.clamp(torch.arange(R, dtype=torch.float64, device=gp.device) * save_every, max=float(nsteps))
    return float(t0) + steps * float(dt), path, tan


def ftle(tangent, duration: float):
    """The finite-time Lyapunov exponent ln λ_max(FᵀF) / (2·|duration|) of flow-map gradients F
    (..., 2, 2) — advect's tangent at a record, `duration` the time integrated to it.  Ridges of the
    field over a grid of seeds are the transport barriers (repelling for dt > 0, attracting for
    dt < 0).  The closed form for a symmetric 2 × 2 matrix; pure torch, on any device, broadcasting
    over the leading dimensions."""
    F = torch.as_tensor(tangent)
    a, b, c, d = F[..., 0, 0], F[..., 0, 1], F[..., 1, 0], F[..., 1, 1]
    p, q, r = a * a + c * c, a * b + c * d, b * b + d * d   # FᵀF = [[p, q], [q, r]]
    lam = 0.5 * (p + r) + torch.sqrt(0.25 * (p - r) ** 2 + q * q)
    return torch.log(lam) / (2.0 * abs(float(duration)))


@dataclass
class FlowDraws:
    """S posterior draws of the flow as functions (draw_flows):
    g_s(x, t) = f_s(x, t) + K((x, t), X)·α_s, with f_s the draw's random Fourier features."""
    gp: GPFit
    alpha: torch.Tensor      # (S, n) device: α_s in the fit's order and padded layout
    features: torch.Tensor   # (S, F_tot, 6) device: rows [τ, w1, w2, b, a1, a2]

    @property
    def n_draws(self) -> int:
        return self.alpha.shape[0]

    def _fit_args(self, desc) -> tuple:
        gp = self.gp
        return (_ptr(self.alpha), gp.n, _ptr(gp.x), gp.n_train, gp.n_pad, ctypes.byref(desc),
                _ptr(self.features), self.features.shape[1], self.n_draws)

    def velocity(self, xg, t: float = 0.0) -> torch.Tensor:
        """The drawn velocities at the points xg (m, 2) and time t: (S, 2m) on the device, each row
        [u(g_1..g_m), v(g_1..g_m)] — sample_posterior's layout (gp2d_paths_eval)."""
        gp = self.gp
        G = _as_points(xg, 2, gp.device)
        m = G.shape[0]
        vel = torch.empty((self.n_draws, 2 * m), dtype=torch.float64, device=gp.device)
        desc = gp.kernel.desc()
        N.check(N.lib().gp2d_paths_eval(*self._fit_args(desc), _ptr(G), m, 2, float(t), _ptr(vel),
                                        _stream_handle(gp.device)), "gp2d_paths_eval")
        return vel


def _draw_matrix(a, shape: tuple, name: str, device) -> torch.Tensor:
    t = a.to(device=device, dtype=torch.float64) if isinstance(a, torch.Tensor) else \
        torch.as_tensor(np.ascontiguousarray(np.asarray(a, dtype=np.float64)), device=device)
    if tuple(t.shape) != shape:
        raise ValueError(f"{name} must have shape {shape}; got {tuple(t.shape)}")
    return t.contiguous()


def draw_flows(gp: GPFit, n_draws: int, n_features: int = 1024, seed: int = 0, features=None, eps=None) -> FlowDraws:
    """n_draws posterior draws of the flow as functions that can be evaluated anywhere — what a
    moving particle needs (advect_draws).  Pathwise conditioning (Matheron's rule; Wilson et al.
    2020): g_s = f_s + K(·, X)·α_s with α_s = K_y⁻¹(y − f_s(X) − ε_s), f_s a prior draw of
    n_features random Fourier features per kernel part (paths.feature_table; every draw has its own,
    so the ensemble's mean and covariance are exactly the posterior's) and ε_s ~ N(0, (noise +
    jitter)·I).  Both come from CPU generators seeded with `seed` (the same seed gives the same
    draws on any machine) or are passed in: features (S, F_tot, 6), eps (S, 2·n_train) in the
    caller's observation order [u…, v…].

    Builds the table, then the residuals R (S × n, padded rows zero) with f_s(X) from
    gp2d_paths_eval at the training points in the fit's own order, then α = R·Wᵀ·W as two products
    on the FP64 GEMM core with the draws as rows (gemm).  A fit of either variance engine serves if
    it holds W and its observations; an ozaki fit's Morton order is applied to eps.  ValueError,
    before any device work, for a trend fit (the vague prior on β has no prior draw), a fit without
    W or without y, the scalar kind and the ARD family."""
    from . import paths as P
    if gp.extra.get("trend") is not None:
        raise ValueError("draw_flows does not support a background flow (trend=): the vague prior on the trend's "
                         "coefficients has no prior draw")
    _require_velocity(gp.kernel, "posterior flow draws need a div-free, curl-free or mixed vector kernel "
                                 "(the scalar kind and the ARD family have no velocity field to follow)")
    if gp.W is None:
        raise ValueError("draw_flows needs the fit's factor W = L⁻¹ for K_y⁻¹ = WᵀW (this fit keeps only its int8 "
                         "planes)")
    if gp.y is None:
        raise ValueError("draw_flows needs the fit's observations y (this fit was not made by engine.fit)")
    S = int(n_draws)
    if S < 1:
        raise ValueError("n_draws must be at least 1")
    ntr, npad, n, dev = gp.n_train, gp.n_pad, gp.n, gp.device
    if features is None:
        features = P.feature_table(gp.kernel, S, n_features, seed)
    elif np.ndim(features) != 3 or np.shape(features)[0] != S or np.shape(features)[2] != P.FEATURE_WIDTH:
        raise ValueError(f"features must have shape (n_draws, F_tot, {P.FEATURE_WIDTH}); got {tuple(np.shape(features))}")
    if eps is None:
        eps = P.noise_draws(S, 2 * ntr, _cv_diag_add(gp), seed)
    gp.check()
    feat = _draw_matrix(features, tuple(np.shape(features)), "features", dev)
    E_ = _draw_matrix(eps, (S, 2 * ntr), "eps", dev).view(S, 2, ntr)
    if gp.perm is not None:   # sorted point i is input point perm[i]
        E_ = E_.index_select(2, gp.perm.to(torch.int64))
    L = N.lib()
    fX = torch.empty((S, 2, ntr), dtype=torch.float64, device=dev)   # f_s(X), the fit's order
    N.check(L.gp2d_paths_eval(None, 0, None, 0, 0, None, _ptr(feat), feat.shape[1], S, _ptr(gp.x), ntr,
                              gp.kernel.input_dim, 0.0, _ptr(fX), _stream_handle(dev)), "gp2d_paths_eval")
    R = torch.zeros((S, 2, npad), dtype=torch.float64, device=dev)
    R[:, :, :ntr] = gp.y.view(2, npad)[None, :, :ntr] - fX - E_
    T = gemm(R.view(S, n), gp.W, transb=True, device=dev)
    alpha = gemm(T, gp.W, device=dev).contiguous()
    return FlowDraws(gp=gp, alpha=alpha, features=feat)


def advect_draws(draws: FlowDraws, x0, t0: float = 0.0, dt: float = None, nsteps: int = None,
                 save_every: int | None = None, vel_scale: float = 1.0):
    """Advect particles through every drawn flow: advect's RK4 of dx/dt = s·g_s(x, t) per draw.
    x0: (m, 2), one start set shared by the draws, or (S, m, 2), the caller's own uncertainty of the
    start.  Returns device tensors (times (R,), paths (R, S, m, 2)); the arguments are advect's.
    One fused kernel per record (gp2d_advect_draws): the update term is advect's training-point sum
    with the draw's α, the prior term a sum of the same shape over the draw's features.  A (draw,
    particle)'s results do not depend on the other draws or particles of the call."""
    if dt is None or nsteps is None:
        raise ValueError("advect_draws needs dt and nsteps")
    gp, S = draws.gp, draws.n_draws
    nsteps = int(nsteps)
    save_every = max(nsteps, 1) if save_every is None else int(save_every)
    R = advect_records(nsteps, save_every)
    per_draw = int(np.ndim(x0) == 3)
    if per_draw and np.shape(x0)[0] != S:
        raise ValueError(f"x0 must be (m, 2) or (n_draws, m, 2) with n_draws = {S}; got {tuple(np.shape(x0))}")
    X0 = _as_points(x0, 2, gp.device)
    m = X0.shape[0] // S if per_draw else X0.shape[0]
    path = torch.empty((R, S, m, 2), dtype=torch.float64, device=gp.device)
    desc = gp.kernel.desc()
    N.check(N.lib().gp2d_advect_draws(*draws._fit_args(desc), _ptr(X0), m, per_draw, float(t0), float(dt), nsteps,
                                      save_every, float(vel_scale), _ptr(path), _stream_handle(gp.device)),
            "gp2d_advect_draws")
    steps = torch.clamp(torch.arange(R, dtype=torch.float64, device=gp.device) * save_every, max=float(nsteps))
    return float(t0) + steps * float(dt), path


def path_spread(paths):
    """The ensemble's position statistics per record and particle: (mean (R, m, 2), cov (R, m, 2, 2),
    count (R, m)) of advect_draws' paths (R, S, m, 2) over the draws — the covariance unbiased
    (1/(count − 1); NaN where fewer than two draws are left).  A draw whose position is NaN (a
    non-finite start) is left out and count says how many were kept.  Pure torch, on any device."""
    P_ = torch.as_tensor(paths)
    ok = torch.isfinite(P_).all(-1)                        # (R, S, m)
    cnt = ok.sum(1)                                        # (R, m)
    z = torch.where(ok[..., None], P_, torch.zeros_like(P_))
    mean = z.sum(1) / cnt[..., None]
    d = torch.where(ok[..., None], P_ - mean[:, None], torch.zeros_like(P_))
    cov = torch.einsum("rsma,rsmb->rmab", d, d) / (cnt - 1).clamp(min=0)[..., None, None]
    cov = torch.where((cnt > 1)[..., None, None], cov, torch.full_like(cov, float("nan")))
    return mean, cov, cnt


def _predict_cov_padded(gp: GPFit, xg, diag_add: float):
    """gp2d_predict_cov: (mean (2m,), the padded q × q covariance, m, mp) on the device."""
    _refuse_sum(gp.kernel, "predict_cov")
    refuse_trend(gp, "predict_cov / sample_posterior")
    _require_velocity(gp.kernel, "the joint covariance needs a div-free, curl-free or mixed vector kernel "
                                 "(the scalar kind and the ARD family are not supported)", gp, "predict_cov")
    L = N.lib()
    G = _as_points(xg, gp.kernel.input_dim, gp.device)
    m = G.shape[0]
    if m < 1:
        raise ValueError("need at least one target point")
    mp = padded_points(m)
    q = 2 * mp
    wbytes = int(L.gp2d_predict_cov_workspace(gp.n, m))
    work = _workspace(wbytes, gp.device)
    mean = torch.empty(2 * m, dtype=torch.float64, device=gp.device)
    cov = torch.empty((q, q), dtype=torch.float64, device=gp.device)
    desc = gp.kernel.desc()
    N.check(L.gp2d_predict_cov(*_f64_fit_args(gp, G, desc), float(diag_add), _ptr(mean), _ptr(cov), q,
                               _ptr(work), wbytes, _stream_handle(gp.device)), "gp2d_predict_cov")
    return mean, cov, m, mp


def _valid_index(m: int, mp: int, device) -> torch.Tensor:
    """Rows of the padded component-major layout that belong to the m points: [u(0..m), v(0..m)]."""
    r = torch.arange(m, device=device)
    return torch.cat([r, mp + r])


def predict_cov(gp: GPFit, xg, diag_add: float = 0.0):
    """Posterior mean and JOINT covariance of the velocity at the points xg: device tensors
    (mean (2m,), cov (2m, 2m)), component-major [u(g_1..g_m), v(g_1..g_m)] like the mean.

    cov = K(g, g) − K*·K_y⁻¹·K*ᵀ + diag_add·I, the matrix the reference forms before it takes the
    diagonal (GP_laser.py:128-129), sklearn's predict(return_cov=True) and, with diag_add = noise,
    GPy's predict(full_cov=True).  Its diagonal is predict's latent variance; the matrix is exactly
    symmetric.  The mean is bit for bit gp2d_predict's.  Dense in the targets: 8·(2·⌈m/64⌉·64)²
    bytes plus two n × q work matrices.

    Works for fits of either variance engine (the product runs on the FP64 engine from the fit's
    W; gp.x, gp.alpha and gp.W share one point order).  ValueError for the scalar kind, the ARD
    family, and a fit without W."""
    mean, cov, m, mp = _predict_cov_padded(gp, xg, diag_add)
    if m == mp:
        return mean, cov
    idx = _valid_index(m, mp, gp.device)
    return mean, cov.index_select(0, idx).index_select(1, idx)


def _jitchol(A: torch.Tensor, maxtries: int, rows: torch.Tensor | None = None):
    """jitchol's (L, jitter, retries taken).  rows: the rows whose diagonal entries set the
    schedule's mean(diag) (all by default; sample_posterior leaves out the padding's ones)."""
    n = A.shape[0]
    if A.dim() != 2 or A.shape[1] != n or n % NB or n < NB or not A.is_cuda or A.dtype != torch.float64 \
            or not A.is_contiguous():
        raise ValueError("jitchol: A must be a contiguous float64 device matrix of order a multiple of 128")
    dev = A.device
    _require_device(dev)
    L = N.lib()
    A0 = A.clone()   # gp2d_potrf overwrites A, failed or not
    dinv = torch.empty((n // NB, NB, NB), dtype=torch.float64, device=dev)
    info = torch.empty(1, dtype=torch.int32, device=dev)

    def factor() -> bool:
        N.check(L.gp2d_potrf(_ptr(A), n, n, _ptr(dinv), _ptr(info), None, 0, _stream_handle(dev)), "gp2d_potrf")
        return int(info.item()) == 0

    if factor():
        return A, 0.0, 0
    d0 = A0.diagonal()
    diag = float(np.mean((d0 if rows is None else d0.index_select(0, rows)).cpu().numpy()))
    if not (np.isfinite(diag) and diag > 0.0):
        raise np.linalg.LinAlgError("not pd: non-positive diagonal elements")
    jit = diag * 1e-6
    for t in range(1, int(maxtries) + 1):
        if not np.isfinite(jit):
            break
        A.copy_(A0)
        A.diagonal().add_(jit)
        if factor():
            return A, jit, t
        jit *= 10.0
    raise np.linalg.LinAlgError("not positive definite, even with jitter.")


def jitchol(A: torch.Tensor, maxtries: int = 5):
    """Cholesky factor of a device SPD matrix with GPy's jitchol retry: (L, jitter).

    A (order a multiple of 128, contiguous float64) is factored IN PLACE by gp2d_potrf: on return
    it holds L (lower, zeros above) with L·Lᵀ = A + jitter·I.  jitter is 0.0 when the plain
    factorisation succeeds; otherwise the schedule fit(jitchol=k) documents — mean(diag A)·1e-6,
    ten times larger on each further try, up to maxtries tries — and numpy.linalg.LinAlgError after
    the last (A then holds the last failed try).  A failed factorisation is a status word, never a
    device fault.  Costs one copy of A, kept for the retries."""
    L, jit, _ = _jitchol(A, maxtries)
    return L, jit


def sample_posterior(gp: GPFit, xg, n_samples: int, seed: int = 0, z: torch.Tensor | None = None,
                     jitter: float = 0.0, maxtries: int = 5):
    """Conditional simulations: n_samples joint draws of the velocity at the points xg from the
    posterior N(mean, Σ) — sklearn's sample_y, GPy's posterior_samples_f.  Returns (samples
    (S, 2m) on the device, each row [u(g_1..g_m), v(g_1..g_m)], info).

    samples = mean + (L·z)ᵀ with L·Lᵀ = Σ + (jitter + retry jitter)·I, Σ the latent covariance of
    predict_cov on its padded layout, factored by jitchol: the Σ of a dense grid is numerically
    singular (smallest eigenvalue at rounding level, either sign), so the retry is part of the
    contract (its mean(diag) is taken over Σ's own diagonal, without the padding's ones).  info =
    {'jitter': the total added to the diagonal, 'tries': retries taken (0: the first factorisation
    succeeded)}.  z: (2m, S) standard normals in the component order; by default
    torch.randn on the device from a torch.Generator seeded with `seed` (the same seed gives the
    same samples).  L·z runs on the FP64 GEMM core (gemm)."""
    mean, cov, m, mp = _predict_cov_padded(gp, xg, 0.0)
    dev = gp.device
    S = int(n_samples)
    if z is None:
        if S < 1:
            raise ValueError("n_samples must be at least 1")
        g = torch.Generator(device=dev)
        g.manual_seed(int(seed))
        z = torch.randn((2 * m, S), generator=g, device=dev, dtype=torch.float64)
    else:
        z = _as_matrix(z, dev)
        if tuple(z.shape) != (2 * m, S):
            raise ValueError(f"z must have shape (2m, n_samples) = ({2 * m}, {S}); got {tuple(z.shape)}")
    if jitter:
        cov.diagonal().add_(float(jitter))
    # padded points are identity rows and columns, decoupled from the rest: the valid rows and
    # columns of L are the factor of the valid part of Σ, and the schedule's mean(diag) is Σ's
    idx = _valid_index(m, mp, dev)
    L, jit, tries = _jitchol(cov, maxtries, rows=idx)
    Lv = L if m == mp else L.index_select(0, idx).index_select(1, idx)
    samples = gemm(Lv, z, device=dev).t() + mean[None, :]
    return samples.contiguous(), {"jitter": float(jitter) + jit, "tries": tries}


def note_guard(stats: dict | None, gp: GPFit):
    """Record a checked fit's accuracy-guard decision in a job stream's `stats` (stats['guard'],
    one dict per job in job order: engine, wbits, kbits, vmin_over_kss, wmax, est)."""
    if stats is not None:
        g = gp.extra.get("guard")
        stats.setdefault("guard", []).append(
            {k: v for k, v in g.items() if k in ("engine", "wbits", "kbits", "vmin_over_kss", "wmax", "est")}
            if g else None)


def note_fit_issued(stats: dict | None):
    """Count a fit enqueued by a job stream (krige_jobs / krige_jobs_sharded) with its host
    time stamp — bench.py checks that every timed job's fit is issued inside its clock."""
    if stats is not None:
        stats["fits_issued"] = stats.get("fits_issued", 0) + 1
        stats.setdefault("fit_issue_times", []).append(time.perf_counter())


def krige_jobs(jobs, variance: str = "ozaki", chunk: int = 8192, var_mode: str = "latent",
               compute_var: bool = True, jitter: float = 0.0, device=None, stats: dict | None = None,
               fits_ahead: int | None = None, batch_fits: int | None = None,
               batch_ahead: bool | None = None, trend: str | None = None):
    """Independent kriging jobs (kernel, x, y, noise, xg), one after another — the reference's
    runKrig.py:1-40 sweep (one GP_laser / krig.kriging fit + grid predict per setting or
    time window) run in one process.  Yields (mean, var) per job, in order, on the current
    stream; results are bit-identical to fit() + Predictor() called per job.

    Job i+1's fit is queued on a side stream as soon as job i's predict is, so the factor
    (latency-bound, a few hundred workgroups) runs on the CUs the predict's GEMMs leave idle
    (bench.py --pipeline).  The fit of job i+1 waits for the work queued on the
    current stream before it (so input tensors made there are ready); a non-SPD K_y of job i
    raises numpy.linalg.LinAlgError when job i is yielded, as fit() would.  The predict
    workspace is reused while consecutive jobs have the same padded size.  Nothing is read
    ahead before the first next(): a fresh generator's first fit is issued by that call (the
    bench times its jobs on a fresh generator for this reason).  `stats` counts the fits issued.

    fits_ahead = k > 1: up to k fits in flight on k side streams, each queued before the
    predict stream waits for the job ahead of it, so consecutive fits also overlap each other
    (gp2d_potrf draws a separate internal stream set per call).  fits_ahead = 0: each job's fit
    and predict strictly one after the other on the current stream — the fastest form for small
    jobs whose latency-bound fit outlasts their predict (config B: a fit beside a predict runs
    ≈ 2.4× longer).  fits_ahead = None (default): auto_fits_ahead() on the first
    job's shape — 1 where its predict outlasts its fit enough to hide it, else 0.

    batch_fits = b > 1 (with fits_ahead = 0): the next b jobs of one matrix order are fitted
    together (engine.fit_batch: one batched factorisation, the fit's latency-bound chain paid
    once per b jobs), then predicted one by one; same bits.  batch_fits = None (default):
    auto_fit_batch() for the back-to-back form, 1 otherwise.  batch_ahead=True: batch g+1's fit
    on a side stream under batch g's predicts; None (default): auto_batch_ahead() on the first
    job's shape."""
    refuse_trend(trend, "krige_jobs", ": fit and predict each job with engine.fit(trend=) and engine.predict")
    dev = _require_device(device)
    main = torch.cuda.current_stream(dev)
    first, it = _peek(iter(jobs))
    if first is None:
        return
    _check_family(first[0], variance)   # a kernel sum on the int8 engine: refused before anything is issued
    n_sides, b, targets = _job_schedule(*_job_mode(first, variance, compute_var, fits_ahead, batch_fits, batch_ahead))
    sides = [side_stream(dev) for _ in range(n_sides)]
    prev_sets = N.lib().gp2d_factor_sets(n_sides) if n_sides > 1 else None   # one internal factor set per side stream
    pred = None

    def issue(group, index):
        s, join = _fit_slot(index, n_sides)
        side = None if s is None else sides[s]
        if side is not None:
            side.wait_stream(main)
        for _ in group:
            note_fit_issued(stats)
        kw = dict(jitter=jitter, device=dev, variance=variance, check=False, join=join)
        with torch.cuda.stream(side):   # no side stream: the current one
            if b == 1:
                kernel, x, y, noise, _ = group[0]
                return [fit(kernel, x, y, noise, **kw)], side
            return fit_batch([job[:4] for job in group], **kw), side

    def predict(job, gp):
        nonlocal pred
        hand_over(gp, stats, main if sides else None)
        pred, out = _predict_job(pred, gp, job[4], chunk, var_mode, compute_var)
        return out

    try:
        yield from _run_schedule(_job_groups(it, b, variance), targets, issue,
                                 lambda issued: take_fits(*issued, main), predict)
    finally:
        if prev_sets is not None:
            N.lib().gp2d_factor_sets(prev_sets)


def _peek(it):
    """(the iterator's first item or None, an iterator that still yields it)."""
    first = next(it, None)
    return first, (it if first is None else itertools.chain([first], it))


def _predictor_for(pred, gp: GPFit, chunk: int) -> Predictor:
    """A job stream's predict workspace for `gp`: the previous one while it fits, else a new one."""
    if pred is None or not pred.fits(gp):
        pred = Predictor(gp, chunk)
    pred.gp = gp
    return pred


def _predict_job(pred, gp: GPFit, xg, chunk: int, var_mode: str, compute_var: bool):
    """One job's predict on the current stream: (the workspace to hand to the next job, (mean, var))."""
    pred = _predictor_for(pred, gp, chunk)
    return pred, pred(xg, var_mode=var_mode, compute_var=compute_var, reuse_grid=True)


def _point_count(x, dim: int) -> int:
    if isinstance(x, torch.Tensor):
        return x.numel() // dim
    return int(np.size(x)) // dim


# job-shape model of auto_fits_ahead, fitted to the one-GPU measurements of DESIGN.md §6
# (profiles/r03_problem_sizes.txt, r03_ring_depth_E_B_ab.txt): a job's predict takes ≈ 1 ms +
# 48 ms · (M / 65,536) · (N / 4096)² on the Ozaki engine (×2.5 on FP64), its fit ≈ 0.061 ms ·
# (n / 128)^1.3 (2.24 ms at n = 2048, 13.6 ms at n = 8192), and a fit beside a predict runs
# ≈ 2.4× longer than alone (its dependent chain is dispatched behind the predict's GEMMs)
_PRED_MS_REF, _FIT_MS_COEF, _FIT_MS_EXP, _FIT_STRETCH = 48.0, 0.061, 1.3, 2.4


def _predict_ms_model(kernel: KernelSpec, n: int, m_grid: int, variance: str, compute_var: bool) -> float:
    scale = (m_grid / 65536.0) * (n / (2.0 * 4096)) ** 2 * (kernel.block_dim / 2.0)
    p = (1.0 + _PRED_MS_REF * scale) * (1.0 if variance == "ozaki" else 2.5)
    return 1.0 + 0.1 * (p - 1.0) if not compute_var else p


def auto_batch_ahead(kernel: KernelSpec, n_train: int, m_grid: int, b: int, variance: str = "ozaki",
                     compute_var: bool = True) -> bool:
    """krige_jobs' default for batched back-to-back jobs: batch g+1's fit under batch g's
    predicts when the batch's predicts outlast its stretched fit by the model of auto_fits_ahead,
    with the batched fit ≈ max(f·(1 + 0.15·(b − 1)), b·(2n³/3) / 46 TF/s) (chain-bound small
    batches, FLOP-bound large ones; profiles/r04_fit_batch.jsonl).  Config B (b = 8): 8.8e6 vs
    7.8e6 points/s back to back; with b = 4, 7.1e6 (profiles/r04_batch_ahead_ab.txt)."""
    if b <= 1:
        return False
    _, n = fit_layout(kernel, max(1, int(n_train)), variance)
    f1 = _FIT_MS_COEF * (n / NB) ** _FIT_MS_EXP
    fb = max(f1 * (1.0 + 0.15 * (b - 1)), b * (2.0 * n ** 3 / 3.0) / 46e9)
    return b * _predict_ms_model(kernel, n, m_grid, variance, compute_var) > (_FIT_STRETCH - 1.0) * fb


def auto_fits_ahead(kernel: KernelSpec, n_train: int, m_grid: int, variance: str = "ozaki",
                    compute_var: bool = True) -> int:
    """krige_jobs' default fits in flight for jobs of this shape: 1 (job i+1's fit under job
    i's predict) when that is faster by the model above, else 0 (each job's fit and predict back
    to back).  A pipelined job takes max(p, 2.4·f) + the fit's displaced GEMM work (≈ 0.1·p),
    a serial one f + p, so the overlap pays when p > 1.4·f.  Measured: config B (N = 1024, 128²
    grid) 4.19e6 points/s back to back vs 2.8–3.3e6 with one fit in flight; the headline
    (N = 4096, 256²) 55.7 vs 61.3 ms per job with one."""
    _, n = fit_layout(kernel, max(1, int(n_train)), variance)
    p = _predict_ms_model(kernel, n, m_grid, variance, compute_var)
    f = _FIT_MS_COEF * (n / NB) ** _FIT_MS_EXP
    return 1 if p > (_FIT_STRETCH - 1.0) * f else 0


FIT_BATCH_MAX = 8
FIT_BATCH_MAX_SMALL = 16        # matrix order ≤ FIT_BATCH_SMALL_N: the chain-bound sizes
FIT_BATCH_SMALL_N = 2048
FIT_BATCH_MAX_BYTES = 16 << 30   # two batches in flight (batch_ahead: g predicted, g+1 fitted)


def fit_problem_bytes(n: int) -> int:
    """Device bytes one problem of a batched fit holds: its n×n matrix (W in place) and its share
    of the TRTRI workspace ((n/2 + NB)² doubles) — the estimate of auto_fit_batch and
    hyper.auto_batch."""
    return 8 * (n * n + (n // 2 + NB) ** 2)


def auto_fit_batch(kernel: KernelSpec, n_train: int, variance: str = "ozaki") -> int:
    """krige_jobs' default batch for back-to-back jobs: up to FIT_BATCH_MAX fits per batched
    factorisation (FIT_BATCH_MAX_SMALL for matrix orders ≤ FIT_BATCH_SMALL_N, whose fit is the
    diagonal chain's latency) while TWO batches' matrices (batch_ahead keeps the predicted batch
    and the next one alive) stay below FIT_BATCH_MAX_BYTES.
    Measured (profiles/r04_fit_batch.jsonl): N_train = 1024, 1/2/4/8 fits in 2.27 / 2.56 / 3.20 /
    4.67 ms (2.28 ms each alone); 4096: 8 fits in 64 ms (13.4 each).  Config B's job stream
    (N_train = 1024, profiles/r04_bfit16_ab.jsonl): 8.33–8.38e6 points/s with 8 fits per batch,
    9.39–9.46e6 with 16, 9.24–9.27e6 with 32."""
    _, n = fit_layout(kernel, max(1, int(n_train)), variance)
    cap = FIT_BATCH_MAX_SMALL if n <= FIT_BATCH_SMALL_N else FIT_BATCH_MAX
    return max(1, min(cap, FIT_BATCH_MAX_BYTES // (2 * fit_problem_bytes(n))))


def _job_mode(first, variance, compute_var, fits_ahead, batch_fits, batch_ahead):
    """krige_jobs' (fits_ahead, batch_fits, batch_ahead) for a stream whose first job is `first`:
    what the caller passed, None replaced by the auto_* rule on that job's shape; a batch only
    with fits_ahead = 0, batch_ahead only for a batch of more than one fit."""
    kernel, x, xg = first[0], first[1], first[4]
    ntr, m = _point_count(x, kernel.input_dim), _point_count(xg, kernel.input_dim)
    if fits_ahead is None:
        fits_ahead = auto_fits_ahead(kernel, ntr, m, variance, compute_var)
    fits_ahead = max(0, int(fits_ahead))
    if fits_ahead == 0 and batch_fits is None:
        batch_fits = auto_fit_batch(kernel, ntr, variance)
    if fits_ahead > 0 or int(batch_fits) <= 1:
        return fits_ahead, 1, False
    if batch_ahead is None:
        batch_ahead = auto_batch_ahead(kernel, ntr, m, int(batch_fits), variance, compute_var)
    return fits_ahead, int(batch_fits), bool(batch_ahead)


def _job_schedule(fits_ahead: int, b: int, batch_ahead: bool):
    """(side streams, jobs per fit, (before, after_take, after_first)) of a job stream's mode.
    The targets are queue lengths of _run_schedule: groups issued before the head group is taken,
    after its hand-over, and after its first predict."""
    if fits_ahead > 1:
        # k fits in flight, each queued before the predict stream waits for the job ahead of it, so
        # consecutive fits also overlap each other (gp2d_potrf draws a factor stream set per side):
        # config B 3.8e6 points/s with two fits in flight, 2.8–3.3e6 with one
        # (profiles/r03_ring_depth_E_B_ab.txt)
        return fits_ahead, 1, (fits_ahead, 0, 0)
    if fits_ahead == 1:
        # job i+1's fit under job i's predict: the headline 55.7 vs 61.3 ms per job back to back
        # (auto_fits_ahead, profiles/r03_problem_sizes.txt)
        return 1, 1, (1, 1, 0)
    if batch_ahead:
        # batch g+1's fit under batch g's predicts, queued after the first of them: config B
        # 8.8e6 vs 7.8e6 points/s back to back (profiles/r04_batch_ahead_ab.txt)
        return 1, b, (1, 0, 1)
    # back to back on the current stream: a small job's fit beside a predict runs ≈ 2.4× longer
    # (config B 4.19e6 points/s vs 2.8–3.3e6 with one fit in flight; batches of b fits pay the
    # fit's chain once, profiles/r04_fit_batch.jsonl)
    return 0, b, (1, 0, 0)


def _fit_slot(index: int, n_sides: int):
    """(side stream, join) of a job stream's index-th issue: the sides in turn, none (the current
    stream, fit's default join) without sides.  With one side the first fit has no predict to
    overlap, so it joins on the host: no wait is left pending on the side stream beside its chain
    (fit(join=...))."""
    if n_sides == 0:
        return None, None
    return index % n_sides, n_sides == 1 and index == 0


def _job_groups(jobs, b, variance):
    """Consecutive jobs in groups of up to b with one matrix order (a job of another order starts
    the next group)."""
    if b == 1:   # one job per fit: no layout to compare, and no job read before it is issued
        yield from ([job] for job in jobs)
        return
    group, n0 = [], None
    for job in jobs:
        n1 = fit_layout(job[0], _point_count(job[1], job[0].input_dim), variance)[1]
        if group and (n1 != n0 or len(group) == b):
            yield group
            group = []
        group.append(job)
        n0 = n1
    if group:
        yield group


def _run_schedule(groups, targets, issue, take, predict):
    """A job stream's one loop.  issue(group, index) queues a group's fit and returns what
    take(issued) needs to hand it over; take returns one (fit, error) per job of the group;
    predict(job, fit) returns the job's result.  fill(t) issues groups until t are queued, so the
    three targets say when the next fit is issued (_job_schedule) and nothing else differs between
    the forms.  An error is raised when its own job is reached."""
    before, after_take, after_first = targets
    queue, index = collections.deque(), itertools.count()

    def fill(target):
        while len(queue) < target:
            group = next(groups, None)
            if group is None:
                return
            queue.append((group, issue(group, next(index))))

    while True:
        fill(before)
        if not queue:
            return
        group, issued = queue.popleft()
        taken = take(issued)
        fill(after_take)
        for q, (job, (gp, err)) in enumerate(zip(group, taken)):
            if err is not None:
                raise err
            out = predict(job, gp)
            if q == 0:
                fill(after_first)
            yield out


def take_fits(fits, stream, main, ready=None):
    """Hand a group of check=False fits over to the predict stream `main`: every fit's status and
    accuracy guard (GPFit.check) under `stream`, the one they were issued on (None: the current
    one), so a guard that re-prepares planes queues that work there — the host waits for these
    fits only, which ran under the previous predicts, never the GPU for the host.  Then, the fits
    having run elsewhere, `main` waits for `ready` (an event recorded after them) or else for
    `stream`: by now that stream holds this group's fits and their guards' work and nothing later,
    because no schedule issues the next group before the head has been taken.  Returns one (fit,
    error or None) per fit; the caller raises an error at its own job."""
    taken = []
    for gp in fits:
        try:
            with torch.cuda.stream(stream):
                gp.check()
            taken.append((gp, None))
        except Exception as e:   # noqa: BLE001 — re-raised when its job is reached
            taken.append((gp, e))
    if ready is not None:
        main.wait_event(ready)
    elif stream is not None:
        main.wait_stream(stream)
    return taken


def hand_over(gp: GPFit, stats: dict | None, main=None):
    """A taken fit's last step before its predict: the guard's decision into `stats`, and — main:
    the predict stream, when the fit ran on another — the guard's own work and the allocator's
    bookkeeping on `main`."""
    note_guard(stats, gp)
    if main is not None:
        gp.ready_on(main).record_stream(main)


# ------------------------------------------------------------------ hyperparameters
def param_names(kernel: KernelSpec) -> tuple:
    """Gradient / parameter order of log_marginal_likelihood: vector2d (l_df, l_cf, ratio, noise);
    vector_st (l_df, l_cf, ratio, var_t, l_t, noise); ARD per term (variance, lengthscale_0..D−1),
    then noise (GPy param_array order, krig.py:459-466); a kernel sum per term t (weight_t, l_df_t,
    l_cf_t, ratio_t[, var_t_t, l_t_t]), then noise."""
    if kernel.family == "vector_sum":
        names = []
        for t, k in enumerate(kernel._sum_terms()):
            names += [f"weight_{t}"] + [f"{n}_{t}" for n in param_names(k)[:-1]]
        return tuple(names + ["noise"])
    if kernel.family == "vector2d":
        return ("l_df", "l_cf", "ratio", "noise")
    if kernel.family == "vector_st":
        return ("l_df", "l_cf", "ratio", "var_t", "l_t", "noise")
    names = []
    for t, ls in enumerate(kernel.lengthscales):
        names += [f"variance_{t}"] + [f"lengthscale_{t}_{d}" for d in range(len(ls))]
    return tuple(names + ["noise"])


def log_marginal_likelihood(gp: GPFit, eval_gradient: bool = False):
    """log p(y | X, θ) of a fit, and optionally ∂/∂θ in natural units (param_names order).

    Replaces the objective of GPy model.optimize (krig.py:450; GP_plots.py:673-765) and
    sklearn log_marginal_likelihood(theta, eval_gradient=True) (_gpr.py:584-650); the
    gradient is the exact one (the reference's myKernel.update_gradients_full is not,
    SURVEY.md §0.2).  Both run in HIP kernels (gp2d_lml, gp2d_lml_grad)."""
    out, g = lml_device(gp, eval_gradient)
    if not eval_gradient:
        return float(out.item())
    return float(out.item()), g.cpu().numpy()


def lml_device(gp: GPFit, eval_gradient: bool = False):
    """log_marginal_likelihood without a host round trip: (lml, grad or None) as device tensors,
    queued on the current stream (hyper.sweep overlaps settings this way)."""
    if gp.y is None:
        raise ValueError("this fit carries no observations (it was not made by engine.fit)")
    L = N.lib()
    s = _stream_handle(gp.device)
    bd = gp.kernel.block_dim
    out = torch.empty(1, dtype=torch.float64, device=gp.device)
    tr = gp.extra.get("trend")
    if tr is not None:   # the restricted likelihood: β̂ integrated out under its vague prior
        N.check(L.gp2d_lml_trend(_ptr(gp.W), gp.n, gp.W.stride(0), _ptr(gp.alpha), _ptr(gp.y), bd * gp.n_train,
                                 ctypes.byref(tr["desc"]), _ptr(tr["block"]), _ptr(out), s), "gp2d_lml_trend")
    else:
        N.check(L.gp2d_lml(_ptr(gp.W), gp.n, gp.W.stride(0), _ptr(gp.alpha), _ptr(gp.y), bd * gp.n_train, _ptr(out),
                           s), "gp2d_lml")
    if not eval_gradient:
        return out, None
    desc = gp.kernel.desc()
    ng = int(L.gp2d_lml_grad_count(ctypes.byref(desc)))
    wbytes = int(L.gp2d_lml_grad_workspace(gp.n))
    work = _workspace(wbytes, gp.device)
    g = torch.empty(ng, dtype=torch.float64, device=gp.device)
    if tr is not None:
        N.check(L.gp2d_lml_grad_trend(_ptr(gp.W), gp.n, gp.W.stride(0), _ptr(gp.alpha), _ptr(gp.x), gp.n_train,
                                      gp.n_pad, ctypes.byref(desc), ctypes.byref(tr["desc"]), _ptr(tr["block"]),
                                      _ptr(g), _ptr(work), wbytes, s), "gp2d_lml_grad_trend")
    else:
        N.check(L.gp2d_lml_grad(_ptr(gp.W), gp.n, gp.W.stride(0), _ptr(gp.alpha), _ptr(gp.x), gp.n_train, gp.n_pad,
                                ctypes.byref(desc), _ptr(g), _ptr(work), wbytes, s), "gp2d_lml_grad")
    return out, g


# ------------------------------------------------------------------ cross-validation
CV_MAX_Q = N.CV_MAX_Q   # components of one held-out group (GP2D_CV_MAX_Q)


def _cv_fit(gp: GPFit, entry: str):
    """What both cross-validation entries need of a fit: W, α and the padded observations."""
    refuse_trend(gp, entry)
    if gp.W is None:
        raise ValueError(f"{entry}: this fit holds no factor W (a receiving rank's planes-only fit); "
                         "cross-validate on the rank that owns the fit")
    if gp.y is None:
        raise ValueError(f"{entry}: this fit carries no observations (it was not made by engine.fit)")
    gp.check()
    return gp.kernel.block_dim, gp.n_train, gp.n_pad, gp.n


def _cv_diag_add(gp: GPFit) -> float:
    """noise + jitter on K_y's diagonal (with a jitchol retry's extra jitter)."""
    return float(gp.extra.get("diag_add", gp.noise)) + float(gp.extra.get("jitchol", 0.0))


def _cv_scores(sum_lpd: float, sum_ru2: float, sum_rv2: float, sum_chi2: float, npts: int) -> dict:
    m = max(int(npts), 1)
    return dict(rmse_u=math.sqrt(sum_ru2 / m), rmse_v=math.sqrt(sum_rv2 / m), mean_lpd=sum_lpd / m,
                msll_chi2=sum_chi2 / m)


def _cv_obs(gp: GPFit, bd: int) -> torch.Tensor:
    """The observations [u…, v…] in the caller's input order, from the fit's padded vector."""
    ntr, npad = gp.n_train, gp.n_pad
    yc = gp.y.view(bd, npad)[:, :ntr]
    if gp.perm is None:
        return yc.reshape(-1).clone()
    out = torch.empty((bd, ntr), dtype=torch.float64, device=gp.device)
    out[:, gp.perm] = yc
    return out.reshape(-1)


def cv_points(gp: GPFit, latent: bool = False) -> dict:
    """Leave-one-point-out cross-validation of a fit without refitting (gp2d_cv_points; DESIGN.md
    §3.9): for every training point the prediction of its observation (u and v together) from all
    the other points.  Replaces one refit per held-out fix of the reference's train / test scoring
    (krig.py:578-646).  Device tensors in the caller's input order: mean, var ([u…, v…]), cuv (the
    u–v predictive covariance; None for a scalar family), lpd (log predictive density per point),
    resid = y − mean; host floats rmse_u, rmse_v (0 for a scalar family), mean_lpd and msll_chi2 =
    mean of rᵀ·P_ii·r (1 per component for a well-calibrated fit).  var is the variance of the
    held-out observation; latent=True subtracts the noise + jitter of K_y's diagonal from it."""
    bd, ntr, npad, n = _cv_fit(gp, "cv_points")
    L, dev = N.lib(), gp.device
    mean = torch.empty(bd * ntr, dtype=torch.float64, device=dev)
    var = torch.empty(bd * ntr, dtype=torch.float64, device=dev)
    cuv = torch.empty(ntr, dtype=torch.float64, device=dev) if bd == 2 else None
    lpd = torch.empty(ntr, dtype=torch.float64, device=dev)
    summary = torch.empty(4, dtype=torch.float64, device=dev)
    wb = int(L.gp2d_cv_points_workspace(n))
    work = _workspace(wb, dev)
    N.check(L.gp2d_cv_points(_ptr(gp.W), n, gp.W.stride(0), _ptr(gp.alpha), _ptr(gp.y), ntr, npad, bd,
                             None if gp.perm is None else _ptr(gp.perm), _ptr(mean), _ptr(var),
                             None if cuv is None else _ptr(cuv), _ptr(lpd), _ptr(summary), _ptr(work), wb,
                             _stream_handle(dev)), "gp2d_cv_points")
    resid = _cv_obs(gp, bd) - mean
    if latent:
        var -= _cv_diag_add(gp)
    s = summary.cpu().tolist()
    return dict(mean=mean, var=var, cuv=cuv, lpd=lpd, resid=resid, **_cv_scores(s[0], s[1], s[2], s[3], ntr))


def _cv_groups_run(gp: GPFit, labels):
    """cv_groups' device call: (mean, var, lpd, info, sorted unique ids, held-out point count, the
    call's workspace, q_pad).  The workspace begins with the last batch's Gram blocks (q_pad²
    doubles per group, in the order of the ids)."""
    bd, ntr, npad, n = _cv_fit(gp, "cv_groups")
    lab = np.asarray(_to_host(labels)).reshape(-1)
    if lab.shape[0] != ntr or not np.issubdtype(lab.dtype, np.integer):
        raise ValueError(f"cv_groups: labels must be {ntr} integers (one per training point)")
    lab = lab.astype(np.int64)
    L, dev = N.lib(), gp.device
    if gp.perm is not None:   # the fit's point i is input point perm[i]
        lab = lab[gp.perm.cpu().numpy()]
    held = np.flatnonzero(lab >= 0)
    if held.size == 0:
        raise ValueError("cv_groups: every label is negative (no group to hold out)")
    order = held[np.argsort(lab[held], kind="stable")]   # the fit's indices, grouped by label
    ids, counts = np.unique(lab[held], return_counts=True)
    over = np.flatnonzero(bd * counts > CV_MAX_Q)
    if over.size:
        g = int(over[0])
        raise ValueError(f"cv_groups: group {int(ids[g])} has {int(counts[g])} points ({bd * int(counts[g])} "
                         f"components), over the cap of {CV_MAX_Q} components")
    ng = int(ids.size)
    gstart = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    qpad = (bd * int(counts.max()) + NB - 1) // NB * NB
    gidx = torch.as_tensor(order.astype(np.int64), device=dev)
    mean = torch.empty(bd * ntr, dtype=torch.float64, device=dev)
    var = torch.empty(bd * ntr, dtype=torch.float64, device=dev)
    lpd = torch.empty(ng, dtype=torch.float64, device=dev)
    info = torch.empty(ng, dtype=torch.int32, device=dev)
    wb = int(L.gp2d_cv_groups_workspace(n, qpad, ng))
    work = _workspace(wb, dev)
    N.check(L.gp2d_cv_groups(_ptr(gp.W), n, gp.W.stride(0), _ptr(gp.alpha), _ptr(gp.y), ntr, npad, bd,
                             gstart.ctypes.data_as(ctypes.c_void_p), _ptr(gidx), ng,
                             None if gp.perm is None else _ptr(gp.perm), _ptr(mean), _ptr(var), _ptr(lpd),
                             _ptr(info), _ptr(work), wb, _stream_handle(dev)), "gp2d_cv_groups")
    return mean, var, lpd, info, ids, int(held.size), work, qpad


def cv_groups(gp: GPFit, labels, latent: bool = False) -> dict:
    """Leave-group-out cross-validation without refitting (gp2d_cv_groups): every group of points
    that share a label (a drifter id, say) is predicted from all the other points.  Replaces one
    refit per held-out drifter (laser_compare_interp.py's scoring; krig.getData(drop_drifters=)).
    labels: N integers in the caller's input order, ids need not be dense; a negative label puts
    the point in no group (NaN in mean, var and resid, excluded from the scores).  Returns device
    tensors mean, var ([u…, v…], the marginal predictive variances), resid, lpd (the joint log
    predictive density per group) beside `labels` (the sorted unique ids, numpy), and the host
    scores of cv_points over the held-out points (mean_lpd = Σ lpd / points).  Raises ValueError
    naming the group that has more than CV_MAX_Q components, LinAlgError for a group whose
    precision block is not positive definite."""
    mean, var, lpd, info, ids, nheld, work, _ = _cv_groups_run(gp, labels)
    del work
    bd, ntr, npad = gp.kernel.block_dim, gp.n_train, gp.n_pad
    bad = np.flatnonzero(info.cpu().numpy())
    if bad.size:
        raise np.linalg.LinAlgError(f"cv_groups: the precision block of group {int(ids[int(bad[0])])} is not "
                                    "positive definite (a failed or ill-conditioned fit)")
    resid = _cv_obs(gp, bd) - mean
    if latent:
        var -= _cv_diag_add(gp)
    # the scores over the held-out points, from the outputs: rᵀ·P_GG·r = α_Gᵀ·r per group
    r = resid.view(bd, ntr)
    a = gp.alpha.view(bd, npad)[:, :ntr]
    if gp.perm is not None:
        ac = torch.empty_like(r)
        ac[:, gp.perm] = a
        a = ac
    keep = ~torch.isnan(r[0])
    zero = torch.zeros((), dtype=torch.float64, device=gp.device)
    ss = torch.stack([lpd.sum(), (r[0][keep] ** 2).sum(), (r[1][keep] ** 2).sum() if bd == 2 else zero,
                      (a[:, keep] * r[:, keep]).sum()]).cpu().tolist()
    return dict(mean=mean, var=var, resid=resid, lpd=lpd, labels=ids, **_cv_scores(ss[0], ss[1], ss[2], ss[3], nheld))


def _loo_call(gp: GPFit, eval_gradient: bool, entry: str):
    """gp2d_loo_grad on the current stream: (value, grad or None, info) as device tensors.  Refuses
    what _cv_fit refuses, without the fit's deferred check (no host round trip)."""
    refuse_trend(gp, entry)
    if gp.W is None:
        raise ValueError(f"{entry}: this fit holds no factor W (a receiving rank's planes-only fit); "
                         "evaluate the objective on the rank that owns the fit")
    if gp.y is None:
        raise ValueError(f"{entry}: this fit carries no observations (it was not made by engine.fit)")
    L, dev = N.lib(), gp.device
    desc = gp.kernel.desc()
    out = torch.empty(1, dtype=torch.float64, device=dev)
    info = torch.empty(1, dtype=torch.int32, device=dev)
    g = torch.empty(int(L.gp2d_lml_grad_count(ctypes.byref(desc))), dtype=torch.float64, device=dev) \
        if eval_gradient else None
    wb = int(L.gp2d_loo_grad_workspace(gp.n))
    work = _workspace(wb, dev)
    N.check(L.gp2d_loo_grad(_ptr(gp.W), gp.n, gp.W.stride(0), _ptr(gp.alpha), _ptr(gp.y), _ptr(gp.x), gp.n_train,
                            gp.n_pad, ctypes.byref(desc), _ptr(out), None if g is None else _ptr(g), _ptr(info),
                            _ptr(work), wb, _stream_handle(dev)), "gp2d_loo_grad")
    return out, g, info


def loo_device(gp: GPFit, eval_gradient: bool = False):
    """loo_log_likelihood without a host round trip: (value, grad or None) as device tensors, queued
    on the current stream, as lml_device (hyper.sweep overlaps settings this way).  A fit whose
    diagonal blocks of K_y⁻¹ are not positive definite gives NaN (loo_log_likelihood raises)."""
    out, g, _ = _loo_call(gp, eval_gradient, "loo_device")
    return out, g


def loo_log_likelihood(gp: GPFit, eval_gradient: bool = False):
    """The leave-one-out log predictive density Σ_i log p(y_i | y_−i, X, θ) of a fit — cv_points'
    mean_lpd × N — and optionally its exact gradient ∂/∂θ in natural units (param_names order), both
    from the fit without refitting (gp2d_loo_grad; Rasmussen & Williams §5.4.2).
    The objective that scores hyperparameters by held-out prediction, where log_marginal_likelihood
    scores them by the evidence; hyper.optimize(objective="loo") maximises it.  Every kernel family
    of log_marginal_likelihood, both variance engines, ordered and unordered fits; a trend fit is
    refused.  Raises LinAlgError for a fit whose K_y⁻¹ has a diagonal block that is not positive
    definite."""
    gp.check()
    out, g, info = _loo_call(gp, eval_gradient, "loo_log_likelihood")
    bad = int(info.item())
    if bad:
        raise np.linalg.LinAlgError(f"loo_log_likelihood: the precision block of point {bad - 1} (the fit's order) "
                                    "is not positive definite (a failed or ill-conditioned fit)")
    if not eval_gradient:
        return float(out.item())
    return float(out.item()), g.cpu().numpy()


def _to_host(a):
    return a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else a


def kernel_grad(kernel: KernelSpec, xa, dL_dK, xb=None, device=None) -> np.ndarray:
    """Σ dL_dK ⊙ ∂K(xa, xb)/∂θ for θ = param_names(kernel) without the noise — the contraction
    GPy's Kern.update_gradients_full performs (myKernel.py:59-105; the exact derivative, not the
    reference's formula).  dL_dK: (bd·Na, bd·Nb) in the reference's component-major layout."""
    dev = _require_device(device)
    L = N.lib()
    d = kernel.input_dim
    A = _as_points(xa, d, dev)
    B = A if xb is None else _as_points(xb, d, dev)
    G = dL_dK.to(device=dev, dtype=torch.float64) if isinstance(dL_dK, torch.Tensor) else \
        torch.as_tensor(np.ascontiguousarray(np.asarray(dL_dK, dtype=np.float64)), device=dev)
    G = G.contiguous()
    bd = kernel.block_dim
    if tuple(G.shape) != (bd * A.shape[0], bd * B.shape[0]):
        raise ValueError(f"dL_dK has shape {tuple(G.shape)}, expected {(bd * A.shape[0], bd * B.shape[0])}")
    desc = kernel.desc()
    ng = int(L.gp2d_kernel_grad_count(ctypes.byref(desc)))
    wbytes = int(L.gp2d_kernel_grad_workspace(A.shape[0], B.shape[0]))
    work = _workspace(wbytes, dev)
    g = torch.empty(ng, dtype=torch.float64, device=dev)
    N.check(L.gp2d_kernel_grad(_ptr(A), A.shape[0], _ptr(B), B.shape[0], ctypes.byref(desc), _ptr(G), G.shape[1],
                               _ptr(g), _ptr(work), wbytes, _stream_handle(dev)), "gp2d_kernel_grad")
    return g.cpu().numpy()


# ------------------------------------------------------------------ dense helpers
def _as_matrix(a, device) -> torch.Tensor:
    if isinstance(a, torch.Tensor):
        t = a.to(device=device, dtype=torch.float64)
    else:
        t = torch.as_tensor(np.ascontiguousarray(np.asarray(a, dtype=np.float64)), device=device)
    return t.reshape(t.shape[0], -1) if t.dim() != 2 else t


def _padded(t: torch.Tensor, rows: int, cols: int) -> torch.Tensor:
    if tuple(t.shape) == (rows, cols) and t.is_contiguous():
        return t
    out = torch.zeros((rows, cols), dtype=torch.float64, device=t.device)
    out[:t.shape[0], :t.shape[1]] = t
    return out


def _up(v: int, m: int) -> int:
    return max(m, (v + m - 1) // m * m)


def gemm(A, B, transb: bool = False, alpha: float = 1.0, C=None, beta: float = 0.0, device=None) -> torch.Tensor:
    """alpha·A·op(B) + beta·C on the FP64 MFMA GEMM core (gp2d_gemm); op(B) = Bᵀ if transb.
    Operands of any shape are zero-padded to the kernel's 128/128/16 tiles (the padding adds
    exact zeros to every sum).  The dense product of GP_scripts.getMean / getCov."""
    dev = _require_device(device)
    A = _as_matrix(A, dev)
    B = _as_matrix(B, dev)
    m, k = A.shape
    n = B.shape[0] if transb else B.shape[1]
    if (B.shape[1] if transb else B.shape[0]) != k:
        raise ValueError(f"gemm: inner dimensions differ ({tuple(A.shape)} x {tuple(B.shape)}, transb={transb})")
    mp, np_, kp = _up(m, NB), _up(n, NB), _up(k, 16)
    Ap = _padded(A, mp, kp)
    Bp = _padded(B, np_, kp) if transb else _padded(B, kp, np_)
    Cp = torch.zeros((mp, np_), dtype=torch.float64, device=dev)
    if C is not None and beta != 0.0:
        Cp[:m, :n] = _as_matrix(C, dev)
    N.check(N.lib().gp2d_gemm(int(bool(transb)), mp, np_, kp, float(alpha), _ptr(Ap), kp, _ptr(Bp), Bp.shape[1],
                              float(beta), _ptr(Cp), np_, _stream_handle(dev)), "gp2d_gemm")
    return Cp[:m, :n]


def spd_inverse(K, device=None, return_factor: bool = False):
    """K⁻¹ of a symmetric positive-definite matrix through the engine's factor:
    L = chol(K) (gp2d_potrf), W = L⁻¹ (gp2d_trtri), K⁻¹ = WᵀW (gp2d_transpose + gp2d_gemm).
    Stands in for np.linalg.inv(K) (GP_scripts.py:50, GP_laser.py:118) on the matrices those
    call sites build; raises numpy.linalg.LinAlgError when K is not positive definite (where
    np.linalg.inv raises only for an exactly singular K).  K is padded to a multiple of 128
    with an identity block, which the block-diagonal inverse leaves decoupled."""
    dev = _require_device(device)
    K = _as_matrix(K, dev)
    n0 = K.shape[0]
    if K.shape[1] != n0:
        raise ValueError("spd_inverse: K must be square")
    L = N.lib()
    n = _up(n0, NB)
    A = torch.eye(n, dtype=torch.float64, device=dev)
    A[:n0, :n0] = K
    s = _stream_handle(dev)
    dinv = torch.empty((n // NB, NB, NB), dtype=torch.float64, device=dev)
    info = torch.empty(1, dtype=torch.int32, device=dev)
    _factor_inverse(A, n, dinv, info, dev)   # the join mode stays the caller's
    _raise_fit_errors(int(info.item()), None)
    Wt = torch.empty((n, n), dtype=torch.float64, device=dev)
    N.check(L.gp2d_transpose(_ptr(A), n, n, _ptr(Wt), s), "gp2d_transpose")
    Ki = torch.empty((n, n), dtype=torch.float64, device=dev)
    N.check(L.gp2d_gemm(1, n, n, n, 1.0, _ptr(Wt), n, _ptr(Wt), n, 0.0, _ptr(Ki), n, s), "gp2d_gemm")
    Ki = Ki[:n0, :n0]
    return (Ki, A[:n0, :n0]) if return_factor else Ki


def timing_enable(on: bool = True):
    N.lib().gp2d_timing_enable(int(bool(on)))


def timing_read():
    ms = ctypes.c_double()
    cnt = ctypes.c_int64()
    fl = ctypes.c_double()
    N.check(N.lib().gp2d_timing_read(ctypes.byref(ms), ctypes.byref(cnt), ctypes.byref(fl)), "gp2d_timing_read")
    return ms.value, cnt.value, fl.value
