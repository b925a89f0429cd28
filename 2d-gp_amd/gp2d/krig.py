"""The reference's ``krig`` module surface, backed by the MI355X engine.

Reference: krig.py (module functions), runKrig.py / runPredict.py (drivers),
GP_laser.py:16-142 (the explicit-numpy posterior).  ``Krig`` is the stateful
fit/predict object the north_star names (`krig.Krig`); the module functions
keep the reference's names, argument meaning and error behaviour.

Differences forced by the environment (documented in DESIGN.md):
  * data files (Filtered_2016_2_7.pkl, .mat outputs, GPy pickles) do not exist:
    functions take a track container (``Tracks``) or ``.npz`` paths; model files
    are ``.npz`` (inputs + hyperparameters, optionally the factor);
  * pyproj / NAD83 is absent: ``project`` is a signed local equirectangular
    projection in km about (lat0, lon0);
  * NetCDF: krig.predict writes filename+'.nc' (CDF-2, printNCFiles layout) through
    ``gp2d.ncio`` (netCDF4 is absent; a self-contained classic-format writer), plus the
    ``.npz`` of the same arrays;
  * hyperparameter optimisation (GPy optimize / optimize_restarts) runs on the GPU
    (``gp2d.hyper``: HIP LML + exact gradient, scipy L-BFGS-B on the host);
  * kernelType 2/3/4 use the spatio-temporal product Kt(var_t, l_t) × div-free /
    curl-free / mixed kernel on (T, Y, X) (engine family 'vector_st', the form of
    scratch.py:506-508) — the reference's myKernel2 (var, lt, ly, lx) is missing from
    the reference itself (krig.py:9), so ly = lx = ℓ here;
    hyper={'temporal': False} gives the purely spatial kernel on (Y, X).
"""
from __future__ import annotations

import os
import time
from dataclasses import dataclass
from datetime import datetime, timedelta

import numpy as np
import torch

from . import data as D
from . import engine as E
from . import hyper as H
from . import ncio as NC

lat0 = 28.8
lon0 = -88.6

KERNEL_NAMES = {"df": "df", "divfree": "df", "div-free": "df", 1: "df",
                "cf": "cf", "curlfree": "cf", "curl-free": "cf", 2: "cf",
                "mixed": "mixed", "combined": "mixed", 3: "mixed",
                "scalar": "scalar", "isotropic": "scalar", 0: "scalar"}


def nad83(lon, lat):
    """Stand-in for the reference's NAD83 / EPSG:3452 projection (krig.py:19; pyproj is absent):
    a signed equirectangular projection in metres, scaled at lat0."""
    R = 6371000.0
    x = R * np.cos(np.deg2rad(lat0)) * np.deg2rad(np.asarray(lon, dtype=np.float64))
    y = R * np.deg2rad(np.asarray(lat, dtype=np.float64))
    return x, y


x_ori, y_ori = nad83(lon0, lat0)   # krig.py:20


def project(lon, lat):
    """Track coordinates to km about (lat0, lon0), with the reference's arithmetic
    (krig.py:291-298): (NAD83(lon, lat) − origin) / 1000."""
    x, y = nad83(lon, lat)
    return (x - x_ori) / 1000.0, (y - y_ori) / 1000.0


def _to_numpy(t):
    return t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)


# =============================================================================== Krig
class Krig:
    """Stateful GP kriging object: ``Krig(...).fit(X, obs).predict(Xg)``.

    kernel: 'df' (divergence-free, GP_scripts divFree=1), 'cf' (curl-free, 2),
    'mixed' (ratio·df + (1−ratio)·cf, GP_laser.py:113), 'scalar' (divFree=0),
    a ``kern.myKernel``/``nonDivK``/``nonRotK`` instance, or an ``engine.KernelSpec``
    (incl. family='ard' for the sklearn model of krig.scikit_prior, and family='vector_sum', a sum
    of vector kernels with one term per flow scale: FP64 engine only; predict(term=t) and
    predict_fields(term=t) give the posterior of term t's contribution alone).
    var_mode: 'latent' (GP_laser.py:128-131), 'gpy' (+noise, GPy model.predict),
    'sklearn' (+noise, clipped at 0, _gpr.py:473-485).
    variance: 'f64' (default) — the FP64-MFMA engine, FP64 arithmetic throughout as in the
    reference; 'ozaki' (opt-in, vector kernels) — the int8 Ozaki-II emulation of the same FP64
    product, held to the 1e-10 gate by its calibrated accuracy guard (engine.apply_guard: more
    W bits, or FP64 past its range).  The job-stream API (engine.krige_jobs) and bench.py use
    'ozaki'; the drop-in object keeps the reference's arithmetic unless asked.
    trend: None (zero-mean, the reference's model), 'constant' or 'linear' — a background flow
    estimated with the fit (engine.fit(trend=); vector kernels, variance='f64').
    predict*, predict_fields*, log_likelihood (the restricted likelihood) and optimize* then use it;
    trend_coefficients() reads it; predict_gradient / predict_diagnostics, predict_cov, sample and
    cross_validate have no trend form yet and raise ValueError.
    """

    def __init__(self, kernel="df", l_df: float = 5.0, l_cf: float = 5.0, ratio: float = None,
                 noise: float = 0.0025, jitter: float = 0.0, var_mode: str = "latent", device=None,
                 chunk: int = 8192, variance: str = "f64", jitchol: int = 0, trend: str | None = None):
        self.spec = self._make_spec(kernel, l_df, l_cf, ratio)
        E._check_trend_fit(self.spec, variance, trend)   # vector kernels on the FP64 engine
        self.trend = trend
        self.jitchol = int(jitchol)   # GPy jitchol retries on a non-PD K_y (engine.fit)
        if variance == "ozaki" and not self.spec.is_vector:
            raise ValueError("the ozaki variance engine supports the vector kernels only")
        E._check_family(self.spec, variance)   # a kernel sum: variance="f64" only
        if variance not in E.VARIANCE_ENGINES:
            raise ValueError(f"variance must be one of {E.VARIANCE_ENGINES}")
        self.variance = variance
        self.noise = float(noise)
        self.jitter = float(jitter)
        self.var_mode = var_mode
        self.device = device
        self.chunk = int(chunk)
        self.gp = None
        self._pred = None
        self._X = None
        self._y = None

    @staticmethod
    def _make_spec(kernel, l_df, l_cf, ratio):
        if isinstance(kernel, E.KernelSpec):
            return kernel
        if hasattr(kernel, "_spec"):
            return kernel._spec()
        kind = KERNEL_NAMES[kernel.lower() if isinstance(kernel, str) else kernel]
        if ratio is None:
            ratio = 0.5 if kind == "mixed" else (0.0 if kind == "cf" else 1.0)
        return E.KernelSpec(kind=kind, l_df=float(l_df), l_cf=float(l_cf), ratio=float(ratio))

    # ------------------------------------------------------------------ fit
    def fit(self, X, obs):
        """X: (N, dim) inputs; obs: (2N,) = [u; v] (or (N, 2) columns u, v) for the
        vector kernels, (N,) for the scalar ARD family."""
        X = np.asarray(X, dtype=np.float64) if not isinstance(X, torch.Tensor) else X
        bd = self.spec.block_dim
        y = obs if isinstance(obs, torch.Tensor) else np.asarray(obs, dtype=np.float64)
        if bd == 2 and not isinstance(y, torch.Tensor) and y.ndim == 2 and y.shape[1] == 2:
            y = np.concatenate([y[:, 0], y[:, 1]])
        self.gp = E.fit(self.spec, X, y, self.noise, jitter=self.jitter, device=self.device,
                        variance=self.variance, jitchol=self.jitchol, trend=self.trend)
        self._pred = E.Predictor(self.gp, self.chunk)
        self._X, self._y = X, y
        return self

    def _check(self):
        if self.gp is None:
            raise RuntimeError("Krig.fit must be called before predict")

    # ------------------------------------------------------------------ predict
    def predict_device(self, Xg, var_mode=None, compute_var=True, term=None):
        """Posterior mean and variance as device tensors ([u..., v...] for vector kernels).
        term=t (a kernel sum): term t's contribution alone, latent variance (a var_mode other than
        'latent' raises: a term is never observed)."""
        self._check()
        if term is not None and var_mode is None:
            var_mode = "latent"
        return self._pred(Xg, var_mode=var_mode or self.var_mode, compute_var=compute_var, term=term)

    def predict(self, Xg, var_mode=None, compute_var=True, term=None):
        """(mean, var) numpy arrays of shape (bd·M, 1), as GPy's model.predict returns
        (krig.py:543-544; f[:M] = u, f[M:] = v, GP_plots.py:768-771).  term: predict_device's."""
        mu, var = self.predict_device(Xg, var_mode=var_mode, compute_var=compute_var, term=term)
        mu = _to_numpy(mu)[:, None]
        return mu, (_to_numpy(var)[:, None] if compute_var else None)

    def predict_grid(self, x, y, var_mode=None, term=None):
        """GP_laser.py:107-136 on the grid meshgrid(x, y): returns uf, vf, uvar, vvar,
        each reshaped to [y.size, x.size].  term: predict_device's."""
        X, Y = np.meshgrid(x, y)
        pts = np.stack([X.reshape(-1), Y.reshape(-1)], 1)
        mu, var = self.predict_device(pts, var_mode=var_mode, term=term)
        mu, var = _to_numpy(mu), _to_numpy(var)
        M = pts.shape[0]
        shp = [np.size(y), -1]
        return (mu[:M].reshape(shp), mu[M:].reshape(shp), var[:M].reshape(shp), var[M:].reshape(shp))

    def predict_fields(self, Xg, fields=E.FIELDS, term=None):
        """Divergence and vorticity of the fitted velocity at the points Xg, with their latent
        variance: {name: (mean, var)} numpy arrays of shape (M,) (engine.predict_field).  For
        points (x1, x2) and observations [f1; f2]: divergence = ∂f1/∂x1 + ∂f2/∂x2, vorticity =
        ∂f2/∂x1 − ∂f1/∂x2 — with points (x, y) and obs [u; v] the usual ∂u/∂x + ∂v/∂y and
        ∂v/∂x − ∂u/∂y; points given as (Y, X) with obs [v; u] give −vorticity.  Replaces the
        finite differences of a predicted grid: exact, with an error bar, on any set of points.
        term=t (a kernel sum): the fields of term t's contribution alone."""
        self._check()
        out = {}
        for name in fields:
            mu, var = E.predict_field(self.gp, Xg, name, chunk=self.chunk, term=term)
            out[name] = (_to_numpy(mu), _to_numpy(var))
        return out

    def predict_fields_grid(self, x, y, term=None):
        """predict_fields on the grid meshgrid(x, y) of predict_grid (points (x, y), components
        (u, v)): {name: (mean, var)}, each reshaped to [y.size, x.size]."""
        X, Y = np.meshgrid(x, y)
        pts = np.stack([X.reshape(-1), Y.reshape(-1)], 1)
        shp = [np.size(y), -1]
        return {name: (mu.reshape(shp), var.reshape(shp))
                for name, (mu, var) in self.predict_fields(pts, term=term).items()}

    def predict_gradient(self, Xg):
        """The velocity gradient tensor at the points Xg with its joint posterior covariance per
        point: (mean (M, 4), cov (M, 4, 4)) numpy arrays, components engine.GRADIENT_COMPONENTS =
        (∂f1/∂x1, ∂f1/∂x2, ∂f2/∂x1, ∂f2/∂x2) — (∂u/∂x, ∂u/∂y, ∂v/∂x, ∂v/∂y) for points (x, y) and
        obs [u; v]; predict_fields' caveat for (Y, X) points stands (engine.predict_gradient)."""
        self._check()
        mu, cov = E.predict_gradient(self.gp, Xg, chunk=self.chunk)
        return _to_numpy(mu), _to_numpy(cov)

    def predict_diagnostics(self, Xg, names=E.DIAGNOSTICS):
        """Kinematic diagnostics of the fitted flow at the points Xg, each with its variance:
        {name: (mean, var)} numpy arrays of shape (M,), names from engine.DIAGNOSTICS — divergence,
        vorticity, normal_strain ∂u/∂x − ∂v/∂y, shear_strain ∂v/∂x + ∂u/∂y, and okubo_weiss
        σ_n² + σ_s² − ζ² with its Gaussian moments (engine.flow_diagnostics of one
        predict_gradient).  Replaces the finite differences of a predicted grid: exact, with error
        bars that account for the covariance between the derivatives, on any set of points."""
        self._check()
        mu, cov = E.predict_gradient(self.gp, Xg, chunk=self.chunk)
        return {name: (_to_numpy(a), _to_numpy(v)) for name, (a, v) in E.flow_diagnostics(mu, cov, names).items()}

    def predict_diagnostics_grid(self, x, y):
        """predict_diagnostics on the grid meshgrid(x, y) of predict_grid (points (x, y), components
        (u, v)): {name: (mean, var)}, each reshaped to [y.size, x.size]."""
        X, Y = np.meshgrid(x, y)
        pts = np.stack([X.reshape(-1), Y.reshape(-1)], 1)
        shp = [np.size(y), -1]
        return {name: (mu.reshape(shp), var.reshape(shp)) for name, (mu, var) in self.predict_diagnostics(pts).items()}

    # ------------------------------------------------------------------ trajectories, FTLE
    def advect(self, X0, t0: float = 0.0, dt: float = None, nsteps: int = None, save_every: int | None = None,
               vel_scale: float = 1.0, tangent: bool = False):
        """Trajectories of particles released at the points X0 (M, 2) at time t0 in the fitted mean
        flow: (times (R,), path (R, M, 2), tangent (R, M, 2, 2) | None) numpy arrays — RK4 with
        nsteps steps of dt (negative: backward), a record every save_every steps and at the end
        (None: start and end only), vel_scale from velocity units to position units per time unit;
        tangent=True adds the flow map's gradient ∂x(t)/∂x(t0) (engine.advect).  Points and
        components pair as in the fit: (x, y) with obs [u; v], or (Y, X) with obs [v; u]."""
        self._check()
        t, path, tan = E.advect(self.gp, X0, t0=t0, dt=dt, nsteps=nsteps, save_every=save_every,
                                vel_scale=vel_scale, tangent=tangent)
        return _to_numpy(t), _to_numpy(path), (None if tan is None else _to_numpy(tan))

    def ftle_grid(self, x, y, t0: float, duration: float, nsteps: int, vel_scale: float = 1.0):
        """The finite-time Lyapunov exponent field of the fitted flow over `duration` (negative:
        backward, attracting structures) from t0, seeded on the grid meshgrid(x, y) of predict_grid
        (points (x, y), components (u, v)) and integrated in nsteps RK4 steps: [y.size, x.size]
        (engine.ftle of engine.advect's tangent at the final record)."""
        self._check()
        X, Y = np.meshgrid(x, y)
        pts = np.stack([X.reshape(-1), Y.reshape(-1)], 1)
        _, _, tan = E.advect(self.gp, pts, t0=t0, dt=float(duration) / int(nsteps), nsteps=nsteps,
                             vel_scale=vel_scale, tangent=True)
        return _to_numpy(E.ftle(tan[-1], duration)).reshape([np.size(y), -1])

    # ------------------------------------------------------------------ path uncertainty
    def draw_flows(self, n_draws: int, n_features: int = 1024, seed: int = 0):
        """n_draws posterior draws of the flow as functions (engine.draw_flows): an engine.FlowDraws,
        whose velocity(Xg, t) gives the draws at any points and which engine.advect_draws integrates."""
        self._check()
        return E.draw_flows(self.gp, n_draws, n_features=n_features, seed=seed)

    def advect_ensemble(self, X0, n_draws: int, t0: float = 0.0, dt: float = None, nsteps: int = None,
                        save_every: int | None = None, vel_scale: float = 1.0, n_features: int = 1024, seed: int = 0):
        """Where a parcel could be, and how sure we are: particles released at X0 ((M, 2), or
        (n_draws, M, 2) for an uncertain release) advected through n_draws posterior draws of the flow.
        Returns numpy arrays (times (R,), paths (R, S, M, 2), mean (R, M, 2), cov (R, M, 2, 2), count
        (R, M)) — the trajectories of every draw and engine.path_spread of them: the ensemble mean
        position (not the path through the mean flow, which Krig.advect gives), its 2 × 2 covariance
        and the number of draws behind them.  The other arguments are advect's."""
        draws = self.draw_flows(n_draws, n_features=n_features, seed=seed)
        t, paths = E.advect_draws(draws, X0, t0=t0, dt=dt, nsteps=nsteps, save_every=save_every, vel_scale=vel_scale)
        mean, cov, cnt = E.path_spread(paths)
        return _to_numpy(t), _to_numpy(paths), _to_numpy(mean), _to_numpy(cov), _to_numpy(cnt)

    # ------------------------------------------------------------------ joint covariance, samples
    def predict_cov(self, Xg):
        """(mean (2M, 1), cov (2M, 2M)) numpy arrays: the posterior mean and the full latent
        covariance Kss − Ks·Ki·Ksᵀ of GP_laser.py:128-129 (of which predict returns the diagonal),
        as sklearn's predict(return_cov=True) and GPy's predict(full_cov=True) minus its noise;
        rows and columns [u(M), v(M)] (engine.predict_cov)."""
        self._check()
        mu, cov = E.predict_cov(self.gp, Xg)
        return _to_numpy(mu)[:, None], _to_numpy(cov)

    def sample(self, Xg, n_samples: int, seed: int = 0):
        """n_samples joint draws of the velocity at the points Xg from the posterior: (S, 2M) numpy,
        each row [u(M), v(M)] — sklearn's sample_y / GPy's posterior_samples_f
        (engine.sample_posterior; the same seed gives the same draws)."""
        self._check()
        return _to_numpy(E.sample_posterior(self.gp, Xg, n_samples, seed=seed)[0])

    def sample_grid(self, x, y, n_samples: int, seed: int = 0):
        """sample on the grid meshgrid(x, y) of predict_grid: (us, vs), each (S, y.size, x.size),
        us[s] and vs[s] one simulated velocity field laid out as predict_grid's uf and vf."""
        X, Y = np.meshgrid(x, y)
        pts = np.stack([X.reshape(-1), Y.reshape(-1)], 1)
        s = self.sample(pts, n_samples, seed=seed)
        M = pts.shape[0]
        shp = [s.shape[0], np.size(y), -1]
        return s[:, :M].reshape(shp), s[:, M:].reshape(shp)

    # ------------------------------------------------------------------ hyperparameters
    def log_likelihood(self, eval_gradient: bool = False):
        """GPy model.log_likelihood() / sklearn log_marginal_likelihood() of the current fit;
        with eval_gradient also ∂/∂θ in param_array order (engine.param_names)."""
        self._check()
        return E.log_marginal_likelihood(self.gp, eval_gradient=eval_gradient)

    def trend_coefficients(self) -> dict:
        """The estimated background flow of a trend fit: β̂, its covariance, the mean flow at the
        centre and the trend's velocity gradient (engine.trend_coefficients)."""
        self._check()
        return E.trend_coefficients(self.gp)

    def _apply(self, res: "H.OptResult"):
        self.spec, self.noise = res.kernel, float(res.noise)
        self.fit(self._X, self._y)
        return res

    def loo_log_likelihood(self, eval_gradient: bool = False):
        """The leave-one-out log predictive density of the current fit (engine.loo_log_likelihood);
        with eval_gradient also ∂/∂θ in param_array order."""
        self._check()
        return E.loo_log_likelihood(self.gp, eval_gradient=eval_gradient)

    def optimize(self, fix=(), messages: bool = False, maxiter: int = 200, objective: str = "lml"):
        """GPy model.optimize (laser_io_methods.py:496): L-BFGS-B on the LML, refit at the optimum.
        objective='loo': on the leave-one-out log predictive density instead (hyper.optimize)."""
        self._check()
        return self._apply(H.optimize(self.spec, self._X, self._y, self.noise, fix=fix, jitter=self.jitter,
                                      device=self.device, maxiter=maxiter, messages=messages, trend=self.trend,
                                      objective=objective))

    def optimize_restarts(self, num_restarts: int = 10, fix=(), seed: int = 0, messages: bool = False,
                          maxiter: int = 200, objective: str = "lml"):
        """GPy model.optimize_restarts (krig.py:450): best of num_restarts L-BFGS-B runs, ranked by
        the objective ('lml' | 'loo') they maximise."""
        self._check()
        return self._apply(H.optimize_restarts(self.spec, self._X, self._y, self.noise, num_restarts=num_restarts,
                                               fix=fix, jitter=self.jitter, device=self.device, seed=seed,
                                               maxiter=maxiter, messages=messages, trend=self.trend,
                                               objective=objective))

    # ------------------------------------------------------------------ cross-validation
    def cross_validate(self, groups=None, latent: bool = False) -> dict:
        """Score the fit on its own training data without refitting (engine.cv_points /
        cv_groups): every point (groups=None) or every group of points sharing an
        integer label (a drifter id; negative = in no group) is predicted from all the others —
        what the reference does by splitting, refitting and predicting (krig.py:578-646).
        numpy results in the predict() conventions: mean, var, resid of shape (bd·N, 1) with
        f[:N] = u and f[N:] = v in the input order; lpd per point, or per group beside `labels`;
        cuv (N, 1) for points of a vector kernel; the floats rmse_u, rmse_v, mean_lpd, msll_chi2.
        var is the held-out observation's variance; latent=True takes the noise off."""
        self._check()
        res = E.cv_points(self.gp, latent=latent) if groups is None else E.cv_groups(self.gp, groups, latent=latent)
        out = {}
        for k, v in res.items():
            if isinstance(v, torch.Tensor):
                v = _to_numpy(v)
                out[k] = v if k == "lpd" else v[:, None]
            else:
                out[k] = v
        return out

    # ------------------------------------------------------------------ state
    @property
    def param_array(self):
        s = self.spec
        if s.is_sum:   # engine.param_names order: per term its weight and its own entries, then noise
            return np.array(list(H.get_params(s, self.noise).values()))
        if s.family == "ard":
            hp = []
            for v, ls in zip(s.variances, s.lengthscales):
                hp += [v, *ls]
            return np.array(hp + [self.noise])
        if s.family == "vector_st":
            return np.array([s.l_df, s.l_cf, s.ratio, s.var_t, s.l_t, self.noise])
        return np.array([s.l_df, s.l_cf, s.ratio, self.noise])

    def save(self, path: str, with_factor: bool = False):
        """Checkpoint: inputs, observations, hyperparameters (and optionally W = L⁻¹, α),
        the analogue of model.pickle (krig.py:412)."""
        self._check()
        s = self.spec
        d = dict(X=_to_numpy(self._X), y=_to_numpy(self._y), family=s.family, kind=str(s.kind), l_df=s.l_df,
                 l_cf=s.l_cf, ratio=s.ratio, variances=np.asarray(s.variances, dtype=np.float64),
                 lengthscales=np.asarray(s.lengthscales, dtype=np.float64), var_t=s.var_t, l_t=s.l_t,
                 noise=self.noise, jitter=self.jitter, jitchol=self.jitchol,
                 jitchol_used=float(self.gp.extra.get("jitchol", 0.0)),
                 var_mode=self.var_mode, variance=self.variance, chunk=self.chunk)
        if s.is_sum:   # the terms, one row each; the top-level fields above keep their defaults
            d.update(sum_family=s.terms[0].family, sum_kinds=np.array([str(t.kind) for t in s.terms]),
                     sum_weights=np.asarray(s.weights, dtype=np.float64),
                     sum_params=np.array([[t.l_df, t.l_cf, t.ratio, t.var_t, t.l_t] for t in s.terms],
                                         dtype=np.float64))
        if self.trend is not None:   # the order; with the factor also the basis the block was made with
            t = self.gp.extra["trend"]
            d.update(trend=self.trend, trend_centre=np.asarray(t["centre"], dtype=np.float64), trend_scale=t["scale"])
        if with_factor:
            d["W"] = _to_numpy(self.gp.W)
            d["alpha"] = _to_numpy(self.gp.alpha)
            if self.gp.perm is not None:   # W and α follow the training points in X[perm] order
                d["perm"] = _to_numpy(self.gp.perm)
        np.savez(path, **d)

    @classmethod
    def load(cls, path: str, device=None, refit: bool = True):
        """Restore a checkpoint written by save(): GPy.load / pickle.load of a fitted model
        (krig.py:478-483).  A checkpoint with the factor (save(with_factor=True)) is restored
        without refitting — W, α and the training order go back to the device as saved, so
        predictions are bit-identical to the saved model's; without it the model is refitted
        from the stored inputs (refit=False then returns an unfitted model)."""
        z = np.load(path, allow_pickle=False)
        fam = str(z["family"])
        if fam == "ard":
            spec = E.KernelSpec(family="ard", variances=tuple(z["variances"].tolist()),
                                lengthscales=tuple(tuple(r) for r in z["lengthscales"].tolist()))
        elif fam == "vector_sum":
            tf = str(z["sum_family"])
            terms = tuple(E.KernelSpec(family=tf, kind=str(kd), l_df=float(p[0]), l_cf=float(p[1]), ratio=float(p[2]),
                                       var_t=float(p[3]), l_t=float(p[4]))
                          for kd, p in zip(z["sum_kinds"].tolist(), z["sum_params"]))
            spec = E.KernelSpec(family="vector_sum", terms=terms, weights=tuple(z["sum_weights"].tolist()))
        else:
            st = dict(var_t=float(z["var_t"]), l_t=float(z["l_t"])) if "var_t" in z.files else {}
            spec = E.KernelSpec(family=fam, kind=str(z["kind"]), l_df=float(z["l_df"]), l_cf=float(z["l_cf"]),
                                ratio=float(z["ratio"]), **st)
        extra = {}
        if "variance" in z.files:   # older checkpoints carry none: they were written by the f64 engine
            extra = dict(variance=str(z["variance"]), chunk=int(z["chunk"]))
        if "jitchol" in z.files:
            extra["jitchol"] = int(z["jitchol"])
        if "trend" in z.files:   # a file without it: the zero-mean model
            extra["trend"] = str(z["trend"])
        k = cls(spec, noise=float(z["noise"]), jitter=float(z["jitter"]), var_mode=str(z["var_mode"]),
                device=device, **extra)
        if "W" in z.files:
            used = float(z["jitchol_used"]) if "jitchol_used" in z.files else 0.0
            basis = (tuple(z["trend_centre"].tolist()), float(z["trend_scale"])) if "trend" in z.files else None
            k._restore(z["X"], z["y"], z["W"], z["alpha"], z["perm"] if "perm" in z.files else None, used, basis)
        elif refit:
            k.fit(z["X"], z["y"])
        return k

    def _restore(self, X, y, W, alpha, perm, jitchol_used: float = 0.0, trend_basis: tuple | None = None):
        """Rebuild the device fit from a saved factor (no assembly, no factorisation).
        `jitchol_used` is the jitter a jitchol retry added to the saved factor's K_y diagonal:
        the Ozaki residue planes take the a-priori moduli count from the diagonal the factor was
        built with (noise + jitter + that jitter), exactly as fit() did.  A trend fit's block is
        recomputed from the restored W with the saved basis (centre, scale): the same launches on the
        same inputs as fit()'s, so the same bits."""
        dev = E._require_device(self.device)
        spec = self.spec
        bd, d = spec.block_dim, spec.input_dim
        Xd = torch.as_tensor(np.ascontiguousarray(np.asarray(X, dtype=np.float64).reshape(-1, d)), device=dev)
        ntr = Xd.shape[0]
        npad, n = E.fit_layout(spec, ntr, self.variance)
        if W.shape != (n, n) or alpha.shape != (n,):
            raise ValueError(f"saved factor has shape {W.shape}, the fit layout needs ({n}, {n})")
        pm = None
        if perm is not None:
            pm = torch.as_tensor(np.asarray(perm, dtype=np.int64), device=dev)
            Xs = torch.empty_like(Xd)
            E.N.check(E.N.lib().gp2d_gather_rows(E._ptr(Xd), E._ptr(pm), ntr, Xd.shape[1], E._ptr(Xs),
                                                 E._stream_handle(dev)), "gp2d_gather_rows")
            Xd = Xs
        Y = E._pad_obs(y, ntr, npad, bd, dev, pm)
        gp = E._make_fit(E._Staged(spec, Xd, ntr, npad, n, pm), self.noise,
                         torch.as_tensor(np.ascontiguousarray(W), device=dev),
                         torch.as_tensor(np.ascontiguousarray(alpha), device=dev), Y, dev)
        gp.extra["jitchol"] = float(jitchol_used)
        gp.extra["diag_add"] = float(self.noise + self.jitter)
        if self.trend is not None:
            gp.extra["trend"] = E._trend_solve(E._Staged(spec, Xd, ntr, npad, n, pm), gp.W, Y, gp.alpha, X,
                                               E.trend_order(self.trend), dev, basis=trend_basis)
            E._settle_trend(gp)
        if self.variance == "ozaki":
            E.ozaki_prepare_guarded(gp, float(self.noise + (self.jitter + jitchol_used)))
        self.gp = gp
        self._pred = E.Predictor(gp, self.chunk)
        self._X, self._y = X, y
        return self


# ===================================================================== module functions
def rmse(ys, y):
    """krig.rmse (krig.py:641-645)."""
    error = np.reshape(np.asarray(ys) - np.asarray(y), [-1])
    return np.sqrt(np.mean(np.square(error)))


def getGrid(to, yo, xo, dt=0.5, dx=0.5, xL=40, yL=40):
    """krig.getGrid (krig.py:648-678) — bit-exact (tests/golden/grids.npz)."""
    return D.get_grid(to, yo, xo, dt, dx, xL, yL)


def boundData(var, varlim, lat, lon, v, u):
    """krig.boundData (krig.py:79-86)."""
    return D.bound_data(var, varlim, lat, lon, v, u)


@dataclass
class Tracks:
    """Drifter track container (the fields of laser_class.interpolated_tracks used by
    krig.getData, krig.py:42-77): time (T,), lat/lon/u/v (T, D)."""
    time: np.ndarray
    lat: np.ndarray
    lon: np.ndarray
    u: np.ndarray
    v: np.ndarray

    @classmethod
    def load(cls, path: str) -> "Tracks":
        z = np.load(path, allow_pickle=False)
        return cls(z["time"], z["lat"], z["lon"], z["u"], z["v"])

    @classmethod
    def synthetic(cls, n_time: int = 96, n_drifters: int = 64, seed: int = 2016) -> "Tracks":
        """Drifters advected through the div-free Gaussian eddy of data.synthetic_tracks."""
        rng = np.random.default_rng(seed)
        x = rng.uniform(0, 60, n_drifters)
        y = rng.uniform(0, 45, n_drifters)
        dt_h = 0.25
        X = np.empty((n_time, n_drifters))
        Y = np.empty((n_time, n_drifters))
        U = np.empty((n_time, n_drifters))
        V = np.empty((n_time, n_drifters))
        for t in range(n_time):
            psi = np.exp(-((x - 30) ** 2 + (y - 22.5) ** 2) / 15.0 ** 2)
            u = psi * (-2 * (y - 22.5) / 15.0 ** 2) + rng.normal(0, 0.02, n_drifters)
            v = -psi * (-2 * (x - 30) / 15.0 ** 2) + rng.normal(0, 0.02, n_drifters)
            X[t], Y[t], U[t], V[t] = x, y, u, v
            x = x + u * 3.6 * dt_h
            y = y + v * 3.6 * dt_h
        R = 6371.0
        lat = lat0 + np.rad2deg(Y / R)
        lon = lon0 + np.rad2deg(X / (R * np.cos(np.deg2rad(lat0))))
        return cls(np.arange(n_time) * dt_h * 3600.0, lat, lon, U, V)


def getData(st, et, tracks: Tracks, drop_drifters=()):
    """krig.getData (krig.py:42-77) on a track container: time in hours from the first
    sample, columns ordered by decreasing number of valid points.  drop_drifters are set to
    NaN first — the reference hard-codes drifter 238 of Filtered_2016_2_7.pkl (krig.py:46-52);
    pass (238,) for that file.  The caller's container is not modified."""
    lat, lon, u, v = (np.array(a, dtype=np.float64) for a in (tracks.lat, tracks.lon, tracks.u, tracks.v))
    for c in drop_drifters:
        lat[:, c] = np.nan
        lon[:, c] = np.nan
        u[:, c] = np.nan
        v[:, c] = np.nan
    time_h = (tracks.time[st:et] - tracks.time[0]) / 3600.0
    latt = lat[st:et, :]
    lont = lon[st:et, :]
    uob = u[st:et, :]
    vob = v[st:et, :]
    valid = np.array([np.size(np.where((~np.isnan(lont[:, i])) & (~np.isnan(latt[:, i])))[0])
                      for i in range(latt.shape[1])])
    order = np.squeeze(valid.argsort(axis=0))[::-1]
    return time_h, latt[:, order], lont[:, order], vob[:, order], uob[:, order], valid[order]


def _prepare(tracks, st, et, lalim, lolim, sample_step, skip, drop_drifters=()):
    """Data selection of krig.kriging (krig.py:274-381): bounds, projection, split,
    NaN filter, T,Y,X stacking.  Returns dict of observation / test arrays.
    Bit-exact with the reference's code on the same tracks (tests/golden/prep_tracks.npz)."""
    time_h, latt, lont, vob, uob, _ = getData(st, et, tracks, drop_drifters)
    if lolim[1] > lolim[0]:
        latt, lont, vob, uob = boundData(lont, lolim, latt, lont, vob, uob)
    if lalim[1] > lalim[0]:
        latt, lont, vob, uob = boundData(latt, lalim, latt, lont, vob, uob)
    xob, yob = nad83(lont, latt)
    tob = np.repeat(time_h[:, None], latt.shape[1], axis=1)
    dob = np.repeat(np.arange(latt.shape[1], dtype=np.int64)[None, :], latt.shape[0], axis=0)   # drifter column
    yob[np.where(np.isnan(lont))] = np.nan
    xob[np.where(np.isnan(lont))] = np.nan
    xob = (xob - x_ori) / 1000.0
    yob = (yob - y_ori) / 1000.0
    if (sample_step < 0) or (skip > 1):
        samples, testt, testd = D.drifter_split(tob.shape[0], tob.shape[1], sample_step, skip)

        def pick(a):
            return np.reshape(a[samples, ::skip], [-1, 1]), np.reshape(a[testt[:, None], testd], [-1, 1])
    else:
        samples, test = D.split_indices(xob.size, sample_step)

        def pick(a):
            return np.reshape(a, [-1])[samples, None], np.reshape(a, [-1])[test, None]
    (to, tt), (yo, yt), (xo, xt) = pick(tob), pick(yob), pick(xob)
    (lat_o, lat_t), (lon_o, lon_t) = pick(latt), pick(lont)
    (uo, ut), (vo, vt) = pick(uob), pick(vob)
    do, dt_ = pick(dob)
    vo_mask = np.where((~np.isnan(xo)) & (~np.isnan(yo)))
    vt_mask = np.where((~np.isnan(xt)) & (~np.isnan(yt)))
    o = [a[vo_mask][:, None] for a in (to, yo, xo, lat_o, lon_o, uo, vo)]
    t = [a[vt_mask][:, None] for a in (tt, yt, xt, lat_t, lon_t, ut, vt)]
    return dict(X=np.concatenate([o[0], o[1], o[2]], 1), LL_o=np.concatenate([o[0], o[3], o[4]], 1),
                uo=o[5], vo=o[6], Xt=np.concatenate([t[0], t[1], t[2]], 1),
                LL_t=np.concatenate([t[0], t[3], t[4]], 1), ut=t[5], vt=t[6],
                drifter_o=do[vo_mask], drifter_t=dt_[vt_mask])


def kriging(st, et, lalim=(0, 0), lolim=(0, 0), sample_step=5, skip=5, nKernels=1, output="rbfModel",
            pkg="gp2d", kernelType=1, laser=1, tracks: Tracks = None, hyper: dict = None, device=None,
            drop_drifters=(), trend=None):
    """krig.kriging (krig.py:259-418): build the GP model(s) for a drifter data window.

    kernelType 1: scalar ARD RBF on (T, Y, X), one model per component (v, u);
    2 / 3 / 4: Kt(var_t, l_t) × div-free / curl-free / mixed vector kernel on (T, Y, X) with
    obs = [v; u] (krig.py:392-404; hyper 'temporal': False → spatial kernel on (Y, X)).
    nKernels > 1 sums nKernels terms (krig.py:405-407): for kernelType 1 identical ARD terms (≤ 2
    supported); for kernelType 2 / 3 / 4 min(nKernels, 3) vector terms of that kind, one per flow
    scale (engine family 'vector_sum'), where hyper's l_df, l_cf, ratio, variance (the terms'
    weights), var_t and l_t may be scalars (repeated) or per-term sequences; a spatio-temporal
    term's amplitude is its var_t, so its weight defaults to 1.  nKernels = 1 is the one-term model
    and its files, unchanged.  Hyperparameters come from `hyper` (no optimisation here).
    Writes output+'.npz' (the .mat of krig.py:417) and the model files; returns the models.
    trend ('constant' | 'linear', kernelType 2 / 3 / 4): a background flow estimated with the fit
    (Krig(trend=)); the first basis coordinate and component are the points' Y and the obs' v.
    """
    if tracks is None:
        raise ValueError("tracks= is required (the reference's Filtered_2016_2_7.pkl is not available)")
    t0 = time.time()
    h = dict(l_df=5.0, l_cf=5.0, ratio=None, noise=0.0025, variance=1.0, lengthscale=(1.0, 1.0, 1.0),
             var_t=1.0, l_t=1.0, temporal=True)
    h.update(hyper or {})
    d = _prepare(tracks, st, et, lalim, lolim, sample_step, skip, drop_drifters)
    X, Xt = d["X"], d["Xt"]
    models = {}
    if kernelType == 1:
        nk = min(int(nKernels), 2)
        spec = E.KernelSpec(family="ard", variances=tuple([h["variance"]] * nk),
                            lengthscales=tuple([tuple(h["lengthscale"])] * nk))
        for name, obs in (("v", d["vo"]), ("u", d["uo"])):
            k = Krig(spec, noise=h["noise"], var_mode="gpy", device=device, trend=trend).fit(X, obs[:, 0])
            k.save(output + f"_{name}.npz")
            models[name] = k
        obs_all = np.concatenate([d["vo"], d["uo"]], 1)
        obst = np.concatenate([d["vt"], d["ut"]], 1)
    else:
        kind = {2: "df", 3: "cf", 4: "mixed"}[int(kernelType)]
        obs_all = np.concatenate([d["vo"], d["uo"]], 0)
        obst = np.concatenate([d["vt"], d["ut"]], 0)
        ratio = h["ratio"] if h["ratio"] is not None else {"df": 1.0, "cf": 0.0, "mixed": 0.5}[kind]
        nk = min(int(nKernels), E.N.SUM_MAX_TERMS)
        if nk > 1:
            def per_term(v):
                v = list(v) if np.ndim(v) else [v] * nk
                if len(v) != nk:
                    raise ValueError(f"a per-term hyperparameter needs {nk} values, got {len(v)}")
                return [float(a) for a in v]
            fam = "vector_st" if h["temporal"] else "vector2d"
            cols = [per_term(h[n]) for n in ("l_df", "l_cf", "var_t", "l_t")] + [per_term(ratio)]
            terms = tuple(E.KernelSpec(family=fam, kind=kind, l_df=a, l_cf=b, ratio=r, var_t=vt, l_t=lt)
                          for a, b, vt, lt, r in zip(*cols))
            spec = E.KernelSpec(family="vector_sum", terms=terms, weights=tuple(per_term(h["variance"])))
            k = Krig(spec, noise=h["noise"], var_mode="gpy", device=device, trend=trend).fit(
                X if h["temporal"] else X[:, 1:3], obs_all[:, 0])
        elif h["temporal"]:
            spec = E.KernelSpec(family="vector_st", kind=kind, l_df=h["l_df"], l_cf=h["l_cf"], ratio=ratio,
                                var_t=h["var_t"], l_t=h["l_t"])
            k = Krig(spec, noise=h["noise"], var_mode="gpy", device=device, trend=trend).fit(X, obs_all[:, 0])
        else:
            k = Krig(kind, l_df=h["l_df"], l_cf=h["l_cf"], ratio=ratio, noise=h["noise"], var_mode="gpy",
                     device=device, trend=trend).fit(X[:, 1:3], obs_all[:, 0])
        tag = {2: "_divFree", 3: "_curlFree", 4: "_combined"}[int(kernelType)]
        k.save(output + tag + ".npz")
        models[tag] = k
    np.savez(output + ".npz", Xo=X, obs=obs_all, Xt=Xt, LL_o=d["LL_o"], LL_t=d["LL_t"], test_points=obst,
             kernelType=kernelType, drifter=d["drifter_o"])
    print("End of script, time : " + str(time.time() - t0))
    return models


def runRestarts(fname, nres=10, nKernels=2, device=None, seed=0, objective="lml"):
    """krig.runRestarts (krig.py:430-468): load a saved model, optimize_restarts its
    hyperparameters (nres runs; objective 'lml' | 'loo' as Krig.optimize_restarts), save it back
    and print old : new values.  Model files are
    .npz (Krig.save) instead of GPy pickles; the restart history is kept in the model file
    (the reference's fname_dict.pkl workaround, krig.py:439-457, is not needed)."""
    t0 = time.time()
    filename = fname if fname.endswith(".npz") else fname + ".npz"
    model = Krig.load(filename, device=device)
    hyp_old = model.param_array.copy()
    res = model.optimize_restarts(num_restarts=nres, seed=seed, objective=objective)
    hyp = model.param_array
    model.save(filename)
    print("Optimized Hyperparameters =================================================")
    names = E.param_names(model.spec)
    for nm, a, b in zip(names, hyp_old, hyp):   # a kernel sum: weight_t, l_df_t, … per term, as krig.py:459-466
        print(f"{nm} = {a}   :   {b}")
    print("===========================================================================")
    print("End of script, time : " + str(time.time() - t0))
    return res


def _vec_cols(model, X):
    """(T, Y, X) rows for the spatio-temporal kernel, (Y, X) for the spatial one."""
    return X if model.spec.input_dim == 3 else X[:, 1:3]


def predict(filename, tlim=(0, 0), ylim=(0, 0), xlim=(0, 0), dt=0.5, dx=0.5, xL=40, yL=40, Simul=0,
            device=None):
    """krig.predict (krig.py:471-574): grid posterior per time slice for the u and v
    models saved by kriging(); writes filename+'.nc' (krig.py:559-570) and filename+'_pred.npz', returns
    (Xp, V, U, VVar, UVar) reshaped [tp, yp, xp]."""
    t0 = time.time()
    f = np.load(filename + ".npz", allow_pickle=False)
    kt = int(f["kernelType"]) if "kernelType" in f.files else 1
    if (ylim[0] == ylim[1]) and (xlim[0] == xlim[1]):
        Xo = f["Xo"]
        Xp, tp, yp, xp = getGrid(Xo[:, 0], Xo[:, 1], Xo[:, 2])
    else:
        Xp, tp, yp, xp = getGrid(tlim, ylim, xlim, dt, dx, xL, yL)
    inc = yp.size * xp.size
    V, U, VV, UV = [], [], [], []
    if kt == 1:
        mv = Krig.load(filename + "_v.npz", device=device)
        mu_ = Krig.load(filename + "_u.npz", device=device)
    else:
        tag = {2: "_divFree", 3: "_curlFree", 4: "_combined"}[kt]
        mvec = Krig.load(filename + tag + ".npz", device=device)
    for i in range(tp.size):                         # krig.py:541-557
        Xp2 = Xp[i * inc:(i + 1) * inc, :]
        if kt == 1:
            v2, vv2 = mv.predict(Xp2)
            u2, uv2 = mu_.predict(Xp2)
        else:
            f2, fv2 = mvec.predict(_vec_cols(mvec, Xp2))
            v2, u2 = f2[:inc], f2[inc:]
            vv2, uv2 = fv2[:inc], fv2[inc:]
        V.append(v2)
        U.append(u2)
        VV.append(vv2)
        UV.append(uv2)
    shp = [tp.size, yp.size, xp.size]
    V, U, VV, UV = (np.reshape(np.concatenate(a, 0), shp) for a in (V, U, VV, UV))
    np.savez(filename + "_pred.npz", time=tp, y=yp, x=xp, v=V, u=U, vvar=VV, uvar=UV)
    # NetCDF-3 product, krig.py:559-570 (createNC + writeNC of v, u, vvar, uvar, hyperparams)
    hyp_v = (mv if kt == 1 else mvec).param_array
    hyp_u = (mu_ if kt == 1 else mvec).param_array
    NC.write_prediction(filename + ".nc", tp, yp, xp, V, U, VV, UV, hyp_v, hyp_u)
    print("End of script, time : " + str(time.time() - t0))
    return Xp, V, U, VV, UV


def predictTest(filename, device=None):
    """krig.predictTest (krig.py:578-616): predict at the held-out test points in 10
    chunks (step = Nt // 10, the py2 integer division of krig.py:593)."""
    f = np.load(filename + ".npz", allow_pickle=False)
    Xt = f["Xt"]
    obst = f["test_points"]
    kt = int(f["kernelType"]) if "kernelType" in f.files else 1
    Nt = Xt.shape[0]
    step = max(Nt // 10, 1)
    if kt == 1:
        mv = Krig.load(filename + "_v.npz", device=device)
        mu_ = Krig.load(filename + "_u.npz", device=device)
    else:
        tag = {2: "_divFree", 3: "_curlFree", 4: "_combined"}[kt]
        mvec = Krig.load(filename + tag + ".npz", device=device)
    V, U, VV, UV = [], [], [], []
    for i in range(0, Nt, step):
        Xt2 = Xt[i:i + step, :] if i + step < Nt else Xt[i:, :]
        if kt == 1:
            v2, vv2 = mv.predict(Xt2)
            u2, uv2 = mu_.predict(Xt2)
        else:
            m = Xt2.shape[0]
            f2, fv2 = mvec.predict(_vec_cols(mvec, Xt2))
            v2, u2, vv2, uv2 = f2[:m], f2[m:], fv2[:m], fv2[m:]
        V.append(v2)
        U.append(u2)
        VV.append(vv2)
        UV.append(uv2)
    V, U, VV, UV = (np.concatenate(a, 0) for a in (V, U, VV, UV))
    np.savez(filename + "_test.npz", Xt=Xt, Vp=V, VpVar=VV, Up=U, UpVar=UV, test_points=obst)
    return V, U, VV, UV


def crossValidate(filename, by="point", device=None):
    """Score the model(s) saved by kriging() on their own training data without a refit
    (Krig.cross_validate): by="point" leaves each observation out in turn, by="drifter" each
    drifter's whole track (the drifter column kriging() stores beside the inputs).  What
    predictTest + rmse (krig.py:578-646) measure on a held-out split — and
    laser_compare_interp.py by dropping drifters — read off the one fit that uses every
    observation.  Returns {model name: cross_validate dict} ('v' and 'u' for kernelType 1, the
    vector model's tag otherwise) and writes filename+'_cv.npz' with their scalar scores."""
    if by not in ("point", "drifter"):
        raise ValueError("by must be 'point' or 'drifter'")
    f = np.load(filename + ".npz", allow_pickle=False)
    kt = int(f["kernelType"]) if "kernelType" in f.files else 1
    groups = None
    if by == "drifter":
        if "drifter" not in f.files:
            raise ValueError(f"{filename}.npz carries no drifter column (written before crossValidate); "
                             "run kriging() again")
        groups = np.asarray(f["drifter"], dtype=np.int64).reshape(-1)
    tags = ("_v", "_u") if kt == 1 else ({2: "_divFree", 3: "_curlFree", 4: "_combined"}[kt],)
    out, scores = {}, {}
    for tag in tags:
        res = Krig.load(filename + tag + ".npz", device=device).cross_validate(groups=groups)
        name = tag[1:] if kt == 1 else tag
        out[name] = res
        for k in ("rmse_u", "rmse_v", "mean_lpd", "msll_chi2"):
            scores[f"{name.lstrip('_')}_{k}"] = res[k]
    np.savez(filename + "_cv.npz", by=by, **scores)
    return out


def _prior_window(fm, tcenter, tlim, xlim, xrange, varname):
    """scikit_prior's observation window (krig.py:146-167): observation and test points within
    ±tlim of tcenter and within xrange of the x window, stacked [obs; test], and the chosen
    velocity component.  Bit-exact with the reference (tests/golden/prior_window.npz); a
    window holding a single point stays 2-D here (the reference's squeeze() would make it 1-D)."""
    to, tt = fm["Xo"][:, 0], fm["Xt"][:, 0]
    xo, xt = fm["Xo"][:, 2], fm["Xt"][:, 2]
    ito = np.where((to >= tcenter - tlim) & (to <= tcenter + tlim) & (xo >= xlim[0] - xrange) & (xo <= xlim[1] + xrange))
    itt = np.where((tt >= tcenter - tlim) & (tt <= tcenter + tlim) & (xt >= xlim[0] - xrange) & (xt <= xlim[1] + xrange))
    Xo = fm["Xo"][ito, :].squeeze(0)
    Xt = fm["Xt"][itt, :].squeeze(0)
    XT = np.concatenate([Xo, Xt], axis=0)
    obs = fm["obs"][ito, :].squeeze(0)
    obst = fm["test_points"][itt, :].squeeze(0)
    col = 1 if varname == "u" else 0
    return XT, np.concatenate([obs[:, col], obst[:, col]])


RADAR_T0 = datetime(2016, 1, 1)             # radar time origin (days), krig.py:110
RADAR_T0D = datetime(2016, 2, 7, 2, 15)     # first time of Filtered_2016_2_7.pkl, krig.py:111


def radar_grid(radar):
    """The HF-radar grid branch of scikit_prior (krig.py:98-118): the radar NetCDF's image
    origin (imageOriginPosition = lon, lat) projected and shifted to the drifter frame in km,
    plus its xCoords / yCoords (m); the first radar time, counted in days from 2016-01-01,
    becomes hours since the drifter data's first time.  Returns (X (M, 3) in T, Y, X order,
    tcenter, yg, xg) with the meshgrid(yg, tg, xg) flattening of krig.py:114-118.
    Reference quirk: that branch never sets `tcenter`, which krig.py:143 then reads (NameError);
    the build takes the radar time tg as the window centre, the evident intent."""
    R = NC.readNC(radar)
    lon_r, lat_r = (float(v) for v in np.asarray(R["imageOriginPosition"], dtype=np.float64).reshape(-1)[:2])
    x0, y0 = nad83(lon_r, lat_r)
    x0 = (x0 - x_ori) / 1000.0
    y0 = (y0 - y_ori) / 1000.0
    xg = x0 + np.asarray(R["xCoords"], dtype=np.float64) / 1000.0
    yg = y0 + np.asarray(R["yCoords"], dtype=np.float64) / 1000.0
    tr = np.asarray(R["time"], dtype=np.float64).reshape(-1)
    tg = np.array([(RADAR_T0 + timedelta(float(tr[0])) - RADAR_T0D).total_seconds() / 3600])
    Yg, Tg, Xg = np.meshgrid(yg, tg, xg)
    X = np.concatenate([Tg.reshape(-1, 1), Yg.reshape(-1, 1), Xg.reshape(-1, 1)], axis=1)
    return X, tg, yg, xg


def scikit_prior(filename0, varname="v", dt=0, tlim=6, radar="", xlim=(0, 0), ylim=(0, 0), dx=0, ind=0, xrange=3,
                 HP=None, device=None):
    """krig.scikit_prior (krig.py:88-207): fixed-hyperparameter scalar GP
    HP0·RBF([lt,ly,lx]) (+ HP4·RBF) + White(noise) on the windowed observations,
    predicted on a radar NetCDF's grid (radar=path, radar_grid, krig.py:98-118), at time dt
    on the getGrid window (xlim/ylim given) or on the grid of a pre-existing
    filename0+'.nc' (krig.py:123-141).  Model inputs come from
    filename0+'.npz' (written by kriging); HP = [var1, lt, ly, lx, (var2, lt, ly, lx,) noise]
    (the GPy param_array the reference loads at krig.py:159-161).
    Writes <filename>_<t>h_scikit_<ind>.nc (createNC if absent, then varname, varname+'var',
    hyperparam_<varname>, krig.py:197-206) and returns (U, Ustd²) reshaped [1, yg, xg]."""
    fm = np.load(filename0 + ".npz", allow_pickle=False)
    if HP is None:
        raise ValueError("HP (hyperparameters) is required: the reference reads them from a GPy pickle")
    HP = np.asarray(HP, dtype=np.float64)
    if radar:                                                         # krig.py:98-118
        X, tcenter, yg, xg = radar_grid(radar)
        filename = filename0 + "_radar"
    elif (xlim[1] > xlim[0]) and (ylim[1] > ylim[0]):
        X, tcenter, yg, xg = getGrid([dt, dt + 1], ylim, xlim, 1, dx)   # krig.py:121
        filename = filename0 + "_cyc"
    else:                                                             # krig.py:123-141
        g = NC.readNC(filename0 + ".nc")
        xg, yg, tg = (np.asarray(g[k], dtype=np.float64) for k in ("x", "y", "time"))
        it = int(dt)
        tcenter = np.array([tg[it]])
        Yg, Tg, Xg = np.meshgrid(yg, tg, xg)
        X = np.concatenate([Tg.reshape(-1, 1), Yg.reshape(-1, 1), Xg.reshape(-1, 1)], 1)
        filename = filename0
        inc = yg.size * xg.size
        X = X[inc * it:inc * it + inc, :]
    filename = filename + "_" + str(np.round(tcenter[0], decimals=2)) + "h_scikit_"
    outFile = filename + str(ind) + ".nc"
    XT, u = _prior_window(fm, tcenter, tlim, xlim, xrange, varname)
    N = HP.size - 1
    variances = [HP[0]]
    lengths = [tuple(HP[1:4])]
    if N > 5:
        variances.append(HP[4])
        lengths.append(tuple(HP[5:8]))
    spec = E.KernelSpec(family="ard", variances=tuple(variances), lengthscales=tuple(lengths))
    # sklearn: WhiteKernel adds noise to K_y and to the predictive diagonal; fit adds alpha=1e-10
    k = Krig(spec, noise=HP[-1], jitter=1e-10, var_mode="sklearn", device=device).fit(XT, u)
    Um, Uvar = k.predict(X)
    U = np.reshape(Um, [tcenter.size, yg.size, xg.size])
    Ustd2 = np.reshape(Uvar, [tcenter.size, yg.size, xg.size])
    if not os.path.isfile(outFile):
        NC.createNC(outFile, tcenter, yg, xg, HP)
    with NC.openNC(outFile, "a") as fi:
        NC.writeNC(fi, varname, U)
        NC.writeNC(fi, varname + "var", Ustd2)
        NC.writeNC(fi, "hyperparam_" + varname, HP)
    return U, Ustd2


def laser(xo, yo, uo, vo, l_df=5, l_cf=5, rate=0.5, noise=0.0025, nsamples=1, dx=0.5, device=None, trend=None):
    """GP_laser.laser (GP_laser.py:16-142) from projected observations (the pickle /
    pyproj loading of GP_laser.py:26-78 is data plumbing outside the hot path):
    stride-3 split, grid over obs ∪ test ± 5 km, mixed kernel rate·K_df + (1−rate)·K_cf
    + noise·I, posterior mean / variance on the grid and mean at the test points.
    Returns (x, y, uf, vf, xo, yo, uo, vo, uvar, vvar, xt, yt, ut, vt, uft, vft).
    trend ('constant' | 'linear'): a background flow estimated with the fit (Krig(trend=))."""
    xo, yo, uo, vo = (np.asarray(a, dtype=np.float64).reshape(-1) for a in (xo, yo, uo, vo))
    if nsamples > 0:
        samples, test = D.split_indices(xo.size, 3)
        xt, yt, ut, vt = xo[test], yo[test], uo[test], vo[test]
        xo, yo, uo, vo = xo[samples], yo[samples], uo[samples], vo[samples]
    else:
        xt = yt = ut = vt = np.array([0.0])
    x, y, Xs, Ys = D.laser_grid(xo, yo, xt, yt, dx=dx)
    k = Krig("mixed", l_df=l_df, l_cf=l_cf, ratio=rate, noise=noise, device=device, trend=trend)
    k.fit(np.stack([xo, yo], 1), np.concatenate([uo, vo]))
    uf, vf, uvar, vvar = k.predict_grid(x, y)
    ft, _ = k.predict(np.stack([xt, yt], 1), compute_var=False)
    ft = ft[:, 0]
    return x, y, uf, vf, xo, yo, uo, vo, uvar, vvar, xt, yt, ut, vt, ft[:ft.size // 2], ft[ft.size // 2:]
