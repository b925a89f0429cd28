// paths.hpp — ensembles advected through posterior draws of the flow: pathwise
// conditioning (Matheron's rule; Wilson et al. 2020) writes a posterior draw as a function,
//   g_s(x, t) = f_s(x, t) + K((x, t), X)·α_s,   α_s = K_y⁻¹(y − f_s(X) − ε_s),
// f_s a prior draw held as a finite sum of random Fourier features,
//   f_s(x, t) = Σ_j (a1_j, a2_j)·sin(w1_j·x1 + w2_j·x2 + τ_j·t + b_j),
// a feature table row [τ, w1, w2, b, a1, a2] per feature and draw (the host folds kind, ratio, sum
// weights and var_t into (a1, a2): the device does not know the kernel family of a feature).
//
// Replaces nothing in the reference, which never draws from its posterior.
//
// The update term is advect.hpp's training-point loop with the draw's own α (advect_pair<false>,
// the same staging, the same slices); the prior term is a second loop of the same shape over the
// draw's features: tiles of 64 features, tile T in slice T mod ADV_SLICES, a wave stages its tile's
// six doubles per feature through its own LDS region with one coalesced read and every lane reads
// them back at wave-uniform addresses.  Both loops add into the same two partial sums per slice,
// which meet in LDS and are added in slice order.  A workgroup is ADV_SLICES waves on 64 points of
// one draw (blockIdx.y): the staged α pair and feature are wave-uniform.  No atomics.  What the
// bits of a (draw, particle) depend on: its position, the draw's α and features, the training data
// and the step — not m, the number of draws, or either index.  Contraction is off as in advect.hpp.
#pragma once
#include "advect.hpp"

namespace gp2d {

constexpr int PATHS_FW = 6;   // doubles per feature: τ, w1, w2, b, a1, a2

// LDS of one workgroup: each slice's staged tile — training points as in AdvectShared, or 64
// feature rows —, the slices' partial sums, the kernel's terms.
template <bool ST>
struct PathsShared {
  static constexpr int PW = AdvectShared<ST, false>::PW;
  static constexpr int TW = PW > PATHS_FW ? PW : PATHS_FW;
  double pts[ADV_SLICES][ADV_TILE * TW];
  double red[ADV_SLICES][2][ADV_TILE];
  AdvectTerm term[GP2D_SUM_MAX_TERMS];
};

// sin θ for a feature's phase.  The device library's sin carries its large-argument reduction into
// the loop (paths_kernel: 113 VGPRs and 42 scalar spills with it); a phase is
// bounded by the domain over the length scale plus 2π, so θ is reduced here: k = rint(θ·2/π),
// r = θ − k·π/2 with π/2 in three parts (the first two of 33 bits: k·part is exact for |k| < 2^20,
// |θ| < 1.6e6; beyond it the error grows with |θ|/1.6e6 ulps of θ, gracefully), then the minimax
// polynomials of sin and cos on |r| ≤ π/4 (the classical fdlibm coefficients) and the quadrant.
// Absolute error below 2 ulp of 1 on the stated range; NaN and ±inf give NaN.  Host-callable for a
// CPU check against the C library.
__host__ __device__ __forceinline__ double paths_sin(double th) {
#pragma clang fp contract(off)
  const double k = __builtin_rint(th * 6.36619772367581382433e-01);
  double r = __builtin_fma(-k, 1.57079632673412561417e+00, th);
  r = __builtin_fma(-k, 6.07710050630396597660e-11, r);
  r = __builtin_fma(-k, 2.02226624879595063154e-21, r);
  const double z = r * r;
  double ps = __builtin_fma(z, 1.58969099521155010221e-10, -2.50507602534068634195e-08);
  ps = __builtin_fma(z, ps, 2.75573137070700676789e-06);
  ps = __builtin_fma(z, ps, -1.98412698298579493134e-04);
  ps = __builtin_fma(z, ps, 8.33333333332248946124e-03);
  ps = __builtin_fma(z, ps, -1.66666666666666324348e-01);
  const double sn = __builtin_fma(r * z, ps, r);
  double pc = __builtin_fma(z, -1.13596475577881948265e-11, 2.08757232129817482790e-09);
  pc = __builtin_fma(z, pc, -2.75573143513906633035e-07);
  pc = __builtin_fma(z, pc, 2.48015872894767294178e-05);
  pc = __builtin_fma(z, pc, -1.38888888888741095749e-03);
  pc = __builtin_fma(z, pc, 4.16666666666666019037e-02);
  const double cs = __builtin_fma(z * z, pc, __builtin_fma(-0.5, z, 1.0));
  // the quadrant k mod 4, in doubles (exact for every finite k)
  const double q = k - 4.0 * __builtin_rint(0.25 * k);   // −2, −1, 0, 1, 2
  const double v = (q == 1.0 || q == -1.0) ? cs : sn;
  return (q == 2.0 || q == -2.0 || q == -1.0) ? -v : v;
}

// g_s (u[0..1]) at the lane's point (g1, g2) — called by every thread of the workgroup; every wave
// returns the same bits for a point.  alpha, feat: the draw's own (alpha == NULL: the feature part
// only).  ts: the time of the update term's temporal factors, the same for the workgroup (formed by
// the staging lane, as in advect_eval); tl: the time of the lane's point in the feature phase.
template <bool ST>
__device__ __forceinline__ void paths_eval(PathsShared<ST>& sh, const double* __restrict__ alpha,
                                           const double* __restrict__ xtr, int64_t ntr, int64_t ntr_pad, int nterms,
                                           const double* __restrict__ feat, int64_t nfeat, double g1, double g2,
                                           double ts, double tl, int slice, int lane, double (&u)[2]) {
#pragma clang fp contract(off)
  constexpr int PW = PathsShared<ST>::PW, PD = ST ? 3 : 2;
  double s[2] = {0.0, 0.0};
  double* tile = sh.pts[slice];
  if (alpha != nullptr) {   // uniform over the launch
    for (int64_t gb = 0; gb < ntr; gb += ADV_SLICES * ADV_TILE) {
      const int64_t i0 = gb + (int64_t)slice * ADV_TILE, i = i0 + lane;
      double px = 0.0, py = 0.0, pu = 0.0, pv = 0.0, pt = 0.0;
      if (i < ntr) {   // xtr has ntr rows; α's padded tail is never read
        px = xtr[i * PD + PD - 2];
        py = xtr[i * PD + PD - 1];
        if constexpr (ST) pt = xtr[i * PD];
        pu = alpha[i];
        pv = alpha[ntr_pad + i];
      }
      tile[lane * PW + 0] = px;
      tile[lane * PW + 1] = py;
      tile[lane * PW + 2] = pu;
      tile[lane * PW + 3] = pv;
      if constexpr (ST) {
        const double dtm = pt - ts;
#pragma unroll 1
        for (int t = 0; t < nterms; ++t)
          tile[lane * PW + 4 + t] = sh.term[t].var_t * exp(-0.5 * (dtm * dtm) * sh.term[t].ilt2);
      }
      __syncthreads();   // one trip count for every wave
      const int cnt = (int)(ntr - i0 < ADV_TILE ? ntr - i0 : ADV_TILE);   // wave-uniform; ≤ 0: nothing
#pragma unroll 1
      for (int t = 0; t < nterms; ++t) {
        AdvectTerm k;
        k.w_df = adv_uniform(sh.term[t].w_df);
        k.w_cf = adv_uniform(sh.term[t].w_cf);
        k.il_df2 = adv_uniform(sh.term[t].il_df2);
        k.il_cf2 = adv_uniform(sh.term[t].il_cf2);
        k.same_len = __builtin_amdgcn_readfirstlane(sh.term[t].same_len);
#pragma unroll 2
        for (int p = 0; p < cnt; ++p) {
          const double* pp = tile + p * PW;   // wave-uniform address
          advect_pair<false>(k, ST ? pp[ST ? 4 + t : 0] : 1.0, pp[0] - g1, pp[1] - g2, pp[2], pp[3], s);
        }
      }
    }
  }
  // the features: the tile's 6·cnt doubles are contiguous — lane l takes elements l, l + 64, …
  for (int64_t fb = 0; fb < nfeat; fb += ADV_SLICES * ADV_TILE) {
    const int64_t f0 = fb + (int64_t)slice * ADV_TILE;
    const int cnt = (int)(nfeat - f0 < ADV_TILE ? nfeat - f0 : ADV_TILE);   // wave-uniform; ≤ 0: nothing
    const int ne = cnt * PATHS_FW;
    // the region is this wave's own: its reads of the last trip (or loop) were issued before these writes
#pragma unroll
    for (int q = 0; q < PATHS_FW; ++q) {
      const int e = lane + q * ADV_TILE;
      tile[e] = e < ne ? feat[f0 * PATHS_FW + e] : 0.0;
    }
    __syncthreads();   // one trip count for every wave
#pragma unroll 2
    for (int p = 0; p < cnt; ++p) {
      const double* pp = tile + p * PATHS_FW;   // wave-uniform address
      const double th = __builtin_fma(pp[1], g1, __builtin_fma(pp[2], g2, __builtin_fma(pp[0], tl, pp[3])));
      const double sn = paths_sin(th);
      s[0] = __builtin_fma(pp[4], sn, s[0]);
      s[1] = __builtin_fma(pp[5], sn, s[1]);
    }
  }
  sh.red[slice][0][lane] = s[0];
  sh.red[slice][1][lane] = s[1];
  __syncthreads();
#pragma unroll
  for (int q = 0; q < 2; ++q) {
    double v = sh.red[0][q][lane];
#pragma unroll
    for (int w = 1; w < ADV_SLICES; ++w) v += sh.red[w][q][lane];   // slice order
    u[q] = v;
  }
}

template <bool ST>
__device__ __forceinline__ void paths_stage_terms(PathsShared<ST>& sh, const AdvectKernel& kp) {
  if (threadIdx.x == 0) {
    sh.term[0] = kp.term[0];
    sh.term[1] = kp.term[1];
    sh.term[2] = kp.term[2];
  }
}

// The velocity of draw blockIdx.y at m fixed points: vel[s][u_1..u_m, v_1..v_m].  xg rows of dim
// doubles, the position in the last two; dim = 3 (alpha == NULL only): the row's own time in the
// first, else every point at time t.  Launch: (⌈m / 64⌉, S) workgroups of 64·ADV_SLICES threads.
template <bool ST>
__global__ __launch_bounds__(ADV_SLICES * ADV_TILE) void paths_eval_kernel(
    const double* __restrict__ alpha, int64_t n, const double* __restrict__ xtr, int64_t ntr, int64_t ntr_pad,
    AdvectKernel kp, const double* __restrict__ feat, int64_t nfeat, const double* __restrict__ xg, int64_t m, int dim,
    double t, double* __restrict__ vel) {
#pragma clang fp contract(off)
  __shared__ PathsShared<ST> sh;
  const int lane = threadIdx.x & 63;
  const int slice = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int64_t j = (int64_t)blockIdx.x * ADV_TILE + lane, d = blockIdx.y;
  const bool valid = j < m;
  paths_stage_terms(sh, kp);
  double g1 = 0.0, g2 = 0.0, tl = t;
  if (valid) {
    g1 = xg[j * dim + dim - 2];
    g2 = xg[j * dim + dim - 1];
    if (dim == 3) tl = xg[j * dim];
  }
  __syncthreads();   // the terms
  double u[2];
  paths_eval<ST>(sh, alpha == nullptr ? nullptr : alpha + d * n, xtr, ntr, ntr_pad, kp.nterms,
                 feat + d * nfeat * PATHS_FW, nfeat, g1, g2, t, tl, slice, lane, u);
  if (valid && slice == 0) {
    vel[d * 2 * m + j] = u[0];
    vel[d * 2 * m + m + j] = u[1];
  }
}

// Record r → record r + 1 of every draw: advect_kernel's RK4 step (its TANGENT = false path) through
// g_s.  xin, xout: S × m × 2.  Launch: (⌈m / 64⌉, S) workgroups of 64·ADV_SLICES threads.
template <bool ST>
__global__ __launch_bounds__(ADV_SLICES * ADV_TILE) void paths_kernel(
    const double* __restrict__ alpha, int64_t n, const double* __restrict__ xtr, int64_t ntr, int64_t ntr_pad,
    AdvectKernel kp, const double* __restrict__ feat, int64_t nfeat, const double* __restrict__ xin,
    double* __restrict__ xout, int64_t m, double t0, double dt, int n0, int nst, double vel_scale) {
#pragma clang fp contract(off)
  __shared__ PathsShared<ST> sh;
  const int lane = threadIdx.x & 63;
  const int slice = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int64_t j = (int64_t)blockIdx.x * ADV_TILE + lane, d = blockIdx.y;
  const bool valid = j < m;
  paths_stage_terms(sh, kp);
  alpha += d * n;
  feat += d * nfeat * PATHS_FW;
  xin += d * m * 2;
  xout += d * m * 2;
  double x1 = 0.0, x2 = 0.0;
  if (valid) {
    x1 = xin[2 * j];
    x2 = xin[2 * j + 1];
    if (!(__builtin_isfinite(x1) && __builtin_isfinite(x2))) x1 = x2 = __builtin_nan("");
  }
  __syncthreads();   // the terms
#pragma unroll 1
  for (int q = 0; q < nst; ++q) {
    const double tn = t0 + (double)(n0 + q) * dt;
    double a1 = 0.0, a2 = 0.0;
    double y1 = x1, y2 = x2;
#pragma unroll 1
    for (int st = 0; st < 4; ++st) {   // stage times t, t + h/2, t + h/2, t + h; weights 1, 2, 2, 1
      const double c = st == 0 ? 0.0 : (st == 3 ? 1.0 : 0.5);
      const double w = (st == 0 || st == 3) ? 1.0 : 2.0;
      const double h = (st == 2 ? 1.0 : 0.5) * dt;   // the next stage's offset
      const double ts = tn + c * dt;
      double u[2];
      paths_eval<ST>(sh, alpha, xtr, ntr, ntr_pad, kp.nterms, feat, nfeat, y1, y2, ts, ts, slice, lane, u);
      const double k1 = vel_scale * u[0], k2 = vel_scale * u[1];
      a1 += w * k1;
      a2 += w * k2;
      y1 = x1 + h * k1;
      y2 = x2 + h * k2;
    }
    const double h6 = dt / 6.0;
    x1 += h6 * a1;
    x2 += h6 * a2;
  }
  if (valid && slice == 0) {
    xout[2 * j] = x1;
    xout[2 * j + 1] = x2;
  }
}

// Record 0 of every draw: x0 (shared: m × 2, or per draw: S × m × 2), a non-finite start as NaN, NaN.
__global__ __launch_bounds__(256) void paths_init_kernel(const double* __restrict__ x0, int64_t m, int per_draw,
                                                         double* __restrict__ path0) {
  const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x, d = blockIdx.y;
  if (j >= m) return;
  const double* src = x0 + (per_draw ? d * m * 2 : 0);
  double x1 = src[2 * j], x2 = src[2 * j + 1];
  if (!(__builtin_isfinite(x1) && __builtin_isfinite(x2))) x1 = x2 = __builtin_nan("");
  path0[(d * m + j) * 2] = x1;
  path0[(d * m + j) * 2 + 1] = x2;
}

}  // namespace gp2d
