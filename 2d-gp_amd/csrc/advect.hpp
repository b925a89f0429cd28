// advect.hpp — particles advected through the fitted flow, with the flow map's gradient
// (DESIGN.md §3.13): classical RK4 of
//   dx/dt = s·μ(x, t),   dF/dt = s·∇μ(x, t)·F,   F(t0) = I,
// μ(x, t) = K(x, X)·α (+ h(x)ᵀβ̂ for a trend fit) the posterior mean velocity, ∇μ its 2 × 2 gradient in
// grad.hpp's component order c = 2a + b, s = vel_scale.  Trajectories, the finite-time Lyapunov
// exponent ln λ_max(FᵀF) / 2|T| and pair separation all integrate this system.
//
// Replaces nothing in the reference, which only reads drifter tracks (laser_io_methods.py) and never
// integrates its reconstructed field.
//
// The posterior mean at a moving point needs α and the training points only — no W, no K* in
// memory: a stage evaluation is one register-resident sum over the training points per particle.
// Mapping: a workgroup is ADV_SLICES waves on the same 64 particles; lane l of every wave holds
// particle 64·blockIdx.x + l for the whole launch (x, F, the stage state: registers).  The training
// points are cut into tiles of 64; tile T belongs to slice T mod ADV_SLICES.  A wave stages its
// tile's points with their α pair through its own LDS region (one coalesced read) and every lane
// reads them back at wave-uniform addresses; the slices' partial sums (2 velocity, 4 gradient) meet
// in LDS and every wave adds them in slice order, so all replicas of a particle carry the same bits
// and wave 0 stores.  No atomics.  What a particle's bits depend on: its own position, the training
// data and the step — not m, its index, or its neighbours.
//
// One exp per pair and part feeds the 2 × 2 block and the third-derivative terms (grad_part) alike;
// a mixed kernel of equal lengths takes one.  The spatio-temporal product's temporal factor is the
// same for every particle, so it is formed once per staged point, not per pair.  Floating-point
// contraction is off in the pair and step arithmetic and the fused operations are written out: the
// TANGENT = false instantiation then forms the path from the same operations as TANGENT = true.
#pragma once
#include "grad.hpp"
#include "trend.hpp"

namespace gp2d {

constexpr int ADV_SLICES = 4;   // waves per workgroup = slices of the training-point loop
constexpr int ADV_TILE = 64;    // training points per staged tile, particles per workgroup

// One term of the kernel (a sum's weight folded in): weights of the div-free and curl-free parts
// (0: the part is absent and its 1/ℓ² is 0), the temporal factor var_t·exp(−Δt²·ilt2/2).
struct AdvectTerm {
  double w_df, w_cf, il_df2, il_cf2, var_t, ilt2;
  int same_len, unused;
};

struct AdvectKernel {
  static_assert(GP2D_SUM_MAX_TERMS == 3, "advect_kernel's staging names every term");
  AdvectTerm term[GP2D_SUM_MAX_TERMS];
  int nterms;
};

// The fit's trend: q = 0 (zero-mean), 2 or 6 coefficients β̂ at block[TB_BETA..].
struct AdvectTrend {
  int q;
  TrendBasis basis;
  const double* block;
};

inline AdvectTerm make_advect_term(const gp2d_kernel_t* k, double w) {
  const VecParams v = make_vec_params(k);
  AdvectTerm t{};
  t.w_df = w * field_weight(k, GP2D_FIELD_VORTICITY);
  t.w_cf = w * field_weight(k, GP2D_FIELD_DIVERGENCE);
  t.il_df2 = (t.w_df != 0.0) ? v.il_df2 : 0.0;
  t.il_cf2 = (t.w_cf != 0.0) ? v.il_cf2 : 0.0;
  t.var_t = v.var_t;
  t.ilt2 = v.ilt2;
  t.same_len = (t.w_df != 0.0 && t.w_cf != 0.0 && v.same_len) ? 1 : 0;
  return t;
}

// a validated kernel of gp2d_advect's families; unused term slots repeat term 0 (never evaluated)
inline AdvectKernel make_advect_kernel(const gp2d_kernel_t* k) {
  AdvectKernel a;
  a.nterms = is_sum_family(k) ? k->nterms : 1;
  for (int t = 0; t < GP2D_SUM_MAX_TERMS; ++t) {
    const int s = t < a.nterms ? t : 0;
    a.term[t] = is_sum_family(k) ? make_advect_term(sum_term(k, s), sum_weight(k, s)) : make_advect_term(k, 1.0);
  }
  return a;
}

// a wave-uniform double into scalar registers
__device__ __forceinline__ double adv_uniform(double v) {
  return __hiloint2double(__builtin_amdgcn_readfirstlane(__double2hiint(v)),
                          __builtin_amdgcn_readfirstlane(__double2loint(v)));
}

constexpr int adv_nsum(bool tangent) { return tangent ? 6 : 2; }

// One training point's share of μ (s[0..1]) and ∇μ (s[2..5]) at a particle: d = the training point
// minus the particle, tf the term's temporal factor at the point, (au, av) the point's α pair.
template <bool TANGENT>
__device__ __forceinline__ void advect_pair(const AdvectTerm& k, double tf, double d1, double d2, double au,
                                            double av, double (&s)[adv_nsum(TANGENT)]) {
#pragma clang fp contract(off)
  const double p11 = d1 * d1, p12 = d1 * d2, p22 = d2 * d2;
  const double r2 = p11 + p22;
  double e_df = 0.0;
  if (k.w_df != 0.0) {   // wave-uniform
    const double a = k.il_df2;
    const double c = r2 * a;
    e_df = exp(-0.5 * c);
    const double sw = (k.w_df * tf) * e_df;
    const double e = sw * a, aux = 1.0 - c;
    const double f11 = e * __builtin_fma(p11, a, aux), f12 = e * (p12 * a), f22 = e * __builtin_fma(p22, a, aux);
    s[0] = __builtin_fma(f11, au, __builtin_fma(f12, av, s[0]));
    s[1] = __builtin_fma(f12, au, __builtin_fma(f22, av, s[1]));
    if constexpr (TANGENT) {   // δ_pa·h_b − T_pab
      const GradPart t = grad_part(sw, a, d1, d2, r2);
      s[2] = __builtin_fma(t.h1 - t.t111, au, __builtin_fma(-t.t112, av, s[2]));
      s[3] = __builtin_fma(t.h2 - t.t112, au, __builtin_fma(-t.t122, av, s[3]));
      s[4] = __builtin_fma(-t.t112, au, __builtin_fma(t.h1 - t.t122, av, s[4]));
      s[5] = __builtin_fma(-t.t122, au, __builtin_fma(t.h2 - t.t222, av, s[5]));
    }
  }
  if (k.w_cf != 0.0) {
    const double a = k.il_cf2;
    const double c = r2 * a;
    const double ecf = k.same_len ? e_df : exp(-0.5 * c);
    const double sw = (k.w_cf * tf) * ecf;
    const double e = sw * a;
    const double g11 = e * __builtin_fma(-p11, a, 1.0), g12 = -e * (p12 * a), g22 = e * __builtin_fma(-p22, a, 1.0);
    s[0] = __builtin_fma(g11, au, __builtin_fma(g12, av, s[0]));
    s[1] = __builtin_fma(g12, au, __builtin_fma(g22, av, s[1]));
    if constexpr (TANGENT) {   // T_pab
      const GradPart t = grad_part(sw, a, d1, d2, r2);
      s[2] = __builtin_fma(t.t111, au, __builtin_fma(t.t112, av, s[2]));
      s[3] = __builtin_fma(t.t112, au, __builtin_fma(t.t122, av, s[3]));
      s[4] = __builtin_fma(t.t112, au, __builtin_fma(t.t122, av, s[4]));
      s[5] = __builtin_fma(t.t122, au, __builtin_fma(t.t222, av, s[5]));
    }
  }
}

// LDS of one workgroup: each slice's staged tile — [x1, x2, α_u, α_v] per point, then for the
// spatio-temporal product every term's temporal factor at the stage time —, the slices' partial
// sums, the kernel's terms, the trend's basis (c1, c2, 1/scale) and β̂.
template <bool ST, bool TANGENT>
struct AdvectShared {
  static constexpr int PW = ST ? 4 + GP2D_SUM_MAX_TERMS : 4;
  double pts[ADV_SLICES][ADV_TILE * PW];
  double red[ADV_SLICES][adv_nsum(TANGENT)][ADV_TILE];
  AdvectTerm term[GP2D_SUM_MAX_TERMS];
  double basis[3], beta[TREND_QMAX];
};

// μ (u[0..1]) and ∇μ (g[0..3]) at the lane's particle (g1, g2) and time ts — called by every
// thread of the workgroup, with the same ts; every wave returns the same bits for a particle.
// The temporal factor var_t·exp(−(t_i − ts)²·ilt2/2) does not depend on the particle: the lane
// that stages point i forms it, once per term, so a pair of the spatio-temporal product costs the
// exps of its spatial parts and no more.
template <bool ST, bool TANGENT>
__device__ __forceinline__ void advect_eval(AdvectShared<ST, TANGENT>& sh, const double* __restrict__ alpha,
                                            const double* __restrict__ xtr, int64_t ntr, int64_t ntr_pad,
                                            int nterms, int tq, double g1, double g2, double ts, int slice,
                                            int lane, double (&u)[2], double (&g)[4]) {
#pragma clang fp contract(off)
  constexpr int PW = AdvectShared<ST, TANGENT>::PW, NS = adv_nsum(TANGENT), PD = ST ? 3 : 2;
  double s[NS];
#pragma unroll
  for (int q = 0; q < NS; ++q) s[q] = 0.0;
  double* tile = sh.pts[slice];
  // every wave takes the same number of trips (the barrier); a slice past the last tile has count ≤ 0
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
    // the region is this wave's own: its reads of the last trip were issued before these writes
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
    for (int t = 0; t < nterms; ++t) {   // wave-uniform trip count
      AdvectTerm k;
      k.w_df = adv_uniform(sh.term[t].w_df);
      k.w_cf = adv_uniform(sh.term[t].w_cf);
      k.il_df2 = adv_uniform(sh.term[t].il_df2);
      k.il_cf2 = adv_uniform(sh.term[t].il_cf2);
      k.same_len = __builtin_amdgcn_readfirstlane(sh.term[t].same_len);
#pragma unroll 2
      for (int p = 0; p < cnt; ++p) {
        const double* pp = tile + p * PW;   // wave-uniform address
        advect_pair<TANGENT>(k, ST ? pp[ST ? 4 + t : 0] : 1.0, pp[0] - g1, pp[1] - g2, pp[2], pp[3], s);
      }
    }
  }
#pragma unroll
  for (int q = 0; q < NS; ++q) sh.red[slice][q][lane] = s[q];
  __syncthreads();
#pragma unroll
  for (int q = 0; q < NS; ++q) {
    double v = sh.red[0][q][lane];
#pragma unroll
    for (int w = 1; w < ADV_SLICES; ++w) v += sh.red[w][q][lane];   // slice order
    s[q] = v;
  }
  u[0] = s[0];
  u[1] = s[1];
#pragma unroll
  for (int c = 0; c < 4; ++c) g[c] = TANGENT ? s[TANGENT ? 2 + c : 0] : 0.0;
  if (tq != 0) {   // h(x)ᵀβ̂: u = β0 + β2·ξ + β3·η, v = β1 + β4·ξ + β5·η
    u[0] += sh.beta[0];
    u[1] += sh.beta[1];
    if (tq == TREND_QMAX) {
      const double is = sh.basis[2];
      const double xi = (g1 - sh.basis[0]) * is, eta = (g2 - sh.basis[1]) * is;
      u[0] += sh.beta[2] * xi + sh.beta[3] * eta;
      u[1] += sh.beta[4] * xi + sh.beta[5] * eta;
      if constexpr (TANGENT) {
#pragma unroll
        for (int c = 0; c < 4; ++c) g[c] += sh.beta[2 + c] * is;
      }
    }
  }
}

// Record r → record r + 1: nst RK4 steps of size dt from step number n0 (step n starts at
// t0 + n·dt — formed from n, not accumulated, so the bits do not depend on where a launch starts).
// xin, xout: m × 2; fin, fout: m × 4 (TANGENT).  A non-finite position turns into NaN and stays NaN.
// Launch: ⌈m / 64⌉ workgroups of 64·ADV_SLICES threads.
template <bool ST, bool TANGENT>
__global__ __launch_bounds__(ADV_SLICES * ADV_TILE) void advect_kernel(
    const double* __restrict__ alpha, const double* __restrict__ xtr, int64_t ntr, int64_t ntr_pad, AdvectKernel kp,
    AdvectTrend tr, const double* __restrict__ xin, const double* __restrict__ fin, double* __restrict__ xout,
    double* __restrict__ fout, int64_t m, double t0, double dt, int n0, int nst, double vel_scale) {
#pragma clang fp contract(off)
  __shared__ AdvectShared<ST, TANGENT> sh;
  const int lane = threadIdx.x & 63;
  const int slice = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int64_t j = (int64_t)blockIdx.x * ADV_TILE + lane;
  const bool valid = j < m;
  if (threadIdx.x == 0) {
    sh.term[0] = kp.term[0];
    sh.term[1] = kp.term[1];
    sh.term[2] = kp.term[2];
    sh.basis[0] = tr.basis.c1;
    sh.basis[1] = tr.basis.c2;
    sh.basis[2] = tr.basis.is;
  }
  if (threadIdx.x < TREND_QMAX) sh.beta[threadIdx.x] = ((int)threadIdx.x < tr.q) ? tr.block[TB_BETA + threadIdx.x] : 0.0;
  double x1 = 0.0, x2 = 0.0;
  double F[4] = {1.0, 0.0, 0.0, 1.0};
  if (valid) {
    x1 = xin[2 * j];
    x2 = xin[2 * j + 1];
    if (!(__builtin_isfinite(x1) && __builtin_isfinite(x2))) x1 = x2 = __builtin_nan("");
    if constexpr (TANGENT) {
#pragma unroll
      for (int c = 0; c < 4; ++c) F[c] = fin[4 * j + c];
    }
  }
  __syncthreads();   // the terms and the trend
#pragma unroll 1
  for (int q = 0; q < nst; ++q) {
    const double tn = t0 + (double)(n0 + q) * dt;
    double a1 = 0.0, a2 = 0.0, aF[4] = {0.0, 0.0, 0.0, 0.0};
    double y1 = x1, y2 = x2, Y[4] = {F[0], F[1], F[2], F[3]};
#pragma unroll 1
    for (int st = 0; st < 4; ++st) {   // stage times t, t + h/2, t + h/2, t + h; weights 1, 2, 2, 1
      const double c = st == 0 ? 0.0 : (st == 3 ? 1.0 : 0.5);
      const double w = (st == 0 || st == 3) ? 1.0 : 2.0;
      const double h = (st == 2 ? 1.0 : 0.5) * dt;   // the next stage's offset
      double u[2], g[4];
      advect_eval<ST, TANGENT>(sh, alpha, xtr, ntr, ntr_pad, kp.nterms, tr.q, y1, y2, tn + c * dt, slice, lane, u, g);
      const double k1 = vel_scale * u[0], k2 = vel_scale * u[1];
      a1 += w * k1;
      a2 += w * k2;
      y1 = x1 + h * k1;
      y2 = x2 + h * k2;
      if constexpr (TANGENT) {
        const double kF[4] = {vel_scale * (g[0] * Y[0] + g[1] * Y[2]), vel_scale * (g[0] * Y[1] + g[1] * Y[3]),
                              vel_scale * (g[2] * Y[0] + g[3] * Y[2]), vel_scale * (g[2] * Y[1] + g[3] * Y[3])};
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          aF[e] += w * kF[e];
          Y[e] = F[e] + h * kF[e];
        }
      }
    }
    const double h6 = dt / 6.0;
    x1 += h6 * a1;
    x2 += h6 * a2;
    if constexpr (TANGENT) {
#pragma unroll
      for (int e = 0; e < 4; ++e) F[e] += h6 * aF[e];
    }
  }
  if (valid && slice == 0) {
    xout[2 * j] = x1;
    xout[2 * j + 1] = x2;
    if constexpr (TANGENT) {
#pragma unroll
      for (int c = 0; c < 4; ++c) fout[4 * j + c] = F[c];
    }
  }
}

// Record 0: path0 = x0 (a non-finite start as NaN, NaN) and tangent0 = I (if asked).
__global__ __launch_bounds__(256) void advect_init_kernel(const double* __restrict__ x0, int64_t m,
                                                          double* __restrict__ path0, double* __restrict__ tangent0) {
  const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (j >= m) return;
  double x1 = x0[2 * j], x2 = x0[2 * j + 1];
  if (!(__builtin_isfinite(x1) && __builtin_isfinite(x2))) x1 = x2 = __builtin_nan("");
  path0[2 * j] = x1;
  path0[2 * j + 1] = x2;
  if (tangent0 != nullptr) {
    tangent0[4 * j] = 1.0;
    tangent0[4 * j + 1] = 0.0;
    tangent0[4 * j + 2] = 0.0;
    tangent0[4 * j + 3] = 1.0;
  }
}

// One launch of advect_kernel<ST, tangent>: ⌈m / 64⌉ workgroups.
template <bool ST>
inline int launch_advect(bool tangent, unsigned grid, hipStream_t s, const double* alpha, const double* xtr,
                         int64_t ntr, int64_t ntr_pad, const AdvectKernel& ak, const AdvectTrend& at,
                         const double* xin, const double* fin, double* xout, double* fout, int64_t m, double t0,
                         double dt, int n0, int nst, double vel_scale) {
  if (tangent)
    advect_kernel<ST, true><<<grid, ADV_SLICES * ADV_TILE, 0, s>>>(alpha, xtr, ntr, ntr_pad, ak, at, xin, fin, xout,
                                                                    fout, m, t0, dt, n0, nst, vel_scale);
  else
    advect_kernel<ST, false><<<grid, ADV_SLICES * ADV_TILE, 0, s>>>(alpha, xtr, ntr, ntr_pad, ak, at, xin, nullptr,
                                                                     xout, nullptr, m, t0, dt, n0, nst, vel_scale);
  return check_launch("advect_kernel");
}

}  // namespace gp2d
