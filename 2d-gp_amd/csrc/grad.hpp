// grad.hpp — the velocity gradient tensor ∇f = (∂f1/∂x1, ∂f1/∂x2, ∂f2/∂x1, ∂f2/∂x2) of the fitted
// GP at the target points, with its 4 × 4 posterior covariance per target.
//
// Replaces nothing in the reference, whose users finite-difference predicted grids (GP_plots.py).
// Every linear kinematic diagnostic (divergence, vorticity, normal and shear strain) is aᵀ∇f, and
// the Okubo–Weiss parameter is quadratic in ∇f, so one predict of ∇f with its joint covariance
// serves them all; fields.hpp's δ and ζ are two of its linear combinations.
//
// Component c = 2a + b: a the field component (0, 1), b the direction (0, 1).  With d = x − g
// (training point minus target point), r² = d1² + d2², a = 1/ℓ², E = exp(−a r²/2),
//   T_pqb(d; ℓ) = E·[a²(δ_pq d_b + δ_pb d_q + δ_qb d_p) − a³ d_p d_q d_b]   (symmetric in p, q, b),
//   h_b(d; ℓ)   = Σ_c T_ccb = E·a²·d_b·(4 − a r²)                          (fields.hpp's h),
//   cov(f_p(x), ∂f_a/∂x_b (g)) = w_cf·T_pab(d; ℓ_cf) + w_df·(δ_pa·h_b(d; ℓ_df) − T_pab(d; ℓ_df)),
// w_df = 1 | 0 | ratio and w_cf = 0 | 1 | 1 − ratio for df | cf | mixed; the spatio-temporal product
// multiplies by its temporal factor.  Prior at zero lag, S_pqbd = δ_pq δ_bd + δ_pb δ_qd + δ_pd δ_qb:
//   cov(∂_b f_a, ∂_d f_c) = w_cf/ℓ_cf⁴·S_acbd + w_df/ℓ_df⁴·(4 δ_ac δ_bd − S_acbd)   (× var_t).
//
// Column layout of the cross-covariance matrix C (n × 4·cp), the contract between
// GradEntry, gemm_f64_kernel's EPI_COLGRAM epilogue and grad_finalize_kernel: target t
// of the chunk, component c, is column 64·(t / 16) + 16·c + (t mod 16).  The four components of a
// target are 16 columns apart inside one 64-column group, which is how a lane of the GEMM holds its
// four column accumulators — all ten products Σ_i V_ia·V_ib of a target are in-lane.
#pragma once
#include "fields.hpp"
#include "gemm_f64.hpp"

namespace gp2d {

constexpr int GRAD_NC = 4;      // components of ∇f per target
constexpr int GRAD_NPAIR = 10;  // entries (a ≤ b) of the symmetric 4 × 4 Gram
static_assert(GRAD_NPAIR == EPI_COLGRAM_PAIRS, "the epilogue and the finalize agree on the pair count");

// column of component c of chunk target t
__host__ __device__ inline int64_t grad_col(int64_t t, int c) { return 64 * (t / 16) + 16 * c + (t % 16); }

// The 4 × 4 prior covariance of ∇f at one point, row-major; a part of weight 0 is left out (its
// length scale may be unset).
inline void grad_prior_cov(const gp2d_kernel_t* k, double out[16]) {
  const double w_df = field_weight(k, GP2D_FIELD_VORTICITY), w_cf = field_weight(k, GP2D_FIELD_DIVERGENCE);
  const double vt = temporal_var(k);
  const double q_df = (w_df != 0.0) ? w_df / (k->l_df * k->l_df * k->l_df * k->l_df) : 0.0;
  const double q_cf = (w_cf != 0.0) ? w_cf / (k->l_cf * k->l_cf * k->l_cf * k->l_cf) : 0.0;
  for (int a = 0; a < 2; ++a)
    for (int b = 0; b < 2; ++b)
      for (int c = 0; c < 2; ++c)
        for (int d = 0; d < 2; ++d) {
          const double S = (double)((a == c && b == d) + (a == b && c == d) + (a == d && c == b));
          const double D = (a == c && b == d) ? 4.0 : 0.0;
          out[4 * (2 * a + b) + 2 * c + d] = vt * (q_cf * S + q_df * (D - S));
        }
}

// One part's third-derivative terms: T111, T112, T122, T222 and h1, h2, all times s = w·tf·E.
struct GradPart { double t111, t112, t122, t222, h1, h2; };
__device__ __forceinline__ GradPart grad_part(double s, double a, double d1, double d2, double r2) {
  const double a2 = s * a * a, a3 = a2 * a;
  const double q1 = a3 * d1 * d1, q2 = a3 * d2 * d2;
  const double hs = a2 * (4.0 - a * r2);
  return {d1 * (3.0 * a2 - q1), d2 * (a2 - q1), d1 * (a2 - q2), d2 * (3.0 * a2 - q2), hs * d1, hs * d2};
}

// cross_cov_kernel's entry for C = cov(observations, ∇f at the targets): (2·na_pad) × 4·cp with
// leading dimension 4·cp, columns in the layout above; rows i and na_pad + i hold the f1 and f2
// cross-covariances of training point i.  The tile's targets own columns [4·jt, 4·jt + 256); for a
// fixed component the wave's 64 lanes store four 128-byte runs per row.  One exp per pair and part
// (one for a mixed kernel of equal lengths), one more for the spatio-temporal product.  Every
// element of the buffer is written — 0.0 for padded training rows and padded targets — since the
// Gram product reads all of it and the workspace is reused.
struct GradEntry : StoresAll {
  static constexpr int ROWS = 2, COLS = GRAD_NC;
  VecParams v;          // point layout, temporal factor, 1/ℓ² of both parts, same_len
  double w_df, w_cf;    // weights of the div-free and curl-free parts (0: the part is absent)
  __device__ __forceinline__ const VecParams& layout() const { return v; }
  // j < cp: the last column written is < 4·cp
  __device__ __forceinline__ int64_t col(int64_t j, int c, int64_t) const { return grad_col(j, c); }
  __device__ __forceinline__ void padded(bool, double (&o)[2][GRAD_NC]) const {
#pragma unroll
    for (int c = 0; c < GRAD_NC; ++c) o[0][c] = o[1][c] = 0.0;
  }
  __device__ __forceinline__ void value(const Point3& a, const Point3& b, bool, double (&o)[2][GRAD_NC]) const {
    padded(false, o);
    double* c1 = o[0];
    double* c2 = o[1];
    const double d1 = a.c[1] - b.c[1], d2 = a.c[2] - b.c[2];
    const double r2 = d1 * d1 + d2 * d2;
    const double tf = time_factor(v, a.c[0] - b.c[0]);
    double e_df = 0.0;
    if (w_df != 0.0) {   // δ_pa·h_b − T_pab
      e_df = exp(-0.5 * r2 * v.il_df2);
      const GradPart t = grad_part(w_df * tf * e_df, v.il_df2, d1, d2, r2);
      c1[0] = t.h1 - t.t111; c1[1] = t.h2 - t.t112; c1[2] = -t.t112; c1[3] = -t.t122;
      c2[0] = -t.t112; c2[1] = -t.t122; c2[2] = t.h1 - t.t122; c2[3] = t.h2 - t.t222;
    }
    if (w_cf != 0.0) {   // T_pab
      const double e = (w_df != 0.0 && v.same_len) ? e_df : exp(-0.5 * r2 * v.il_cf2);
      const GradPart t = grad_part(w_cf * tf * e, v.il_cf2, d1, d2, r2);
      c1[0] += t.t111; c1[1] += t.t112; c1[2] += t.t112; c1[3] += t.t122;
      c2[0] += t.t112; c2[1] += t.t122; c2[2] += t.t122; c2[3] += t.t222;
    }
  }
};

inline GradEntry make_grad_entry(const gp2d_kernel_t* k) {
  GradEntry p;
  p.v = make_vec_params(k);
  p.w_df = field_weight(k, GP2D_FIELD_VORTICITY);
  p.w_cf = field_weight(k, GP2D_FIELD_DIVERGENCE);
  return p;
}

// Per target of the chunk: the mean's partial sums of its four columns and the ten Gram partials
// (G[bi][pair][t], pair = (a ≤ b) row by row, leading dimensions 10·cp and cp), each summed over
// the row blocks in ascending order.  mean[(c0 + t)·4 + c]; cov[(c0 + t)·16 + 4a + b] = prior_ab −
// G_ab, stored into (a, b) and (b, a) from one value: exactly symmetric.  Padded targets write
// nothing.  Launch: ⌈cv / 64⌉ workgroups of 64.
struct GradPrior { double p[GRAD_NC * GRAD_NC]; };
__global__ __launch_bounds__(64) void grad_finalize_kernel(
    const double* __restrict__ pm, const double* __restrict__ G, int64_t nseg, int64_t cp, int64_t cv,
    int64_t c0, GradPrior prior, int compute_cov, double* __restrict__ mean, double* __restrict__ cov) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= cv) return;
  const int64_t ncols = GRAD_NC * cp;
#pragma unroll
  for (int c = 0; c < GRAD_NC; ++c) {
    const int64_t col = grad_col(t, c);
    double mu = 0.0;
#pragma unroll 8
    for (int64_t g = 0; g < nseg; ++g) mu += pm[g * ncols + col];
    mean[(c0 + t) * GRAD_NC + c] = mu;
  }
  if (!compute_cov) return;
  double* o = cov + (c0 + t) * (GRAD_NC * GRAD_NC);
  int pair = 0;
#pragma unroll
  for (int a = 0; a < GRAD_NC; ++a)
#pragma unroll
    for (int b = a; b < GRAD_NC; ++b, ++pair) {
      double q = 0.0;
#pragma unroll 8
      for (int64_t g = 0; g < nseg; ++g) q += G[(g * GRAD_NPAIR + pair) * cp + t];
      const double v = prior.p[GRAD_NC * a + b] - q;
      o[GRAD_NC * a + b] = v;
      o[GRAD_NC * b + a] = v;
    }
}

}  // namespace gp2d
