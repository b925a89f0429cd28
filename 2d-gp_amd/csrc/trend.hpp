// trend.hpp — a constant or linear background flow estimated with the fit (universal kriging:
// explicit basis functions with a vague prior on their coefficients, Rasmussen & Williams §2.7;
// DESIGN.md §3.11).
//
// Replaces nothing in the reference, whose models are all zero-mean (krig.py, GP_laser.py never
// subtract or model a mean flow).
//
// Basis coordinates ξ = (x1 − c1)/s, η = (x2 − c2)/s (gp2d_trend_t: centre c, scale s; the two
// spatial coordinates of a point, so the basis is steady in time for the spatio-temporal product):
//   u = β0 + β2·ξ + β3·η,   v = β1 + β4·ξ + β5·η       order 0: q = 2 (β0, β1); order 1: q = 6.
// H (q × n) holds the basis at the observations (zero columns for padded points).  With W = L⁻¹:
//   G = W·Hᵀ, z = W·y, A = GᵀG, β̂ = A⁻¹Gᵀz, α′ = Wᵀ(z − Gβ̂), B0 = WᵀG = K_y⁻¹Hᵀ.
// A target column with cross-covariance k* and basis vector h*:
//   mean = k*ᵀα′ + h*ᵀβ̂,   var = prior − ‖W k*‖² + rᵀA⁻¹r,   r = h* − B0ᵀk*.
// B0ᵀk* has the form of the mean α·k*: the predict's mean pass takes q more right-hand sides and
// reads K*ᵀ once for all of them (mean_part_multi_kernel).
//
// Every vector set here is a table of TREND_RHS = 8 doubles per row (row-major, unused entries 0),
// so a row is one aligned 64-byte piece whose address is wave-uniform where a thread owns a column.
// All reductions have a fixed order; nothing is atomic.  The trend block's layout: predict_host.hpp.
#pragma once
#include "common.hpp"
#include "predict.hpp"

namespace gp2d {

constexpr int TREND_QMAX = 6;   // coefficients of the linear trend
constexpr int TREND_RHS = 8;    // doubles per table row: [y | α′, the q basis columns, 0…]
// trend block (doubles): β̂ | A⁻¹ (row stride TREND_QMAX) | log|A| | status | the right-hand sides
constexpr int TB_BETA = 0, TB_AINV = 8, TB_LOGDET = 44, TB_STATUS = 45, TB_RHS = 48;
// A pivot of A's factor at or below this fraction of its diagonal entry: A is singular to rounding
// (order 1 on collinear points leaves ~1e-16 of it; cond(A) of a valid basis is ~10).
constexpr double TREND_PIVOT_TOL = 1e-10;

struct TrendBasis {
  double c1, c2, is;   // centre and 1 / scale
};

// h* of a predict whose columns are not velocity components: the same for every target (a derived
// field's h_δ or h_ζ; zeros for one term of a sum).  Formed on the host (trend_field_h).
struct TrendH {
  double v[TREND_QMAX];
};

// h (Q entries) of component comp (0: u, 1: v) at basis coordinates (ξ, η)
template <int Q>
__device__ __forceinline__ void trend_basis(int comp, double xi, double eta, double (&h)[Q]) {
  const double u = comp == 0 ? 1.0 : 0.0, v = 1.0 - u;
  h[0] = u;
  h[1] = v;
  if constexpr (Q == TREND_QMAX) {
    h[2] = u * xi; h[3] = u * eta;
    h[4] = v * xi; h[5] = v * eta;
  }
}

// Y[i] = [y_i, H[0..Q)[i], 0…] for the n = 2·npad observation rows (component-major).
template <int Q>
__global__ __launch_bounds__(256) void trend_rhs_kernel(const double* __restrict__ y, const double* __restrict__ xtr,
                                                        int64_t ntr, int64_t npad, int pdim, TrendBasis tb,
                                                        double* __restrict__ Y) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= 2 * npad) return;
  const int comp = i >= npad ? 1 : 0;
  const int64_t p = i - comp * npad;
  double h[Q];
#pragma unroll
  for (int a = 0; a < Q; ++a) h[a] = 0.0;
  if (p < ntr) {
    const double xi = (xtr[p * pdim + pdim - 2] - tb.c1) * tb.is, eta = (xtr[p * pdim + pdim - 1] - tb.c2) * tb.is;
    trend_basis<Q>(comp, xi, eta, h);
  }
  double* row = Y + i * TREND_RHS;
  row[0] = y[i];
#pragma unroll
  for (int a = 0; a < TREND_RHS - 1; ++a) row[1 + a] = a < Q ? h[a < Q ? a : 0] : 0.0;
}

// Z[i][r] = Σ_{k ≤ i} W[i][k]·Y[k][r], r < NR, for lower-triangular W: one wave per row, lanes
// stride the row (trmv_n_lower_kernel's pattern); W is read once for all NR vectors.
template <int NR>
__global__ __launch_bounds__(256) void trmv_n_lower_multi_kernel(const double* __restrict__ W, int64_t n, int64_t ldw,
                                                                 const double* __restrict__ Y, double* __restrict__ Z) {
  const int64_t i = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (i >= n) return;
  const double* w = W + i * ldw;
  double s[NR];
#pragma unroll
  for (int r = 0; r < NR; ++r) s[r] = 0.0;
  for (int64_t k = lane; k <= i; k += 64) {
    const double wk = w[k];
    const double* yk = Y + k * TREND_RHS;
#pragma unroll
    for (int r = 0; r < NR; ++r) s[r] += wk * yk[r];
  }
#pragma unroll
  for (int r = 0; r < NR; ++r)
    for (int o = 32; o > 0; o >>= 1) s[r] += __shfl_xor(s[r], o);
  if (lane == 0) {
    double* row = Z + i * TREND_RHS;
#pragma unroll
    for (int r = 0; r < TREND_RHS; ++r) row[r] = r < NR ? s[r < NR ? r : 0] : 0.0;
  }
}

// A = GᵀG and g = Gᵀz from the table Z = [z | G] (n rows), then A's Cholesky factor, A⁻¹, log|A| and
// β̂ = A⁻¹g into the trend block — one block, fixed order: a thread's rows in order, lanes by the
// xor tree, the four waves in order; the q × q algebra on one thread in LDS.  A pivot at or below
// TREND_PIVOT_TOL of its diagonal entry (or not finite): status = its 1-based order and NaN results.
template <int Q>
__global__ __launch_bounds__(256) void trend_solve_kernel(const double* __restrict__ Z, int64_t n,
                                                          double* __restrict__ block) {
  constexpr int NP = Q * (Q + 1) / 2 + Q;   // A's upper triangle by rows, then g
  __shared__ double red[4][NP];
  __shared__ double A[Q][Q], L[Q][Q], X[Q][Q], g[Q], w[Q];
  const int tid = threadIdx.x;
  double acc[NP];
#pragma unroll
  for (int t = 0; t < NP; ++t) acc[t] = 0.0;
  for (int64_t i = tid; i < n; i += 256) {
    const double* row = Z + i * TREND_RHS;
    double v[Q + 1];
#pragma unroll
    for (int r = 0; r <= Q; ++r) v[r] = row[r];
    int t = 0;
#pragma unroll
    for (int a = 0; a < Q; ++a)
#pragma unroll
      for (int b = a; b < Q; ++b) acc[t++] += v[1 + a] * v[1 + b];
#pragma unroll
    for (int a = 0; a < Q; ++a) acc[t++] += v[1 + a] * v[0];
  }
#pragma unroll
  for (int t = 0; t < NP; ++t) {
    for (int o = 32; o > 0; o >>= 1) acc[t] += __shfl_xor(acc[t], o);
    if ((tid & 63) == 0) red[tid >> 6][t] = acc[t];
  }
  __syncthreads();
  if (tid != 0) return;
  int t = 0;
  for (int a = 0; a < Q; ++a)
    for (int b = a; b < Q; ++b, ++t) A[a][b] = A[b][a] = ((red[0][t] + red[1][t]) + red[2][t]) + red[3][t];
  for (int a = 0; a < Q; ++a, ++t) g[a] = ((red[0][t] + red[1][t]) + red[2][t]) + red[3][t];
  int status = 0;
  double logdet = 0.0;
  for (int j = 0; j < Q && status == 0; ++j) {
    double d = A[j][j];
    for (int k = 0; k < j; ++k) d -= L[j][k] * L[j][k];
    if (!(d > TREND_PIVOT_TOL * A[j][j]) || !__builtin_isfinite(d)) {
      status = j + 1;
      break;
    }
    const double l = sqrt(d);
    L[j][j] = l;
    logdet += 2.0 * log(l);
    for (int i = j + 1; i < Q; ++i) {
      double s = A[i][j];
      for (int k = 0; k < j; ++k) s -= L[i][k] * L[j][k];
      L[i][j] = s / l;
    }
  }
  for (int a = 0; a < TB_RHS; ++a) block[a] = 0.0;
  block[TB_STATUS] = (double)status;
  if (status != 0) {
    const double bad = __builtin_nan("");
    for (int a = 0; a < Q; ++a) {
      block[TB_BETA + a] = bad;
      for (int b = 0; b < Q; ++b) block[TB_AINV + a * TREND_QMAX + b] = bad;
    }
    block[TB_LOGDET] = bad;
    return;
  }
  // X = L⁻¹ (lower), w = X·g, β̂ = Xᵀ·w, A⁻¹ = XᵀX
  for (int j = 0; j < Q; ++j) {
    for (int i = 0; i < j; ++i) X[i][j] = 0.0;
    X[j][j] = 1.0 / L[j][j];
    for (int i = j + 1; i < Q; ++i) {
      double s = 0.0;
      for (int k = j; k < i; ++k) s += L[i][k] * X[k][j];
      X[i][j] = -s / L[i][i];
    }
  }
  for (int i = 0; i < Q; ++i) {
    double s = 0.0;
    for (int k = 0; k <= i; ++k) s += X[i][k] * g[k];
    w[i] = s;
  }
  for (int a = 0; a < Q; ++a) {
    double s = 0.0;
    for (int k = a; k < Q; ++k) s += X[k][a] * w[k];
    block[TB_BETA + a] = s;
    for (int b = a; b < Q; ++b) {
      double c = 0.0;
      for (int k = b; k < Q; ++k) c += X[k][a] * X[k][b];
      block[TB_AINV + a * TREND_QMAX + b] = c;
      block[TB_AINV + b * TREND_QMAX + a] = c;
    }
  }
  block[TB_LOGDET] = logdet;
}

// part[seg][j][r] = Σ_{i in seg, i ≥ j} W[i][j]·V[i][r], r < NR, with V = [z − Gβ̂ | G] formed from
// the table Z = [z | G] and the block's β̂ on the fly (trmv_t_lower_part_kernel's pattern: a thread
// owns a column, segments of 128 rows).  The row loop is the same for every thread — the entries
// above the diagonal are masked, not skipped — so a row's table entry has a wave-uniform address.
template <int NR>
__global__ __launch_bounds__(256) void trmv_t_lower_multi_part_kernel(const double* __restrict__ W, int64_t n,
                                                                      int64_t ldw, const double* __restrict__ Z,
                                                                      const double* __restrict__ block,
                                                                      double* __restrict__ part) {
  const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t seg = blockIdx.y, i0 = seg * NB;
  if (j >= n) return;
  double s[NR];
#pragma unroll
  for (int r = 0; r < NR; ++r) s[r] = 0.0;
  if (i0 + NB > (int64_t)blockIdx.x * 256) {   // the block's first column reaches into the segment
    double beta[NR - 1];
#pragma unroll
    for (int a = 0; a < NR - 1; ++a) beta[a] = block[TB_BETA + a];
#pragma unroll 4
    for (int r = 0; r < NB; ++r) {
      const int64_t i = i0 + r;
      const double* v = Z + i * TREND_RHS;
      const double w = (i >= j) ? W[i * ldw + j] : 0.0;
      double v0 = v[0];
#pragma unroll
      for (int a = 0; a < NR - 1; ++a) {
        v0 -= beta[a] * v[1 + a];
        s[1 + a] += w * v[1 + a];
      }
      s[0] += w * v0;
    }
  }
  double* out = part + (seg * n + j) * TREND_RHS;
#pragma unroll
  for (int r = 0; r < TREND_RHS; ++r) out[r] = r < NR ? s[r < NR ? r : 0] : 0.0;
}

// rhs[j][r] = Σ_seg part[seg][j][r] in segment order (the block's right-hand sides [α′ | B0]);
// alpha[j] = rhs[j][0].  One thread per table entry.
__global__ __launch_bounds__(256) void trend_sum_kernel(const double* __restrict__ part, int64_t nseg, int64_t n,
                                                        double* __restrict__ alpha, double* __restrict__ rhs) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= n * TREND_RHS) return;
  double s = 0.0;
  for (int64_t g = 0; g < nseg; ++g) s += part[g * n * TREND_RHS + t];
  rhs[t] = s;
  if (t % TREND_RHS == 0) alpha[t / TREND_RHS] = s;
}

// pm[r][seg][c] = Σ_{rows in seg} rhs[row][r]·B[row][c], r < NR (B = K*ᵀ of a chunk, n × ncols):
// mean_part_kernel with NR right-hand sides for one read of B.  A thread owns a column; a row's
// right-hand sides are one wave-uniform 64-byte table row.
template <int NR>
__global__ __launch_bounds__(256) void mean_part_multi_kernel(const double* __restrict__ B, int64_t ldb,
                                                              int64_t ncols, const double* __restrict__ rhs,
                                                              int64_t nseg, double* __restrict__ pm) {
  const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t r0 = (int64_t)blockIdx.y * MEAN_SEG;
  if (c >= ncols) return;
  double s[NR];
#pragma unroll
  for (int a = 0; a < NR; ++a) s[a] = 0.0;
#pragma unroll 8
  for (int r = 0; r < MEAN_SEG; ++r) {
    const double b = B[(r0 + r) * ldb + c];
    const double* v = rhs + (r0 + r) * TREND_RHS;
#pragma unroll
    for (int a = 0; a < NR; ++a) s[a] += v[a] * b;
  }
#pragma unroll
  for (int a = 0; a < NR; ++a) pm[((int64_t)a * nseg + blockIdx.y) * ncols + c] = s[a];
}

// predict_finalize_kernel with the trend's terms: the partials summed in segment order; h* is the
// basis at the target's own coordinates for its component (velocity: a column's u or v) or the
// launch's constant hc (a derived field's h_δ = (0,0,1,0,0,1)/s, h_ζ = (0,0,0,−1,1,0)/s; zeros for
// one term of a sum); mean = Σ pm[0] + h*ᵀβ̂, var = prior − Σ v² + rᵀA⁻¹r + add with r = h* − B0ᵀk*,
// clipped if asked.
template <int Q>
__global__ __launch_bounds__(256) void predict_trend_finalize_kernel(
    const double* __restrict__ pm, const double* __restrict__ P, int64_t nseg, int64_t ncols, int64_t cpad,
    int64_t cvalid, int64_t c0, int64_t m, double kss, double add, int clip, int compute_var,
    double* __restrict__ mean, double* __restrict__ var, const double* __restrict__ xg, int pdim, TrendBasis tb,
    int velocity, TrendH hc, const double* __restrict__ block) {
  const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= ncols) return;
  const int64_t comp = c / cpad, loc = c - comp * cpad;
  if (loc >= cvalid) return;
  double s[Q + 1];
#pragma unroll
  for (int a = 0; a <= Q; ++a) {
    double t = 0.0;
#pragma unroll 8
    for (int64_t g = 0; g < nseg; ++g) t += pm[((int64_t)a * nseg + g) * ncols + c];
    s[a] = t;
  }
  double h[Q];
#pragma unroll
  for (int a = 0; a < Q; ++a) h[a] = hc.v[a];
  if (velocity) {
    const double* x = xg + (c0 + loc) * pdim + pdim - 2;
    trend_basis<Q>((int)comp, (x[0] - tb.c1) * tb.is, (x[1] - tb.c2) * tb.is, h);
  }
  double mu = s[0];
#pragma unroll
  for (int a = 0; a < Q; ++a) mu += h[a] * block[TB_BETA + a];
  const int64_t o = comp * m + c0 + loc;
  mean[o] = mu;
  if (compute_var) {
    double q = 0.0;
#pragma unroll 8
    for (int64_t g = 0; g < nseg; ++g) q += P[g * ncols + c];
    double r[Q];
#pragma unroll
    for (int a = 0; a < Q; ++a) r[a] = h[a] - s[1 + a];
    double quad = 0.0;
#pragma unroll
    for (int a = 0; a < Q; ++a) {
      double t = 0.0;
#pragma unroll
      for (int b = 0; b < Q; ++b) t += block[TB_AINV + a * TREND_QMAX + b] * r[b];
      quad += r[a] * t;
    }
    double v = kss - q + quad + add;
    if (clip && v < 0.0) v = 0.0;
    var[o] = v;
  }
}

// REML from gp2d_lml's value with α′: ‖z − Gβ̂‖² = yᵀα′ (Hα′ = 0), so only −½ log|A| + ½ q log 2π is
// left to add.
__global__ void lml_trend_terms_kernel(double* __restrict__ out, const double* __restrict__ block, int q) {
  if (threadIdx.x == 0 && blockIdx.x == 0)
    out[0] = out[0] - 0.5 * block[TB_LOGDET] + 0.5 * (double)q * log(2.0 * M_PI);
}

// C ← C − B0·A⁻¹·B0ᵀ on C's stored lower triangle (row ≥ column): the rank-q update that turns
// K_y⁻¹ into the REML gradient's weight matrix.  A thread per entry; B0 from the block's table.
template <int Q>
__global__ __launch_bounds__(256) void trend_rank_update_kernel(double* __restrict__ C, int64_t n,
                                                                const double* __restrict__ block) {
  const int64_t j = (int64_t)blockIdx.y * 256 + threadIdx.x;
  const int64_t i = blockIdx.x;
  if (j > i || j >= n) return;
  const double* bi = block + TB_RHS + i * TREND_RHS + 1;   // wave-uniform
  const double* bj = block + TB_RHS + j * TREND_RHS + 1;
  double s = 0.0;
#pragma unroll
  for (int a = 0; a < Q; ++a) {
    double t = 0.0;
#pragma unroll
    for (int b = 0; b < Q; ++b) t += block[TB_AINV + a * TREND_QMAX + b] * bj[b];
    s += bi[a] * t;
  }
  C[i * n + j] -= s;
}

}  // namespace gp2d
