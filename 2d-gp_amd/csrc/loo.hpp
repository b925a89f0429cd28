// loo.hpp — the leave-one-out log predictive density of a fit and its exact hyperparameter
// gradient (gp2d_loo_grad; Rasmussen & Williams §5.4.2).
//
// Replaces nothing in the reference, which scores held-out fixes by refitting (krig.py:578-646) and
// tunes by the marginal likelihood alone; this is the objective that connects the two.
//
// With P = K_y⁻¹ = WᵀW, α = P·y and P_ii the bd × bd diagonal block of point i (components
// {c·np + i}):
//   Σ_i = P_ii⁻¹,  r_i = Σ_i·α_i,  lpd_i = −½ α_iᵀr_i + ½ log det P_ii − (bd/2) log 2π,  L = Σ_i lpd_i
//   ∂L/∂θ = ½ tr((α sᵀ + s αᵀ − P·D·P) ∂K_y/∂θ),   s = P·r,   D = blockdiag(r_i r_iᵀ + Σ_i).
// Every D_i is positive definite, D_i = C_i·C_iᵀ (closed-form Cholesky), so P·D·P = B·Bᵀ with
// B = P·C: a symmetric product whose lower tiles are what the pair loop (lml.hpp) reads, through
// the LooWeights policy below.
//
// Stages (gp2d.hip, loo_grad_impl): P on the FP64 GEMM | loo_point_kernel | s by the triangular
// products of gp2d_potrs_inv | loo_scale_kernel | M = B·Bᵀ on the FP64 GEMM | pair_grad_kernel.
// No atomics; every sum has a fixed order.  Workspace layout: lml_host.hpp (LooGradWork).
#pragma once
#include "lml.hpp"

namespace gp2d {

constexpr int LOO_POINT_THREADS = 1024;

// The point pass, one block: thread t takes points t, t + 1024, … in ascending order, then the
// block adds the threads' sums in a fixed tree.  P: n × n, lower triangle stored (row ≥ column).
// Writes r (n entries, component-major), the Cholesky entries of D_i (np entries each; bd = 1:
// c11 = √D_i, c21 = c22 = 0), value[0] = Σ lpd and info[0] = 0, or 1 + the first point whose P_ii
// or D_i is not positive definite (that point gets r = 0, C = 0 and adds nothing; value is NaN).
// Padded points (i ≥ ntr) are never read: r = 0, C = 0.
__global__ __launch_bounds__(LOO_POINT_THREADS) void loo_point_kernel(
    const double* __restrict__ P, int64_t n, int64_t np, int64_t ntr, int bd, const double* __restrict__ alpha,
    double* __restrict__ r, double* __restrict__ c11, double* __restrict__ c21, double* __restrict__ c22,
    double* __restrict__ value, int* __restrict__ info) {
  __shared__ double red[LOO_POINT_THREADS];
  __shared__ int64_t bad[LOO_POINT_THREADS];
  const int tid = threadIdx.x;
  double sum = 0.0;
  int64_t first_bad = INT64_MAX;
  for (int64_t i = tid; i < np; i += LOO_POINT_THREADS) {
    double ru = 0.0, rv = 0.0, a = 0.0, b = 0.0, c = 0.0;
    if (i < ntr) {
      bool ok;
      double lpd = 0.0;
      const double puu = P[i * n + i], au = alpha[i];
      if (bd == 2) {
        const double pvu = P[(np + i) * n + i], pvv = P[(np + i) * n + np + i], av = alpha[np + i];
        const double det = puu * pvv - pvu * pvu;
        ok = puu > 0.0 && det > 0.0;
        if (ok) {
          const double idet = 1.0 / det;
          const double suu = pvv * idet, suv = -pvu * idet, svv = puu * idet;   // Σ_i
          ru = suu * au + suv * av;
          rv = suv * au + svv * av;
          lpd = -0.5 * (au * ru + av * rv) + 0.5 * log(det) - log(2.0 * M_PI);
          const double duu = ru * ru + suu, duv = ru * rv + suv, dvv = rv * rv + svv;
          ok = duu > 0.0;
          if (ok) {
            a = sqrt(duu);
            b = duv / a;
            const double schur = dvv - b * b;
            ok = schur > 0.0;
            if (ok) c = sqrt(schur);
          }
        }
      } else {
        ok = puu > 0.0;
        if (ok) {
          const double sig = 1.0 / puu;
          ru = sig * au;
          lpd = -0.5 * au * ru + 0.5 * log(puu) - 0.5 * log(2.0 * M_PI);
          const double d = ru * ru + sig;
          ok = d > 0.0;
          if (ok) a = sqrt(d);
        }
      }
      if (ok) {
        sum += lpd;
      } else {
        ru = rv = a = b = c = 0.0;
        if (first_bad == INT64_MAX) first_bad = i;
      }
    }
    r[i] = ru;
    if (bd == 2) r[np + i] = rv;
    c11[i] = a;
    c21[i] = b;
    c22[i] = c;
  }
  red[tid] = sum;
  bad[tid] = first_bad;
  __syncthreads();
  for (int s = LOO_POINT_THREADS / 2; s > 0; s >>= 1) {
    if (tid < s) {
      red[tid] += red[tid + s];
      bad[tid] = min(bad[tid], bad[tid + s]);
    }
    __syncthreads();
  }
  if (tid == 0) {
    const bool fail = bad[0] != INT64_MAX;
    value[0] = fail ? __builtin_nan("") : red[0];
    info[0] = fail ? (int)min(bad[0] + 1, (int64_t)INT32_MAX) : 0;
  }
}

// One 64 × 64 tile of the symmetric P, rows 64·ra.., columns 64·rc.., staged in LDS from the
// stored triangle: a tile below the diagonal as it is, a tile above it as its mirror image (the
// global reads run along the stored tile's rows either way), a diagonal tile's stored half only.
// at(r, c) then reads the LDS tile or its transpose.  Launch: 256 threads, tx = column, ty = row
// phase; the tile's pitch of 65 doubles keeps both read directions off a common bank.
struct LooTile {
  bool above, diag;
  __device__ __forceinline__ void load(double (*t)[65], const double* __restrict__ P, int64_t n, int64_t ra,
                                       int64_t rc, int tx, int ty) {
    above = ra < rc;
    diag = ra == rc;
    const int64_t r0 = 64 * (above ? rc : ra), c0 = 64 * (above ? ra : rc);   // the stored tile
#pragma unroll 4
    for (int r = ty; r < 64; r += 4)
      if (!diag || r >= tx) t[r][tx] = P[(r0 + r) * n + c0 + tx];
  }
  __device__ __forceinline__ double at(const double (*t)[65], int r, int c) const {
    return (above || (diag && r < c)) ? t[c][r] : t[r][c];
  }
};

// The scale pass: the full n × n matrix B = P·C from P's stored lower triangle,
//   B[a, j] = P[a, j]·c11_j + P[a, np + j]·c21_j,   B[a, np + j] = P[a, np + j]·c22_j   (BD = 2)
//   B[a, j] = P[a, j]·c11_j                                                              (BD = 1).
// Grid (np / 64 point tiles, n / 64 row tiles) of 256 threads; a thread owns column tx of 16 rows.
// BD = 2 stages the v-column tile first and keeps its 16 values in registers while the u-column
// tile takes the LDS tile's place.  Global reads and writes are 512-byte runs.
template <int BD>
__global__ __launch_bounds__(256) void loo_scale_kernel(const double* __restrict__ P, int64_t n, int64_t np,
                                                        const double* __restrict__ c11,
                                                        const double* __restrict__ c21,
                                                        const double* __restrict__ c22, double* __restrict__ B) {
  __shared__ double t[64][65];
  const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
  const int64_t tj = blockIdx.x, ta = blockIdx.y;
  const int64_t j = 64 * tj + tx, a0 = 64 * ta;
  LooTile tile;
  double pv[16];
  if (BD == 2) {
    tile.load(t, P, n, ta, np / 64 + tj, tx, ty);
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 16; ++i) pv[i] = tile.at(t, ty + 4 * i, tx);
    __syncthreads();
  }
  tile.load(t, P, n, ta, tj, tx, ty);
  __syncthreads();
  const double a = c11[j];
  if (BD == 2) {
    const double b = c21[j], c = c22[j];
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int r = ty + 4 * i;
      double* row = B + (a0 + r) * n;
      row[j] = tile.at(t, r, tx) * a + pv[i] * b;
      row[np + j] = pv[i] * c;
    }
  } else {
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int r = ty + 4 * i;
      B[(a0 + r) * n + j] = tile.at(t, r, tx) * a;
    }
  }
}

// The LOO gradient's weights for pair_grad_kernel: the stored (row ≥ column) entries of
// α sᵀ + s αᵀ − M, M = B·Bᵀ (n × n, lower triangle), np the component stride of α, s and M.
// TraceWeights' triangle conventions: the vu entry (np + p, q) for every pair at weight 2; uu and
// vv for p ≥ q, weight 2 off the diagonal and 1 on it; the diagonal also feeds the noise slot.
struct LooWeights {
  const double* M;
  int64_t n;
  const double* alpha;
  const double* s;
  int64_t np;
  struct VecCol { double au, av, su, sv; };
  struct ArdCol { double a, s; };
  __device__ __forceinline__ VecCol column(const VecFamily&, int64_t q) const {
    return {alpha[q], alpha[np + q], s[q], s[np + q]};
  }
  __device__ __forceinline__ VecCol column(const SumVecFamily&, int64_t q) const {
    return {alpha[q], alpha[np + q], s[q], s[np + q]};
  }
  __device__ __forceinline__ ArdCol column(const ArdFamily&, int64_t q) const { return {alpha[q], s[q]}; }
  __device__ __forceinline__ bool pair(const VecFamily&, int64_t p, int64_t q, const VecCol& cq, VecWeight& w,
                                       double* acc) const {
    return vec_pair(p, q, cq, w, acc);
  }
  __device__ __forceinline__ bool pair(const SumVecFamily&, int64_t p, int64_t q, const VecCol& cq, VecWeight& w,
                                       double* acc) const {
    return vec_pair(p, q, cq, w, acc);
  }
  __device__ __forceinline__ bool vec_pair(int64_t p, int64_t q, const VecCol& cq, VecWeight& w, double* acc) const {
    const double apu = alpha[p], apv = alpha[np + p], spu = s[p], spv = s[np + p];
    const double* mu = M + p * n;          // row p (u)
    const double* mv = M + (np + p) * n;   // row np+p (v)
    const double mvu = apv * cq.su + spv * cq.au - mv[q];
    w.w11 = w.w22 = 0.0;
    if (p >= q) {
      const double wt = (p == q) ? 1.0 : 2.0;
      w.w11 = wt * (apu * cq.su + spu * cq.au - mu[q]);
      w.w22 = wt * (apv * cq.sv + spv * cq.av - mv[np + q]);
      if (p == q) acc[VecFamily::NOISE] += w.w11 + w.w22;
    }
    w.w12 = 2.0 * mvu;
    return true;
  }
  __device__ __forceinline__ bool pair(const ArdFamily&, int64_t p, int64_t q, const ArdCol& cq, double& w,
                                       double* acc) const {
    if (p < q) return false;
    w = ((p == q) ? 1.0 : 2.0) * (alpha[p] * cq.s + s[p] * cq.a - M[p * n + q]);
    if (p == q) acc[ArdFamily::NOISE] += w;
    return true;
  }
};

}  // namespace gp2d
