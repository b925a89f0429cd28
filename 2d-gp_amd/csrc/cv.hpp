// cv.hpp — cross-validation of a fit without refitting.
//
// With P = K_y⁻¹ = WᵀW and α = P·y, the predictive distribution of the observations y_G of any
// index set G given all the others is Gaussian with covariance P_GG⁻¹ and mean y_G − P_GG⁻¹·α_G
// (Rasmussen & Williams §5.4.2, block form).  Everything below reads only (W, α, y): it serves
// every kernel family and both variance engines.  Replaces the train / test refits of the
// reference (krig.py:578-646 predictTest / getRMSE / rmse; laser_compare_interp.py's held-out
// drifters).
//
// Layout: bd = 1 or 2 components per point, n = bd·npad, component c of point i is column
// c·npad + i of W (lower triangular: column j is zero above row j).
//
// Leave one point out (its u and v together): P_ii is the 2 × 2 Gram of columns i and npad + i —
// one pass over W's lower triangle (cv_point_partial_kernel) and one workgroup that sums the
// partials in segment order, inverts the blocks in closed form and reduces the scores
// (cv_point_finish_kernel).
// Leave a group out: the group's columns are gathered and transposed into a q_pad × n row-major
// panel (cv_gather_t_kernel), gemm_f64_kernel forms the lower tiles of panel·panelᵀ on the FP64
// matrix cores (one batch entry per group), cv_gram_finish_kernel mirrors them into an exactly
// symmetric block with identity padding, the batched factor inverts its Cholesky factor, and
// cv_group_solve_kernel reads the group's results off W_p = L_p⁻¹.
// No atomics anywhere; every sum has a fixed order.
#pragma once
#include "common.hpp"
#include "factor_host.hpp"

namespace gp2d {

constexpr int CV_RSEG = 256;                     // rows per partial sum of the point pass
constexpr int CV_MAX_Q = 1024;                   // GP2D_CV_MAX_Q: components per held-out group
constexpr int CV_MAX_BATCH = 64;                 // groups per batched factor (gp2d_potrf_batched's limit)
constexpr double CV_LOG_2PI = 1.8378770664093454835606594728112;

// ------------------------------------------------------------------ leave one point out
// Pass 1: thread = point i of a 256-point block, blockIdx.y = 256-row segment; consecutive
// threads read consecutive columns, so the u and the v loads are both coalesced.  part[seg][0..3)
// [npad] = Σ_r W[r,i]², Σ_r W[r,npad+i]², Σ_r W[r,i]·W[r,npad+i] over the segment's rows.  A segment
// that ends above the block's first u column holds zeros only and is skipped; one that ends above
// its first v column has no v terms (column npad + i is zero above row npad + i).
__global__ __launch_bounds__(256) void cv_point_partial_kernel(const double* __restrict__ W, int64_t ldw, int64_t n,
                                                               int64_t npad, int bd, double* __restrict__ part) {
  const int64_t c0 = (int64_t)blockIdx.x * 256, i = c0 + threadIdx.x, seg = blockIdx.y;
  if (i >= npad) return;
  const int64_t r0 = seg * CV_RSEG, r1 = min<int64_t>(n, r0 + CV_RSEG);
  double uu = 0.0, vv = 0.0, uv = 0.0;
  if (bd == 2 && r1 > npad + c0) {
    const double* __restrict__ wu = W + i;
    const double* __restrict__ wv = W + npad + i;
#pragma unroll 8
    for (int64_t r = r0; r < r1; ++r) {
      const double a = wu[r * ldw], b = wv[r * ldw];
      uu = fma(a, a, uu);
      vv = fma(b, b, vv);
      uv = fma(a, b, uv);
    }
  } else if (r1 > c0) {
#pragma unroll 8
    for (int64_t r = r0; r < r1; ++r) {
      const double a = W[r * ldw + i];
      uu = fma(a, a, uu);
    }
  }
  double* __restrict__ p = part + seg * 3 * npad;
  p[i] = uu;
  p[npad + i] = vv;
  p[2 * npad + i] = uv;
}

// Sum of (s[0..4)) over the 1024 threads of a workgroup in a fixed order: lanes by xor shuffles,
// then the 16 waves in wave order by thread 0.
__device__ __forceinline__ void cv_block_sum4(double (&s)[4], double (*red)[16]) {
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    for (int o = 32; o > 0; o >>= 1) s[k] += __shfl_xor(s[k], o);
    if (lane == 0) red[k][w] = s[k];
  }
  __syncthreads();
  if (tid == 0) {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      double t = red[k][0];
      for (int q = 1; q < 16; ++q) t += red[k][q];
      s[k] = t;
    }
  }
}

// Pass 2 (one workgroup): per training point P_ii from the partials in segment order, S = P_ii⁻¹,
// r = S·α_i, mean y_i − r, variances and covariance of S, lpd_i = −½ α_iᵀr + ½ log det P_ii −
// (bd/2) log 2π, scattered to position out_order[i]; summary = (Σ lpd, Σ r_u², Σ r_v², Σ rᵀP_ii r)
// (rᵀP_ii r = α_iᵀr).  Padded points (i ≥ ntr) are never read.
__global__ __launch_bounds__(1024) void cv_point_finish_kernel(const double* __restrict__ part, int64_t nseg,
                                                               int64_t npad, int64_t ntr, int bd,
                                                               const double* __restrict__ alpha,
                                                               const double* __restrict__ y,
                                                               const int64_t* __restrict__ out_order,
                                                               double* __restrict__ mean, double* __restrict__ var,
                                                               double* __restrict__ cuv, double* __restrict__ lpd,
                                                               double* __restrict__ summary) {
  __shared__ double red[4][16];
  double s[4] = {0.0, 0.0, 0.0, 0.0};
  for (int64_t i = threadIdx.x; i < ntr; i += 1024) {
    double uu = 0.0, vv = 0.0, uv = 0.0;
    for (int64_t g = 0; g < nseg; ++g) {
      const double* __restrict__ p = part + g * 3 * npad;
      uu += p[i];
      if (bd == 2) {
        vv += p[npad + i];
        uv += p[2 * npad + i];
      }
    }
    const int64_t o = out_order ? out_order[i] : i;
    const bool put = o >= 0 && o < ntr;   // a bad order entry writes nothing
    const double au = alpha[i];
    double l, ru, rv = 0.0, chi;
    if (bd == 2) {
      const double av = alpha[npad + i];
      const double det = fma(uu, vv, -uv * uv);
      const double suu = vv / det, svv = uu / det, suv = -uv / det;
      ru = fma(suu, au, suv * av);
      rv = fma(suv, au, svv * av);
      chi = fma(au, ru, av * rv);
      l = -0.5 * chi + 0.5 * log(det) - CV_LOG_2PI;
      if (put) {
        mean[o] = y[i] - ru;
        mean[ntr + o] = y[npad + i] - rv;
        var[o] = suu;
        var[ntr + o] = svv;
        if (cuv) cuv[o] = suv;
      }
    } else {
      const double suu = 1.0 / uu;
      ru = suu * au;
      chi = au * ru;
      l = -0.5 * chi + 0.5 * log(uu) - 0.5 * CV_LOG_2PI;
      if (put) {
        mean[o] = y[i] - ru;
        var[o] = suu;
      }
    }
    if (put) lpd[o] = l;
    s[0] += l;
    s[1] = fma(ru, ru, s[1]);
    s[2] = fma(rv, rv, s[2]);
    s[3] += chi;
  }
  cv_block_sum4(s, red);
  if (threadIdx.x == 0)
    for (int k = 0; k < 4; ++k) summary[k] = s[k];
}

// ------------------------------------------------------------------ leave a group out
// One batch of groups for a launch: group b's points are gidx[start[b] .. start[b+1]).
struct CvBatch { int64_t start[CV_MAX_BATCH + 1]; };

// Column of W behind component a of a group of cnt points (a = c·cnt + j: component-major inside
// the group), −1 for a padded component or an index outside [0, ntr).
__device__ __forceinline__ int64_t cv_group_col(const int64_t* __restrict__ gidx, int64_t s0, int64_t cnt, int bd,
                                                int64_t npad, int64_t ntr, int a) {
  if (a >= bd * cnt) return -1;
  const int64_t c = a / cnt, j = a - c * cnt;
  const int64_t i = gidx[s0 + j];
  return (i >= 0 && i < ntr) ? c * npad + i : -1;
}

// Gather-transpose: panel[b][a][r] = W[r, col(a)] for r ≥ col(a), 0 above the column's diagonal and
// in the padded rows a ≥ q_b (q_pad × n row-major per group).  64 × 64 tiles through LDS: the
// loads run along the gathered columns, the stores along r.  Grid (n/64, q_pad/64, groups).
__global__ __launch_bounds__(256) void cv_gather_t_kernel(const double* __restrict__ W, int64_t ldw, int64_t n,
                                                          int64_t npad, int64_t ntr, int bd,
                                                          const int64_t* __restrict__ gidx, CvBatch bt, int qpad,
                                                          double* __restrict__ panel) {
  __shared__ double tile[64][65];
  const int b = blockIdx.z, a0 = blockIdx.y * 64;
  const int64_t r0 = (int64_t)blockIdx.x * 64;
  const int64_t s0 = bt.start[b], cnt = bt.start[b + 1] - s0;
  const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
  const int64_t col = cv_group_col(gidx, s0, cnt, bd, npad, ntr, a0 + tx);
  for (int rr = ty; rr < 64; rr += 4) {
    const int64_t r = r0 + rr;
    tile[rr][tx] = (col >= 0 && r >= col) ? W[r * ldw + col] : 0.0;
  }
  __syncthreads();
  double* __restrict__ out = panel + (int64_t)b * qpad * n;
  for (int aa = ty; aa < 64; aa += 4) out[(int64_t)(a0 + aa) * n + r0 + tx] = tile[tx][aa];
}

// The GEMM wrote the lower tiles of panel·panelᵀ into gram[b] (diagonal tiles: their lower
// triangle).  Each pair (a, b), (b, a) is stored from the one value of the lower triangle, into
// gram (kept for inspection) and into the factor's input; rows and columns a ≥ q are identity.
// Grid (q_pad/16, q_pad/16, groups) of 16 × 16 threads; blocks above the diagonal do nothing.
__global__ __launch_bounds__(256) void cv_gram_finish_kernel(double* __restrict__ gram, double* __restrict__ fac,
                                                             CvBatch bt, int bd, int qpad) {
  if (blockIdx.x > blockIdx.y) return;
  const int g = blockIdx.z;
  const int q = (int)(bd * (bt.start[g + 1] - bt.start[g]));
  const int a = blockIdx.y * 16 + (threadIdx.x >> 4), b = blockIdx.x * 16 + (threadIdx.x & 15);
  if (b > a) return;
  double* __restrict__ G = gram + (int64_t)g * qpad * qpad;
  double* __restrict__ F = fac + (int64_t)g * qpad * qpad;
  const double v = (a < q) ? G[(int64_t)a * qpad + b] : (a == b ? 1.0 : 0.0);   // b ≤ a < q
  G[(int64_t)a * qpad + b] = v;
  G[(int64_t)b * qpad + a] = v;
  F[(int64_t)a * qpad + b] = v;
  F[(int64_t)b * qpad + a] = v;
}

__global__ __launch_bounds__(256) void cv_fill_kernel(double* __restrict__ x, int64_t count, double v) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < count) x[i] = v;
}

// One workgroup per group, from W_p = L_p⁻¹ (lower, q_pad × q_pad, the group's q × q block first):
//   t = W_p·α_G  (one wave per row, lanes over the columns, xor-shuffle sum),
//   r = W_pᵀ·t, var_b = Σ_{a ≥ b} W_p[a,b]²  (one thread per column, rows in order: coalesced),
//   lpd = −½ α_Gᵀ r − Σ_a log W_p[a,a] − (q/2) log 2π  (sums in component order by thread 0).
// mean = y_G − r and var are scattered to out_order[i] of each point i of the group.
__global__ __launch_bounds__(256) void cv_group_solve_kernel(const double* __restrict__ fac, CvBatch bt, int bd,
                                                             int qpad, int64_t npad, int64_t ntr,
                                                             const int64_t* __restrict__ gidx,
                                                             const double* __restrict__ alpha,
                                                             const double* __restrict__ y,
                                                             const int64_t* __restrict__ out_order,
                                                             double* __restrict__ mean, double* __restrict__ var,
                                                             double* __restrict__ lpd_group) {
  __shared__ double sa[CV_MAX_Q], st[CV_MAX_Q], sr[CV_MAX_Q];
  const int g = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int64_t s0 = bt.start[g], cnt = bt.start[g + 1] - s0;
  const int q = (int)(bd * cnt);
  const double* __restrict__ Wp = fac + (int64_t)g * qpad * qpad;
  for (int a = tid; a < q; a += 256) {
    const int64_t col = cv_group_col(gidx, s0, cnt, bd, npad, ntr, a);
    sa[a] = col >= 0 ? alpha[col] : 0.0;
  }
  __syncthreads();
  for (int a = wv; a < q; a += 4) {
    double t = 0.0;
    for (int b = lane; b <= a; b += 64) t = fma(Wp[(int64_t)a * qpad + b], sa[b], t);
    for (int o = 32; o > 0; o >>= 1) t += __shfl_xor(t, o);
    if (lane == 0) st[a] = t;
  }
  __syncthreads();
  for (int b = tid; b < q; b += 256) {
    double r = 0.0, v = 0.0;
    for (int a = b; a < q; ++a) {
      const double w = Wp[(int64_t)a * qpad + b];
      r = fma(w, st[a], r);
      v = fma(w, w, v);
    }
    sr[b] = r;
    const int64_t c = b / cnt, j = b - c * cnt;
    const int64_t i = gidx[s0 + j];
    if (i >= 0 && i < ntr) {
      const int64_t o = out_order ? out_order[i] : i;
      if (o >= 0 && o < ntr) {
        mean[c * ntr + o] = y[c * npad + i] - r;
        var[c * ntr + o] = v;
      }
    }
  }
  __syncthreads();
  if (tid == 0) {
    double quad = 0.0, ld = 0.0;
    for (int a = 0; a < q; ++a) {
      quad = fma(sa[a], sr[a], quad);
      ld += log(Wp[(int64_t)a * qpad + a]);
    }
    lpd_group[g] = -0.5 * quad - ld - 0.5 * q * CV_LOG_2PI;
  }
}

// ------------------------------------------------------------------ workspaces
// gp2d_cv_points: the partial sums [segments][3][n] (npad ≤ n).
inline size_t cv_points_bytes(int64_t n) {
  return n > 0 ? F64 * 3 * (size_t)((n + CV_RSEG - 1) / CV_RSEG) * (size_t)n : 0;
}

// gp2d_cv_groups with nb groups per batch: the Gram blocks (first, so that a caller can read the
// last batch's back) | the factor's blocks | their inverted diagonal blocks | the batched TRTRI's
// buffers | the gathered panels (nb × q_pad × n).
struct CvGroupWork {
  size_t gram = 0, fac = 0, dinv = 0, trtri = 0, panel = 0, total = 0;
  CvGroupWork(int64_t n, int64_t qpad, int nb) {
    const size_t blk = F64 * (size_t)qpad * (size_t)qpad * (size_t)nb;
    fac = blk;
    dinv = fac + blk;
    trtri = dinv + F64 * (size_t)nb * (size_t)qpad * NB;
    panel = trtri + TrtriWork(qpad, nb, false).total;
    total = panel + F64 * (size_t)nb * (size_t)qpad * (size_t)n;
  }
};
// Groups per batch that gp2d_cv_groups_workspace sizes for: up to 64, fewer while the panels
// would pass 1 GiB.
inline int cv_groups_batch(int64_t n, int64_t qpad, int ngroups) {
  const int64_t fit = ((int64_t)1 << 30) / ((int64_t)F64 * qpad * n);
  return (int)std::max<int64_t>(1, std::min<int64_t>({(int64_t)CV_MAX_BATCH, (int64_t)ngroups, fit}));
}

}  // namespace gp2d
