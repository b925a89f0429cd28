// postcov.hpp — joint posterior covariance of the velocity at the target points,
//   Σ = K(g, g) − VᵀV,   V = W·K*ᵀ  (n × q),
// in the padded component-major layout of K_y: q = 2·mp, mp = ⌈m/64⌉·64, rows and columns
// [u(g_1..g_m), pad, v(g_1..g_m), pad].
//
// Replaces the reference's full matrix
//   Kss = compute_K(Xs, Ys, …);  Cov = Kss − np.dot(Ks, np.dot(Ki, Ks.T))     GP_laser.py:128-129
// (of which it keeps the diagonal, :130-131), sklearn predict(return_cov=True) and GPy
// predict(full_cov=True).  V is gp2d_predict's own product stored instead of column-squared
// (gemm_f64_kernel<false, EPI_STORE>, a_lower); this header holds the TN product VᵀV with the prior
// regenerated in its epilogue (the workspace layout of gp2d_predict_cov is in predict_host.hpp).
//
// postcov_kernel: one lower 128×128 tile of Σ per 256-thread workgroup (tri_tile, as the c_lower
// SYRK); the product is gemm_f64.hpp's tile_product with both operands K-major: the A fragment
// A[i][k] = V[k][i0+i] and the B fragment B[k][j] = V[k][j0+j] are read from the same kind of LDS
// image (KMajorImage, which carries the bank-conflict argument), and a diagonal tile loads and
// stages one panel for both.  K ascends over all n rows of V in one fixed order, so the result is
// reproducible bit for bit.
//
// Epilogue: element (R, C) of the tile is prior(R, C) − acc, the prior block k(g_i, g_j) from
// vec_block_st (the assembly's device function), + diag_add where R == C; rows and columns of
// padded points are identity.  The value is stored at (R, C) and, from the same register value,
// at (C, R): the 4×4 (lane group, register) blocks of each MFMA tile are transposed in the wave
// (two __shfl_xor steps) so that a lane holds 4 consecutive rows of one column and the mirror is
// one 32-byte store, 128 contiguous bytes per column.  A diagonal tile keeps only its elements
// with C ≤ R and mirrors those with C < R, so no element is written twice.  The q × q prior is
// never stored or read.
#pragma once
#include "assemble.hpp"
#include "factor_host.hpp"
#include "gemm_f64.hpp"
#include "predict.hpp"

namespace gp2d {

struct PostcovParams {
  const double* V; int64_t ldv;   // n × q, row-major
  int n, q;                       // n a multiple of 16, q of 128
  const double* xg;               // m target points (pdim doubles each)
  int m, mp;                      // valid and padded points per component (q = 2·mp)
  VecParams vp;
  double diag_add;
  double* C; int64_t ldc;         // q × q
};

typedef double d4u __attribute__((ext_vector_type(4), aligned(8)));

// the prior's entry for matrix row R and column C (component-major, mp points per component)
__device__ __forceinline__ double postcov_prior(const PostcovParams& p, int R, int C, double diag_add) {
  const int cr = R >= p.mp, cc = C >= p.mp;
  const int i = R - cr * p.mp, j = C - cc * p.mp;
  if (i >= p.m || j >= p.m) return R == C ? 1.0 : 0.0;
  double ta, a1, a2, tb, b1, b2;
  vec_point(p.vp, p.xg, i, ta, a1, a2);
  vec_point(p.vp, p.xg, j, tb, b1, b2);
  double k11, k12, k22;
  vec_block_st(p.vp, ta - tb, a1 - b1, a2 - b2, k11, k12, k22);
  const double k = (cr != cc) ? k12 : (cr ? k22 : k11);
  return R == C ? k + diag_add : k;
}

__global__ __launch_bounds__(256, 2) void postcov_kernel(PostcovParams p) {
  __shared__ double smem[TILE_LDS];

  int bi, bj;
  tri_tile(blockIdx.x, bi, bj);
  const int i0 = bi * GBM, j0 = bj * GBN;
  const bool diag_tile = bi == bj;   // one panel serves both operands

  d4 acc[4][4];
  tile_product<KMajorImage, KMajorImage>(acc, p.V, p.ldv, i0, p.V, p.ldv, j0, 0, p.n, smem, diag_tile);

  const AccMap at(i0, j0);   // acc[mi][ni][r] is element (R, C) = (at.row(mi, r), at.col(ni))
  const int lk = (threadIdx.x & 63) >> 4;
  double* __restrict__ Cm = p.C;
#pragma unroll
  for (int mi = 0; mi < 4; ++mi)
#pragma unroll
    for (int ni = 0; ni < 4; ++ni) {
      const int Cc = at.col(ni);
      double v[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int R = at.row(mi, r);
        v[r] = postcov_prior(p, R, Cc, p.diag_add) - acc[mi][ni][r];
        if (!diag_tile || Cc <= R) Cm[(int64_t)R * p.ldc + Cc] = v[r];
      }
      // transpose the 4×4 (lk, r) block: afterwards v[r] is element (R0 + r, Cc), R0 below
      {
        const bool o = lk & 1;
        const double s0 = __shfl_xor(o ? v[0] : v[1], 16), s1 = __shfl_xor(o ? v[2] : v[3], 16);
        if (o) { v[0] = s0; v[2] = s1; } else { v[1] = s0; v[3] = s1; }
      }
      {
        const bool o = lk & 2;
        const double s0 = __shfl_xor(o ? v[0] : v[2], 32), s1 = __shfl_xor(o ? v[1] : v[3], 32);
        if (o) { v[0] = s0; v[1] = s1; } else { v[2] = s0; v[3] = s1; }
      }
      const int R0 = at.row(mi, 0) + 3 * lk;   // row 16·mi + 4·lk of the wave's sub-tile
      double* mrow = Cm + (int64_t)Cc * p.ldc + R0;   // the mirror: row Cc, columns R0..R0+3
      if (!diag_tile) {
        *reinterpret_cast<d4u*>(mrow) = d4u{v[0], v[1], v[2], v[3]};
      } else {
#pragma unroll
        for (int r = 0; r < 4; ++r)
          if (Cc < R0 + r) mrow[r] = v[r];
      }
    }
}

inline int launch_postcov(const PostcovParams& p, hipStream_t s) {
  if (p.q <= 0) return 0;
  if ((p.q % GBM) || (p.n % GBK) || p.n <= 0 || p.q != 2 * p.mp) {
    set_error("postcov: q must be 2·mp and a multiple of 128, n a positive multiple of 16");
    return -2;
  }
  const int t = p.q / GBM;
  postcov_kernel<<<dim3(t * (t + 1) / 2), 256, 0, s>>>(p);
  return check_launch("postcov_kernel");
}

}  // namespace gp2d
