// assemble.hpp — covariance assembly kernels.
//
// Replaces the reference's kernel builders:
//   GP_scripts.myKernel      GP_scripts.py:6-42   (vectorised mixed df/cf kernel)
//   GP_scripts.nonDivK       GP_scripts.py:57-69  (one 2×2 block, divFree ∈ {0,1,2})
//   GP_scripts.compute_K/_Ks GP_scripts.py:74-123 (component-major 2×2 layout)
//   myKernel.{myKernel,nonDivK,nonRotK}.K   myKernel.py:27-53, 159-176, 255-271
//   sklearn RBF(ARD)+White as built in krig.scikit_prior   krig.py:174-180
//
// Every cross-covariance of the library — these, fields.hpp's and grad.hpp's — is assembled by one
// kernel, cross_cov_kernel<Entry>: a thread evaluates one (row point i, column point j) pair and
// stores the pair's block; a wave covers 64 consecutive column points, so every store of the
// kernels here is a coalesced 512-byte row segment.  Work is exp-bound VALU; HBM traffic is what a
// pair writes (32 B for the 2×2 block).
#pragma once
#include "common.hpp"
#include "../../include/gp2d.h"

#include <type_traits>

namespace gp2d {

inline bool is_vector_family(const gp2d_kernel_t* k) {
  return k->family == GP2D_FAMILY_VECTOR2D || k->family == GP2D_FAMILY_VECTOR_ST;
}

// Prior variance of the spatio-temporal product's temporal factor (Kt.Kdiag, myKernel.py:362-363);
// 1 for the purely spatial families.
inline double temporal_var(const gp2d_kernel_t* k) {
  return (k->family == GP2D_FAMILY_VECTOR_ST) ? k->var[0] : 1.0;
}

struct VecParams {
  int kind;
  int pdim;               // point stride: 2 (x1, x2), or 3 (t, x1, x2) for the spatio-temporal product
  double var_t, ilt2;     // temporal factor var_t·exp(−Δt²·ilt2/2) (pdim = 3)
  double il_df2, il_cf2;  // 1/ℓ²
  double l_df2;           // ℓ² (scalar kind: the σ² factor of GP_scripts.py:68)
  double ratio, cratio;   // ratio, 1 − ratio
  int same_len;           // ℓ_df == ℓ_cf: one exp serves both parts
};

struct ArdParams {
  int dim, nterms;
  double var[2];
  double ils[2][3];  // 1/ls
};

inline VecParams make_vec_params(const gp2d_kernel_t* k) {
  VecParams p;
  p.kind = k->kind;
  p.il_df2 = 1.0 / (k->l_df * k->l_df);
  p.il_cf2 = 1.0 / (k->l_cf * k->l_cf);
  p.l_df2 = k->l_df * k->l_df;
  p.ratio = k->ratio;
  p.cratio = 1.0 - k->ratio;
  p.same_len = (k->l_df == k->l_cf);
  p.pdim = (k->family == GP2D_FAMILY_VECTOR_ST) ? 3 : 2;
  p.var_t = temporal_var(k);
  p.ilt2 = (p.pdim == 3) ? 1.0 / (k->ls[0][0] * k->ls[0][0]) : 0.0;
  return p;
}

inline ArdParams make_ard_params(const gp2d_kernel_t* k) {
  ArdParams p;
  p.dim = k->dim;
  p.nterms = k->nterms;
  for (int t = 0; t < 2; ++t) {
    p.var[t] = k->var[t];
    for (int d = 0; d < 3; ++d) p.ils[t][d] = (k->ls[t][d] != 0.0) ? 1.0 / k->ls[t][d] : 0.0;
  }
  return p;
}

// 2×2 block of the SE vector kernels.
__device__ __forceinline__ void vec_block(const VecParams& p, double d1, double d2,
                                          double& k11, double& k12, double& k22) {
  const double r2 = d1 * d1 + d2 * d2;
  const double p11 = d1 * d1, p12 = d1 * d2, p22 = d2 * d2;
  if (p.kind == GP2D_KIND_SCALAR) {
    const double c = r2 * p.il_df2;
    const double s = p.il_df2 * exp(-0.5 * c) * p.l_df2;  // (1/σ²)·exp(−C/2)·σ²
    k11 = s; k12 = s; k22 = s;
    return;
  }
  double f11 = 0.0, f12 = 0.0, f22 = 0.0;
  double e_df = 0.0;
  if (p.kind == GP2D_KIND_DIVFREE || p.kind == GP2D_KIND_MIXED) {
    const double c = r2 * p.il_df2;
    e_df = exp(-0.5 * c);
    const double e = p.il_df2 * e_df;
    const double aux = 1.0 - c;  // (p−1) − C, p = 2
    f11 = e * (p11 * p.il_df2 + aux);
    f12 = e * (p12 * p.il_df2);
    f22 = e * (p22 * p.il_df2 + aux);
    if (p.kind == GP2D_KIND_DIVFREE) { k11 = f11; k12 = f12; k22 = f22; return; }
  }
  const double ccf = r2 * p.il_cf2;
  const double ecf = (p.kind == GP2D_KIND_MIXED && p.same_len) ? e_df : exp(-0.5 * ccf);
  const double e = p.il_cf2 * ecf;
  const double g11 = e * (1.0 - p11 * p.il_cf2);
  const double g12 = -e * (p12 * p.il_cf2);
  const double g22 = e * (1.0 - p22 * p.il_cf2);
  if (p.kind == GP2D_KIND_CURLFREE) { k11 = g11; k12 = g12; k22 = g22; return; }
  k11 = p.ratio * f11 + p.cratio * g11;
  k12 = p.ratio * f12 + p.cratio * g12;
  k22 = p.ratio * f22 + p.cratio * g22;
}

// Coordinates of vector-family point i: time (0 for the purely spatial family) and (x1, x2).
__device__ __forceinline__ void vec_point(const VecParams& p, const double* __restrict__ x, int64_t i, double& t,
                                          double& a, double& b) {
  if (p.pdim == 3) {
    t = x[3 * i]; a = x[3 * i + 1]; b = x[3 * i + 2];
  } else {
    t = 0.0; a = x[2 * i]; b = x[2 * i + 1];
  }
}

// Temporal factor of the spatio-temporal product (GPy RBF on t, myKernel.py:349-352); 1 otherwise.
__device__ __forceinline__ double time_factor(const VecParams& p, double dt) {
  return (p.pdim == 3) ? p.var_t * exp(-0.5 * dt * dt * p.ilt2) : 1.0;
}

// Full 2×2 block of a vector-family kernel: spatial block × temporal factor.
__device__ __forceinline__ void vec_block_st(const VecParams& p, double dt, double d1, double d2, double& k11,
                                             double& k12, double& k22) {
  vec_block(p, d1, d2, k11, k12, k22);
  if (p.pdim == 3) {
    const double f = time_factor(p, dt);
    k11 *= f; k12 *= f; k22 *= f;
  }
}

__device__ __forceinline__ double ard_value(const ArdParams& p, const double* a, const double* b) {
  double k = 0.0;
  for (int t = 0; t < p.nterms; ++t) {
    double s = 0.0;
    for (int d = 0; d < p.dim; ++d) {
      const double z = (a[d] - b[d]) * p.ils[t][d];
      s += z * z;
    }
    k += p.var[t] * exp(-0.5 * s);
  }
  return k;
}

// ---- The pair-tile kernel and its entries.

// A point of any family: at most 3 coordinates, the unused ones 0.
struct Point3 { double c[3]; };

// Point i of a family's point array — in global memory or in the kernel's staged tile.  A vector
// family's is (t, x1, x2), ARD's its first `dim` coordinates.
__device__ __forceinline__ Point3 read_point(const VecParams& p, const double* __restrict__ x, int64_t i) {
  Point3 a;
  vec_point(p, x, i, a.c[0], a.c[1], a.c[2]);
  return a;
}
__device__ __forceinline__ Point3 read_point(const ArdParams& p, const double* __restrict__ x, int64_t i) {
  Point3 a;
#pragma unroll
  for (int d = 0; d < 3; ++d) a.c[d] = (d < p.dim) ? x[i * p.dim + d] : 0.0;
  return a;
}
__device__ __forceinline__ int point_stride(const VecParams& p) { return p.pdim; }
__device__ __forceinline__ int point_stride(const ArdParams& p) { return p.dim; }

// Block: 64 (column points) × 4 thread rows; each thread does ASM_ROWS / 4 row points so that the
// column point's coordinates are loaded once.
constexpr int ASM_ROWS = 16;
constexpr int ASM_LOWER = 2;   // `symmetric` mode: K_y's lower triangle only (gp2d_assemble)

// out (ROWS·na_pad rows, leading dimension ld) = the cross-covariance of the row points xa with the
// column points j_off + [0, 64·gridDim.x) of xb.  The kernel owns the walk: the workgroup's 64
// column points are staged once through LDS (wave 0 loads the tile with one coalesced 0.5–1.5 KB
// read, every wave reads it back), the row point of a wave is wave-uniform (readfirstlane'd index:
// scalar loads), a pair with a padded point gets the entry's fixed value instead of an evaluation,
// and the pair's ROWS × COLS block goes to rows r·na_pad + i, columns entry.col(j, c, nb_pad).
// An Entry, passed by value, supplies what differs:
//   ROWS, COLS       the block shape of a pair;
//   layout()         the family's point layout (read_point, point_stride);
//   skip(i, jt, na_pad)   true: the row point is skipped whole, before any evaluation;
//   keep(i, j)       once per row point: which of the block's stores are kept
//                    (Keep::at(r, c)).  StoresAll: nothing skipped, every store kept;
//   col(j, c, np)    the column of entry c of column point j;
//   value(a, b, diag, v), padded(diag, v)   the block of a valid pair and of a padded one; diag
//                    is i == j;
//   stage()          optional: called by every thread before the kernel's barrier, for an entry
//                    that keeps data of its own in LDS (SumEntry).
// Launch: grid (column points / 64, ⌈na_pad / ASM_ROWS⌉), 256 threads (launch_cross_cov).
struct KeepAll {
  __device__ __forceinline__ bool at(int, int) const { return true; }
};
struct StoresAll {
  using Keep = KeepAll;
  __device__ __forceinline__ bool skip(int64_t, int64_t, int64_t) const { return false; }
  __device__ __forceinline__ Keep keep(int64_t, int64_t) const { return {}; }
};

// An entry that stages data of its own through LDS has stage(), called by every thread before the
// kernel's barrier (SumEntry).
template <class Entry, class = void>
struct entry_stages : std::false_type {};
template <class Entry>
struct entry_stages<Entry, std::void_t<decltype(&Entry::stage)>> : std::true_type {};

template <class Entry>
__global__ __launch_bounds__(256) void cross_cov_kernel(
    const double* __restrict__ xa, int64_t na, int64_t na_pad,
    const double* __restrict__ xb, int64_t nb, int64_t nb_pad,
    Entry e, double* __restrict__ out, int64_t ld, int64_t j_off) {
  __shared__ double colpts[3 * 64];
  const int pdim = point_stride(e.layout());
  __builtin_assume(j_off >= 0);   // column points count from 0: col()'s j / 16, j % 16 are shifts (grad_col)
  const int64_t jt = j_off + (int64_t)blockIdx.x * 64;   // the tile's first column point
  const int lane = threadIdx.x & 63;
  const int ty = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int64_t j = jt + lane;
  const bool jv = j < nb;
  if (ty == 0) {
    for (int t = lane; t < pdim * 64; t += 64) {   // the tile's points, coalesced
      const int64_t g = jt * pdim + t;
      colpts[t] = (g < nb * pdim) ? xb[g] : 0.0;
    }
  }
  if constexpr (entry_stages<Entry>::value) e.stage();
  __syncthreads();
  const Point3 b = read_point(e.layout(), colpts, lane);
#pragma unroll 1
  for (int q = 0; q < ASM_ROWS / 4; ++q) {
    const int64_t i = (int64_t)blockIdx.y * ASM_ROWS + ty + 4 * q;   // wave-uniform
    if (i >= na_pad) break;
    if (e.skip(i, jt, na_pad)) continue;
    const typename Entry::Keep keep = e.keep(i, j);
    double v[Entry::ROWS][Entry::COLS];
    if (jv && i < na) {
      e.value(read_point(e.layout(), xa, i), b, i == j, v);
    } else {
      e.padded(i == j, v);
    }
#pragma unroll
    for (int c = 0; c < Entry::COLS; ++c) {
#pragma unroll
      for (int r = 0; r < Entry::ROWS; ++r)
        if (keep.at(r, c)) out[(r * na_pad + i) * ld + e.col(j, c, nb_pad)] = v[r][c];
    }
  }
}

// symmetric modes (xa == xb) of the two covariance entries: a valid diagonal pair gets diag_add,
// a padded one the identity.
__device__ __forceinline__ double padded_diag(int symmetric, bool diag) { return (symmetric && diag) ? 1.0 : 0.0; }

// The 2×2 block of a vector family into the four component blocks (component-major).
// symmetric = ASM_LOWER writes only the lower triangle (C ≤ R) of the n × n matrix (n = 2·na_pad)
// — all gp2d_potrf uses (its diagonal kernel loads the 32×32 sub-blocks whole but never uses, nor
// stores, their upper parts; the rest of the upper triangle it zeroes at its end) — i.e. K_uu's
// and K_vv's lower halves and all of K_vu: half the stores, n(n+1)/2 doubles (GP_scripts.py:80-88
// likewise fills one triangle of compute_K and mirrors it).  Row segments wholly above the diagonal
// are skipped per wave (no kernel evaluation either when all four blocks' segments are).
// col_comp (gp2d_assemble_cols): only the columns of component col_comp (0: u, 1: v; −1: both)
// are written — the same per-element arithmetic.
// The instantiation sits at the SGPR limit of eight waves per SIMD (96, handed out in blocks of 16;
// DESIGN.md §3.1), which is why lower mode keeps one flag per row point and not four comparisons.
struct VecEntry {
  static constexpr int ROWS = 2, COLS = 2;
  VecParams p;
  double diag_add;
  int symmetric, col_comp;
  // lower mode has xa == xb, so one padded count np: matrix column c·np + j is kept in matrix row
  // r·np + i iff it is ≤ the row, i.e. r > c (all of K_vu), or r == c and j ≤ i
  struct Keep {
    bool lower, tri;   // tri: j ≤ i
    int comp;
    __device__ __forceinline__ bool at(int r, int c) const {
      return comp != 1 - c && (!lower || (r == c ? tri : r > c));   // comp ∈ {−1, 0, 1}
    }
  };
  __device__ __forceinline__ const VecParams& layout() const { return p; }
  // a row pair whose every segment is above the diagonal is skipped whole
  __device__ __forceinline__ bool skip(int64_t i, int64_t jt, int64_t na_pad) const {
    return symmetric == ASM_LOWER && jt > na_pad + i;
  }
  __device__ __forceinline__ Keep keep(int64_t i, int64_t j) const {
    return {symmetric == ASM_LOWER, j <= i, col_comp};
  }
  __device__ __forceinline__ int64_t col(int64_t j, int c, int64_t nb_pad) const { return c * nb_pad + j; }
  __device__ __forceinline__ void value(const Point3& a, const Point3& b, bool diag, double (&v)[2][2]) const {
    double k11, k12, k22;
    vec_block_st(p, a.c[0] - b.c[0], a.c[1] - b.c[1], a.c[2] - b.c[2], k11, k12, k22);
    if (symmetric && diag) { k11 += diag_add; k22 += diag_add; }
    v[0][0] = k11; v[0][1] = k12; v[1][0] = k12; v[1][1] = k22;
  }
  __device__ __forceinline__ void padded(bool diag, double (&v)[2][2]) const {
    const double dd = padded_diag(symmetric, diag);
    v[0][0] = dd; v[0][1] = 0.0; v[1][0] = 0.0; v[1][1] = dd;
  }
};

// ---- A sum of vector kernels (GP2D_FAMILY_VECTOR_SUM, include/gp2d.h): k[0] the header, k[1..T]
// the terms.
inline bool is_sum_family(const gp2d_kernel_t* k) { return k->family == GP2D_FAMILY_VECTOR_SUM; }
inline const gp2d_kernel_t* sum_term(const gp2d_kernel_t* k, int t) { return k + 1 + t; }
inline double sum_weight(const gp2d_kernel_t* k, int t) { return k->ls[0][t]; }

// The combinator of cross_cov_kernel's entries: Σ_t w_t·(term t's block).  Point layout, column
// map, skipped rows, kept stores and the padded pair's block are term 0's (every term shares them:
// one family, one `symmetric` mode); the terms carry no diag_add of their own, it is added once,
// after the sum, on the block's diagonal.  The first term is formed without an add (w_0·v_0), so a
// one-term sum of weight 1 gives its term's bits.
// The entry is a kernel argument and is addressed by compile-time index only (a run-time index
// would move it to scratch).  Held there whole, three terms need about 160 SGPRs of the 102 a wave
// has (VecEntry alone sits at 96), and the unrolled evaluation spilled 64 of them; so the terms are
// staged once per workgroup through LDS (stage(), which cross_cov_kernel calls before its barrier)
// and value() walks them with a wave-uniform run-time loop over the LDS copies: one term's
// parameters live at a time, one copy of the evaluation's code.
template <class Term>
struct SumEntry {
  static_assert(GP2D_SUM_MAX_TERMS == 3, "stage() names every term");
  static constexpr int ROWS = Term::ROWS, COLS = Term::COLS;
  using Keep = typename Term::Keep;
  struct Staged { Term term; double w; };
  Term term[GP2D_SUM_MAX_TERMS];
  double w[GP2D_SUM_MAX_TERMS];
  int nterms;
  int add_diag;      // a symmetric mode: a valid diagonal pair gets diag_add
  double diag_add;
  __device__ __forceinline__ static Staged* staged() {
    __shared__ Staged s[GP2D_SUM_MAX_TERMS];
    return s;
  }
  __device__ __forceinline__ void stage() const {
    if (threadIdx.x == 0) {
      staged()[0] = {term[0], w[0]};
      staged()[1] = {term[1], w[1]};
      staged()[2] = {term[2], w[2]};
    }
  }
  __device__ __forceinline__ decltype(auto) layout() const { return term[0].layout(); }
  __device__ __forceinline__ bool skip(int64_t i, int64_t jt, int64_t na_pad) const { return term[0].skip(i, jt, na_pad); }
  __device__ __forceinline__ Keep keep(int64_t i, int64_t j) const { return term[0].keep(i, j); }
  __device__ __forceinline__ int64_t col(int64_t j, int c, int64_t nb_pad) const { return term[0].col(j, c, nb_pad); }
  __device__ __forceinline__ void value(const Point3& a, const Point3& b, bool diag, double (&v)[ROWS][COLS]) const {
#pragma unroll 1
    for (int t = 0; t < nterms; ++t) {   // wave-uniform trip count, nterms ≥ 1
      const Staged st = staged()[t];
      double tv[ROWS][COLS];
      st.term.value(a, b, diag, tv);
#pragma unroll
      for (int r = 0; r < ROWS; ++r)
#pragma unroll
        for (int c = 0; c < COLS; ++c) v[r][c] = t ? v[r][c] + st.w * tv[r][c] : st.w * tv[r][c];
    }
    if (add_diag && diag) {
#pragma unroll
      for (int r = 0; r < (ROWS < COLS ? ROWS : COLS); ++r) v[r][r] += diag_add;
    }
  }
  __device__ __forceinline__ void padded(bool diag, double (&v)[ROWS][COLS]) const { term[0].padded(diag, v); }
};

// The sum of 2×2 blocks: VecEntry's modes (symmetric, lower triangle, col_comp) per term, the terms'
// own diag_add 0.  Unused term slots repeat term 0 (never evaluated).
inline SumEntry<VecEntry> make_sum_vec_entry(const gp2d_kernel_t* k, double diag_add, int symmetric, int col_comp) {
  SumEntry<VecEntry> e;
  e.nterms = k->nterms;
  e.add_diag = symmetric != 0;
  e.diag_add = diag_add;
  for (int t = 0; t < GP2D_SUM_MAX_TERMS; ++t) {
    const int s = t < k->nterms ? t : 0;
    e.term[t] = VecEntry{make_vec_params(sum_term(k, s)), 0.0, symmetric, col_comp};
    e.w[t] = sum_weight(k, s);
  }
  return e;
}

// One value per pair: sklearn's sum of ARD RBF terms.
struct ArdEntry : StoresAll {
  static constexpr int ROWS = 1, COLS = 1;
  ArdParams p;
  double diag_add;
  int symmetric;
  __device__ __forceinline__ const ArdParams& layout() const { return p; }
  __device__ __forceinline__ int64_t col(int64_t j, int, int64_t) const { return j; }
  __device__ __forceinline__ void value(const Point3& a, const Point3& b, bool diag, double (&v)[1][1]) const {
    // plain arrays: indexed by ard_value's run-time loops, they stay in registers (the Point3s did not)
    const double pa[3] = {a.c[0], a.c[1], a.c[2]}, pb[3] = {b.c[0], b.c[1], b.c[2]};
    double k = ard_value(p, pa, pb);
    if (symmetric && diag) k += diag_add;
    v[0][0] = k;
  }
  __device__ __forceinline__ void padded(bool diag, double (&v)[1][1]) const { v[0][0] = padded_diag(symmetric, diag); }
};

}  // namespace gp2d
