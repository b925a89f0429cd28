// lml_host.hpp — the workspace layouts of the hyperparameter path (gp2d_lml_grad,
// gp2d_kernel_grad) and of gp2d_potrs_inv, as byte-offset tables.  gp2d.hip takes every size it
// reports for them and every pointer it carves from here; the kernels get plain pointers.
#pragma once
#include "factor_host.hpp"
#include "lml.hpp"

namespace gp2d {

// Blocks of pair_grad_kernel's grid = rows of LML_MAXG partial sums that grad_sum_kernel adds:
// column tiles of PT_TILE points (the padded column count) × row blocks of LML_ROWS points.
constexpr int64_t grad_blocks(int64_t ncols_pad, int64_t nrows) {
  return (ncols_pad / PT_TILE) * ((nrows + LML_ROWS - 1) / LML_ROWS);
}
constexpr size_t grad_partial_bytes(int64_t nblk) { return F64 * (size_t)nblk * LML_MAXG; }

// Workspace of gp2d_lml_grad: C = K_y⁻¹ (n × n) | the partial sums.  The size is a
// function of n = bd·ntr_pad alone, so the partials are sized for one column tile and one row
// point more than n × n points, which holds the launch's grad_blocks(ntr_pad, ntr) for either bd.
struct LmlGradWork {
  size_t C = 0, partial = 0, total = 0;
  constexpr explicit LmlGradWork(int64_t n) {
    partial = F64 * (size_t)n * (size_t)n;
    total = partial + grad_partial_bytes(grad_blocks(n + PT_TILE, n + 1));
  }
  struct Ptrs { double* C; double* partial; };
  Ptrs at(void* w) const { return {work_at(w, C), work_at(w, partial)}; }
};
constexpr bool lml_grad_work_ok(int64_t n) {
  const LmlGradWork w(n);
  const size_t nn = F64 * (size_t)n * (size_t)n;
  bool ok = regions_ok({w.C, w.partial, w.total}, {nn, grad_partial_bytes((n / 64 + 1) * (n / 16 + 1))});
  for (int bd = 1; bd <= 2; ++bd)   // the fullest launch: ntr = ntr_pad = n / bd
    ok = ok && w.partial + grad_partial_bytes(grad_blocks(n / bd, n / bd)) <= w.total;
  return ok;
}
static_assert(lml_grad_work_ok(128) && lml_grad_work_ok(256) && lml_grad_work_ok(8192) && lml_grad_work_ok(32768),
              "lml_grad workspace: regions out of order, overlapping, misaligned or too few partials");

// Workspace of gp2d_kernel_grad: the partial sums of its launch, nb columns padded to whole tiles
// × na rows.  An empty point set sizes as one point.
struct KernelGradWork {
  size_t partial = 0, total = 0;
  constexpr KernelGradWork(int64_t na, int64_t nb) {
    total = grad_partial_bytes(grad_blocks(round_up(nb < 1 ? 1 : nb, PT_TILE), na < 1 ? 1 : na));
  }
  struct Ptrs { double* partial; };
  Ptrs at(void* w) const { return {work_at(w, partial)}; }
};
static_assert(KernelGradWork(0, 0).total == 72 && KernelGradWork(16, 64).total == 72 &&
                  KernelGradWork(17, 65).total == 4 * 72 && KernelGradWork(4096, 4096).total == 64 * 256 * 72,
              "kernel_grad workspace: one row of partials per block of the launch");

// Workspace of gp2d_potrs_inv: z = W·y (n) | the n / 128 row segments' partial sums of Wᵀ·z
// (n each), sized for one segment more.
struct PotrsWork {
  size_t z = 0, part = 0, total = 0;
  constexpr explicit PotrsWork(int64_t n) {
    part = F64 * (size_t)n;
    total = part + F64 * (size_t)(n / NB + 1) * (size_t)n;
  }
  struct Ptrs { double* z; double* part; };
  Ptrs at(void* w) const { return {work_at(w, z), work_at(w, part)}; }
};
constexpr bool potrs_work_ok(int64_t n) {
  const PotrsWork w(n);
  return regions_ok({w.z, w.part, w.total}, {F64 * (size_t)n, F64 * (size_t)(n / NB + 1) * (size_t)n});
}
static_assert(potrs_work_ok(128) && potrs_work_ok(256) && potrs_work_ok(8192) && PotrsWork(0).total == 0,
              "potrs workspace: regions out of order, overlapping or misaligned");

// Workspace of gp2d_loo_grad (loo.hpp): P = K_y⁻¹, later M = B·Bᵀ (n × n) | B = P·C (n × n) | r (n) |
// s = P·r (n) | the Cholesky entries c11, c21, c22 of the D_i (n each: np ≤ n points) | the
// triangular products' workspace (PotrsWork) | the pair loop's partial sums, sized as LmlGradWork's.
struct LooGradWork {
  size_t P = 0, B = 0, r = 0, s = 0, c = 0, potrs = 0, partial = 0, total = 0;
  constexpr explicit LooGradWork(int64_t n) {
    const size_t nn = F64 * (size_t)n * (size_t)n, v = F64 * (size_t)n;
    B = nn;
    r = B + nn;
    s = r + v;
    c = s + v;
    potrs = c + 3 * v;
    partial = potrs + PotrsWork(n).total;
    total = partial + grad_partial_bytes(grad_blocks(n + PT_TILE, n + 1));
  }
  struct Ptrs { double *P, *B, *r, *s, *c11, *c21, *c22; void* potrs; double* partial; };
  Ptrs at(void* w, int64_t n) const {
    double* cc = work_at(w, c);
    return {work_at(w, P), work_at(w, B), work_at(w, r), work_at(w, s), cc, cc + n, cc + 2 * n,
            work_at<char>(w, potrs), work_at(w, partial)};
  }
};
constexpr bool loo_grad_work_ok(int64_t n) {
  const LooGradWork w(n);
  const size_t nn = F64 * (size_t)n * (size_t)n, v = F64 * (size_t)n;
  bool ok = regions_ok({w.P, w.B, w.r, w.s, w.c, w.potrs, w.partial, w.total},
                       {nn, nn, v, v, 3 * v, PotrsWork(n).total, grad_partial_bytes((n / 64 + 1) * (n / 16 + 1))});
  for (int bd = 1; bd <= 2; ++bd)   // the fullest launch: ntr = ntr_pad = n / bd
    ok = ok && w.partial + grad_partial_bytes(grad_blocks(n / bd, n / bd)) <= w.total;
  return ok && w.potrs % 16 == 0;
}
static_assert(loo_grad_work_ok(128) && loo_grad_work_ok(384) && loo_grad_work_ok(8192) && loo_grad_work_ok(32768),
              "loo_grad workspace: regions out of order, overlapping, misaligned or too few partials");

}  // namespace gp2d
