// fields.hpp — cross-covariance of the velocity observations with a derived scalar field of
// the same GP: the divergence δ = ∂f1/∂x1 + ∂f2/∂x2 or the vorticity ζ = ∂f2/∂x1 − ∂f1/∂x2 at
// the target points (DESIGN.md "Derived fields").
//
// Replaces nothing in the reference, which finite-differences its predicted grids downstream
// (GP_plots.py); a derivative of a GP is a GP, so both fields follow from the same fit
// (W = L⁻¹, α) with this matrix in place of K* and the field's prior variance in place of kss.
//
// With d = x − g (training point minus target point), r² = d1² + d2² and
//   h_p(d; ℓ) = exp(−r²/2ℓ²) · d_p · (4 − r²/ℓ²) / ℓ⁴,
// differentiating the 2×2 SE blocks of assemble.hpp in the target point gives
//   cov(f_p(x), δ(g)) = w_cf · h_p(d; ℓ_cf),
//   cov(f_1(x), ζ(g)) = −w_df · h_2(d; ℓ_df),   cov(f_2(x), ζ(g)) = +w_df · h_1(d; ℓ_df),
// w_df = 1 | 0 | ratio and w_cf = 0 | 1 | 1 − ratio for df | cf | mixed: the div-free part has no
// divergence and the curl-free part no vorticity.  The spatio-temporal product multiplies both by
// its temporal factor (time_factor).  Var δ = 8·w_cf/ℓ_cf⁴, Var ζ = 8·w_df/ℓ_df⁴ (× var_t).
#pragma once
#include "assemble.hpp"

namespace gp2d {

// weight of the kernel part that carries `field`; 0 where the field vanishes by kind
inline double field_weight(const gp2d_kernel_t* k, int field) {
  const bool curl = field == GP2D_FIELD_VORTICITY;
  switch (k->kind) {
    case GP2D_KIND_DIVFREE: return curl ? 1.0 : 0.0;
    case GP2D_KIND_CURLFREE: return curl ? 0.0 : 1.0;
    default: return curl ? k->ratio : 1.0 - k->ratio;
  }
}

// cross_cov_kernel's entry for C = cov(observations, field at the targets): (2·na_pad) × cp with
// leading dimension cp; rows i and na_pad + i of column j hold the f1 and f2 cross-covariances of
// training point i with target j.  One exp per pair (two for the spatio-temporal product).  Every
// element of the buffer is written — 0.0 for padded training rows and padded target columns —
// since the variance GEMM reads all of it and the workspace is reused.
struct FieldEntry : StoresAll {
  static constexpr int ROWS = 2, COLS = 1;
  VecParams v;   // point layout and temporal factor (pdim, var_t, ilt2); the 2×2 block is not used
  int curl;      // 0: divergence, 1: vorticity
  double il2;    // 1/ℓ² of the part that carries the field (ℓ_cf for δ, ℓ_df for ζ)
  double w4;     // its weight over ℓ⁴
  __device__ __forceinline__ const VecParams& layout() const { return v; }
  __device__ __forceinline__ int64_t col(int64_t j, int, int64_t) const { return j; }
  __device__ __forceinline__ void value(const Point3& a, const Point3& b, bool, double (&o)[2][1]) const {
    const double d1 = a.c[1] - b.c[1], d2 = a.c[2] - b.c[2];
    const double c = (d1 * d1 + d2 * d2) * il2;
    const double s = w4 * exp(-0.5 * c) * (4.0 - c) * time_factor(v, a.c[0] - b.c[0]);
    const double h1 = s * d1, h2 = s * d2;
    o[0][0] = curl ? -h2 : h1;
    o[1][0] = curl ? h1 : h2;
  }
  __device__ __forceinline__ void padded(bool, double (&o)[2][1]) const { o[0][0] = 0.0; o[1][0] = 0.0; }
};

inline FieldEntry make_field_entry(const gp2d_kernel_t* k, int field) {
  FieldEntry p;
  p.v = make_vec_params(k);
  p.curl = (field == GP2D_FIELD_VORTICITY);
  p.il2 = p.curl ? p.v.il_df2 : p.v.il_cf2;
  p.w4 = field_weight(k, field) * p.il2 * p.il2;
  return p;
}

// true where the field vanishes by the kernel's kind (δ of DIVFREE, ζ of CURLFREE)
inline bool field_vanishes(const gp2d_kernel_t* k, int field) {
  return field_weight(k, field) == 0.0 && k->kind != GP2D_KIND_MIXED;
}

// A sum's field cross-covariance: Σ_t w_t·(term t's).  A term in which the field vanishes by kind
// contributes exact zeros whatever its unused length scale holds.
inline SumEntry<FieldEntry> make_sum_field_entry(const gp2d_kernel_t* k, int field) {
  SumEntry<FieldEntry> e;
  e.nterms = k->nterms;
  e.add_diag = 0;
  e.diag_add = 0.0;
  for (int t = 0; t < GP2D_SUM_MAX_TERMS; ++t) {
    const int s = t < k->nterms ? t : 0;
    e.term[t] = make_field_entry(sum_term(k, s), field);
    if (field_vanishes(sum_term(k, s), field)) e.term[t].il2 = e.term[t].w4 = 0.0;
    e.w[t] = sum_weight(k, s);
  }
  return e;
}

}  // namespace gp2d
