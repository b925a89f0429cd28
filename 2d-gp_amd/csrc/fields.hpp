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

struct FieldParams {
  VecParams v;   // point layout and temporal factor (pdim, var_t, ilt2); the 2×2 block is not used
  int curl;      // 0: divergence, 1: vorticity
  double il2;    // 1/ℓ² of the part that carries the field (ℓ_cf for δ, ℓ_df for ζ)
  double w4;     // its weight over ℓ⁴
};

// weight of the kernel part that carries `field`; 0 where the field vanishes by kind
inline double field_weight(const gp2d_kernel_t* k, int field) {
  const bool curl = field == GP2D_FIELD_VORTICITY;
  switch (k->kind) {
    case GP2D_KIND_DIVFREE: return curl ? 1.0 : 0.0;
    case GP2D_KIND_CURLFREE: return curl ? 0.0 : 1.0;
    default: return curl ? k->ratio : 1.0 - k->ratio;
  }
}

inline FieldParams make_field_params(const gp2d_kernel_t* k, int field) {
  FieldParams p;
  p.v = make_vec_params(k);
  p.curl = (field == GP2D_FIELD_VORTICITY);
  p.il2 = p.curl ? p.v.il_df2 : p.v.il_cf2;
  p.w4 = field_weight(k, field) * p.il2 * p.il2;
  return p;
}

// C = cov(observations, field at the targets): (2·na_pad) × cp with leading dimension cp; rows i
// and na_pad + i of column j hold the f1 and f2 cross-covariances of training point i with target
// j.  The thread mapping is assemble_vec_kernel's: a workgroup's 64 target points are staged once
// through LDS, the training point of a wave is wave-uniform (scalar loads), every store is a
// coalesced 512-byte row segment; one exp per pair (two for the spatio-temporal product).  Every
// element of the buffer is written — 0.0 for padded training rows and padded target columns —
// since the variance GEMM reads all of it and the workspace is reused.
// Launch: grid (cp / 64, ⌈na_pad / ASM_ROWS⌉), 256 threads; cp a multiple of 64.
__global__ __launch_bounds__(256) void assemble_field_kernel(
    const double* __restrict__ xa, int64_t na, int64_t na_pad,
    const double* __restrict__ xg, int64_t m, int64_t cp, FieldParams p, double* __restrict__ out) {
  __shared__ double colpts[3 * 64];
  const int pdim = p.v.pdim;
  const int64_t jt = (int64_t)blockIdx.x * 64;   // the tile's first target point
  const int lane = threadIdx.x & 63;
  const int ty = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int64_t j = jt + lane;
  const bool jv = j < m;
  if (ty == 0) {
    for (int e = lane; e < pdim * 64; e += 64) {   // the tile's points, coalesced
      const int64_t g = jt * pdim + e;
      colpts[e] = (g < m * pdim) ? xg[g] : 0.0;
    }
  }
  __syncthreads();
  double b0 = 0.0, b1, b2;
  if (pdim == 3) {
    b0 = colpts[3 * lane]; b1 = colpts[3 * lane + 1]; b2 = colpts[3 * lane + 2];
  } else {
    b1 = colpts[2 * lane]; b2 = colpts[2 * lane + 1];
  }
#pragma unroll 1
  for (int q = 0; q < ASM_ROWS / 4; ++q) {
    const int64_t i = (int64_t)blockIdx.y * ASM_ROWS + ty + 4 * q;   // wave-uniform
    if (i >= na_pad) break;
    double c1 = 0.0, c2 = 0.0;
    if (jv && i < na) {
      double a0, a1, a2;
      vec_point(p.v, xa, i, a0, a1, a2);
      const double d1 = a1 - b1, d2 = a2 - b2;
      const double c = (d1 * d1 + d2 * d2) * p.il2;
      const double s = p.w4 * exp(-0.5 * c) * (4.0 - c) * time_factor(p.v, a0 - b0);
      const double h1 = s * d1, h2 = s * d2;
      c1 = p.curl ? -h2 : h1;
      c2 = p.curl ? h1 : h2;
    }
    out[i * cp + j] = c1;
    out[(na_pad + i) * cp + j] = c2;
  }
}

}  // namespace gp2d
