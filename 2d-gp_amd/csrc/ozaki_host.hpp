// ozaki_host.hpp — the two buffer layouts of the int8 (Ozaki-II) predict, as offset tables.
// gp2d.hip takes every size it reports and every pointer it carves from here; nothing else
// knows the layouts (the kernels in ozaki.hpp get plain pointers).
#pragma once
#include <algorithm>
#include "ozaki.hpp"

namespace gp2d {

// block flags of one chunk: [cp/64 grid blocks][npad/64 training blocks] bytes
constexpr size_t oz_flag_bytes(int64_t n, int64_t chunk) {
  return (size_t)round_up((round_up(chunk < 1 ? 1 : chunk, IBN) / OZ_KS_P) * (n / 2 / OZ_KS_T), 256);
}
// slab lists + prefix counts of one chunk (ints)
constexpr size_t oz_list_bytes(int64_t n, int64_t chunk) {
  const int64_t nbj = 2 * round_up(chunk < 1 ? 1 : chunk, IBN) / IBN, ks = n / IBK;
  return sizeof(int) * (size_t)(nbj * ks + nbj * (ks / 4 + 1));
}

// K* residue planes of a whole grid (gp2d_ozaki_kstar → gp2d_predict_ozaki_planes), chunk > 0:
// per chunk the nmod planes (n × 2·cp_max bytes each), then the chunk's block flags
struct KstarBuf {
  size_t planes, flag_bytes, stride;
  KstarBuf(int64_t n, int64_t chunk, int nmod)
      : planes((size_t)nmod * (size_t)n * (size_t)(2 * round_up(chunk, IBN))), flag_bytes(oz_flag_bytes(n, chunk)),
        stride(planes + flag_bytes) {}
  size_t planes_at(int64_t ci) const { return (size_t)ci * stride; }   // byte offsets of chunk ci
  size_t flags_at(int64_t ci) const { return (size_t)ci * stride + planes; }
};

// Workspace of one predict chunk for a fit with nmod moduli (the layout follows nmod), as byte
// offsets: bres | cres | pm | P | flags | skip.  inline_planes (gp2d_predict_ozaki): the K* planes
// and their flags live here; otherwise (gp2d_predict_ozaki_planes) they come from a KstarBuf and
// both regions are empty.  No moduli or no rows: an empty workspace.
struct OzakiWork {
  size_t bres = 0, cres = 0, pm = 0, P = 0, flags = 0, skip = 0, total = 0;
  constexpr OzakiWork(int64_t n, int64_t chunk, int nmod, bool inline_planes) {
    if (nmod <= 0 || n <= 0) return;
    const size_t ncols = (size_t)(2 * round_up(chunk < 1 ? 1 : chunk, IBN));
    const size_t plane = (size_t)nmod * (size_t)n * ncols;
    const size_t ks_rows = (size_t)(n / 2 / OZ_KS_T + 1);    // ozaki_kstar_kernel's segments (mean partials), + 1
    const size_t crt_rows = (size_t)(n / OZ_CRT_ROWS + 1);   // ozaki_crt_colsq_kernel's segments (Σ V² partials), + 1
    // The planes path sizes pm for the larger count.  Only ozaki_kstar_kernel writes pm (ks_rows − 1
    // rows, all that predict_finalize_kernel reads), so ks_rows would do — and it is the maximum
    // anyway, since OZ_CRT_ROWS ≥ 2·OZ_KS_T; callers allocate by the exported sizes, so it stays.
    cres = bres + (inline_planes ? plane : 0);
    pm = cres + plane;
    P = pm + sizeof(double) * ncols * (inline_planes ? ks_rows : std::max(ks_rows, crt_rows));
    flags = P + sizeof(double) * ncols * crt_rows;
    skip = flags + (inline_planes ? oz_flag_bytes(n, chunk) : 0);
    total = skip + oz_list_bytes(n, chunk);
  }
  struct Ptrs { int8_t* bres; uint8_t* cres; double* pm; double* P; uint8_t* flags; int* skip; };
  Ptrs at(void* work) const {
    char* w = static_cast<char*>(work);
    return {reinterpret_cast<int8_t*>(w + bres), reinterpret_cast<uint8_t*>(w + cres), reinterpret_cast<double*>(w + pm),
            reinterpret_cast<double*>(w + P), reinterpret_cast<uint8_t*>(w + flags), reinterpret_cast<int*>(w + skip)};
  }
};

// W residue planes (gp2d_ozaki_prepare*): per modulus one n × n slab-blocked plane holding the
// lower triangle of W; the int8 GEMM never reads a row block past its diagonal tile.  With
// npad = n/2 a multiple of 256 (a 256-row tile then never straddles the u- and v-observation
// rows) the planes also carry S = W_L + W_R of the v-observation rows — row i, column k < npad:
// W[i][k] + W[i][npad + k] — for the three-product variance, in the part of each plane that the
// triangular product never reads: element (i − npad, npad + k), i.e. layout row blocks
// 0 … npad/256 − 1, slabs npad/64 … n/64 − 1.  S of the u-observation rows is W_L itself.
// 0: this n has no S region (the four-product path).  The choice depends on n alone, so planes
// made ahead and the predict that consumes them agree without extra state.
constexpr int64_t oz_s_npad(int64_t n) { return (n > 0 && n % (2 * IBM) == 0) ? n / 2 : 0; }

// The block products of one chunk's variance GEMM V = W·K*ᵀ (n rows; cp grid points padded to
// 256, columns [u-out | v-out]), in stream order, with their grids in tiles.
//   four products (any n): one launch, V_u = W_L·a + W_R·c and V_v = W_L·c + W_R·b with the (v,u)
//     block of K* read from its equal (u,v) block c;
//   three products (oz_s_npad(n) > 0; K* planes hold a − c, c, b − c), S = W_L + W_R:
//     P1 = S·c → V_v's columns,  P2 = W_L·(a − c) → V_u's columns,  P3 = W_R·(b − c) on the
//     v-observation rows (W_R is zero above them).
//     spare (the K* planes are the workspace's own, gp2d_predict_ozaki): the products are
//       independent and the CRT pass adds their residues (V_u: P1 + P2; V_v: P1, + P3 on the
//       v-observation rows; mod m).  P3 goes where the K* planes have room that nothing reads: the
//       (v,u) block, which is never stored — of layout row block cp/256 + bj the slabs below n/128,
//       256·n/2 contiguous bytes, exactly P3's column block bj with its columns n/2 apart.  c3 tells
//       the launch of P3 and the CRT pass where that is (offsets from a modulus's K* plane).
//     otherwise (planes made ahead belong to the caller and are not written): P2's epilogue adds P1
//       → V_u; P3 adds P1 in place → V_v, after P2, which reads what P3 overwrites.
//     Residues add mod m, so either way V's residues are the four-product ones.
struct OzakiProducts {
  int count;
  IgemmProd prod[3];
  unsigned gx[3], gy[3];
  bool sum_in_crt = false;   // P3 lies in the K* planes and the CRT pass adds the products
  int64_t p3_off = 0, p3_blk = 0;   // P3's first byte in a modulus's K* plane; bytes between its column blocks
  OzakiProducts(int64_t n, int64_t cp, bool three, bool spare) {
    const int nb = (int)(n / IBM), nbh = (int)(cp / IBN), hs = (int)(n / 2 / IBK);
    if (!three) {
      count = 1;
      prod[0] = IgemmProd::plain((int)n, true);
      prod[0].alias_rb = nbh;
      prod[0].alias_ks = hs;
      gx[0] = 2u * nbh;
      gy[0] = (unsigned)nb;
      return;
    }
    const int nb2 = nb / 2, npad = (int)(n / 2), vcol = (int)cp;
    count = 3;
    sum_in_crt = spare;
    p3_off = cp * n;             // layout row block cp/256, slab 0
    p3_blk = (int64_t)IBN * n;   // one layout row block
    const int add = spare ? -1 : vcol;
    // P3 among the K* planes: its rows count from the first v-observation row (c_off), leading dimension n/2
    const int64_t o3 = spare ? -(int64_t)npad : 0, b3 = spare ? p3_blk : 0;
    //         bi0  a_slab0 a_fold  a_fold_slab0 b_rb0 b_slab0 alias_rb alias_ks k_bi0 k_cap c_col0             add_col0 c_off c_blk
    prod[0] = {0,   0,      nb2,    hs,          0,    hs,     INT_MAX, 0,       0,    npad, vcol,              -1,      0,    0};
    prod[1] = {0,   0,      INT_MAX, 0,          0,    0,      INT_MAX, 0,       0,    npad, 0,                 add,     0,    0};
    prod[2] = {nb2, hs,     INT_MAX, 0,          nbh,  hs,     INT_MAX, 0,       nb2,  npad, spare ? 0 : vcol,  add,     o3,   b3};
    gx[0] = gx[1] = gx[2] = (unsigned)nbh;
    gy[0] = gy[1] = (unsigned)nb;
    gy[2] = (unsigned)nb2;
  }
};

// regions in order without overlap (the total is the end of the last by construction), doubles on
// 8 bytes, ints on 4, the planes' two regions empty exactly when the planes are not inline
constexpr bool ozaki_work_ok(int64_t n, int64_t chunk, int nmod) {
  for (int inl = 0; inl < 2; ++inl) {
    const OzakiWork w(n, chunk, nmod, inl);
    if (w.bres != 0 || (w.cres > w.bres) != inl || w.pm <= w.cres || w.P <= w.pm || w.flags <= w.P ||
        w.skip < w.flags || (w.skip > w.flags) != inl || w.total <= w.skip || w.pm % 8 || w.P % 8 || w.skip % 4)
      return false;
  }
  return true;
}
static_assert(ozaki_work_ok(256, 128, 12) && ozaki_work_ok(256, 128, 16) && ozaki_work_ok(8192, 8192, 13),
              "OzakiWork: regions out of order, overlapping or misaligned");

}  // namespace gp2d
