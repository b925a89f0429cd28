// factor_host.hpp — the shape of the blocked TRTRI (pairs per level, K-split rule, buffer sizes)
// and the three workspace layouts of the FP64 factor, as byte-offset tables.  gp2d.hip takes every
// factor workspace size it reports and every pointer it carves from here; nothing else knows the
// layouts (the kernels get plain pointers).
#pragma once
#include <algorithm>
#include <initializer_list>
#include "common.hpp"
#include "dfact.hpp"

namespace gp2d {

// ---- TRTRI by recursive doubling over 128-blocks: at level g every pair (left = [s·2g, s·2g+g),
// right = [s·2g+g, s·2g+2g)) forms T = L[R, left]·W[left, left], then W[R, left] = −W[R, R]·T.
// A level is at most two launches: `count` consecutive pairs with a right part of Rn blocks, the
// first with its left part at block Ls and its right part at Rs — the full pairs, then a ragged one.
struct TrtriPair { int Ls, Rs, Rn, count; };
struct TrtriLevel {
  TrtriPair pair[2];
  int npairs;
  constexpr const TrtriPair* begin() const { return pair; }   // for (const TrtriPair& pr : level)
  constexpr const TrtriPair* end() const { return pair + npairs; }
};
constexpr TrtriLevel trtri_level_pairs(int nbk, int g) {
  const int full = nbk / (2 * g);                // pairs whose right part has g blocks
  const int rem = nbk - full * 2 * g;            // trailing blocks
  TrtriLevel lv{{{0, 0, 0, 0}, {0, 0, 0, 0}}, 0};
  if (full > 0) lv.pair[lv.npairs++] = {0, g, g, full};
  if (rem > g) lv.pair[lv.npairs++] = {full * 2 * g, full * 2 * g + g, rem - g, 1};
  return lv;
}
// GemmParams::ksplit (tiles with a longer K range are cut in half) for a product with kblocks ×
// oblocks tiles per pair, 0 = no split
constexpr int trtri_ksplit(int kblocks, int oblocks) {
  return (kblocks >= 4 && kblocks * oblocks <= 256) ? 2 * NB : 0;
}
constexpr size_t trtri_split_doubles(int nbk) {   // T2: the largest high half of any split product
  size_t m = 0;
  for (int g = 1; g < nbk; g *= 2)
    for (const TrtriPair& pr : trtri_level_pairs(nbk, g))
      if (trtri_ksplit(g, pr.Rn) || trtri_ksplit(pr.Rn, g))
        m = std::max(m, (size_t)pr.count * pr.Rn * NB * g * NB);
  return m;
}
// T of the widest level of an order-n inverse: pairs × (g·NB)² doubles ≤ (n/2 + 128)²
constexpr size_t trtri_t_doubles(int64_t n) { return (size_t)(n / 2 + NB) * (size_t)(n / 2 + NB); }

template <class T = double>
inline T* work_at(void* work, size_t off) { return reinterpret_cast<T*>(static_cast<char*>(work) + off); }
constexpr size_t F64 = sizeof(double);

// TRTRI workspace (gp2d_trtri, gp2d_trtri_batched).  Lone form (own_dinv): T | the n/128 inverted
// diagonal blocks (used when the caller has none) | T2.  Batched form: T × nprob | T2 × nprob,
// problem q's at + q·pT and + q·pT2 doubles.  No problems: an empty workspace.
struct TrtriWork {
  size_t T = 0, dinv = 0, T2 = 0, total = 0;
  int64_t pT = 0, pT2 = 0;
  constexpr TrtriWork(int64_t n, int nprob, bool own_dinv) {
    if (nprob < 1) return;
    pT = (int64_t)trtri_t_doubles(n);
    pT2 = (int64_t)trtri_split_doubles((int)(n / NB));
    dinv = F64 * (size_t)nprob * (size_t)pT;
    T2 = dinv + (own_dinv ? F64 * (size_t)(n / NB) * NB * NB : 0);
    total = T2 + F64 * (size_t)nprob * (size_t)pT2;
  }
  struct Ptrs { double* T; double* dinv; double* T2; };
  Ptrs at(void* work) const { return {work_at(work, T), work_at(work, dinv), work_at(work, T2)}; }
};

// The fused inverse (gp2d_potrf_inv) splits the top level of the recursive doubling at h, the
// largest power of two below nb, i.e. the TRTRI's own top-level split.
constexpr int inv_top_split(int nb) { int h = 1; while (2 * h < nb) h *= 2; return h; }

// Its workspace: T1, the lower levels' T (one half at a time; the left half, h blocks, is the
// larger) | T2, the top level's T, (nb−h)·128 × h·128 | T3, the split products' high halves.
// One block (n ≤ 128) has no inverse GEMMs: an empty workspace.
struct PotrfInvWork {
  size_t T1 = 0, T2 = 0, T3 = 0, total = 0;
  int h = 0;
  constexpr explicit PotrfInvWork(int64_t n) {
    const int nb = (int)(n / NB);
    if (nb <= 1) return;
    h = inv_top_split(nb);
    T2 = F64 * trtri_t_doubles((int64_t)h * NB);
    T3 = T2 + F64 * (size_t)(nb - h) * NB * (size_t)h * NB;
    total = T3 + F64 * std::max({trtri_split_doubles(h), trtri_split_doubles(nb - h), trtri_split_doubles(nb)});
  }
  struct Ptrs { double* T1; double* T2; double* T3; };
  Ptrs at(void* work) const { return {work_at(work, T1), work_at(work, T2), work_at(work, T3)}; }
};

// Workspace of the distributed factor (gp2d_dfact_panel, gp2d_dfact_invstep): the DF_SBT inverted
// 128×128 diagonal blocks | an int status word | the head's TRTRI buffers T, T2 (a batched-form
// TrtriWork of one order-DF_SB problem) | the TRTRI step's out-of-place X[s] (DF_SB rows × n, at
// A's column positions).
constexpr size_t DFACT_STATUS_BYTES = 64;   // the status word's slot
constexpr size_t DFACT_XT_PAD_BYTES = 64;   // between the head's T2 and Xt
struct DfactWork {
  size_t dinv = 0, status = 0, T = 0, T2 = 0, Xt = 0, total = 0;
  constexpr explicit DfactWork(int64_t n) {
    const TrtriWork head(DF_SB, 1, false);
    status = F64 * (size_t)DF_SBT * NB * NB;
    T = status + DFACT_STATUS_BYTES;
    T2 = T + head.T2;
    Xt = T + head.total + DFACT_XT_PAD_BYTES;
    total = Xt + F64 * (size_t)DF_SB * (size_t)(n > 0 ? n : 0);
  }
  struct Ptrs { double* dinv; int* status; double* T; double* T2; double* Xt; };
  Ptrs at(void* w) const { return {work_at(w, dinv), work_at<int>(w, status), work_at(w, T), work_at(w, T2), work_at(w, Xt)}; }
};

// Regions at off[0..k−1] with off[k] the total: from 0, on 8 bytes, each with the `need` bytes of
// its user before the next begins (in order, no overlap), the last ending exactly at the total.
constexpr bool regions_ok(std::initializer_list<size_t> off, std::initializer_list<size_t> need) {
  const size_t *o = off.begin(), *r = need.begin(), k = need.size();
  if (off.size() != k + 1 || o[0] != 0 || o[k - 1] + r[k - 1] != o[k]) return false;
  for (size_t i = 0; i < k; ++i)
    if (o[i] % 8 || o[i] + r[i] > o[i + 1]) return false;
  return true;
}
constexpr bool factor_work_ok(int64_t n) {   // n a multiple of 128, at least 256
  const TrtriWork l(n, 1, true), b(n, 3, false);
  const PotrfInvWork f(n);
  const DfactWork d(n);
  const size_t nb = (size_t)(n / NB), h = (size_t)f.h, r = nb - h, blk = F64 * NB * NB;
  const size_t t = F64 * trtri_t_doubles(n), t2 = F64 * trtri_split_doubles((int)nb);
  const size_t f3 = F64 * std::max({trtri_split_doubles((int)h), trtri_split_doubles((int)r), trtri_split_doubles((int)nb)});
  return regions_ok({l.T, l.dinv, l.T2, l.total}, {t, nb * blk, t2}) &&
         regions_ok({b.T, b.T2, b.total}, {3 * t, 3 * t2}) && b.dinv == b.T2 && b.pT * F64 == t && b.pT2 * F64 == t2 &&
         h >= r && r >= 1 &&   // so T1, sized for h blocks, holds either half's lower levels
         regions_ok({f.T1, f.T2, f.T3, f.total}, {F64 * trtri_t_doubles((int64_t)h * NB), h * r * blk, f3}) &&
         regions_ok({d.dinv, d.status, d.T, d.T2, d.Xt, d.total},
                    {DF_SBT * blk, sizeof(int), F64 * trtri_t_doubles(DF_SB), F64 * trtri_split_doubles(DF_SBT),
                     F64 * DF_SB * (size_t)n});
}
static_assert(factor_work_ok(256) && factor_work_ok(512) && factor_work_ok(640) && factor_work_ok(8192) &&
                  PotrfInvWork(640).h == 4 && PotrfInvWork(128).total == 0 && TrtriWork(640, 0, false).total == 0,
              "factor workspaces: regions out of order, overlapping or misaligned");

}  // namespace gp2d
