// predict_host.hpp — the workspace layouts of the FP64 predicts (gp2d_predict and
// gp2d_predict_field; gp2d_predict_grad; gp2d_predict_cov; the trend fit, block and predicts), as byte-offset tables.  gp2d.hip takes every FP64 predict
// workspace size it reports and every pointer it carves from here; nothing else knows the layouts
// (the kernels in predict.hpp, gemm_f64.hpp and postcov.hpp get plain pointers).
#pragma once
#include "factor_host.hpp"
#include "gemm_f64.hpp"
#include "predict.hpp"
#include "trend.hpp"

namespace gp2d {

// Partial sums of a reduction over the n rows: one row of ncols per 128-row segment — the mean's
// (mean_part_kernel's grid.y, MEAN_SEG rows each) and the variance's Σ v² (the EPI_COLSQ epilogue,
// GBM rows each: the same count) — sized for one row more.
static_assert(MEAN_SEG == GBM, "the mean's and the COLSQ partials share one segment count");
constexpr int64_t predict_segments(int64_t n) { return n / MEAN_SEG; }
constexpr size_t predict_partial_bytes(int64_t n, int64_t ncols) {
  return F64 * (size_t)(predict_segments(n) + 1) * (size_t)ncols;
}

// Columns a chunked predict's workspace is sized for: bd components of `chunk` targets padded to
// whole point tiles, rounded up to whole GEMM column tiles.  chunk < 1 sizes as one tile.
constexpr int64_t predict_sized_cols(int64_t chunk, int bd) {
  return round_up(bd * round_up(chunk < 1 ? 1 : chunk, PT_TILE), GBN);
}

// Workspace of gp2d_predict and gp2d_predict_field: K*ᵀ of a chunk (n × ncols) | the mean's
// partial sums | the Σ v² partial sums.  The exported sizes are PredictWork(n, predict_sized_cols(
// chunk, bd)); the entries carve with ncols = bd·chunk (gp2d_predict) and ncols = chunk
// (gp2d_predict_field), which their argument checks (chunk a positive multiple of 64, the column
// count a multiple of 128) make equal to the sized count — a workspace of the exported size is
// exactly what a call uses.  (n < 1 is no call's shape; the size functions answer it with this same
// arithmetic, n = 0: the two partial rows.)
struct PredictWork {
  size_t Ks = 0, pm = 0, P = 0, total = 0;
  constexpr PredictWork(int64_t n, int64_t ncols) {
    pm = F64 * (size_t)n * (size_t)ncols;
    P = pm + predict_partial_bytes(n, ncols);
    total = P + predict_partial_bytes(n, ncols);
  }
  struct Ptrs { double* Ks; double* pm; double* P; };
  Ptrs at(void* w) const { return {work_at(w, Ks), work_at(w, pm), work_at(w, P)}; }
};
constexpr bool predict_work_ok(int64_t n, int64_t ncols) {
  const PredictWork w(n, ncols);
  const size_t part = F64 * (size_t)(n / 128 + 1) * (size_t)ncols;
  return regions_ok({w.Ks, w.pm, w.P, w.total}, {F64 * (size_t)n * (size_t)ncols, part, part}) &&
         w.total == F64 * (size_t)ncols * (size_t)(n + 2 * (n / 128 + 1));
}
static_assert(predict_work_ok(128, 128) && predict_work_ok(256, 256) && predict_work_ok(8192, 16384) &&
                  predict_sized_cols(8192, 2) == 16384 && predict_sized_cols(64, 1) == 128 &&
                  predict_sized_cols(0, 2) == 128 && predict_sized_cols(100, 2) == 256,
              "predict workspace: regions out of order, overlapping or misaligned");

// The trend block gp2d_trend_fit writes and the trend predicts and likelihoods read (trend.hpp's
// TB_* offsets, in doubles): β̂ (q, padded to 8) | A⁻¹ (q × q at row stride TREND_QMAX) | log|A| |
// status (0, or the 1-based order of A's failed pivot) | the right-hand sides, n rows of TREND_RHS
// doubles: [α′_i, B0[i][0..q), 0…].  The table starts on a 128-byte boundary of the block, so a row
// is one aligned 64-byte piece when the block itself is 64-byte aligned.
struct TrendBlock {
  size_t beta = 0, ainv = 0, logdet = 0, status = 0, rhs = 0, doubles = 0;
  constexpr explicit TrendBlock(int64_t n) {
    ainv = beta + 8;
    logdet = ainv + (size_t)TREND_QMAX * TREND_QMAX;
    status = logdet + 1;
    rhs = round_up((int64_t)status + 1, 16);
    doubles = rhs + (size_t)TREND_RHS * (size_t)(n > 0 ? n : 0);
  }
};
constexpr int trend_q(int order) { return order == 0 ? 2 : TREND_QMAX; }
static_assert(TrendBlock(0).beta == TB_BETA && TrendBlock(0).ainv == TB_AINV && TrendBlock(0).logdet == TB_LOGDET &&
                  TrendBlock(0).status == TB_STATUS && TrendBlock(0).rhs == TB_RHS && TrendBlock(0).doubles == 48 &&
                  TrendBlock(256).doubles == 48 + 8 * 256 && TREND_QMAX + 1 <= TREND_RHS && TREND_QMAX <= 8 &&
                  TB_RHS % 8 == 0 && trend_q(0) == 2 && trend_q(1) == 6,
              "trend block: the kernels' offsets and the layout disagree");

// Workspace of gp2d_trend_fit: the table Y = [y | Hᵀ] (n rows of TREND_RHS) | Z = W·Y | the n / 128
// row segments' partial sums of Wᵀ·[z − Gβ̂ | G] (n rows of TREND_RHS each), sized for one segment more.
struct TrendFitWork {
  size_t Y = 0, Z = 0, part = 0, total = 0;
  constexpr explicit TrendFitWork(int64_t n) {
    const size_t tab = F64 * (size_t)TREND_RHS * (size_t)(n > 0 ? n : 0);
    Z = tab;
    part = 2 * tab;
    total = part + (size_t)((n > 0 ? n : 0) / NB + 1) * tab;
  }
  struct Ptrs { double* Y; double* Z; double* part; };
  Ptrs at(void* w) const { return {work_at(w, Y), work_at(w, Z), work_at(w, part)}; }
};
constexpr bool trend_fit_work_ok(int64_t n) {
  const TrendFitWork w(n);
  const size_t tab = F64 * 8 * (size_t)n;
  return regions_ok({w.Y, w.Z, w.part, w.total}, {tab, tab, (size_t)(n / 128 + 1) * tab}) &&
         w.total == tab * (size_t)(3 + n / 128);
}
static_assert(trend_fit_work_ok(128) && trend_fit_work_ok(256) && trend_fit_work_ok(16384) &&
                  TrendFitWork(0).total == 0,
              "trend_fit workspace: regions out of order, overlapping or misaligned");

// Workspace of gp2d_predict_trend and gp2d_predict_field_trend: PredictWork's regions with q + 1
// sets of mean partials (pm[r][segment][column], right-hand side 0 = α′) in place of one.
struct PredictTrendWork {
  size_t Ks = 0, pm = 0, P = 0, total = 0;
  constexpr PredictTrendWork(int64_t n, int64_t ncols, int order) {
    pm = F64 * (size_t)n * (size_t)ncols;
    P = pm + (size_t)(trend_q(order) + 1) * predict_partial_bytes(n, ncols);
    total = P + predict_partial_bytes(n, ncols);
  }
  PredictWork::Ptrs at(void* w) const { return {work_at(w, Ks), work_at(w, pm), work_at(w, P)}; }
};
constexpr bool predict_trend_work_ok(int64_t n, int64_t ncols, int order) {
  const PredictTrendWork w(n, ncols, order);
  const size_t part = F64 * (size_t)(n / 128 + 1) * (size_t)ncols, q1 = order == 0 ? 3 : 7;
  return regions_ok({w.Ks, w.pm, w.P, w.total}, {F64 * (size_t)n * (size_t)ncols, q1 * part, part}) &&
         w.total == PredictWork(n, ncols).total + (q1 - 1) * part;
}
static_assert(predict_trend_work_ok(128, 128, 0) && predict_trend_work_ok(256, 256, 1) &&
                  predict_trend_work_ok(8192, 16384, 1),
              "predict_trend workspace: regions out of order, overlapping or misaligned");

// Workspace of gp2d_predict_grad: C = cov(observations, ∇f) of a chunk (n × 4·chunk, grad.hpp's
// column layout) | the mean's partial sums (4·chunk columns) | the Gram partial sums (10 per target
// and 128-row segment, the EPI_COLGRAM epilogue).  chunk is a positive multiple of 64, so a chunk's
// padded target count never exceeds it; chunk < 1 sizes as one tile.
struct PredictGradWork {
  size_t C = 0, pm = 0, G = 0, total = 0;
  constexpr PredictGradWork(int64_t n, int64_t chunk) {
    const int64_t cp = round_up(chunk < 1 ? 1 : chunk, PT_TILE);
    pm = F64 * (size_t)(n > 0 ? n : 0) * (size_t)(4 * cp);
    G = pm + predict_partial_bytes(n > 0 ? n : 0, 4 * cp);
    total = G + predict_partial_bytes(n > 0 ? n : 0, EPI_COLGRAM_PAIRS * cp);
  }
  struct Ptrs { double* C; double* pm; double* G; };
  Ptrs at(void* w) const { return {work_at(w, C), work_at(w, pm), work_at(w, G)}; }
};
constexpr bool predict_grad_work_ok(int64_t n, int64_t chunk) {
  const PredictGradWork w(n, chunk);
  const size_t seg = (size_t)(n / 128 + 1);
  return regions_ok({w.C, w.pm, w.G, w.total},
                    {F64 * (size_t)n * (size_t)(4 * chunk), F64 * seg * (size_t)(4 * chunk),
                     F64 * seg * (size_t)(10 * chunk)}) &&
         w.total == F64 * (size_t)chunk * (size_t)(4 * n + 14 * (n / 128 + 1));
}
static_assert(predict_grad_work_ok(128, 64) && predict_grad_work_ok(384, 256) && predict_grad_work_ok(8192, 8192) &&
                  PredictGradWork(256, 0).total == PredictGradWork(256, 64).total,
              "predict_grad workspace: regions out of order, overlapping or misaligned");

// Padded target count and matrix order of gp2d_predict_cov.
constexpr int64_t postcov_mp(int64_t m) { return round_up(m < 1 ? 1 : m, PT_TILE); }
constexpr int64_t postcov_q(int64_t m) { return 2 * postcov_mp(m); }

// Workspace of gp2d_predict_cov: K*ᵀ (n × q) | V = W·K*ᵀ (n × q) | the mean's partial sums
// ((n / MEAN_SEG) segments × q).
struct PredictCovWork {
  size_t Ks = 0, V = 0, pm = 0, total = 0;
  constexpr PredictCovWork(int64_t n, int64_t m) {
    const size_t nq = F64 * (size_t)(n > 0 ? n : 0) * (size_t)postcov_q(m);
    V = nq;
    pm = 2 * nq;
    total = pm + predict_partial_bytes(n > 0 ? n : 0, postcov_q(m));
  }
  struct Ptrs { double* Ks; double* V; double* pm; };
  Ptrs at(void* w) const { return {work_at(w, Ks), work_at(w, V), work_at(w, pm)}; }
};
constexpr bool predict_cov_work_ok(int64_t n, int64_t m) {
  const PredictCovWork w(n, m);
  const size_t nq = F64 * (size_t)n * (size_t)postcov_q(m);
  return regions_ok({w.Ks, w.V, w.pm, w.total}, {nq, nq, F64 * (size_t)(n / MEAN_SEG + 1) * (size_t)postcov_q(m)});
}
static_assert(predict_cov_work_ok(128, 1) && predict_cov_work_ok(384, 130) && predict_cov_work_ok(8192, 4096) &&
                  postcov_q(1) == 128 && postcov_q(100) == 256 && postcov_q(130) == 384,
              "predict_cov workspace: regions out of order, overlapping or misaligned");

}  // namespace gp2d
