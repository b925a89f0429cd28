// gp2d.hip — C ABI of the MI355X GP-kriging engine (include/gp2d.h).
//
// Host orchestration of the kernels in assemble.hpp / gemm_f64.hpp /
// factor.hpp / predict.hpp.  All work is enqueued on the caller's HIP stream;
// nothing here synchronises except gp2d_timing_read().
#include "common.hpp"
#ifndef GP2D_RELEASE
#error "libgp2d.so is built with -DGP2D_RELEASE=1 (python __graft_entry__.py build)"
#endif
#include "assemble.hpp"
#include "gemm_f64.hpp"
#include "factor.hpp"
#include "predict.hpp"
#include "trend.hpp"
#include "fields.hpp"
#include "grad.hpp"
#include "advect.hpp"
#include "paths.hpp"
#include "postcov.hpp"
#include "predict_host.hpp"
#include "ozaki.hpp"
#include "ozaki_host.hpp"
#include "factor_host.hpp"
#include "cv.hpp"
#include "lml.hpp"
#include "loo.hpp"
#include "lml_host.hpp"
#include "dfact.hpp"
#include "order.hpp"
#include "../../include/gp2d.h"

#include <dlfcn.h>

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <cmath>
#include <atomic>
#include <functional>
#include <limits>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

namespace gp2d {

static thread_local std::string g_err;
void set_error(const std::string& msg) { g_err = msg; }

static inline hipStream_t S(void* s) { return reinterpret_cast<hipStream_t>(s); }

// The leading-dimension contract of include/gp2d.h ("Leading dimensions"): a matrix that any kernel
// reads or writes in 16-byte pairs (d2 at base + row·ld + even column) needs an even ld and a
// 16-byte aligned base; every other matrix only ld >= its row length.
static inline bool ld_even(int64_t ld, int64_t row) { return ld >= row && ld % 2 == 0; }
static inline bool aligned16(const void* p) { return reinterpret_cast<uintptr_t>(p) % 16 == 0; }

// ---------------------------------------------------------------- timing hooks
struct Timing {
  std::mutex mu;
  bool on = false;
  std::vector<std::pair<hipEvent_t, hipEvent_t>> ev;
  std::vector<double> flops;
  std::vector<hipEvent_t> pool;
  hipEvent_t get() {
    if (!pool.empty()) { hipEvent_t e = pool.back(); pool.pop_back(); return e; }
    hipEvent_t e; hipEventCreate(&e); return e;
  }
};
static Timing g_timing;

// Times what is enqueued on the stream from its construction to stop() or the end of its scope,
// when the hooks are on (and `enabled`): an event pair from the pool around that span, recorded with
// its flop count — also when a launch inside failed and the function returned, so the pair goes
// back to the pool at the next gp2d_timing_read().
struct TimedLaunch {
  TimedLaunch(hipStream_t stream, double flop, bool enabled = true) : s(stream), flops(flop) {
    std::lock_guard<std::mutex> lk(g_timing.mu);
    if (enabled && g_timing.on) { e0 = g_timing.get(); e1 = g_timing.get(); hipEventRecord(e0, s); }
  }
  void stop() {
    if (!e0) return;
    std::lock_guard<std::mutex> lk(g_timing.mu);
    hipEventRecord(e1, s);
    g_timing.ev.push_back({e0, e1});
    g_timing.flops.push_back(flops);
    e0 = nullptr;
  }
  ~TimedLaunch() { stop(); }
  TimedLaunch(const TimedLaunch&) = delete;
  TimedLaunch& operator=(const TimedLaunch&) = delete;
 private:
  hipStream_t s;
  double flops;
  hipEvent_t e0 = nullptr, e1 = nullptr;
};

// coordinates per point: (x1, x2), (t, x1, x2), or the ARD dimension
static int point_dim(const gp2d_kernel_t* k) {
  if (is_sum_family(k)) k = sum_term(k, 0);   // every term shares the family
  return k->family == GP2D_FAMILY_VECTOR2D ? 2 : (k->family == GP2D_FAMILY_VECTOR_ST ? 3 : k->dim);
}

static int validate_kernel(const gp2d_kernel_t* k);

// A sum's descriptor array (include/gp2d.h): the header, then every term.
static int validate_sum(const gp2d_kernel_t* k) {
  GP2D_REQUIRE(k->nterms >= 1 && k->nterms <= GP2D_SUM_MAX_TERMS, "sum: nterms must be 1..3");
  for (int t = 0; t < k->nterms; ++t) {
    const gp2d_kernel_t* kt = sum_term(k, t);
    GP2D_REQUIRE(!is_sum_family(kt), "sum: a term must not be a sum itself");
    GP2D_REQUIRE(kt->family != GP2D_FAMILY_ARD_RBF, "sum: ARD terms are not supported (vector families only)");
    GP2D_REQUIRE(kt->family == sum_term(k, 0)->family,
                 "sum: the terms must be all VECTOR2D or all VECTOR_ST, not mixed");
    GP2D_REQUIRE(sum_weight(k, t) > 0.0, "sum: every weight must be > 0");
    if (validate_kernel(kt) != 0) {
      set_error("sum: term " + std::to_string(t) + " is invalid: " + g_err);
      return -2;
    }
  }
  return 0;
}

// Entries without a sum instantiation refuse one on the host, before any launch.
static int refuse_sum(const gp2d_kernel_t* k, const char* entry) {
  if (k != nullptr && is_sum_family(k)) {
    set_error(std::string(entry) + ": a kernel sum (GP2D_FAMILY_VECTOR_SUM) is not supported by this entry");
    return -2;
  }
  return 0;
}

static int validate_kernel(const gp2d_kernel_t* k) {
  GP2D_REQUIRE(k != nullptr, "kernel descriptor is NULL");
  if (is_sum_family(k)) return validate_sum(k);
  if (is_vector_family(k)) {
    GP2D_REQUIRE(k->kind >= 0 && k->kind <= 3, "vector2d kind must be 0..3");
    GP2D_REQUIRE(k->l_df > 0.0, "l_df must be > 0");
    if (k->kind == GP2D_KIND_CURLFREE || k->kind == GP2D_KIND_MIXED) GP2D_REQUIRE(k->l_cf > 0.0, "l_cf must be > 0");
    if (k->family == GP2D_FAMILY_VECTOR_ST)
      GP2D_REQUIRE(k->var[0] > 0.0 && k->ls[0][0] > 0.0, "spatio-temporal var_t and l_t must be > 0");
  } else if (k->family == GP2D_FAMILY_ARD_RBF) {
    GP2D_REQUIRE(k->dim >= 1 && k->dim <= 3, "ARD dim must be 1..3");
    GP2D_REQUIRE(k->nterms >= 1 && k->nterms <= 2, "ARD nterms must be 1..2");
    for (int t = 0; t < k->nterms; ++t)
      for (int d = 0; d < k->dim; ++d) GP2D_REQUIRE(k->ls[t][d] > 0.0, "ARD length scales must be > 0");
  } else {
    set_error("unknown kernel family");
    return -2;
  }
  return 0;
}

// The Ozaki engine's scale bound |K*| ≤ max(1/ℓ_df², 1/ℓ_cf²) and its CRT range check
// (|V| ≤ 4√kss) hold for the mixed kernel only when ratio ∈ [0, 1] (a convex combination of
// the two parts; kss > 0).  GP_laser's free `rate` outside that range is still accepted by the
// FP64 engine; the Ozaki entry points reject it.
static int validate_ozaki_kernel(const gp2d_kernel_t* k) {
  GP2D_CHECK(refuse_sum(k, "ozaki"));   // no K* instantiation, scale bound or error model for sums
  GP2D_CHECK(validate_kernel(k));
  GP2D_REQUIRE(is_vector_family(k), "ozaki: vector families only");
  if (k->kind == GP2D_KIND_MIXED)
    GP2D_REQUIRE(k->ratio >= 0.0 && k->ratio <= 1.0, "ozaki: mixed-kernel ratio must be in [0, 1]");
  return 0;
}

// One cross_cov_kernel launch: `ncols` (a multiple of 64) column points of xb from j_off on, against
// every row point of xa.
template <class Entry>
static int launch_cross_cov(const Entry& e, const double* xa, int64_t na, int64_t na_pad, const double* xb,
                            int64_t nb, int64_t nb_pad, double* out, int64_t ld, int64_t j_off, int64_t ncols,
                            hipStream_t s) {
  const dim3 grid((unsigned)(ncols / 64), (unsigned)((na_pad + ASM_ROWS - 1) / ASM_ROWS));
  cross_cov_kernel<<<grid, 256, 0, s>>>(xa, na, na_pad, xb, nb, nb_pad, e, out, ld, j_off);
  return check_launch("cross_cov_kernel");
}

static int assemble_impl(const double* xa, int64_t na, int64_t na_pad, const double* xb, int64_t nb,
                         int64_t nb_pad, const gp2d_kernel_t* k, double diag_add, int symmetric, double* out,
                         int64_t ld, hipStream_t s) {
  GP2D_CHECK(validate_kernel(k));
  GP2D_REQUIRE(na_pad % PT_TILE == 0 && nb_pad % PT_TILE == 0, "padded point counts must be multiples of 64");
  GP2D_REQUIRE(na <= na_pad && nb <= nb_pad && na >= 0 && nb >= 0, "point counts exceed padded counts");
  if (na_pad == 0 || nb_pad == 0) return 0;
  const int bd = gp2d_block_dim(k);
  GP2D_REQUIRE(ld >= bd * nb_pad, "assemble: ld must be >= block_dim × nb_pad");
  GP2D_REQUIRE(symmetric >= 0 && symmetric <= ASM_LOWER, "symmetric must be 0, 1 or 2");
  GP2D_REQUIRE(symmetric != ASM_LOWER || (bd == 2 && xa == xb && na == nb && na_pad == nb_pad),
               "symmetric = 2 (lower block triangle) needs a vector kernel and xa == xb");
  if (is_sum_family(k))   // its own instantiation: the one-term path stays VecEntry's
    return launch_cross_cov(make_sum_vec_entry(k, diag_add, symmetric, -1), xa, na, na_pad, xb, nb, nb_pad, out, ld,
                            0, nb_pad, s);
  if (bd == 2)
    return launch_cross_cov(VecEntry{make_vec_params(k), diag_add, symmetric, -1}, xa, na, na_pad, xb, nb, nb_pad,
                            out, ld, 0, nb_pad, s);
  return launch_cross_cov(ArdEntry{{}, make_ard_params(k), diag_add, symmetric}, xa, na, na_pad, xb, nb, nb_pad,
                          out, ld, 0, nb_pad, s);
}


// ------------------------------------------------------------- Ozaki constants
// pairwise coprime, largest first (the count a product needs takes the first nmod); the last four
// (primes) are reached only by the guard's widest precisions at large n
static const int kModuli[OZ_MAXMOD] = {256, 255, 253, 251, 247, 241, 239, 233, 229, 227,
                                       223, 217, 211, 199, 197, 193, 191, 181, 179, 173};

// number of moduli for a bound on log2 max|Pint| (one guard bit: Π m_l > 2·max|Pint|)
static int ozaki_nmod_bits(double log2_pmax) {
  const double need = log2_pmax + 2.0;
  double bits = 0.0;
  for (int l = 0; l < OZ_MAXMOD; ++l) {
    bits += std::log2((double)kModuli[l]);
    if (bits > need) return l + 1;
  }
  return -1;
}
// worst case (sizing): |Pint| ≤ n·2^{pW}·2^{pB−1} at the largest W precision the guard can pick
static int ozaki_nmod_for(int64_t n) { return ozaki_nmod_bits(std::log2((double)n) + OZ_PW_MAX + OZ_PB_MAX - 1.0); }
// precisions of a call: 0 → the defaults OZ_PW / OZ_PB; otherwise OZ_PW .. OZ_PW_MAX (W rows)
// and OZ_PB .. OZ_PB_MAX (K*)
static int ozaki_wbits(int wbits) { return wbits == 0 ? OZ_PW : wbits; }
static int ozaki_kbits(int kbits) { return kbits == 0 ? OZ_PB : kbits; }
static int valid_bits(int wbits, int kbits) {
  GP2D_REQUIRE(wbits == 0 || (wbits >= OZ_PW && wbits <= OZ_PW_MAX), "ozaki: wbits must be 0 or 49..60");
  GP2D_REQUIRE(kbits == 0 || (kbits >= OZ_PB && kbits <= OZ_PB_MAX), "ozaki: kbits must be 0 or 45..50");
  return 0;
}

static int64_t modinv(int64_t a, int64_t m) {  // a⁻¹ mod m (a, m coprime)
  int64_t t = 0, nt = 1, r = m, nr = ((a % m) + m) % m;
  while (nr) {
    const int64_t q = r / nr;
    int64_t tmp = t - q * nt; t = nt; nt = tmp;
    tmp = r - q * nr; r = nr; nr = tmp;
  }
  return (t % m + m) % m;
}

static double kstar_bound(const gp2d_kernel_t* k) {
  // |K*| entries: div-free and curl-free parts are each bounded by 1/ℓ² (see ozaki.hpp);
  // the temporal factor of the spatio-temporal product is ≤ var_t
  const double vt = temporal_var(k);
  switch (k->kind) {
    case GP2D_KIND_SCALAR: return vt;
    case GP2D_KIND_DIVFREE: return vt / (k->l_df * k->l_df);
    case GP2D_KIND_CURLFREE: return vt / (k->l_cf * k->l_cf);
    default: return vt * std::max(1.0 / (k->l_df * k->l_df), 1.0 / (k->l_cf * k->l_cf));
  }
}

static int make_ozaki_consts(int nmod, const gp2d_kernel_t* k, OzakiConsts& oc, int pw = OZ_PW, int pb = OZ_PB) {
  oc.nmod = nmod;
  oc.pw = pw;
  oc.pb = pb;
  GP2D_REQUIRE(oc.nmod > 0 && oc.nmod <= OZ_MAXMOD, "ozaki: bad number of moduli");
  double M = 1.0;
  for (int l = 0; l < oc.nmod; ++l) M *= (double)kModuli[l];
  oc.M = M;
  for (int l = 0; l < OZ_MAXMOD; ++l) {
    oc.m[l] = kModuli[l];
    oc.md[l] = (double)kModuli[l];
    oc.inv_m[l] = 1.0 / (double)kModuli[l];
    const int c26 = (int)(((int64_t)1 << OZ_SPLIT) % kModuli[l]);
    oc.c26[l] = (double)(2 * c26 > kModuli[l] ? c26 - kModuli[l] : c26);   // centred
    oc.h[l] = oc.t[l] = 0.0;
  }
  for (int l = 0; l < oc.nmod; ++l) {
    const int64_t ml = kModuli[l];
    int64_t Ml = 1;  // (M / m_l) mod m_l
    for (int q = 0; q < oc.nmod; ++q)
      if (q != l) Ml = (Ml * (kModuli[q] % ml)) % ml;
    const int64_t inv = modinv(Ml, ml);
    const double x = (double)inv / (double)ml;
    const double h = std::ldexp(std::rint(std::ldexp(x, OZ_HBITS)), -OZ_HBITS);
    oc.h[l] = h;
    oc.t[l] = ((double)inv - h * (double)ml) / (double)ml;  // h·m_l is exact (≤ 41 bits)
  }
  const double bmax = kstar_bound(k);
  oc.sB = pb - 1 - (int)std::ceil(std::log2(bmax));
  oc.vlimit = 4.0 * std::sqrt(gp2d_kernel_diag(k));
  return 0;
}

}  // namespace gp2d

using namespace gp2d;

extern "C" {

int gp2d_abi_version(void) { return GP2D_ABI_VERSION; }
const char* gp2d_build_info(void) {
  static const std::string info = "release gfx950 abi=" + std::to_string(GP2D_ABI_VERSION) +
                                  " oz_pw=" + std::to_string(OZ_PW) + " oz_pb=" + std::to_string(OZ_PB) +
                                  " ks_ppl=" + std::to_string(OZ_KS_PPL) + " crt_rpl=" + std::to_string(OZ_CRT_RPL);
  return info.c_str();
}
int64_t gp2d_padded_points(int64_t n) { return round_up(n < 1 ? 1 : n, PT_TILE); }
int gp2d_block_dim(const gp2d_kernel_t* k) { return (k && k->family == GP2D_FAMILY_ARD_RBF) ? 1 : 2; }

double gp2d_kernel_diag(const gp2d_kernel_t* k) {
  if (!k) return 0.0;
  if (is_sum_family(k)) {   // Σ w_t·diag_t, the first term without an add (a one-term sum of weight 1: its term's)
    if (k->nterms < 1 || k->nterms > GP2D_SUM_MAX_TERMS) return 0.0;
    double s = 0.0;
    for (int t = 0; t < k->nterms; ++t) {
      if (is_sum_family(sum_term(k, t))) return 0.0;
      const double d = sum_weight(k, t) * gp2d_kernel_diag(sum_term(k, t));
      s = t ? s + d : d;
    }
    return s;
  }
  if (k->family == GP2D_FAMILY_ARD_RBF) {
    double s = 0.0;
    for (int t = 0; t < k->nterms; ++t) s += k->var[t];
    return s;
  }
  const double vt = temporal_var(k);
  switch (k->kind) {
    case GP2D_KIND_SCALAR: return vt * ((1.0 / k->l_df) * (1.0 / k->l_df) * (k->l_df * k->l_df));
    case GP2D_KIND_DIVFREE: return vt * (1.0 / (k->l_df * k->l_df));
    case GP2D_KIND_CURLFREE: return vt * (1.0 / (k->l_cf * k->l_cf));
    default: return vt * (k->ratio * (1.0 / (k->l_df * k->l_df)) + (1.0 - k->ratio) * (1.0 / (k->l_cf * k->l_cf)));
  }
}

const char* gp2d_last_error(void) { return g_err.c_str(); }

int gp2d_assemble(const double* xa, int64_t na, int64_t na_pad, const double* xb, int64_t nb, int64_t nb_pad,
                  const gp2d_kernel_t* k, double diag_add, int symmetric, double* out, int64_t ld, void* stream) {
  return assemble_impl(xa, na, na_pad, xb, nb, nb_pad, k, diag_add, symmetric, out, ld, S(stream));
}

int gp2d_assemble_cols(const double* x, int64_t n, int64_t n_pad, const gp2d_kernel_t* k, double diag_add,
                       double* out, int64_t ld, int64_t c0, int64_t ncols, void* stream) {
  GP2D_CHECK(validate_kernel(k));
  GP2D_REQUIRE(is_vector_family(k) || is_sum_family(k), "assemble_cols: vector kernel families only");
  GP2D_REQUIRE(n_pad % PT_TILE == 0 && n >= 0 && n <= n_pad, "assemble_cols: bad point counts");
  GP2D_REQUIRE(ld >= 2 * n_pad, "assemble_cols: ld too small");
  GP2D_REQUIRE(c0 >= 0 && ncols >= 0 && c0 % 64 == 0 && ncols % 64 == 0 && c0 + ncols <= 2 * n_pad &&
                   (ncols == 0 || c0 / n_pad == (c0 + ncols - 1) / n_pad),
               "assemble_cols: the column range must be 64-aligned and inside one component");
  if (ncols == 0 || n_pad == 0) return 0;
  const int comp = (int)(c0 / n_pad);
  if (is_sum_family(k))
    return launch_cross_cov(make_sum_vec_entry(k, diag_add, 1, comp), x, n, n_pad, x, n, n_pad, out, ld,
                            c0 - (int64_t)comp * n_pad, ncols, S(stream));
  return launch_cross_cov(VecEntry{make_vec_params(k), diag_add, 1, comp}, x, n, n_pad, x, n, n_pad, out, ld,
                          c0 - (int64_t)comp * n_pad, ncols, S(stream));
}

}  // extern "C"

// ------------------------------------------------------------------------ POTRF
#define GP2D_EV(call) do { if ((call) != hipSuccess) { set_error(#call " failed"); return -1; } } while (0)

namespace {
// POTRF streams (a pool of sets per device, created lazily): `crit` carries the critical path
// (block-column updates, diagonal block, panel TRSM) at the highest priority, `bulk` the
// trailing SYRK, `inv` (low priority) the triangular inverse of the fused factor
// (gp2d_potrf_inv).  (Hardware CU masks splitting the CUs between the streams were measured
// slower at every split)  One factorisation enqueue at a time per set (its
// mutex is held across potrf_impl's enqueue sequence).
enum FactorEvent { EV_PAN, EV_HEAD, EV_JOIN, EV_START, EV_AUX0, EV_AUX1, EV_COUNT };
struct FactorSet {
  std::mutex enqueue;                     // one factorisation enqueue at a time per set
  hipStream_t crit = nullptr, bulk = nullptr, aux = nullptr, inv = nullptr;
  std::vector<hipEvent_t> ev;             // the EV_COUNT fixed events
  std::vector<hipEvent_t> blk;            // one per block column (fused inverse)
};
// per device, up to GP2D_FACTOR_CTX stream sets, of which gp2d_factor_sets(k) puts k in use
// (default 1: every factorisation shares one set, as before the pool).  A caller stream keeps
// the set it was first given (sets dealt in order of first use), so with k > 1
// factorisations enqueued from different caller streams run concurrently on different sets
// — their chains interleave instead of queueing behind each other on one set of in-order
// streams
struct FactorPool {
  std::vector<std::unique_ptr<FactorSet>> sets;
  std::vector<std::pair<hipStream_t, int>> owner;   // caller stream → its set
};
struct FactorStreams { std::mutex mu; std::vector<FactorPool> dev; };   // the pool of each device
constexpr int GP2D_FACTOR_CTX = 4;
FactorStreams g_fs;
std::atomic<int> g_factor_sets{1};   // sets in use (gp2d_factor_sets); 1: every caller shares one
thread_local int t_factor_join = 0;   // gp2d_factor_join: this thread's factorisations join on the host

__global__ void stream_touch_kernel(int) {}

// Sets are created on first use (fewer streams, fewer HW queues shared), and each new stream is
// used at once by an empty kernel: HIP binds a stream to a hardware queue at its first command
// (the least-used queue of its priority once GPU_MAX_HW_QUEUES are taken), so touching the set
// here fixes its queues at creation, not at whatever point of the caller's stream use the first
// factorisation falls (gp2d_factor_warm, DESIGN.md §6 "bench state").  Caller holds g_fs.mu.
int ensure_factor_sets(std::vector<std::unique_ptr<FactorSet>>& sets, int count) {
  while ((int)sets.size() < count) {
    int lo = 0, hi = 0;
    if (hipDeviceGetStreamPriorityRange(&lo, &hi) != hipSuccess) { lo = 0; hi = 0; }
    auto f = std::make_unique<FactorSet>();
    // crit (diagonal kernels, skinny panel GEMMs) and aux at the highest priority, bulk (the
    // trailing SYRK) and inv (the fused inverse's GEMMs) at the lowest.  Keeping CUs free of
    // the bulk stream (CU-masked streams) was measured slower.
    if (hipStreamCreateWithPriority(&f->crit, hipStreamNonBlocking, hi) != hipSuccess ||
        hipStreamCreateWithPriority(&f->bulk, hipStreamNonBlocking, lo) != hipSuccess ||
        hipStreamCreateWithPriority(&f->aux, hipStreamNonBlocking, hi) != hipSuccess ||
        hipStreamCreateWithPriority(&f->inv, hipStreamNonBlocking, lo) != hipSuccess) {
      set_error("hipStreamCreate failed"); return -1;
    }
    for (hipStream_t st : {f->crit, f->bulk, f->aux, f->inv}) {
      stream_touch_kernel<<<1, 64, 0, st>>>(0);
      if (check_launch("stream_touch_kernel") != 0) return -1;
    }
    f->ev.resize(EV_COUNT);
    for (auto& e : f->ev)
      if (hipEventCreateWithFlags(&e, hipEventDisableTiming) != hipSuccess) { set_error("hipEventCreate failed"); return -1; }
    sets.push_back(std::move(f));
  }
  return 0;
}

// this device's pool, grown to fit (NULL: no device).  Caller holds g_fs.mu.
FactorPool* device_pool() {
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) { set_error("factor: no HIP device"); return nullptr; }
  if ((int)g_fs.dev.size() <= dev) g_fs.dev.resize(dev + 1);
  return &g_fs.dev[dev];
}
int factor_sets_in_use() { return std::max(1, std::min(GP2D_FACTOR_CTX, g_factor_sets.load())); }

// The set of a factorisation enqueued from `caller`, with nblk block-column events: a known
// stream keeps its set while that set is in use; a new one (or one whose set is no longer in
// use) gets the next set in turn, remembered for up to 256 streams.
FactorSet* factor_streams(int nblk, hipStream_t caller) {
  std::lock_guard<std::mutex> lk(g_fs.mu);
  FactorPool* pool = device_pool();
  if (!pool) return nullptr;
  const int want = factor_sets_in_use();
  int used = 0;
  std::pair<hipStream_t, int>* mine = nullptr;
  for (auto& pr : pool->owner) {
    used += pr.second < want;
    if (pr.first == caller) mine = &pr;
  }
  int idx = mine ? mine->second : -1;
  if (idx < 0 || idx >= want) {
    idx = used % want;
    if (mine) mine->second = idx;
    else if (pool->owner.size() < 256) pool->owner.emplace_back(caller, idx);
  }
  if (ensure_factor_sets(pool->sets, idx + 1) != 0) return nullptr;
  FactorSet& f = *pool->sets[idx];
  while ((int)f.blk.size() < nblk) {
    hipEvent_t e;
    if (hipEventCreateWithFlags(&e, hipEventDisableTiming) != hipSuccess) { set_error("hipEventCreate failed"); return nullptr; }
    f.blk.push_back(e);
  }
  return &f;
}

// The two skinny K = 128 launches of a right-looking factorisation of the order-n matrix at A;
// nprob problems at A + q·sA with their diagonal inverses at dinv + q·sD (problem batch).
// In-place panel TRSM below diagonal block k:  L21 = A21 · inv(L11)ᵀ
int launch_panel(double* A, int64_t lda, int64_t n, int k, const double* dinv, hipStream_t s, int nprob = 1,
                 int64_t sA = 0, int64_t sD = 0) {
  const int k0 = k * NB;
  const int rows = (int)(n - k0 - NB);
  if (rows <= 0) return 0;
  double* P = A + (int64_t)(k0 + NB) * lda + k0;
  gemm_f64_panel_kernel<PNL_TRSM_R, PNL_TRSM_CB><<<dim3((unsigned)(rows / PNL_TRSM_R), (unsigned)nprob, 1), 256, 0, s>>>(
      P, lda, dinv + (int64_t)k * NB * NB, NB, P, lda, 1.0, 0.0, sA, sD, sA);
  return check_launch("gemm_f64_panel_kernel");
}
// A[j.., j] −= L[j.., p] · L[j, p]ᵀ: block column j receives panel p (B = the NB rows of block
// j of the panel)
int launch_colupdate(double* A, int64_t lda, int64_t n, int j, int p, hipStream_t s, int nprob = 1, int64_t sA = 0) {
  const int64_t j0 = (int64_t)j * NB;
  const double* Lp = A + j0 * lda + (int64_t)p * NB;
  gemm_f64_panel_kernel<PNL_UPD_R, PNL_UPD_CB>
      <<<dim3((unsigned)((n - j0) / PNL_UPD_R), (unsigned)nprob, NB / PNL_UPD_CB), 256, 0, s>>>(
          Lp, lda, Lp, lda, A + j0 * lda + j0, lda, -1.0, 1.0, sA, sA, sA);
  return check_launch("gemm_f64_panel_kernel");
}

// ---- TRTRI by recursive doubling over 128-blocks (in place; the diagonal blocks already hold
// W_kk = L_kk⁻¹; pairs, K-split rule and buffer sizes in factor_host.hpp): one batched launch
// per level and product.
//
// The products are triangular in K (T's column block j needs k ≥ j, W21's row block i k ≤ i),
// so a launch that is a single round of workgroups lasts as long as its longest tile, twice the
// average: the lower levels ran at 25–33 TF/s.  In a product with at most 256
// tiles per pair and K ≥ 512, every tile longer than 256 is cut at its middle (GemmParams::
// ksplit): the low halves go to the destination, the high halves to T2, then add_into_kernel
// sums them.  The decision depends on the product's shape only, so every caller (gp2d_trtri, both
// halves of the fused inverse) sums each product in the same order.
//
// One product of the level-g pairs `pr` of the matrix at A, K-split and summed where the shape
// asks for it:  which = 0:  T = L[R, L] · W[L, L]   (rh × bw; W[L, L] bw × bw lower),
//               which = 1:  W[R, L] = −W[R, R] · T  (W[R, R] rh × rh lower).
// Problem batch: nprob problems at A + q·sA, each with its own T (+ q·pT) and T2 (+ q·pT2);
// every problem's products are the lone launch's (the same tiles, K ranges and split sums).
int trtri_product(int which, double* A, int64_t lda, int g, const TrtriPair& pr, double* T, double* T2, hipStream_t s,
                  int nprob = 1, int64_t sA = 0, int64_t pT = 0, int64_t pT2 = 0) {
  const int64_t Lo = (int64_t)pr.Ls * NB, Ro = (int64_t)pr.Rs * NB;
  const int bw = g * NB, rh = pr.Rn * NB;
  const int64_t stride = (int64_t)2 * g * NB * (lda + 1);   // next pair's diagonal offset
  const int64_t tstride = (int64_t)rh * bw;                  // next pair's T
  double* RL = A + Ro * lda + Lo;
  GemmParams p = gemm_params();
  if (which == 0) {
    p.A = RL; p.lda = lda; p.sA = stride; p.pA = sA;
    p.B = A + Lo * lda + Lo; p.ldb = lda; p.sB = stride; p.pB = sA;
    p.C = T; p.ldc = bw; p.sC = tstride; p.pC = pT;
    p.M = rh; p.N = bw; p.K = bw; p.b_lower = 1;
    p.cols_first = 1;   // column block j needs k ≥ j: long-K tiles first
    p.ksplit = trtri_ksplit(g, pr.Rn);
  } else {
    p.A = A + Ro * lda + Ro; p.lda = lda; p.sA = stride; p.pA = sA;
    p.B = T; p.ldb = bw; p.sB = tstride; p.pB = pT;
    p.C = RL; p.ldc = lda; p.sC = stride; p.pC = sA;
    p.M = rh; p.N = bw; p.K = rh; p.a_lower = 1; p.alpha = -1.0;
    p.rev_rows = 1;     // row block i needs k ≤ i: long-K tiles first
    p.ksplit = trtri_ksplit(pr.Rn, g);
  }
  p.pC2 = pT2;
  if (p.ksplit) { p.zcnt = pr.count; p.C2 = T2; p.ldc2 = bw; p.sC2 = tstride; }
  GP2D_CHECK((launch_gemm<false, EPI_STORE>(p, pr.count, s, nprob)));
  if (!p.ksplit) return 0;
  add_into_kernel<<<dim3((unsigned)((bw + 511) / 512), (unsigned)rh, (unsigned)(pr.count * nprob)), 256, 0, s>>>(
      p.C, p.ldc, p.sC, T2, bw, tstride, rh, bw, pr.count, p.pC, pT2);
  return check_launch("add_into_kernel");
}

int trtri_levels(double* A, int64_t lda, int nbk, double* T, double* T2, hipStream_t s, int nprob = 1,
                 int64_t sA = 0, int64_t pT = 0, int64_t pT2 = 0) {
  for (int g = 1; g < nbk; g *= 2)
    for (const TrtriPair& pr : trtri_level_pairs(nbk, g))
      for (int which = 0; which < 2; ++which)
        GP2D_CHECK(trtri_product(which, A, lda, g, pr, T, T2, s, nprob, sA, pT, pT2));
  return 0;
}

// Trailing-update schedule of potrf_impl: G panels per SYRK (K = 128·G) and whether the SYRK
// is split into the next group's head and the rest.  Measured (profiles/r04_potrf_sched_ab*.jsonl,
// engine.fit at N_train = 1024 … 16384): four panels with the split tie the pairs where the fit
// is chain-bound (N ≤ 4096: 2.2 / 4.8 / 13.4 ms) and win where the SYRK dominates (N = 8192:
// 61.2 vs 63.9 ms; config D: 399 vs 417 ms); eight panels (K = 1024) gain nothing over four.
// GP2D_POTRF_G (2 | 4 | 8) / GP2D_POTRF_SPLIT override the choice (measurement only).
struct PotrfSchedule { int G; bool split; };
PotrfSchedule potrf_schedule() {
  PotrfSchedule ps{4, true};
  static const char* eg = std::getenv("GP2D_POTRF_G");
  static const char* es = std::getenv("GP2D_POTRF_SPLIT");
  if (eg && (std::atoi(eg) == 2 || std::atoi(eg) == 4 || std::atoi(eg) == 8)) ps.G = std::atoi(eg);
  if (es) ps.split = std::atoi(es) != 0;
  return ps;
}

// nprob SPD matrices of order n at A + q·sA (one: sA = 0)
struct PotrfJob { double* A; int64_t n, lda; int nprob; int64_t sA; };

// The trailing update of group P..P+g−1, enqueued once panel P+g−1 is factored on crit:
//   bulk: once panel P+g−1 is final, columns ≥ P+g+1 ← panels P..P+g−1 in ONE K = 128·g SYRK —
//         g = 2 halves the launches and the C read-modify-write traffic per flop of K = 128
//         updates; g = 4 again (the tile runs 58 vs 51 TF/s at K = 512 than at 256, m = 32640,
//         profiles/r03_syrk_k512_ab.txt) — split (`split`) into a head, the next group's g
//         block columns, and the rest, so the next group's prefix (the chain of g−1 diagonal
//         blocks, during which the chip would otherwise idle) waits for the head only and runs
//         beside the rest.
// Regions: crit/aux write block columns ≤ P+g, the head columns P+g+1..P+2g, the rest the
// columns beyond; bulk is in order, so the rest of group q precedes the head of group q+1,
// which covers columns it also updates.  EV_HEAD is the head's event (the whole SYRK's when
// unsplit, or when nothing is left to update); the rest needs no event of its own.
int potrf_trailing_update(const PotrfJob& m, int P, int g, const PotrfSchedule& ps, FactorSet& f) {
  GP2D_EV(hipEventRecord(f.ev[EV_PAN], f.crit));
  GP2D_EV(hipStreamWaitEvent(f.bulk, f.ev[EV_PAN], 0));
  const int64_t n = m.n, lda = m.lda;
  const int64_t f0 = (int64_t)(P + g + 1) * NB;
  const int hw = (ps.split && f0 < n) ? std::min<int>(g, (int)((n - f0) / NB)) : 0;   // head block columns
  GemmParams q = gemm_params();
  q.lda = lda; q.ldb = lda; q.ldc = lda;
  q.K = g * NB; q.alpha = -1.0; q.beta = 1.0;
  q.pA = q.pB = q.pC = m.sA;
  auto from = [&](int64_t c0) {   // the update of every row from c0 on, columns from c0 on
    q.A = q.B = m.A + c0 * lda + (int64_t)P * NB;
    q.C = m.A + c0 * lda + c0;
    q.M = (int)(n - c0);
  };
  if (hw > 0) {   // head: block columns [P+g+1, P+g+1+hw), every row below, lower tiles
    from(f0);
    q.N = hw * NB; q.cyc_lower = 1; q.mask_off = 0;
    GP2D_CHECK((launch_gemm<true, EPI_STORE>(q, 1, f.bulk, m.nprob)));
    GP2D_EV(hipEventRecord(f.ev[EV_HEAD], f.bulk));
    q.cyc_lower = 0;
  }
  const int64_t f1 = f0 + (int64_t)hw * NB;
  if (f1 < n) {   // the rest (or, unsplit, the whole trailing matrix): lower tiles
    from(f1);
    q.N = q.M; q.c_lower = 1;
    GP2D_CHECK((launch_gemm<true, EPI_STORE>(q, 1, f.bulk, m.nprob)));
  }
  if (hw == 0) GP2D_EV(hipEventRecord(f.ev[EV_HEAD], f.bulk));
  return 0;
}

// The fused inverse splits the top level of the recursive doubling at h (inv_top_split): once
// block column h−1 is factored, W[0:h, 0:h] (every lower level inside the left half) and the
// top product T = L[h:, 0:h]·W11 depend on final data only, so they run on `inv` under the
// second half of the factorisation; after the last block only W22 = L22⁻¹ and W21 = −W22·T
// remain.  The same products (trtri_product) on the same operands as trtri_levels over all nb
// blocks, so the result is bit-identical to gp2d_potrf + gp2d_trtri.
// left half final (block column h−1 factored on crit): W11 and T = L21·W11 under the rest
int potrf_inv_left_half(const PotrfJob& m, int h, const PotrfInvWork::Ptrs& w, FactorSet& f) {
  GP2D_EV(hipEventRecord(f.blk[0], f.crit));
  GP2D_EV(hipStreamWaitEvent(f.inv, f.blk[0], 0));
  GP2D_CHECK(trtri_levels(m.A, m.lda, h, w.T1, w.T3, f.inv));
  return trtri_product(0, m.A, m.lda, h, {0, h, (int)(m.n / NB) - h, 1}, w.T2, w.T3, f.inv);
}
// after the last block (crit has joined bulk): W22 = L22⁻¹ (its lower levels) and the top
// level's W21 = −W22·T; crit then waits for `inv`
int potrf_inv_finish(const PotrfJob& m, int h, const PotrfInvWork::Ptrs& w, FactorSet& f) {
  const int nb = (int)(m.n / NB);
  GP2D_EV(hipEventRecord(f.ev[EV_JOIN], f.crit));
  GP2D_EV(hipStreamWaitEvent(f.inv, f.ev[EV_JOIN], 0));
  GP2D_CHECK(trtri_levels(m.A + (int64_t)h * NB * (m.lda + 1), m.lda, nb - h, w.T1, w.T3, f.inv));
  GP2D_CHECK(trtri_product(1, m.A, m.lda, h, {0, h, nb - h, 1}, w.T2, w.T3, f.inv));
  GP2D_EV(hipEventRecord(f.ev[EV_JOIN], f.inv));
  GP2D_EV(hipStreamWaitEvent(f.crit, f.ev[EV_JOIN], 0));
  return 0;
}

// Right-looking blocked Cholesky (NB = 128) with look-ahead on internal streams and the
// trailing update delayed over pairs of panels:
//   crit: for pair (k, k+1): block column k+1 ← panel k, factor k+1; block column k+2 ←
//         panels k and k+1, factor k+2 (diagonal block + panel TRSM each),
//   bulk: SYRK of columns ≥ k+3 with both panels (K = 256),
// so the single-workgroup diagonal kernel hides under the chip-wide SYRK.  Data regions are
// disjoint (block columns k+1, k+2 vs ≥ k+3); bulk waits for panel k+1, crit waits for the
// pair's SYRK before it updates block column k+3.  The caller's stream is joined at both ends.
// With `fused` the factor is inverted in place on the way (gp2d_potrf_inv; workspace pointers
// in `w`, unused for a single block): the diagonal kernels store W_kk, the left half of the
// inverse and the top-level product T = L21·W11 run on `inv` under the second half of the
// factorisation, W22 and W21 after it.
// Problem batch (nprob > 1, gp2d_potrf_batched): nprob SPD matrices at A + q·sA, their
// diagonal inverses at dinv + q·n·128, info_dev[q]; every launch below carries all problems
// (workgroups per problem: the diagonal kernel's one, the panel GEMMs' grid.y, the SYRK's and
// zeroing's grid.z), so the chain's latency is paid once for the batch and each problem's
// arithmetic is that of a lone factorisation, bit for bit.
int potrf_impl(double* A, int64_t n, int64_t lda, double* dinv, int* info_dev, hipStream_t s, bool fused,
               const PotrfInvWork::Ptrs& w = {}, int nprob = 1, int64_t sA = 0) {
  GP2D_REQUIRE(n % NB == 0 && n > 0, "potrf: n must be a positive multiple of 128");
  GP2D_REQUIRE(lda >= n && lda % 2 == 0, "potrf: lda must be >= n and even");
  GP2D_REQUIRE(dinv != nullptr, "potrf: dinv buffer is required");
  GP2D_REQUIRE(nprob >= 1 && (nprob == 1 || (!fused && sA >= n * lda)), "potrf: bad problem batch");
  GP2D_REQUIRE(aligned16(A), "potrf: A must be 16-byte aligned");
  const PotrfJob m{A, n, lda, nprob, sA};
  const int64_t sD = n * NB;   // one problem's diagonal inverses
  const int nb = (int)(n / NB);
  const int h = fused ? inv_top_split(nb) : 0;
  FactorSet* fs = factor_streams(fused ? 1 : 0, s);
  if (!fs) return -1;
  FactorSet& f = *fs;
  // a set's streams and events are shared by every factorisation that draws it: two host
  // threads on one set would interleave their records and waits, so its enqueue is serialised
  std::lock_guard<std::mutex> enqueue_lock(f.enqueue);
  hipStream_t sc = f.crit, sb = f.bulk, sa = f.aux;
  hipEvent_t e_join = f.ev[EV_JOIN], e_start = f.ev[EV_START];
  hipEvent_t e_auxc[2] = {f.ev[EV_AUX0], f.ev[EV_AUX1]};   // aux's first update of an even / odd block column
  if (info_dev) GP2D_EV(hipMemsetAsync(info_dev, 0, sizeof(int) * (size_t)nprob, s));   // the call resets info
  GP2D_EV(hipEventRecord(e_join, s));
  GP2D_EV(hipStreamWaitEvent(sc, e_join, 0));
  GP2D_EV(hipStreamWaitEvent(sb, e_join, 0));
  if (fused) GP2D_EV(hipStreamWaitEvent(f.inv, e_join, 0));
  // diagonal block j (Cholesky + inverse) and its panel TRSM; then (fused) the inverse's
  // GEMMs whose inputs block column j completes
  auto factor = [&](int j) -> int {
    potrf_diag_kernel<<<nprob, 256, 0, sc>>>(A, lda, j * NB, dinv, info_dev, fused ? 1 : 0, sA, sD);
    GP2D_CHECK(check_launch("potrf_diag_kernel"));
    GP2D_CHECK(launch_panel(A, lda, n, j, dinv, sc, nprob, sA, sD));
    if (fused && nb > 1 && j == h - 1) GP2D_CHECK(potrf_inv_left_half(m, h, w, f));
    return 0;
  };
  GP2D_CHECK(factor(0));
  // Delayed trailing updates over groups of G panels (potrf_schedule: G = 4 with a head/rest
  // split; G = 2 unsplit is the round-3 schedule).  Group q = panels P..P+g−1 (panel P factored on entry;
  // block columns P+1..P+g hold every panel < P):
  //   crit  prefix: for r = P..P+g−1: block column r+1 ← panel r (skinny K = 128 update), then
  //         factor(r+1) — the last one, block column P+g, is the next group's first panel and is
  //         factored while the group's SYRK runs (one-column look-ahead);
  //   aux:  as soon as panel r is final, block columns r+2..P+g ← panel r, so each column's
  //         older panels arrive under the diagonal kernel of its predecessor (same-column
  //         updates are ordered: crit waits for aux's last update of a column before its own);
  //   bulk: the group's trailing update (potrf_trailing_update).
  const PotrfSchedule ps = potrf_schedule();
  int P = 0;
  while (P + 1 < nb) {
    const int g = std::min(ps.G, nb - 1 - P);   // panels P..P+g−1, look-ahead column P+g ≤ nb−1
    for (int r = P; r < P + g; ++r) {
      // panel r is final (factored on crit; for r = P after the previous group's head / SYRK
      // reached columns P+1..P+g, which crit waited for)
      GP2D_EV(hipEventRecord(e_start, sc));
      if (r + 2 <= P + g) {   // aux: columns r+2.., the next one first (crit waits for it at r+1)
        GP2D_EV(hipStreamWaitEvent(sa, e_start, 0));
        for (int c = r + 2; c <= P + g; ++c) {
          GP2D_CHECK(launch_colupdate(A, lda, n, c, r, sa, nprob, sA));
          if (c == r + 2) GP2D_EV(hipEventRecord(e_auxc[c & 1], sa));
        }
      }
      if (r == P + g - 1) GP2D_CHECK(potrf_trailing_update(m, P, g, ps, f));   // the group's panels are final
      // block column r+1 ≥ P+2 received panels P..r−1 on aux (the last of them recorded as the
      // first update of batch r−1); the same-column updates must not overlap
      if (r > P) GP2D_EV(hipStreamWaitEvent(sc, e_auxc[(r + 1) & 1], 0));
      GP2D_CHECK(launch_colupdate(A, lda, n, r + 1, r, sc, nprob, sA));
      GP2D_CHECK(factor(r + 1));
    }
    // the next group's columns P+g+1..P+2g must have received this group's head (the whole
    // SYRK when unsplit) before crit or aux update them
    GP2D_EV(hipStreamWaitEvent(sc, f.ev[EV_HEAD], 0));
    P += g;
  }
  GP2D_EV(hipEventRecord(e_join, sb));
  GP2D_EV(hipStreamWaitEvent(sc, e_join, 0));
  if (fused && nb > 1) GP2D_CHECK(potrf_inv_finish(m, h, w, f));
  GP2D_EV(hipEventRecord(e_join, sc));
  // The caller's wait below stays pending for the whole chain.  A pending wait on a hardware
  // queue that the CP services beside crit's, aux's or bulk's slows the chain's dispatches:
  // a 4096-point fit took 13.4 ms with the caller on the null stream and 15.8–19 ms on
  // torch's pool streams (tools/probe_single_job.py, profiles/r03_caller_join.txt).  With
  // gp2d_factor_join(1) the host waits for the chain first, so the wait is enqueued complete.
  if (t_factor_join) GP2D_EV(hipEventSynchronize(e_join));
  GP2D_EV(hipStreamWaitEvent(s, e_join, 0));
  dim3 zg((unsigned)((n / 2 + 255) / 256), (unsigned)n, (unsigned)nprob);
  zero_upper_kernel<<<zg, 256, 0, s>>>(A, n, lda, sA);
  return check_launch("zero_upper_kernel");
}
}  // namespace

extern "C" {
size_t gp2d_potrf_workspace(int64_t) { return 0; }

int gp2d_factor_sets(int k) {
  const int prev = g_factor_sets.load();
  if (k >= 1) {
    std::lock_guard<std::mutex> lk(g_fs.mu);
    g_factor_sets.store(std::min(k, GP2D_FACTOR_CTX));
    // a new batch of concurrent factorisations: forget which caller stream had which set, so
    // the next k caller streams are dealt sets 0..k−1 in order of first use (torch's stream
    // pools hand the same streams out again; a remembered mapping could put two streams of
    // one batch on the same set, where their chains would queue behind each other)
    if (k > 1)
      for (FactorPool& pool : g_fs.dev) pool.owner.clear();
  }
  return prev;
}

int gp2d_factor_warm(int nsets, void* stream) {
  GP2D_REQUIRE(nsets >= 1 && nsets <= GP2D_FACTOR_CTX, "factor_warm: nsets must be 1..4");
  std::lock_guard<std::mutex> lk(g_fs.mu);
  FactorPool* pool = device_pool();
  if (!pool) return -1;
  // the caller's stream first (the predict stream of a job stream): then the factor sets
  stream_touch_kernel<<<1, 64, 0, S(stream)>>>(0);
  GP2D_CHECK(check_launch("stream_touch_kernel"));
  return ensure_factor_sets(pool->sets, nsets);
}

int gp2d_factor_set_of(void* stream) {
  std::lock_guard<std::mutex> lk(g_fs.mu);
  FactorPool* pool = device_pool();
  if (!pool) return -1;
  for (const auto& pr : pool->owner)
    if (pr.first == S(stream)) return pr.second < factor_sets_in_use() ? pr.second : -1;
  return -1;
}

int gp2d_factor_join(int host) {
  const int prev = t_factor_join;
  if (host >= 0) t_factor_join = host != 0;
  return prev;
}

int gp2d_potrf(double* A, int64_t n, int64_t lda, double* dinv, int* info_dev, void*, size_t, void* stream) {
  return potrf_impl(A, n, lda, dinv, info_dev, S(stream), false);
}

size_t gp2d_potrf_inv_workspace(int64_t n) { return PotrfInvWork(n).total; }

int gp2d_potrf_inv(double* A, int64_t n, int64_t lda, double* dinv, int* info_dev, void* work, size_t work_bytes,
                   void* stream) {
  GP2D_REQUIRE(n % NB == 0 && n > 0, "potrf_inv: n must be a positive multiple of 128");
  if (n == NB) return potrf_impl(A, n, lda, dinv, info_dev, S(stream), true);   // no inverse GEMMs: W = dinv
  const PotrfInvWork w(n);
  GP2D_REQUIRE(work != nullptr && work_bytes >= w.total, "potrf_inv: workspace too small");
  return potrf_impl(A, n, lda, dinv, info_dev, S(stream), true, w.at(work));
}

// ------------------------------------------------------------------------ TRTRI
// T buffers of the widest level (+ dinv if not supplied, + the high halves of the K-split products)
size_t gp2d_trtri_workspace(int64_t n) { return TrtriWork(n, 1, true).total; }

int gp2d_trtri(double* A, int64_t n, int64_t lda, const double* dinv, void* work, size_t work_bytes, void* stream) {
  GP2D_REQUIRE(n % NB == 0 && n > 0, "trtri: n must be a positive multiple of 128");
  GP2D_REQUIRE(ld_even(lda, n), "trtri: lda must be >= n and even");
  const TrtriWork lay(n, 1, true);
  GP2D_REQUIRE(work != nullptr && work_bytes >= lay.total, "trtri: workspace too small");
  GP2D_REQUIRE(aligned16(A), "trtri: A must be 16-byte aligned");
  hipStream_t s = S(stream);
  const int nb = (int)(n / NB);
  const TrtriWork::Ptrs w = lay.at(work);
  if (!dinv) {
    trti2_diag_kernel<<<nb, 256, 0, s>>>(A, lda, w.dinv);
    GP2D_CHECK(check_launch("trti2_diag_kernel"));
    dinv = w.dinv;
  }
  put_diag_blocks_kernel<<<dim3(NB * NB / 256, nb), 256, 0, s>>>(A, lda, dinv);
  GP2D_CHECK(check_launch("put_diag_blocks_kernel"));
  return trtri_levels(A, lda, nb, w.T, w.T2, s);
}

// ------------------------------------------------------------------------ batched factor
// nprob independent fits of one size in one chain (a hyperparameter sweep's settings, a job
// stream's next jobs): problem q's matrix at A + q·sA, its diagonal inverses at dinv + q·n·128,
// its info word at info_dev[q].  Each problem's results are those of gp2d_potrf / gp2d_trtri
// alone, bit for bit (tests/test_gpu_batched.py).
int gp2d_potrf_batched(double* A, int64_t n, int64_t lda, int64_t sA, int nprob, double* dinv, int* info_dev,
                       void* stream) {
  GP2D_REQUIRE(nprob >= 1 && nprob <= 64, "potrf_batched: nprob must be 1..64");
  GP2D_REQUIRE(nprob == 1 || (sA >= n * lda && sA % 2 == 0), "potrf_batched: sA must be >= n·lda and even");
  return potrf_impl(A, n, lda, dinv, info_dev, S(stream), false, {}, nprob, nprob > 1 ? sA : 0);
}

size_t gp2d_trtri_batched_workspace(int64_t n, int nprob) { return TrtriWork(n, nprob, false).total; }

int gp2d_trtri_batched(double* A, int64_t n, int64_t lda, int64_t sA, int nprob, const double* dinv, void* work,
                       size_t work_bytes, void* stream) {
  GP2D_REQUIRE(n % NB == 0 && n > 0, "trtri_batched: n must be a positive multiple of 128");
  GP2D_REQUIRE(nprob >= 1 && nprob <= 64, "trtri_batched: nprob must be 1..64");
  GP2D_REQUIRE(ld_even(lda, n), "trtri_batched: lda must be >= n and even");
  GP2D_REQUIRE(nprob == 1 || (sA >= n * lda && sA % 2 == 0), "trtri_batched: sA must be >= n·lda and even");
  GP2D_REQUIRE(dinv != nullptr, "trtri_batched: dinv (from gp2d_potrf_batched) is required");
  const TrtriWork lay(n, nprob, false);
  GP2D_REQUIRE(work != nullptr && work_bytes >= lay.total, "trtri_batched: workspace too small");
  GP2D_REQUIRE(aligned16(A), "trtri_batched: A must be 16-byte aligned");
  hipStream_t s = S(stream);
  const int nb = (int)(n / NB);
  const TrtriWork::Ptrs w = lay.at(work);
  put_diag_blocks_kernel<<<dim3(NB * NB / 256, nb, nprob), 256, 0, s>>>(A, lda, dinv, nprob > 1 ? sA : 0, n * NB);
  GP2D_CHECK(check_launch("put_diag_blocks_kernel"));
  return trtri_levels(A, lda, nb, w.T, w.T2, s, nprob, nprob > 1 ? sA : 0, lay.pT, lay.pT2);
}

// ------------------------------------------------------------------------ distributed factor
// One job's POTRF + TRTRI over P ranks (dfact.hpp): 512-column super-blocks dealt block-
// cyclically, a panel broadcast per step by the caller.  Every GEMM below is gemm_f64_kernel;
// the per-element arithmetic does not depend on P (each tile sums the same K range in the same
// order), so any P gives the bits of P = 1.
int gp2d_dfact_sb(void) { return DF_SB; }

size_t gp2d_dfact_panel_doubles(int64_t n) { return (size_t)(n > 0 ? n : 0) * DF_SB; }

size_t gp2d_dfact_workspace(int64_t n) { return DfactWork(n).total; }   // layout: factor_host.hpp

static int dfact_args(const double* A, int64_t n, int64_t lda, int s, bool w = false) {
  GP2D_REQUIRE(A != nullptr, "dfact: NULL matrix");
  GP2D_REQUIRE(n > 0 && n % DF_SB == 0, "dfact: n must be a positive multiple of 512");
  GP2D_REQUIRE(n <= INT32_MAX && ld_even(lda, n),   // the parameter is ldw in the W-reading entries
               w ? "dfact: ldw must be >= n and even" : "dfact: lda must be >= n and even");
  GP2D_REQUIRE(s >= 0 && (int64_t)s * DF_SB < n, "dfact: super-block index out of range");
  return 0;
}

// Owner's step: super-column s (rows s·512..n) factored on ONE stream, a right-looking
// Cholesky over its four 128-wide sub-columns — diagonal block j (Cholesky + inverse D_j),
// its panel TRSM down to row n, the updates of sub-columns j+1..3 by sub-column j — then
// copied into the panel buffer with its 512×512 head replaced by D_s = L_ss⁻¹ (the diagonal
// blocks D_j put in, the off-diagonal blocks by the in-place recursive-doubling TRTRI on the
// head).  Receivers apply D_s in one K = 512 product (gp2d_dfact_invstep).
int gp2d_dfact_panel(double* A, int64_t n, int64_t lda, int s, double* panel, int* info_dev, void* work,
                     size_t work_bytes, void* stream) {
  GP2D_CHECK(dfact_args(A, n, lda, s));
  GP2D_REQUIRE(panel != nullptr && info_dev != nullptr, "dfact_panel: NULL panel or info");
  const DfactWork lay(n);
  GP2D_REQUIRE(work != nullptr && work_bytes >= lay.total, "dfact_panel: workspace too small");
  GP2D_REQUIRE(aligned16(A) && aligned16(panel), "dfact_panel: A and panel must be 16-byte aligned");
  hipStream_t st = S(stream);
  const int64_t s0 = (int64_t)s * DF_SB;
  double* As = A + s0 * lda + s0;                  // the super-column from its diagonal down
  const int64_t rows = n - s0;                     // ≥ 512
  const DfactWork::Ptrs w = lay.at(work);          // w.dinv: [DF_SBT][128][128]
  GP2D_EV(hipMemsetAsync(w.status, 0, sizeof(int), st));
  for (int j = 0; j < DF_SBT; ++j) {
    potrf_diag_kernel<<<1, 256, 0, st>>>(As, lda, j * NB, w.dinv, w.status, 0);
    GP2D_CHECK(check_launch("potrf_diag_kernel"));
    GP2D_CHECK(launch_panel(As, lda, rows, j, w.dinv, st));   // sub-column j below its diagonal block
    for (int j2 = j + 1; j2 < DF_SBT; ++j2)        // sub-column j2 (rows ≥ its diagonal) −= L_j · L_j[j2 rows]ᵀ
      GP2D_CHECK(launch_colupdate(As, lda, rows, j2, j, st));
  }
  dfact_info_kernel<<<1, 64, 0, st>>>(info_dev, w.status, s0);
  GP2D_CHECK(check_launch("dfact_info_kernel"));
  GP2D_EV(hipMemcpy2DAsync(panel, DF_SB * sizeof(double), As, lda * sizeof(double), DF_SB * sizeof(double), rows,
                           hipMemcpyDeviceToDevice, st));
  // head: D_j on the diagonal, then W[R, L] = −W[R, R]·(L[R, L]·W[L, L]) level by level
  put_diag_blocks_kernel<<<dim3(NB * NB / 256, DF_SBT), 256, 0, st>>>(panel, DF_SB, w.dinv);
  GP2D_CHECK(check_launch("put_diag_blocks_kernel"));
  return trtri_levels(panel, DF_SB, DF_SBT, w.T, w.T2, st);
}

// first owned super-column ≥ t (rank r of P), and how many owned ones lie in [t, t_hi)
static void dfact_owned(int t, int t_hi, int P, int r, int& first, int& count) {
  first = t + ((r - t) % P + P) % P;
  count = first < t_hi ? (t_hi - 1 - first) / P + 1 : 0;
}

int gp2d_dfact_update(double* A, int64_t n, int64_t lda, int s, const double* panel, int nranks, int rank,
                      int t_lo, int t_hi, void* stream) {
  GP2D_CHECK(dfact_args(A, n, lda, s));
  GP2D_REQUIRE(panel != nullptr, "dfact_update: NULL panel");
  GP2D_REQUIRE(nranks >= 1 && rank >= 0 && rank < nranks, "dfact_update: bad rank / world size");
  const int nsb = (int)(n / DF_SB);
  int first, count;
  dfact_owned(std::max(t_lo, s + 1), std::min(t_hi, nsb), nranks, rank, first, count);
  if (count == 0) return 0;
  GP2D_REQUIRE(aligned16(A) && aligned16(panel), "dfact_update: A and panel must be 16-byte aligned");
  // A[rows ≥ t·512, t] −= L21[t rows..] · L21[t block]ᵀ for the owned t, lower tiles only (K = 512)
  const int64_t r0 = (int64_t)(s + 1) * DF_SB;
  const double* L21 = panel + (int64_t)DF_SB * DF_SB;   // global row r0 + i at panel row i
  GemmParams q = gemm_params();
  q.A = L21; q.lda = DF_SB;
  q.B = L21 + ((int64_t)first * DF_SB - r0) * DF_SB; q.ldb = DF_SB;
  q.C = A + r0 * lda + (int64_t)first * DF_SB; q.ldc = lda;
  q.M = (int)(n - r0); q.N = count * DF_SB; q.K = DF_SB;
  q.alpha = -1.0; q.beta = 1.0;
  q.jgrp = DF_SBT; q.jstep = nranks;
  q.cyc_lower = 1; q.mask_off = DF_SBT * (s + 1) - DF_SBT * first;
  return launch_gemm<true, EPI_STORE>(q, 1, S(stream));
}

int gp2d_dfact_invstep(double* A, int64_t n, int64_t lda, int s, const double* panel, int nranks, int rank,
                       void* work, size_t work_bytes, void* stream) {
  GP2D_CHECK(dfact_args(A, n, lda, s));
  GP2D_REQUIRE(panel != nullptr, "dfact_invstep: NULL panel");
  GP2D_REQUIRE(nranks >= 1 && rank >= 0 && rank < nranks, "dfact_invstep: bad rank / world size");
  const DfactWork lay(n);
  GP2D_REQUIRE(work != nullptr && work_bytes >= lay.total, "dfact_invstep: workspace too small");
  GP2D_REQUIRE(aligned16(A) && aligned16(panel), "dfact_invstep: A and panel must be 16-byte aligned");
  hipStream_t st = S(stream);
  const int64_t s0 = (int64_t)s * DF_SB;
  if (s % nranks == rank) {   // this rank's W column block s starts as the identity block column
    dfact_reset_col_kernel<<<(unsigned)n, DF_SB / 2, 0, st>>>(A, n, lda, s0);
    GP2D_CHECK(check_launch("dfact_reset_col_kernel"));
  }
  int first, count;
  dfact_owned(0, s + 1, nranks, rank, first, count);
  if (count == 0) return 0;
  // X[s] = D_s · R[s] out of place into Xt (DF_SB × n, A's column positions; D_s lower: row
  // block i reads k < 128(i+1)), then R[t > s] −= L21 · X[s] from Xt, then Xt → X[s]
  double* Xt = lay.at(work).Xt;
  double* Xs = A + s0 * lda;
  auto cyc = [&](GemmParams& q) { q.jgrp = DF_SBT; q.jstep = nranks; };
  {
    GemmParams q = gemm_params();
    q.A = panel; q.lda = DF_SB;
    q.B = Xs + (int64_t)first * DF_SB; q.ldb = lda;
    q.C = Xt + (int64_t)first * DF_SB; q.ldc = n;
    q.M = DF_SB; q.N = count * DF_SB; q.K = DF_SB; q.a_lower = 1;
    cyc(q);
    GP2D_CHECK((launch_gemm<false, EPI_STORE>(q, 1, st)));
  }
  const int64_t rows = n - s0 - DF_SB;
  if (rows > 0) {   // R[t > s] −= L21 · X[s]
    GemmParams q = gemm_params();
    q.A = panel + (int64_t)DF_SB * DF_SB; q.lda = DF_SB;
    q.B = Xt + (int64_t)first * DF_SB; q.ldb = n;
    q.C = Xs + (int64_t)DF_SB * lda + (int64_t)first * DF_SB; q.ldc = lda;
    q.M = (int)rows; q.N = count * DF_SB; q.K = DF_SB;
    q.alpha = -1.0; q.beta = 1.0;
    cyc(q);
    GP2D_CHECK((launch_gemm<false, EPI_STORE>(q, 1, st)));
  }
  dfact_copy_owned_kernel<<<dim3((unsigned)count, DF_SB), DF_SB / 2, 0, st>>>(Xt, n, Xs, lda, first, nranks);
  return check_launch("dfact_copy_owned_kernel");
}

static int dfact_blocks_args(const double* W, int64_t n, int64_t ldw, int t0, int dt, int count) {
  GP2D_CHECK(dfact_args(W, n, ldw, t0, true));
  GP2D_REQUIRE(count >= 1 && dt >= 1 && (int64_t)(t0 + (count - 1) * dt) * DF_SB < n,
               "dfact: super-column list out of range");
  return 0;
}

int gp2d_dfact_zpart(const double* W, int64_t n, int64_t ldw, int t0, int dt, int count, const double* y,
                     double* zpart, void* stream) {
  GP2D_CHECK(dfact_blocks_args(W, n, ldw, t0, dt, count));
  GP2D_REQUIRE(y != nullptr && zpart != nullptr, "dfact_zpart: NULL vector");
  dfact_zpart_kernel<<<dim3((unsigned)((n + 3) / 4), (unsigned)count), 256, 0, S(stream)>>>(W, n, ldw, t0, dt, y,
                                                                                          zpart);
  return check_launch("dfact_zpart_kernel");
}

int gp2d_dfact_zsum(const double* parts, int nparts, int64_t n, double* z, void* stream) {
  GP2D_REQUIRE(parts != nullptr && z != nullptr && nparts >= 1 && n > 0, "dfact_zsum: bad arguments");
  sum_segments_kernel<<<(unsigned)((n + 255) / 256), 256, 0, S(stream)>>>(parts, nparts, n, z);
  return check_launch("sum_segments_kernel");
}

size_t gp2d_dfact_alpha_workspace(int64_t n, int count) {
  return (size_t)(count > 0 ? count : 0) * (size_t)((n > 0 ? n : 0) / 128) * DF_SB * sizeof(double);
}

int gp2d_dfact_alpha_blocks(const double* W, int64_t n, int64_t ldw, int t0, int dt, int count, const double* z,
                            double* alpha, void* work, size_t work_bytes, void* stream) {
  GP2D_CHECK(dfact_blocks_args(W, n, ldw, t0, dt, count));
  GP2D_REQUIRE(z != nullptr && alpha != nullptr, "dfact_alpha_blocks: NULL vector");
  GP2D_REQUIRE(work != nullptr && work_bytes >= gp2d_dfact_alpha_workspace(n, count),
               "dfact_alpha_blocks: workspace too small");
  const int64_t nseg = n / 128;
  double* part = static_cast<double*>(work);
  dfact_alpha_part_kernel<<<dim3(DF_SB / 256, (unsigned)nseg, (unsigned)count), 256, 0, S(stream)>>>(W, n, ldw, t0,
                                                                                                   dt, z, part);
  GP2D_CHECK(check_launch("dfact_alpha_part_kernel"));
  dfact_alpha_sum_kernel<<<dim3(DF_SB / 256, (unsigned)count), 256, 0, S(stream)>>>(part, nseg, alpha);
  return check_launch("dfact_alpha_sum_kernel");
}

int gp2d_copy2d(double* dst, int64_t ldd, const double* src, int64_t lds, int64_t rows, int64_t cols,
                void* stream) {
  GP2D_REQUIRE(rows >= 0 && cols >= 0, "copy2d: negative size");
  if (rows == 0 || cols == 0) return 0;
  GP2D_REQUIRE(dst && src && ldd >= cols && lds >= cols, "copy2d: NULL buffer or leading dimension < cols");
  GP2D_EV(hipMemcpy2DAsync(dst, ldd * sizeof(double), src, lds * sizeof(double), cols * sizeof(double), rows,
                           hipMemcpyDeviceToDevice, S(stream)));
  return 0;
}

size_t gp2d_pack_lower_doubles(int64_t n) {
  const int64_t nb = n > 0 ? n / NB : 0;
  return (size_t)(NB * NB) * (size_t)(nb * (nb + 1) / 2);
}

int gp2d_pack_lower(double* W, int64_t n, int64_t ldw, double* packed, int unpack, void* stream) {
  GP2D_REQUIRE(W && packed, "pack_lower: NULL buffer");
  GP2D_REQUIRE(n > 0 && n % NB == 0 && ldw >= n && ldw % 2 == 0,
               "pack_lower: n must be a positive multiple of 128, ldw >= n and even");
  GP2D_REQUIRE(aligned16(W) && aligned16(packed), "pack_lower: W and packed must be 16-byte aligned");
  const dim3 g((unsigned)((n + 511) / 512), (unsigned)(n / NB));
  if (unpack) pack_lower_kernel<true><<<g, 256, 0, S(stream)>>>(W, n, ldw, packed);
  else pack_lower_kernel<false><<<g, 256, 0, S(stream)>>>(W, n, ldw, packed);
  return check_launch("pack_lower_kernel");
}

int gp2d_zero_upper(double* A, int64_t n, int64_t lda, void* stream) {
  GP2D_REQUIRE(A != nullptr && n > 0 && n % NB == 0 && lda >= n && lda % 2 == 0,
               "zero_upper: n must be a positive multiple of 128, lda >= n and even");
  GP2D_REQUIRE(aligned16(A), "zero_upper: A must be 16-byte aligned");
  dim3 zg((unsigned)((n / 2 + 255) / 256), (unsigned)n);
  zero_upper_kernel<<<zg, 256, 0, S(stream)>>>(A, n, lda);
  return check_launch("zero_upper_kernel");
}

// ------------------------------------------------------------------------ POTRS
size_t gp2d_potrs_workspace(int64_t n) { return PotrsWork(n).total; }

int gp2d_potrs_inv(const double* W, int64_t n, int64_t ldw, const double* y, double* alpha, void* work,
                   size_t work_bytes, void* stream) {
  GP2D_REQUIRE(n % NB == 0 && n > 0, "potrs: n must be a positive multiple of 128");
  GP2D_REQUIRE(ldw >= n, "potrs: ldw must be >= n");
  GP2D_REQUIRE(work != nullptr && work_bytes >= gp2d_potrs_workspace(n), "potrs: workspace too small");
  hipStream_t s = S(stream);
  const auto [z, part] = PotrsWork(n).at(work);
  trmv_n_lower_kernel<<<(unsigned)((n + 3) / 4), 256, 0, s>>>(W, n, ldw, y, z);
  GP2D_CHECK(check_launch("trmv_n_lower_kernel"));
  const int64_t nseg = n / NB;
  trmv_t_lower_part_kernel<<<dim3((unsigned)((n + 255) / 256), (unsigned)nseg), 256, 0, s>>>(W, n, ldw, z, part);
  GP2D_CHECK(check_launch("trmv_t_lower_part_kernel"));
  sum_segments_kernel<<<(unsigned)((n + 255) / 256), 256, 0, s>>>(part, nseg, n, alpha);
  return check_launch("sum_segments_kernel");
}

// ---------------------------------------------------------------------- PREDICT
// The launches every predict entry is built from (workspace layouts: predict_host.hpp).
static int launch_mean_partials(const double* B, int64_t ncols, int64_t n, const double* alpha, double* pm,
                                hipStream_t s) {
  const dim3 grid((unsigned)((ncols + 255) / 256), (unsigned)predict_segments(n));
  mean_part_kernel<<<grid, 256, 0, s>>>(B, ncols, ncols, alpha, pm);
  return check_launch("mean_part_kernel");
}

// predict_finalize_kernel's arguments: the partial sums and their segment counts, the chunk (ncols
// columns = components of cp padded, cv valid targets, the first being target c0 of m), the
// variance's terms (prior − Σ v² + add, clipped at 0 if asked), the outputs and the caller's order
struct Finalize {
  const double* pm; int64_t nmseg;
  const double* P; int64_t npseg;
  int64_t ncols, cp, cv, c0, m;
  double prior, add;
  int clip, compute_var;
  double* mean; double* var;
  const int64_t* order;
};
static int launch_finalize(const Finalize& f, hipStream_t s) {
  predict_finalize_kernel<<<(unsigned)((f.ncols + 63) / 64), 64, 0, s>>>(
      f.pm, f.nmseg, f.P, f.npseg, f.ncols, f.cp, f.cv, f.c0, f.m, f.prior, f.add, f.clip, f.compute_var, f.mean,
      f.var, f.order);
  return check_launch("predict_finalize_kernel");
}

// V = W·K*ᵀ: W = L⁻¹ (n × n, lower triangular), K*ᵀ = B (n × ncols).  The caller adds P / ldp
// (EPI_COLSQ: Σ v² per column) or C / ldc (EPI_STORE: V itself).
static GemmParams wk_gemm_params(const double* W, int64_t ldw, int64_t n, const double* B, int64_t ncols) {
  GemmParams p = gemm_params();
  p.A = W; p.lda = ldw;
  p.B = B; p.ldb = ncols;
  p.M = (int)n; p.N = (int)ncols; p.K = (int)n;
  p.a_lower = 1; p.rev_rows = 1;
  p.xcd_cols = 0;  // XCD-grouped order measured 4% slower (64.9 vs 67.6 TF/s); kept for study
  return p;
}

// A trend fit's share of a chunked predict (trend.hpp): the basis, the fit's trend block, whether the
// columns are velocity components (h* = the basis at the target; only if with_basis) or share the
// constant hc (a derived field's, or zeros), and the target layout.
struct TrendPredict {
  int order;
  TrendBasis basis;
  const double* block;
  int with_basis, velocity, pdim;
  TrendH hc;
};

// h* of a derived field: h_δ = (0,0,1,0,0,1)/s, h_ζ = (0,0,0,−1,1,0)/s at order 1, zero at order 0
static TrendH trend_field_h(const TrendPredict& t, int field) {
  TrendH h{};
  if (t.with_basis && t.order == 1) {
    if (field == GP2D_FIELD_DIVERGENCE) { h.v[2] = t.basis.is; h.v[5] = t.basis.is; }
    else { h.v[3] = -t.basis.is; h.v[4] = t.basis.is; }
  }
  return h;
}

// mean_part_multi_kernel in place of mean_part_kernel: right-hand side 0 = α′, then B0's columns
static int launch_mean_partials_trend(const double* B, int64_t ncols, int64_t n, const TrendPredict& t, double* pm,
                                      hipStream_t s) {
  const int64_t nseg = predict_segments(n);
  const dim3 grid((unsigned)((ncols + 255) / 256), (unsigned)nseg);
  const double* rhs = t.block + TB_RHS;
  if (t.order == 0) mean_part_multi_kernel<3><<<grid, 256, 0, s>>>(B, ncols, ncols, rhs, nseg, pm);
  else mean_part_multi_kernel<TREND_QMAX + 1><<<grid, 256, 0, s>>>(B, ncols, ncols, rhs, nseg, pm);
  return check_launch("mean_part_multi_kernel");
}

static int launch_finalize_trend(const Finalize& f, const TrendPredict& t, const double* xg, hipStream_t s) {
  const unsigned grid = (unsigned)((f.ncols + 63) / 64);
  if (t.order == 0)
    predict_trend_finalize_kernel<2><<<grid, 64, 0, s>>>(f.pm, f.P, f.nmseg, f.ncols, f.cp, f.cv, f.c0, f.m, f.prior,
                                                         f.add, f.clip, f.compute_var, f.mean, f.var, xg, t.pdim,
                                                         t.basis, t.velocity, t.hc, t.block);
  else
    predict_trend_finalize_kernel<TREND_QMAX><<<grid, 64, 0, s>>>(f.pm, f.P, f.nmseg, f.ncols, f.cp, f.cv, f.c0, f.m,
                                                                  f.prior, f.add, f.clip, f.compute_var, f.mean,
                                                                  f.var, xg, t.pdim, t.basis, t.velocity, t.hc,
                                                                  t.block);
  return check_launch("predict_trend_finalize_kernel");
}

// What differs between the chunked predicts: columns per target, the variance's terms, whether
// the product goes to the timing hooks, and the chunk's cross-covariance — assemble(the chunk's
// targets, valid count, padded count, out) writes K*ᵀ (n × bd·cp: rows = training components,
// columns = target components).  gram (the gradient predict, bd = 4 columns per target in grad.hpp's
// layout): the product's epilogue is EPI_COLGRAM into ten partials per target in place of Σ v² per
// column, and the finalize is grad_finalize_kernel with the 4 × 4 prior.
struct ChunkedPredict {
  int bd;
  double prior = 0.0, add = 0.0;
  int clip = 0;
  bool timed = false;
  std::function<int(const double* xg, int64_t cv, int64_t cp, double* Ks)> assemble;
  bool gram = false;
  GradPrior prior4{};
  const TrendPredict* trend = nullptr;   // a trend fit's predict: the multi-right-hand-side mean pass and finalize
};

// One chunked predict over the m targets (dim coordinates each): per chunk assemble, mean partials,
// Σ v² (or Gram) partials of W·K*ᵀ if the variance is asked for, finalize.  Ks, pm, P: the chunk's
// cross-covariance, the mean's partials and the product's partials in the caller's workspace.
static int predict_chunks(const ChunkedPredict& v, const double* W, int64_t n, int64_t ldw, const double* alpha,
                          int64_t ntr, const double* xg, int dim, int64_t m, int compute_var, double* mean,
                          double* var, int64_t chunk, double* Ks, double* pm, double* P, hipStream_t s) {
  static_assert(GBN == 2 * PT_TILE, "a chunk's bd·cp columns fill whole GEMM column tiles");
  const int64_t nseg = predict_segments(n);
  for (int64_t c0 = 0; c0 < m; c0 += chunk) {
    const int64_t cv = std::min<int64_t>(chunk, m - c0);
    const int64_t cp = round_up(cv, std::max<int64_t>(PT_TILE, GBN / v.bd));   // whole point tiles (grad: 16-groups)
    const int64_t ncols = v.bd * cp;
    GP2D_CHECK(v.assemble(xg + c0 * dim, cv, cp, Ks));
    if (v.trend) GP2D_CHECK(launch_mean_partials_trend(Ks, ncols, n, *v.trend, pm, s));
    else GP2D_CHECK(launch_mean_partials(Ks, ncols, n, alpha, pm, s));
    if (compute_var) {
      GemmParams p = wk_gemm_params(W, ldw, n, Ks, ncols);
      p.P = P; p.ldp = v.gram ? GRAD_NPAIR * cp : ncols;
      const double nv = (double)v.bd * (double)ntr;  // algorithmic order (valid points)
      TimedLaunch t(s, (double)v.bd * (double)cv * nv * nv, v.timed);  // 2·(2N)² per point (vector2d)
      GP2D_CHECK(v.gram ? (launch_gemm<false, EPI_COLGRAM>(p, 1, s)) : (launch_gemm<false, EPI_COLSQ>(p, 1, s)));
    }
    if (v.gram) {
      grad_finalize_kernel<<<(unsigned)((cv + 63) / 64), 64, 0, s>>>(pm, P, nseg, cp, cv, c0, v.prior4, compute_var,
                                                                      mean, var);
      GP2D_CHECK(check_launch("grad_finalize_kernel"));
    } else if (v.trend) {   // xg: all m targets; the kernel indexes them by c0 + its column
      GP2D_CHECK(launch_finalize_trend({pm, nseg, P, nseg, ncols, cp, cv, c0, m, v.prior, v.add, v.clip, compute_var,
                                        mean, var, nullptr}, *v.trend, xg, s));
    } else {
      GP2D_CHECK(launch_finalize({pm, nseg, P, nseg, ncols, cp, cv, c0, m, v.prior, v.add, v.clip, compute_var, mean,
                                  var, nullptr}, s));
    }
  }
  return 0;
}

// gp2d_predict's and gp2d_predict_field's carve of their shared layout
static int predict_chunks(const ChunkedPredict& v, const double* W, int64_t n, int64_t ldw, const double* alpha,
                          int64_t ntr, const double* xg, int dim, int64_t m, int compute_var, double* mean,
                          double* var, int64_t chunk, void* work, hipStream_t s) {
  const auto [Ks, pm, P] = v.trend ? PredictTrendWork(n, v.bd * chunk, v.trend->order).at(work)
                                   : PredictWork(n, v.bd * chunk).at(work);
  return predict_chunks(v, W, n, ldw, alpha, ntr, xg, dim, m, compute_var, mean, var, chunk, Ks, pm, P, s);
}

// ---- the trend descriptor's checks (every trend entry, before any launch) and its basis
static int validate_trend(const gp2d_trend_t* t, const double* block, const char* entry) {
  const std::string e(entry);
  GP2D_REQUIRE(t != nullptr, e + ": trend is NULL");
  GP2D_REQUIRE(t->order == 0 || t->order == 1, e + ": trend order must be 0 (constant) or 1 (linear)");
  GP2D_REQUIRE(std::isfinite(t->scale) && t->scale > 0.0, e + ": trend scale must be finite and > 0");
  GP2D_REQUIRE(std::isfinite(t->centre[0]) && std::isfinite(t->centre[1]), e + ": trend centre must be finite");
  GP2D_REQUIRE(block != nullptr, e + ": block is NULL");
  GP2D_REQUIRE(reinterpret_cast<uintptr_t>(block) % 64 == 0, e + ": block must be 64-byte aligned");
  return 0;
}
static TrendBasis trend_basis_of(const gp2d_trend_t* t) { return {t->centre[0], t->centre[1], 1.0 / t->scale}; }

int gp2d_trend_coefficients(int order) { return (order == 0 || order == 1) ? trend_q(order) : -2; }
size_t gp2d_trend_block_doubles(int64_t n) { return TrendBlock(n).doubles; }
size_t gp2d_predict_trend_workspace(int64_t n, int64_t chunk, int bd, int order) {
  return PredictTrendWork(n, predict_sized_cols(chunk, bd), order == 0 ? 0 : 1).total;
}

size_t gp2d_predict_workspace(int64_t n, int64_t chunk, int bd) {
  return PredictWork(n, predict_sized_cols(chunk, bd)).total;
}

// gp2d_predict, and with tp gp2d_predict_trend (tp's column kind and pdim are set here)
static int predict_impl(const double* W, int64_t n, int64_t ldw, const double* alpha, const double* xtr, int64_t ntr,
                        int64_t ntr_pad, const double* xg, int64_t m, const gp2d_kernel_t* k, int var_mode,
                        double noise, int compute_var, double* mean, double* var, int64_t chunk, void* work,
                        size_t work_bytes, void* stream, TrendPredict* tp) {
  GP2D_CHECK(validate_kernel(k));
  const int bd = gp2d_block_dim(k);
  GP2D_REQUIRE(tp == nullptr || bd == 2, "predict_trend: k must be a vector kernel (two components per point)");
  GP2D_REQUIRE(n == bd * ntr_pad, "predict: n must equal block_dim × ntr_pad");
  GP2D_REQUIRE(n % NB == 0, "predict: n must be a multiple of 128");
  GP2D_REQUIRE(ld_even(ldw, n), tp ? "predict_trend: wld must be >= n and even" : "predict: ldw must be >= n and even");
  GP2D_REQUIRE(chunk > 0 && chunk % PT_TILE == 0, "predict: chunk must be a positive multiple of 64");
  GP2D_REQUIRE(bd * chunk % GBN == 0, "predict: block_dim × chunk must be a multiple of 128");
  GP2D_REQUIRE(work != nullptr && work_bytes >= (tp ? gp2d_predict_trend_workspace(n, chunk, bd, tp->order)
                                                    : gp2d_predict_workspace(n, chunk, bd)),
               "predict: workspace too small");
  GP2D_REQUIRE(var_mode >= 0 && var_mode <= 2, "predict: bad var_mode");
  if (m <= 0) return 0;
  GP2D_REQUIRE(aligned16(W), "predict: W must be 16-byte aligned");
  hipStream_t s = S(stream);
  ChunkedPredict v;
  v.bd = bd;
  v.prior = gp2d_kernel_diag(k);
  v.add = (var_mode == GP2D_VAR_LATENT) ? 0.0 : noise;
  v.clip = (var_mode == GP2D_VAR_CLIPPED);
  v.timed = true;
  v.assemble = [=](const double* xc, int64_t cv, int64_t cp, double* Ks) {
    return assemble_impl(xtr, ntr, ntr_pad, xc, cv, cp, k, 0.0, 0, Ks, bd * cp, s);
  };
  if (tp) {
    tp->velocity = tp->with_basis;   // one term of a sum: h* = 0 for every column
    tp->hc = TrendH{};
    tp->pdim = point_dim(k);
    v.trend = tp;
  }
  return predict_chunks(v, W, n, ldw, alpha, ntr, xg, point_dim(k), m, compute_var, mean, var, chunk, work, s);
}

int gp2d_predict(const double* W, int64_t n, int64_t ldw, const double* alpha, const double* xtr, int64_t ntr,
                 int64_t ntr_pad, const double* xg, int64_t m, const gp2d_kernel_t* k, int var_mode, double noise,
                 int compute_var, double* mean, double* var, int64_t chunk, void* work, size_t work_bytes,
                 void* stream) {
  return predict_impl(W, n, ldw, alpha, xtr, ntr, ntr_pad, xg, m, k, var_mode, noise, compute_var, mean, var, chunk,
                      work, work_bytes, stream, nullptr);
}

// ------------------------------------------------------- PREDICT (derived fields)
static bool field_kernel_ok(const gp2d_kernel_t* k) {
  if (k != nullptr && is_sum_family(k)) {   // a validated sum: every term non-scalar
    for (int t = 0; t < k->nterms; ++t)
      if (sum_term(k, t)->kind == GP2D_KIND_SCALAR) return false;
    return true;
  }
  return k != nullptr && is_vector_family(k) && k->kind != GP2D_KIND_SCALAR;
}

double gp2d_field_prior_var(const gp2d_kernel_t* k, int field) {
  if (validate_kernel(k) != 0 || !field_kernel_ok(k) ||
      (field != GP2D_FIELD_DIVERGENCE && field != GP2D_FIELD_VORTICITY))
    return std::nan("");
  if (is_sum_family(k)) {   // Σ w_t·var_t
    double s = 0.0;
    for (int t = 0; t < k->nterms; ++t) {
      const double d = sum_weight(k, t) * gp2d_field_prior_var(sum_term(k, t), field);
      s = t ? s + d : d;
    }
    return s;
  }
  const double w = field_weight(k, field);
  if (w == 0.0) return 0.0;   // the field vanishes by kind (its length scale may be unset)
  const double l = (field == GP2D_FIELD_VORTICITY) ? k->l_df : k->l_cf;
  const double vt = temporal_var(k);
  const double l2 = l * l;
  return vt * (8.0 * w / (l2 * l2));
}

size_t gp2d_predict_field_workspace(int64_t n, int64_t chunk) { return gp2d_predict_workspace(n, chunk, 1); }

// gp2d_predict_field, and with tp gp2d_predict_field_trend (tp's h* and pdim are set here)
static int predict_field_impl(const double* W, int64_t n, int64_t ldw, const double* alpha, const double* xtr,
                              int64_t ntr, int64_t ntr_pad, const double* xg, int64_t m, const gp2d_kernel_t* k,
                              int field, int compute_var, double* mean, double* var, int64_t chunk, void* work,
                              size_t work_bytes, void* stream, TrendPredict* tp) {
  GP2D_CHECK(validate_kernel(k));
  GP2D_REQUIRE(field_kernel_ok(k), "predict_field: div-free, curl-free or mixed vector kernels only");
  GP2D_REQUIRE(field == GP2D_FIELD_DIVERGENCE || field == GP2D_FIELD_VORTICITY,
               "predict_field: field must be GP2D_FIELD_DIVERGENCE or GP2D_FIELD_VORTICITY");
  GP2D_REQUIRE(n == 2 * ntr_pad, "predict_field: n must equal 2 × ntr_pad");
  GP2D_REQUIRE(n % NB == 0 && n > 0, "predict_field: n must be a positive multiple of 128");
  GP2D_REQUIRE(ntr >= 0 && ntr <= ntr_pad, "predict_field: bad point count");
  GP2D_REQUIRE(ld_even(ldw, n),
               tp ? "predict_field_trend: wld must be >= n and even" : "predict_field: ldw must be >= n and even");
  GP2D_REQUIRE(chunk > 0 && chunk % GBN == 0, "predict_field: chunk must be a positive multiple of 128");
  GP2D_REQUIRE(work != nullptr && work_bytes >= (tp ? gp2d_predict_trend_workspace(n, chunk, 1, tp->order)
                                                    : gp2d_predict_field_workspace(n, chunk)),
               "predict_field: workspace too small");
  if (m <= 0) return 0;
  GP2D_REQUIRE(aligned16(W), "predict_field: W must be 16-byte aligned");
  hipStream_t s = S(stream);
  bool vanishes = !is_sum_family(k) && field_vanishes(k, field);
  if (is_sum_family(k)) {   // only where the field vanishes in every term
    vanishes = true;
    for (int t = 0; t < k->nterms; ++t) vanishes = vanishes && field_vanishes(sum_term(k, t), field);
  }
  if (vanishes && tp == nullptr) {
    // div-free flow has no divergence, curl-free flow no vorticity: exact zeros, no GEMM
    if (hipMemsetAsync(mean, 0, sizeof(double) * (size_t)m, s) != hipSuccess ||
        (compute_var && hipMemsetAsync(var, 0, sizeof(double) * (size_t)m, s) != hipSuccess)) {
      set_error("predict_field: hipMemsetAsync failed");
      return -1;
    }
    return 0;
  }
  // one component per target: the prior is the field's prior variance, no noise, no clipping; untimed
  ChunkedPredict v;
  v.bd = 1;
  v.prior = gp2d_field_prior_var(k, field);
  // cov(observations, field) for the chunk: rows = training components, cols = target points
  if (is_sum_family(k)) {
    const SumEntry<FieldEntry> fe = make_sum_field_entry(k, field);
    v.assemble = [=](const double* xc, int64_t cv, int64_t cp, double* Ks) {
      return launch_cross_cov(fe, xtr, ntr, ntr_pad, xc, cv, cp, Ks, cp, 0, cp, s);
    };
  } else {
    FieldEntry fe = make_field_entry(k, field);
    if (vanishes) fe.il2 = fe.w4 = 0.0;   // (a trend predict) exact zeros whatever the unused length scale holds
    v.assemble = [=](const double* xc, int64_t cv, int64_t cp, double* Ks) {
      return launch_cross_cov(fe, xtr, ntr, ntr_pad, xc, cv, cp, Ks, cp, 0, cp, s);
    };
  }
  if (tp) {   // a field that vanishes by kind keeps the general path: exact-zero K*, the trend's terms remain
    tp->velocity = 0;
    tp->hc = trend_field_h(*tp, field);
    tp->pdim = point_dim(k);
    v.trend = tp;
  }
  return predict_chunks(v, W, n, ldw, alpha, ntr, xg, point_dim(k), m, compute_var, mean, var, chunk, work, s);
}

int gp2d_predict_field(const double* W, int64_t n, int64_t ldw, const double* alpha, const double* xtr, int64_t ntr,
                       int64_t ntr_pad, const double* xg, int64_t m, const gp2d_kernel_t* k, int field,
                       int compute_var, double* mean, double* var, int64_t chunk, void* work, size_t work_bytes,
                       void* stream) {
  return predict_field_impl(W, n, ldw, alpha, xtr, ntr, ntr_pad, xg, m, k, field, compute_var, mean, var, chunk, work,
                            work_bytes, stream, nullptr);
}

// ------------------------------------------------------- TREND (background flow, trend.hpp)
size_t gp2d_trend_workspace(int64_t n, int order) { (void)order; return TrendFitWork(n).total; }

int gp2d_trend_fit(const double* W, int64_t n, int64_t wld, const double* y, const double* xtr, int64_t ntr,
                   int64_t ntr_pad, int dim, const gp2d_trend_t* trend, double* alpha_out, double* block_out,
                   void* work, size_t work_bytes, void* stream) {
  GP2D_CHECK(validate_trend(trend, block_out, "trend_fit"));
  GP2D_REQUIRE(W && y && xtr && alpha_out, "trend_fit: NULL argument");
  GP2D_REQUIRE(n % NB == 0 && n > 0, "trend_fit: n must be a positive multiple of 128");
  GP2D_REQUIRE(n == 2 * ntr_pad && ntr_pad % PT_TILE == 0, "trend_fit: n must equal 2 × ntr_pad");
  GP2D_REQUIRE(ntr >= 1 && ntr <= ntr_pad, "trend_fit: bad point count");
  GP2D_REQUIRE(dim == 2 || dim == 3, "trend_fit: dim must be 2 or 3");
  GP2D_REQUIRE(wld >= n, "trend_fit: wld must be >= n");
  GP2D_REQUIRE(work != nullptr && work_bytes >= gp2d_trend_workspace(n, trend->order),
               "trend_fit: workspace too small");
  hipStream_t s = S(stream);
  const auto [Y, Z, part] = TrendFitWork(n).at(work);
  const TrendBasis tb = trend_basis_of(trend);
  const int64_t nseg = n / NB;
  const unsigned rows = (unsigned)((n + 255) / 256);
  const dim3 tgrid(rows, (unsigned)nseg);
  if (trend->order == 0) {
    trend_rhs_kernel<2><<<rows, 256, 0, s>>>(y, xtr, ntr, ntr_pad, dim, tb, Y);
    GP2D_CHECK(check_launch("trend_rhs_kernel"));
    trmv_n_lower_multi_kernel<3><<<(unsigned)((n + 3) / 4), 256, 0, s>>>(W, n, wld, Y, Z);
    GP2D_CHECK(check_launch("trmv_n_lower_multi_kernel"));
    trend_solve_kernel<2><<<1, 256, 0, s>>>(Z, n, block_out);
    GP2D_CHECK(check_launch("trend_solve_kernel"));
    trmv_t_lower_multi_part_kernel<3><<<tgrid, 256, 0, s>>>(W, n, wld, Z, block_out, part);
  } else {
    trend_rhs_kernel<TREND_QMAX><<<rows, 256, 0, s>>>(y, xtr, ntr, ntr_pad, dim, tb, Y);
    GP2D_CHECK(check_launch("trend_rhs_kernel"));
    trmv_n_lower_multi_kernel<TREND_QMAX + 1><<<(unsigned)((n + 3) / 4), 256, 0, s>>>(W, n, wld, Y, Z);
    GP2D_CHECK(check_launch("trmv_n_lower_multi_kernel"));
    trend_solve_kernel<TREND_QMAX><<<1, 256, 0, s>>>(Z, n, block_out);
    GP2D_CHECK(check_launch("trend_solve_kernel"));
    trmv_t_lower_multi_part_kernel<TREND_QMAX + 1><<<tgrid, 256, 0, s>>>(W, n, wld, Z, block_out, part);
  }
  GP2D_CHECK(check_launch("trmv_t_lower_multi_part_kernel"));
  trend_sum_kernel<<<(unsigned)((n * TREND_RHS + 255) / 256), 256, 0, s>>>(part, nseg, n, alpha_out,
                                                                           block_out + TB_RHS);
  return check_launch("trend_sum_kernel");
}

int gp2d_predict_trend(const double* W, int64_t n, int64_t wld, const double* alpha, const double* xtr, int64_t ntr,
                       int64_t ntr_pad, const double* xg, int64_t m, const gp2d_kernel_t* k, int var_mode,
                       double noise, int compute_var, double* mean, double* var, int64_t chunk, void* work,
                       size_t work_bytes, void* stream, const gp2d_trend_t* trend, const double* block,
                       int with_basis) {
  GP2D_CHECK(validate_trend(trend, block, "predict_trend"));
  TrendPredict tp{trend->order, trend_basis_of(trend), block, with_basis != 0, 0, 2, TrendH{}};
  return predict_impl(W, n, wld, alpha, xtr, ntr, ntr_pad, xg, m, k, var_mode, noise, compute_var, mean, var, chunk,
                      work, work_bytes, stream, &tp);
}

int gp2d_predict_field_trend(const double* W, int64_t n, int64_t wld, const double* alpha, const double* xtr,
                             int64_t ntr, int64_t ntr_pad, const double* xg, int64_t m, const gp2d_kernel_t* k,
                             int field, int compute_var, double* mean, double* var, int64_t chunk, void* work,
                             size_t work_bytes, void* stream, const gp2d_trend_t* trend, const double* block,
                             int with_basis) {
  GP2D_CHECK(validate_trend(trend, block, "predict_field_trend"));
  TrendPredict tp{trend->order, trend_basis_of(trend), block, with_basis != 0, 0, 2, TrendH{}};
  return predict_field_impl(W, n, wld, alpha, xtr, ntr, ntr_pad, xg, m, k, field, compute_var, mean, var, chunk, work,
                            work_bytes, stream, &tp);
}

// ------------------------------------------------------- PREDICT (velocity gradient tensor)
int gp2d_grad_prior_cov(const gp2d_kernel_t* k, double out[16]) {
  if (out == nullptr) {
    set_error("grad_prior_cov: out is NULL");
    return -2;
  }
  for (int i = 0; i < 16; ++i) out[i] = std::nan("");
  GP2D_CHECK(refuse_sum(k, "grad_prior_cov"));
  GP2D_CHECK(validate_kernel(k));
  GP2D_REQUIRE(field_kernel_ok(k), "grad_prior_cov: div-free, curl-free or mixed vector kernels only");
  grad_prior_cov(k, out);
  return 0;
}

size_t gp2d_predict_grad_workspace(int64_t n, int64_t chunk) { return PredictGradWork(n, chunk).total; }

int gp2d_predict_grad(const double* W, int64_t n, int64_t ldw, const double* alpha, const double* xtr, int64_t ntr,
                      int64_t ntr_pad, const double* xg, int64_t m, const gp2d_kernel_t* k, int compute_cov,
                      double* mean, double* cov, int64_t chunk, void* work, size_t work_bytes, void* stream) {
  GP2D_CHECK(refuse_sum(k, "predict_grad"));
  GP2D_CHECK(validate_kernel(k));
  GP2D_REQUIRE(field_kernel_ok(k), "predict_grad: div-free, curl-free or mixed vector kernels only");
  GP2D_REQUIRE(n == 2 * ntr_pad, "predict_grad: n must equal 2 × ntr_pad");
  GP2D_REQUIRE(n % NB == 0 && n > 0, "predict_grad: n must be a positive multiple of 128");
  GP2D_REQUIRE(ntr >= 0 && ntr <= ntr_pad, "predict_grad: bad point count");
  GP2D_REQUIRE(ld_even(ldw, n), "predict_grad: ldw must be >= n and even");
  GP2D_REQUIRE(chunk > 0 && chunk % PT_TILE == 0, "predict_grad: chunk must be a positive multiple of 64");
  GP2D_REQUIRE(n < (int64_t)1 << 30 && chunk < (int64_t)1 << 28, "predict_grad: n or chunk out of range");
  GP2D_REQUIRE(work != nullptr && work_bytes >= gp2d_predict_grad_workspace(n, chunk),
               "predict_grad: workspace too small");
  if (m <= 0) return 0;
  GP2D_REQUIRE(aligned16(W), "predict_grad: W must be 16-byte aligned");
  hipStream_t s = S(stream);
  const GradEntry ge = make_grad_entry(k);
  // four columns per target in grad.hpp's layout; the 4 × 4 prior, no noise, no clipping; untimed
  ChunkedPredict v;
  v.bd = GRAD_NC;
  v.gram = true;
  grad_prior_cov(k, v.prior4.p);
  v.assemble = [=](const double* xc, int64_t cv, int64_t cp, double* C) {
    return launch_cross_cov(ge, xtr, ntr, ntr_pad, xc, cv, cp, C, GRAD_NC * cp, 0, cp, s);
  };
  const auto [C, pm, G] = PredictGradWork(n, chunk).at(work);
  return predict_chunks(v, W, n, ldw, alpha, ntr, xg, point_dim(k), m, compute_cov, mean, cov, chunk, C, pm, G, s);
}

// ------------------------------------------------- ADVECT (trajectories and the flow map's gradient)
int64_t gp2d_advect_records(int nsteps, int save_every) {
  GP2D_REQUIRE(nsteps >= 0, "advect_records: nsteps must be >= 0");
  GP2D_REQUIRE(save_every >= 1, "advect_records: save_every must be >= 1");
  return 1 + ((int64_t)nsteps + save_every - 1) / save_every;
}

int gp2d_advect(const double* alpha, int64_t n, const double* xtr, int64_t ntr, int64_t ntr_pad,
                const gp2d_kernel_t* k, const gp2d_trend_t* trend, const double* block, const double* x0, int64_t m,
                double t0, double dt, int nsteps, int save_every, double vel_scale, double* path, double* tangent,
                void* stream) {
  if (validate_kernel(k) != 0) {
    set_error("advect: k is invalid: " + g_err);
    return -2;
  }
  GP2D_REQUIRE(field_kernel_ok(k),
               "advect: k must be a div-free, curl-free or mixed vector kernel (KIND_SCALAR and the ARD family "
               "have no velocity gradient)");
  GP2D_REQUIRE(ntr_pad > 0 && ntr_pad % PT_TILE == 0, "advect: ntr_pad must be a positive multiple of 64");
  GP2D_REQUIRE(n == 2 * ntr_pad, "advect: n must equal 2 × ntr_pad");
  GP2D_REQUIRE(ntr > 0 && ntr <= ntr_pad, "advect: ntr must be in 1..ntr_pad");
  GP2D_REQUIRE(nsteps >= 0, "advect: nsteps must be >= 0");
  GP2D_REQUIRE(save_every >= 1, "advect: save_every must be >= 1");
  GP2D_REQUIRE(nsteps == 0 || (std::isfinite(dt) && dt != 0.0), "advect: dt must be finite and non-zero");
  GP2D_REQUIRE(std::isfinite(t0), "advect: t0 must be finite");
  GP2D_REQUIRE(std::isfinite(vel_scale), "advect: vel_scale must be finite");
  GP2D_REQUIRE((trend == nullptr) == (block == nullptr),
               "advect: trend and block must be both NULL (a zero-mean fit) or both set");
  if (trend != nullptr) GP2D_CHECK(validate_trend(trend, block, "advect"));
  GP2D_REQUIRE(m >= 0 && m < (int64_t)1 << 36, "advect: m out of range");
  if (m == 0) return 0;
  GP2D_REQUIRE(alpha != nullptr, "advect: alpha is NULL");
  GP2D_REQUIRE(xtr != nullptr, "advect: xtr is NULL");
  GP2D_REQUIRE(x0 != nullptr, "advect: x0 is NULL");
  GP2D_REQUIRE(path != nullptr, "advect: path is NULL");
  hipStream_t s = S(stream);
  const AdvectKernel ak = make_advect_kernel(k);
  AdvectTrend at{0, TrendBasis{0.0, 0.0, 1.0}, nullptr};
  if (trend != nullptr) at = AdvectTrend{trend_q(trend->order), trend_basis_of(trend), block};
  const bool st = point_dim(k) == 3;
  const unsigned grid = (unsigned)((m + ADV_TILE - 1) / ADV_TILE);
  advect_init_kernel<<<(unsigned)((m + 255) / 256), 256, 0, s>>>(x0, m, path, tangent);
  GP2D_CHECK(check_launch("advect_init_kernel"));
  // one launch per saved segment: record r → record r + 1, never more than save_every steps
  int64_t r = 0;
  for (int n0 = 0; n0 < nsteps; n0 += save_every, ++r) {
    const int nst = std::min(save_every, nsteps - n0);
    const double* xin = path + r * m * 2;
    double* xout = path + (r + 1) * m * 2;
    const double* fin = tangent ? tangent + r * m * 4 : nullptr;
    double* fout = tangent ? tangent + (r + 1) * m * 4 : nullptr;
    GP2D_CHECK(st ? launch_advect<true>(tangent != nullptr, grid, s, alpha, xtr, ntr, ntr_pad, ak, at, xin, fin, xout,
                                        fout, m, t0, dt, n0, nst, vel_scale)
                  : launch_advect<false>(tangent != nullptr, grid, s, alpha, xtr, ntr, ntr_pad, ak, at, xin, fin,
                                         xout, fout, m, t0, dt, n0, nst, vel_scale));
  }
  return 0;
}

// ------------------------------------------------- PATHS (ensembles through posterior draws of the flow)
// what gp2d_paths_eval and gp2d_advect_draws ask of the fit and of the feature table
static int validate_draws(const char* e, const gp2d_kernel_t* k, int64_t n, int64_t ntr, int64_t ntr_pad,
                          int64_t nfeat, int ndraws) {
  const std::string who(e);
  if (validate_kernel(k) != 0) {
    set_error(who + ": k is invalid: " + g_err);
    return -2;
  }
  GP2D_REQUIRE(field_kernel_ok(k),
               who + ": k must be a div-free, curl-free or mixed vector kernel (KIND_SCALAR and the ARD family "
                     "have no velocity draw)");
  GP2D_REQUIRE(ntr_pad > 0 && ntr_pad % PT_TILE == 0, who + ": ntr_pad must be a positive multiple of 64");
  GP2D_REQUIRE(n == 2 * ntr_pad, who + ": n must equal 2 × ntr_pad");
  GP2D_REQUIRE(ntr > 0 && ntr <= ntr_pad, who + ": ntr must be in 1..ntr_pad");
  GP2D_REQUIRE(nfeat >= 0 && nfeat < (int64_t)1 << 31, who + ": nfeat must be >= 0 (and below 2^31)");
  GP2D_REQUIRE(ndraws >= 1, who + ": ndraws must be >= 1");
  GP2D_REQUIRE(ndraws <= 65535, who + ": ndraws must be <= 65535 (one grid row per draw)");
  return 0;
}

int gp2d_paths_eval(const double* alpha, int64_t n, const double* xtr, int64_t ntr, int64_t ntr_pad,
                    const gp2d_kernel_t* k, const double* feat, int64_t nfeat, int ndraws, const double* xg, int64_t m,
                    int dim, double t, double* vel, void* stream) {
  GP2D_REQUIRE((alpha == nullptr) == (k == nullptr),
               "paths_eval: alpha and k must be both NULL (the feature part alone) or both set");
  if (k != nullptr) {
    GP2D_CHECK(validate_draws("paths_eval", k, n, ntr, ntr_pad, nfeat, ndraws));
    GP2D_REQUIRE(dim == 2, "paths_eval: dim must be 2 with alpha (rows (x1, x2), every point at time t)");
  } else {
    GP2D_REQUIRE(nfeat >= 0 && nfeat < (int64_t)1 << 31, "paths_eval: nfeat must be >= 0 (and below 2^31)");
    GP2D_REQUIRE(ndraws >= 1, "paths_eval: ndraws must be >= 1");
    GP2D_REQUIRE(ndraws <= 65535, "paths_eval: ndraws must be <= 65535 (one grid row per draw)");
    GP2D_REQUIRE(dim == 2 || dim == 3, "paths_eval: dim must be 2 (x1, x2) or 3 (t, x1, x2)");
  }
  GP2D_REQUIRE(std::isfinite(t), "paths_eval: t must be finite");
  GP2D_REQUIRE(nfeat == 0 || feat != nullptr, "paths_eval: feat is NULL with nfeat > 0");
  GP2D_REQUIRE(m >= 0 && m < (int64_t)1 << 36, "paths_eval: m out of range");
  if (m == 0) return 0;
  GP2D_REQUIRE(k == nullptr || xtr != nullptr, "paths_eval: xtr is NULL");
  GP2D_REQUIRE(xg != nullptr, "paths_eval: xg is NULL");
  GP2D_REQUIRE(vel != nullptr, "paths_eval: vel is NULL");
  hipStream_t s = S(stream);
  AdvectKernel ak{};
  if (k != nullptr) ak = make_advect_kernel(k);
  const dim3 grid((unsigned)((m + ADV_TILE - 1) / ADV_TILE), (unsigned)ndraws);
  if (k != nullptr && point_dim(k) == 3)
    paths_eval_kernel<true><<<grid, ADV_SLICES * ADV_TILE, 0, s>>>(alpha, n, xtr, ntr, ntr_pad, ak, feat, nfeat, xg, m,
                                                                   dim, t, vel);
  else
    paths_eval_kernel<false><<<grid, ADV_SLICES * ADV_TILE, 0, s>>>(alpha, n, xtr, ntr, ntr_pad, ak, feat, nfeat, xg,
                                                                    m, dim, t, vel);
  return check_launch("paths_eval_kernel");
}

int gp2d_advect_draws(const double* alpha, int64_t n, const double* xtr, int64_t ntr, int64_t ntr_pad,
                      const gp2d_kernel_t* k, const double* feat, int64_t nfeat, int ndraws, const double* x0,
                      int64_t m, int x0_per_draw, double t0, double dt, int nsteps, int save_every, double vel_scale,
                      double* path, void* stream) {
  GP2D_CHECK(validate_draws("advect_draws", k, n, ntr, ntr_pad, nfeat, ndraws));
  GP2D_REQUIRE(nsteps >= 0, "advect_draws: nsteps must be >= 0");
  GP2D_REQUIRE(save_every >= 1, "advect_draws: save_every must be >= 1");
  GP2D_REQUIRE(nsteps == 0 || (std::isfinite(dt) && dt != 0.0), "advect_draws: dt must be finite and non-zero");
  GP2D_REQUIRE(std::isfinite(t0), "advect_draws: t0 must be finite");
  GP2D_REQUIRE(std::isfinite(vel_scale), "advect_draws: vel_scale must be finite");
  GP2D_REQUIRE(x0_per_draw == 0 || x0_per_draw == 1, "advect_draws: x0_per_draw must be 0 or 1");
  GP2D_REQUIRE(nfeat == 0 || feat != nullptr, "advect_draws: feat is NULL with nfeat > 0");
  GP2D_REQUIRE(m >= 0 && m < (int64_t)1 << 36, "advect_draws: m out of range");
  if (m == 0) return 0;
  GP2D_REQUIRE(alpha != nullptr, "advect_draws: alpha is NULL");
  GP2D_REQUIRE(xtr != nullptr, "advect_draws: xtr is NULL");
  GP2D_REQUIRE(x0 != nullptr, "advect_draws: x0 is NULL");
  GP2D_REQUIRE(path != nullptr, "advect_draws: path is NULL");
  hipStream_t s = S(stream);
  const AdvectKernel ak = make_advect_kernel(k);
  const bool st = point_dim(k) == 3;
  const int64_t rec = (int64_t)ndraws * m * 2;   // doubles per record
  paths_init_kernel<<<dim3((unsigned)((m + 255) / 256), (unsigned)ndraws), 256, 0, s>>>(x0, m, x0_per_draw, path);
  GP2D_CHECK(check_launch("paths_init_kernel"));
  const dim3 grid((unsigned)((m + ADV_TILE - 1) / ADV_TILE), (unsigned)ndraws);
  // one launch per saved segment, as in gp2d_advect
  int64_t r = 0;
  for (int n0 = 0; n0 < nsteps; n0 += save_every, ++r) {
    const int nst = std::min(save_every, nsteps - n0);
    const double* xin = path + r * rec;
    double* xout = path + (r + 1) * rec;
    if (st)
      paths_kernel<true><<<grid, ADV_SLICES * ADV_TILE, 0, s>>>(alpha, n, xtr, ntr, ntr_pad, ak, feat, nfeat, xin, xout,
                                                                m, t0, dt, n0, nst, vel_scale);
    else
      paths_kernel<false><<<grid, ADV_SLICES * ADV_TILE, 0, s>>>(alpha, n, xtr, ntr, ntr_pad, ak, feat, nfeat, xin,
                                                                 xout, m, t0, dt, n0, nst, vel_scale);
    GP2D_CHECK(check_launch("paths_kernel"));
  }
  return 0;
}

// ------------------------------------------------- PREDICT (joint posterior covariance)
size_t gp2d_predict_cov_workspace(int64_t n, int64_t m) { return PredictCovWork(n, m).total; }

int gp2d_predict_cov(const double* W, int64_t n, int64_t ldw, const double* alpha, const double* xtr, int64_t ntr,
                     int64_t ntr_pad, const double* xg, int64_t m, const gp2d_kernel_t* k, double diag_add,
                     double* mean, double* cov, int64_t ldc, void* work, size_t work_bytes, void* stream) {
  GP2D_CHECK(refuse_sum(k, "predict_cov"));
  GP2D_CHECK(validate_kernel(k));
  GP2D_REQUIRE(field_kernel_ok(k), "predict_cov: div-free, curl-free or mixed vector kernels only");
  GP2D_REQUIRE(n == 2 * ntr_pad, "predict_cov: n must equal 2 × ntr_pad");
  GP2D_REQUIRE(n % NB == 0 && n > 0, "predict_cov: n must be a positive multiple of 128");
  GP2D_REQUIRE(ntr >= 0 && ntr <= ntr_pad, "predict_cov: bad point count");
  GP2D_REQUIRE(ld_even(ldw, n), "predict_cov: ldw must be >= n and even");
  GP2D_REQUIRE(m >= 0 && postcov_q(m) < (int64_t)1 << 30 && n < (int64_t)1 << 30,
               "predict_cov: m or n out of range");
  if (m == 0) return 0;
  const int64_t mp = postcov_mp(m), q = postcov_q(m);
  GP2D_REQUIRE(ldc >= q, "predict_cov: ldc must be at least q = 2·⌈m/64⌉·64");
  const PredictCovWork lay(n, m);
  GP2D_REQUIRE(work != nullptr && work_bytes >= lay.total, "predict_cov: workspace too small");
  GP2D_REQUIRE(aligned16(W), "predict_cov: W must be 16-byte aligned");
  hipStream_t s = S(stream);
  const PredictCovWork::Ptrs w = lay.at(work);

  // K*ᵀ: rows = training components, columns = target components; the mean as in gp2d_predict
  GP2D_CHECK(assemble_impl(xtr, ntr, ntr_pad, xg, m, mp, k, 0.0, 0, w.Ks, q, s));
  GP2D_CHECK(launch_mean_partials(w.Ks, q, n, alpha, w.pm, s));
  GP2D_CHECK(launch_finalize({w.pm, predict_segments(n), nullptr, 0, q, mp, m, 0, m, 0.0, 0.0, 0, 0, mean, nullptr,
                              nullptr}, s));

  // V = W·K*ᵀ, gp2d_predict's product stored
  GemmParams g = wk_gemm_params(W, ldw, n, w.Ks, q);
  g.C = w.V; g.ldc = q;
  GP2D_CHECK((launch_gemm<false, EPI_STORE>(g, 1, s)));

  // Σ = K(g, g) − VᵀV (+ diag_add·I), padded points identity
  PostcovParams p;
  p.V = w.V; p.ldv = q;
  p.n = (int)n; p.q = (int)q;
  p.xg = xg;
  p.m = (int)m; p.mp = (int)mp;
  p.vp = make_vec_params(k);
  p.diag_add = diag_add;
  p.C = cov; p.ldc = ldc;
  TimedLaunch t(s, 2.0 * (double)ntr * (double)(2 * m) * (double)(2 * m));  // 2N·(2m)², the lower half
  return launch_postcov(p, s);
}

// ------------------------------------------------------------ PREDICT (Ozaki-II)
int gp2d_ozaki_nmod(int64_t n) { return ozaki_nmod_for(n); }

size_t gp2d_ozaki_wres_bytes(int64_t n) {
  const int nm = ozaki_nmod_for(n);
  return nm > 0 ? (size_t)nm * (size_t)n * (size_t)n : 0;
}

static int launch_w_res(const double* W, int64_t n, WRows ldw, const OzakiConsts& oc, int8_t* wres,
                        const double* rowscale, hipStream_t s) {
  // with the S planes of the three-product variance wherever this n has them (ozaki_host.hpp)
  ozaki_w_res_kernel<<<dim3((unsigned)(n / 64), (unsigned)(n / 256)), 256, 0, s>>>(W, n, ldw, oc, wres, rowscale,
                                                                                   oz_s_npad(n));
  return check_launch("ozaki_w_res_kernel");
}

// argument checks of both preparations (bufs_ok: the a-priori paths also refuse NULL buffers)
static int prepare_args(const gp2d_kernel_t* k, int wbits, int kbits, int64_t n, bool bufs_ok, const int* nmod_out) {
  GP2D_CHECK(validate_ozaki_kernel(k));
  GP2D_CHECK(valid_bits(wbits, kbits));
  GP2D_REQUIRE(n % IBM == 0 && n > 0, "ozaki: n must be a positive multiple of 256");
  GP2D_REQUIRE(bufs_ok, "ozaki: NULL buffer");
  GP2D_REQUIRE(nmod_out != nullptr, "ozaki: nmod_out is NULL");
  return 0;
}

// Tail of both preparations: the constants of nmod moduli, the row scales (they need the modulus
// product: finished from the data-driven path's exponents, or made here in the a-priori path's one
// fused pass over W), the residue planes of W, the count.
static int prepare_finish(int nmod, const gp2d_kernel_t* k, int pw, int pb, const double* W, int64_t n, WRows wr,
                          int8_t* wres, double* rowscale, bool fused, int* nmod_out, hipStream_t s) {
  OzakiConsts oc;
  GP2D_CHECK(make_ozaki_consts(nmod, k, oc, pw, pb));
  if (fused) {
    ozaki_w_scale_kernel<<<(unsigned)n, 256, 0, s>>>(W, n, wr, pw, rowscale, nullptr, oc.M, oc.sB, 1);
    GP2D_CHECK(check_launch("ozaki_w_scale_kernel"));
  } else {
    ozaki_rowscale_final_kernel<<<(unsigned)((n + 255) / 256), 256, 0, s>>>(rowscale, n, oc.M, oc.sB);
    GP2D_CHECK(check_launch("ozaki_rowscale_final_kernel"));
  }
  GP2D_CHECK(launch_w_res(W, n, wr, oc, wres, rowscale, s));
  *nmod_out = nmod;
  return 0;
}

int gp2d_ozaki_prepare(const double* W, int64_t n, int64_t ldw, const gp2d_kernel_t* k, int wbits, int kbits,
                       int8_t* wres, double* rowscale, int* nmod_out, void* stream) {
  // ldw = 0 would select WRows' packed layout (gp2d_ozaki_prepare_packed's): refused here
  GP2D_REQUIRE(ld_even(ldw, n), "ozaki: ldw must be >= n and even");
  GP2D_CHECK(prepare_args(k, wbits, kbits, n, true, nmod_out));
  GP2D_REQUIRE(aligned16(W), "ozaki: W must be 16-byte aligned");
  const int pw = ozaki_wbits(wbits), pb = ozaki_kbits(kbits);
  hipStream_t s = S(stream);
  double* l1 = reinterpret_cast<double*>(wres);  // scratch: the planes are written afterwards
  ozaki_w_scale_kernel<<<(unsigned)n, 256, 0, s>>>(W, n, WRows{ldw}, pw, rowscale, l1, 0.0, 0, 0);
  GP2D_CHECK(check_launch("ozaki_w_scale_kernel"));
  std::vector<double> hl1((size_t)n), hs((size_t)n);
  if (hipMemcpyAsync(hl1.data(), l1, sizeof(double) * n, hipMemcpyDeviceToHost, s) != hipSuccess ||
      hipMemcpyAsync(hs.data(), rowscale, sizeof(double) * n, hipMemcpyDeviceToHost, s) != hipSuccess ||
      hipStreamSynchronize(s) != hipSuccess) {
    set_error("ozaki: reading the row bounds failed");
    return -1;
  }
  // Bound on |Pint_ij| = |Σ_k Wint_ik·Bint_kj| per row i, the smaller of
  //   (a) ‖Wint_i‖₁ · max|Bint|  ≤ l1_i · 2^{pB−1}                      (always valid), and
  //   (b) 2^{s_i+s_B}·|V_ij| + rounding terms, with |V_ij| ≤ ‖V_j‖₂ ≤ √kss (the posterior
  //       variance kss − ‖V_j‖² is ≥ 0; factor 2 of slack), rounding ≤ n·2^{pB−2} + l1_i + n.
  // (b) is ≈ 5 bits tighter on the rows of L⁻¹; the identity rows of padded points take (a).
  // A violated bound cannot pass silently: the CRT kernel poisons columns with |V| > 4√kss.
  int sB = 0;
  {
    OzakiConsts probe;
    GP2D_CHECK(make_ozaki_consts(1, k, probe, pw, pb));
    sB = probe.sB;
  }
  const double sq = 2.0 * std::sqrt(gp2d_kernel_diag(k));
  double bmax = 1.0;
  for (int64_t i = 0; i < n; ++i) {
    const double a = std::ldexp(hl1[i] * 1.01, pb - 1);
    const double b = std::ldexp(sq, (int)hs[i] + sB) + std::ldexp((double)n, pb - 2) + hl1[i] + (double)n;
    bmax = std::max(bmax, std::min(a, b));
  }
  const int nmod = ozaki_nmod_bits(std::log2(bmax));
  GP2D_REQUIRE(nmod > 0, "ozaki: row bound exceeds the modulus table");
  return prepare_finish(nmod, k, pw, pb, W, n, WRows{ldw}, wres, rowscale, false, nmod_out, s);
}

static int prepare_apriori(const double* W, int64_t n, WRows wr, const gp2d_kernel_t* k, double diag_add,
                           int wbits, int kbits, int8_t* wres, double* rowscale, int* nmod_out, hipStream_t s) {
  GP2D_CHECK(prepare_args(k, wbits, kbits, n, W != nullptr && wres != nullptr && rowscale != nullptr, nmod_out));
  const int pw = ozaki_wbits(wbits), pb = ozaki_kbits(kbits);
  // the a-priori count bounds the data-driven one for any fit with this K_y diagonal (no host
  // round trip); a violated bound could only come from a failed factor and is poisoned by CRT
  const int nmod = gp2d_ozaki_nmod_apriori(n, k, diag_add, pw, pb);
  GP2D_REQUIRE(nmod > 0, "ozaki: a-priori bound exceeds the modulus table");
  GP2D_REQUIRE(aligned16(W), "ozaki: W (or the packed payload) must be 16-byte aligned");
  // no L1 norms (the count is a-priori): one pass over W for the row exponents, one for the planes
  return prepare_finish(nmod, k, pw, pb, W, n, wr, wres, rowscale, true, nmod_out, s);
}

int gp2d_ozaki_prepare_async(const double* W, int64_t n, int64_t ldw, const gp2d_kernel_t* k, double diag_add,
                             int wbits, int kbits, int8_t* wres, double* rowscale, int* nmod_out, void* stream) {
  GP2D_REQUIRE(ld_even(ldw, n), "ozaki: ldw must be >= n and even");
  return prepare_apriori(W, n, WRows{ldw}, k, diag_add, wbits, kbits, wres, rowscale, nmod_out, S(stream));
}

int gp2d_ozaki_prepare_packed(const double* packed, int64_t n, const gp2d_kernel_t* k, double diag_add, int wbits,
                              int kbits, int8_t* wres, double* rowscale, int* nmod_out, void* stream) {
  GP2D_REQUIRE(n % NB == 0, "ozaki: n must be a multiple of 128 (the packing's row blocks)");
  return prepare_apriori(packed, n, WRows{0}, k, diag_add, wbits, kbits, wres, rowscale, nmod_out, S(stream));
}

// ---- accuracy guard: what W precision the variance needs for this fit
size_t gp2d_ozaki_guard_workspace(int64_t n) {
  if (n <= 0) return 0;
  return 2 * sizeof(double) * (size_t)((n + OZ_GUARD_RSEG - 1) / OZ_GUARD_RSEG) * (size_t)n;
}

int gp2d_ozaki_guard(const double* W, int64_t n, int64_t ldw, int64_t ntr, int64_t npad, double diag_add,
                     double* stats, void* work, size_t work_bytes, void* stream) {
  GP2D_REQUIRE(W && stats && n > 0 && ntr >= 1 && npad >= ntr && (n == npad || n == 2 * npad),
               "ozaki_guard: bad arguments");
  GP2D_REQUIRE(ldw >= n, "ozaki_guard: ldw must be >= n");
  // any δ: the formula is algebra on K = K_y − δI.  δ ≤ 0 (no noise, or a caller's negative
  // "noise") gives a latent variance ≤ 0 at the observations, where no precision bounds the
  // relative error — stats[0] ≤ 0 sends the fit to the FP64 engine
  GP2D_REQUIRE(std::isfinite(diag_add), "ozaki_guard: the diagonal addition (noise + jitter) must be finite");
  GP2D_REQUIRE(work != nullptr && work_bytes >= gp2d_ozaki_guard_workspace(n), "ozaki_guard: workspace too small");
  hipStream_t s = S(stream);
  const int64_t nseg = (n + OZ_GUARD_RSEG - 1) / OZ_GUARD_RSEG;
  double* psum = static_cast<double*>(work);
  double* pmax = psum + nseg * n;
  ozaki_guard_colsq_kernel<<<dim3((unsigned)((n + 255) / 256), (unsigned)nseg), 256, 0, s>>>(W, n, ldw, psum, pmax);
  GP2D_CHECK(check_launch("ozaki_guard_colsq_kernel"));
  ozaki_guard_finish_kernel<<<1, 1024, 0, s>>>(psum, pmax, n, nseg, ntr, npad, diag_add, stats);
  return check_launch("ozaki_guard_finish_kernel");
}

// Elementwise relative error of the ozaki variance, modelled as the sum of its two rounding
// terms, with X = kss / v_min (v_min: the smallest latent posterior variance at the observations,
// gp2d_ozaki_guard's stats[0]):
//   W rows at wbits:  A·2^(49 − wbits)·X^1.5   (Σ_i V_ij·δV_ij with δW ∝ the row maxima)
//   K* at kbits:      B·2^(45 − kbits)·X       (2·δK*·K_y⁻¹k*, ‖K_y⁻¹k*‖ ≲ 1 at the observations)
// A, B: the minimax fit (every measurement at or under the model) to full-grid measurements of the
// emulation against the same engine at its maximal precision (60 / 50 bits), 9 settings (ℓ 2..12
// km, noise 1e-4..5e-2, X = 84..30,145) × 11 precisions (W 49..58, K* 45..50 bits;
// tools/probe_guard.py, profiles/r05_guard_calib.jsonl), raised by 1.2× — the largest margin that
// keeps the bench's own setting (X = 827) at 49 / 45 bits, where it measures 5.9e-11.
static constexpr double OZ_GUARD_A = 2.87e-15, OZ_GUARD_B = 3.58e-14;
double gp2d_ozaki_error_model(double kss, double vmin, int wbits, int kbits) {
  if (!(kss > 0.0)) return INFINITY;
  if (!(vmin > 0.0)) return INFINITY;   // a non-positive latent variance: no precision covers it
  const double X = kss / vmin;
  return OZ_GUARD_A * std::ldexp(1.0, OZ_PW - ozaki_wbits(wbits)) * X * std::sqrt(X) +
         OZ_GUARD_B * std::ldexp(1.0, OZ_PB - ozaki_kbits(kbits)) * X;
}

// The cheapest (wbits, kbits) — fewest total bits, i.e. moduli; then the smaller model — whose
// modelled error is ≤ target: 1 and the bits; 0 if none (the FP64 engine); −1 on bad input.
int gp2d_ozaki_guard_bits(double kss, double vmin, double target, int* wbits, int* kbits) {
  if (!(target > 0.0) || wbits == nullptr || kbits == nullptr) return -1;
  for (int tot = OZ_PW + OZ_PB; tot <= OZ_PW_MAX + OZ_PB_MAX; ++tot) {
    int bw = 0, bk = 0;
    double best = INFINITY;
    for (int pb = OZ_PB; pb <= OZ_PB_MAX; ++pb) {
      const int pw = tot - pb;
      if (pw < OZ_PW || pw > OZ_PW_MAX) continue;
      const double e = gp2d_ozaki_error_model(kss, vmin, pw, pb);
      if (e <= target && e < best) { best = e; bw = pw; bk = pb; }
    }
    if (bw) {
      *wbits = bw;
      *kbits = bk;
      return 1;
    }
  }
  return 0;   // beyond the int8 engine's precision range: the FP64 engine
}

// ---- zero-slab skipping: K* block flags → per-B-tile slab lists (ozaki_slab_list_kernel)
static int g_oz_skip = 1;
void gp2d_ozaki_set_skip(int on) { g_oz_skip = on ? 1 : 0; }

// ---- three block products instead of four (OzakiProducts, ozaki_host.hpp) wherever n allows it;
// off: the four-product path everywhere.  K* planes made ahead carry the form of the setting they
// were made under, so a predict must run under the same one.
static int g_oz_three = 1;
void gp2d_ozaki_set_three_products(int on) { g_oz_three = on ? 1 : 0; }
static bool ozaki_three(int64_t n) { return g_oz_three && oz_s_npad(n) > 0; }

// ---- the predict workspace (inline K* planes, or planes from gp2d_ozaki_kstar): its sizes here
// and its pointers in predict_ozaki_impl both come from OzakiWork (ozaki_host.hpp)
size_t gp2d_predict_ozaki_workspace(int64_t n, int64_t chunk) {
  return OzakiWork(n, chunk, ozaki_nmod_for(n), true).total;
}

size_t gp2d_predict_ozaki_workspace_nmod(int64_t n, int64_t chunk, int nmod) {
  if (nmod <= 0 || nmod > ozaki_nmod_for(n)) return 0;
  return std::max(OzakiWork(n, chunk, nmod, true).total, OzakiWork(n, chunk, nmod, false).total);
}

size_t gp2d_predict_ozaki_planes_workspace(int64_t n, int64_t chunk) {
  return OzakiWork(n, chunk, ozaki_nmod_for(n), false).total;
}

// The chunk of grid points starting at c0: valid points, points padded to whole 256-row tiles
// per component half (B aliasing), columns, the chunk's grid points, ozaki_kstar_kernel's grid
struct OzakiChunk {
  int64_t cv, cp, ncols;
  const double* xg;
  dim3 kgrid;
  OzakiChunk(const double* xg0, int64_t m, int64_t c0, int64_t chunk, int64_t ntr_pad, const gp2d_kernel_t* k)
      : cv(std::min<int64_t>(chunk, m - c0)), cp(round_up(cv, IBN)), ncols(2 * cp), xg(xg0 + point_dim(k) * c0),
        kgrid((unsigned)((ntr_pad + OZ_KS_T - 1) / OZ_KS_T), (unsigned)(cp / OZ_KS_P)) {}
};

// ozaki_kstar_kernel on chunk c, with buffer stores whenever a plane (n × 2·cp bytes) is below 2 GiB
static int launch_kstar(const OzakiChunk& c, hipStream_t s, const double* xtr, int64_t ntr, int64_t npad,
                        const VecParams& vp, const double* alpha, const OzakiConsts& oc, int8_t* bres, double* pm,
                        uint8_t* flags) {
  // planes of (a − c, c, b − c) for the three-product GEMM, else (a, c, b)
  const int form = !ozaki_three(2 * npad) ? KS_PLAIN : oc.pb <= 49 ? KS_DIFF_X : KS_DIFF_R;
  const bool off32 = (uint64_t)(2 * npad) * (uint64_t)c.ncols < (1ull << 31);
  auto launch = [&](auto off32_c, auto form_c) {
    ozaki_kstar_kernel<decltype(off32_c)::value, decltype(form_c)::value>
        <<<c.kgrid, 256, 0, s>>>(xtr, ntr, npad, c.xg, c.cv, c.cp, vp, alpha, oc, bres, pm, flags);
  };
  auto pick = [&](auto off32_c) {
    if (form == KS_PLAIN) launch(off32_c, std::integral_constant<int, KS_PLAIN>{});
    else if (form == KS_DIFF_X) launch(off32_c, std::integral_constant<int, KS_DIFF_X>{});
    else launch(off32_c, std::integral_constant<int, KS_DIFF_R>{});
  };
  if (off32) pick(std::true_type{});
  else pick(std::false_type{});
  return check_launch("ozaki_kstar_kernel");
}

// One chunked predict over the m grid points, in the workspace `work` laid out by `lay`.  K*
// residue planes come either from the inline ozaki_kstar_kernel (pre == nullptr: planes in the
// workspace, mean partials Σ α·K*) or from gp2d_ozaki_kstar run earlier (planes and block flags
// per chunk in pre_base as *pre lays them out; the same kernel then runs mean-only, so the mean
// is bit-identical to the inline path).  The int8 GEMMs skip the K slabs whose K* tile is all
// zero (exact: they add nothing); flags → slab lists per chunk in `skip` (oz_list_bytes).
static int predict_ozaki_impl(const int8_t* wres, const double* rowscale, int nmod, int kbits, int64_t n,
                              const double* alpha, const double* xtr, int64_t ntr,
                              int64_t ntr_pad, const double* xg, int64_t m, const gp2d_kernel_t* k, int var_mode,
                              double noise, int compute_var, double* mean, double* var,
                              const int64_t* out_order, int64_t chunk, const OzakiWork& lay, void* work,
                              const KstarBuf* pre, const int8_t* pre_base, hipStream_t s) {
  const auto [bres, cres, pm, P, flags, skip] = lay.at(work);
  OzakiConsts oc;
  GP2D_CHECK(make_ozaki_consts(nmod, k, oc, OZ_PW, ozaki_kbits(kbits)));   // pw is in the row scales already
  const int nm = oc.nmod;
  // the GEMM epilogue's biased sums (ozaki_mod_u32) stay below 2^32 for K = n < 2^17
  GP2D_REQUIRE(n < 131072, "ozaki: the int8 GEMM epilogue needs n < 131072 (N_train < 65536)");
  const int64_t nmseg = (ntr_pad + OZ_KS_T - 1) / OZ_KS_T;
  const int64_t npseg = (n + OZ_CRT_ROWS - 1) / OZ_CRT_ROWS;
  const double kss = gp2d_kernel_diag(k);
  const double add = (var_mode == GP2D_VAR_LATENT) ? 0.0 : noise;
  const int clip = (var_mode == GP2D_VAR_CLIPPED);
  const VecParams vp = make_vec_params(k);
  OzakiConsts oc_mean_only = oc;
  oc_mean_only.nmod = 0;   // mean only: K*·α without the residue planes
  int64_t ci = 0;
  for (int64_t c0 = 0; c0 < m; c0 += chunk, ++ci) {
    const OzakiChunk c(xg, m, c0, chunk, ntr_pad, k);
    const int64_t cv = c.cv, cp = c.cp, ncols = c.ncols;
    const int8_t* B = pre ? pre_base + pre->planes_at(ci) : bres;
    const uint8_t* F = pre ? reinterpret_cast<const uint8_t*>(pre_base + pre->flags_at(ci)) : flags;
    const size_t bplane = (size_t)ncols * n;
    const bool inline_planes = compute_var && !pre;
    GP2D_CHECK(launch_kstar(c, s, xtr, ntr, ntr_pad, vp, alpha, inline_planes ? oc : oc_mean_only,
                            pre ? nullptr : bres, pm, inline_planes ? flags : nullptr));
    const int nbj = (int)(ncols / IBN), kslabs = (int)(n / IBK);
    const bool use_skip = compute_var && g_oz_skip && kslabs <= (1 << 20);
    int* slist = skip;
    int* scnt = skip + (int64_t)nbj * kslabs;
    if (use_skip) {
      ozaki_slab_list_kernel<<<(unsigned)nbj, 64, 0, s>>>(F, (int)(ntr_pad / OZ_KS_T), nbj, kslabs, slist, scnt);
      GP2D_CHECK(check_launch("ozaki_slab_list_kernel"));
    }
    if (compute_var) {
      const double nv = 2.0 * (double)ntr;
      TimedLaunch timed(s, 2.0 * (double)cv * nv * nv);  // FP64-equivalent algorithmic flop
      // The chunk's block products (OzakiProducts: three where n allows, else four in one launch),
      // each over the moduli.  Four products, small n: every modulus in one launch (moduli on
      // grid.z: no launch gap and no tail between the moduli, −3 % per chunk at n = 2048,
      // profiles/r04_zbatch.txt); large n: one launch per modulus (the same within 0.2 %).  Three
      // products: always every modulus in one launch per product — three shorter launches per
      // modulus would each end in a tail of their own (measured).  With the K* planes
      // in the workspace the three products are independent: P3 goes into the planes' unread block
      // and the CRT pass adds the residues; with the caller's planes P2 and P3 add P1 in their epilogue
      const bool three = ozaki_three(n);
      const OzakiProducts prods(n, cp, three, !pre);
      const int zper = (three || n <= kIgemmZBatchMaxN) ? nm : 1;
      for (int l0 = 0; l0 < nm; l0 += zper) {
        const int nz = std::min(zper, nm - l0);
        // 256 output columns per workgroup, one workgroup per CU (the 128-wide shape with two
        // workgroups per CU measured −5 %: tools/microbench/igemm_bench.hip)
        constexpr int tbn = 256, nst = I_NSTAGE;
        const int8_t* Al = wres + (size_t)l0 * n * n;
        const int8_t* Bl = B + (size_t)l0 * bplane;
        for (int q = 0; q < prods.count; ++q) {
          // the output: V's plane in cres, or (P3 where the CRT pass sums) its place in the K* planes
          const bool in_b = prods.sum_in_crt && q == 2;
          uint8_t* Cl = in_b ? reinterpret_cast<uint8_t*>(bres) + (size_t)l0 * bplane + prods.p3_off
                             : cres + (size_t)l0 * n * ncols;
          IgemmZ zb{(int64_t)n * n, (int64_t)bplane, in_b ? (int64_t)bplane : (int64_t)n * ncols, {}};
          for (int u = 0; u < nz; ++u) zb.m[u] = oc.m[l0 + u];
          const dim3 ggrid(prods.gx[q], prods.gy[q], (unsigned)nz);
          igemm_nt_mod_kernel<tbn, nst><<<ggrid, 2 * tbn, 0, s>>>(Al, Bl, Cl, in_b ? n / 2 : n, kslabs, oc.m[l0],
                                                                  prods.prod[q], use_skip ? slist : nullptr,
                                                                  use_skip ? scnt : nullptr, zb);
          GP2D_CHECK(check_launch("igemm_nt_mod_kernel"));
        }
      }
      timed.stop();
      if (prods.sum_in_crt) {
        const dim3 cgrid((unsigned)((cp + OZ_CRT_BCOLS - 1) / OZ_CRT_BCOLS), (unsigned)npseg);
        ozaki_crt_colsq_kernel<true><<<cgrid, 256, 0, s>>>(cres, n, ncols, oc, rowscale, P,
                                                           reinterpret_cast<const uint8_t*>(bres) + prods.p3_off,
                                                           (int64_t)bplane, prods.p3_blk);
      } else {
        const dim3 cgrid((unsigned)((ncols + OZ_CRT_BCOLS - 1) / OZ_CRT_BCOLS), (unsigned)npseg);
        ozaki_crt_colsq_kernel<false><<<cgrid, 256, 0, s>>>(cres, n, ncols, oc, rowscale, P, nullptr, 0, 0);
      }
      GP2D_CHECK(check_launch("ozaki_crt_colsq_kernel"));
    }
    GP2D_CHECK(launch_finalize({pm, nmseg, P, npseg, ncols, cp, cv, c0, m, kss, add, clip, compute_var, mean, var,
                                out_order}, s));
  }
  return 0;
}

// Argument checks of both predict entry points, in their order (ptrs_ok: the planes path also
// requires alpha and the planes).  1: no grid points, nothing to do.
static int predict_ozaki_args(const gp2d_kernel_t* k, int64_t n, int64_t ntr_pad, int64_t chunk, int var_mode,
                              bool ptrs_ok, int64_t m, int nmod, int kbits, const OzakiWork& lay, const void* work,
                              size_t work_bytes) {
  GP2D_CHECK(validate_ozaki_kernel(k));
  GP2D_REQUIRE(n == 2 * ntr_pad && n % IBM == 0, "ozaki: n must equal 2·ntr_pad and be a multiple of 256");
  GP2D_REQUIRE(chunk > 0 && chunk % (IBN / 2) == 0, "ozaki: chunk must be a positive multiple of 128");
  GP2D_REQUIRE(var_mode >= 0 && var_mode <= 2, "predict: bad var_mode");
  GP2D_REQUIRE(ptrs_ok, "ozaki_planes: alpha and the K* planes are required");
  if (m <= 0) return 1;
  GP2D_REQUIRE(nmod > 0 && nmod <= ozaki_nmod_for(n), "ozaki: nmod exceeds the moduli table");
  GP2D_REQUIRE(work != nullptr && work_bytes >= lay.total, "ozaki: workspace too small");
  return valid_bits(0, kbits);
}

int gp2d_predict_ozaki(const int8_t* wres, const double* rowscale, int nmod, int kbits, int64_t n, const double* alpha,
                       const double* xtr,
                       int64_t ntr, int64_t ntr_pad, const double* xg, int64_t m, const gp2d_kernel_t* k,
                       int var_mode, double noise, int compute_var, double* mean, double* var,
                       const int64_t* out_order, int64_t chunk, void* work, size_t work_bytes, void* stream) {
  const OzakiWork lay(n, chunk, nmod, true);
  const int rc = predict_ozaki_args(k, n, ntr_pad, chunk, var_mode, true, m, nmod, kbits, lay, work, work_bytes);
  if (rc != 0) return rc < 0 ? rc : 0;
  return predict_ozaki_impl(wres, rowscale, nmod, kbits, n, alpha, xtr, ntr, ntr_pad, xg, m, k, var_mode, noise,
                            compute_var, mean, var, out_order, chunk, lay, work, nullptr, nullptr, S(stream));
}

// ---- K* residue planes ahead of the fit (they depend on the points and the kernel only)
int gp2d_ozaki_nmod_apriori(int64_t n, const gp2d_kernel_t* k, double diag_add, int wbits, int kbits) {
  // gp2d_ozaki_prepare's per-row bound (b) with the largest row exponent any fit can have:
  // W_ii = 1/L_ii ≥ 1/√(K_y,ii) (L_ii² = K_y,ii − Σ L_ik²), so max_k |W_ik| ≥ 1/√(kss + diag_add)
  // and s_i = p−1−⌊log2 max|W_i|⌋ ≤ s_max.  (1 − 2^-40) absorbs the rounding of L_ii; the
  // identity rows of padded points take bound (a) = 1.01·2^{2p−2}.  prepare's data-driven
  // count never exceeds this one.
  if (validate_ozaki_kernel(k) != 0 || n <= 0 || valid_bits(wbits, kbits) != 0) return -1;
  const int pw = ozaki_wbits(wbits), pb = ozaki_kbits(kbits);
  const double kss = gp2d_kernel_diag(k);
  const double dmin = (1.0 - std::ldexp(1.0, -40)) / std::sqrt(kss + diag_add);
  const int smax = pw - 1 - (int)std::floor(std::log2(dmin));
  OzakiConsts probe;
  if (make_ozaki_consts(1, k, probe, pw, pb) != 0) return -1;
  const double sq = 2.0 * std::sqrt(kss);
  const double b = std::ldexp(sq, smax + probe.sB) + std::ldexp((double)n, pb - 2) + std::ldexp((double)n, pw) +
                   (double)n;
  const double a_id = 1.01 * std::ldexp(1.0, pw + pb - 2);
  return ozaki_nmod_bits(std::log2(std::max(b, a_id)));
}

size_t gp2d_ozaki_kstar_bytes(int64_t n, int64_t m, int64_t chunk, int nmod) {
  if (n <= 0 || m <= 0 || chunk <= 0 || nmod <= 0) return 0;
  return (size_t)((m + chunk - 1) / chunk) * KstarBuf(n, chunk, nmod).stride;
}

int gp2d_ozaki_kstar(const double* xtr, int64_t ntr, int64_t ntr_pad, const double* xg, int64_t m,
                     const gp2d_kernel_t* k, int nmod, int kbits, int64_t chunk, int8_t* bres, size_t bres_bytes,
                     void* stream) {
  GP2D_CHECK(validate_ozaki_kernel(k));
  const int64_t n = 2 * ntr_pad;
  GP2D_REQUIRE(ntr_pad > 0 && n % IBM == 0 && ntr <= ntr_pad, "ozaki_kstar: 2·ntr_pad must be a multiple of 256");
  GP2D_REQUIRE(chunk > 0 && chunk % (IBN / 2) == 0, "ozaki_kstar: chunk must be a positive multiple of 128");
  GP2D_REQUIRE(nmod > 0 && nmod <= OZ_MAXMOD, "ozaki_kstar: bad number of moduli");
  GP2D_CHECK(valid_bits(0, kbits));
  if (m <= 0) return 0;
  GP2D_REQUIRE(bres != nullptr && bres_bytes >= gp2d_ozaki_kstar_bytes(n, m, chunk, nmod),
               "ozaki_kstar: plane buffer too small");
  OzakiConsts oc;
  GP2D_CHECK(make_ozaki_consts(nmod, k, oc, OZ_PW, ozaki_kbits(kbits)));
  const VecParams vp = make_vec_params(k);
  const KstarBuf buf(n, chunk, nmod);
  hipStream_t s = S(stream);
  int64_t ci = 0;
  for (int64_t c0 = 0; c0 < m; c0 += chunk, ++ci) {
    const OzakiChunk c(xg, m, c0, chunk, ntr_pad, k);
    GP2D_CHECK(launch_kstar(c, s, xtr, ntr, ntr_pad, vp, nullptr, oc, bres + buf.planes_at(ci), nullptr,
                            reinterpret_cast<uint8_t*>(bres + buf.flags_at(ci))));
  }
  return 0;
}

int gp2d_predict_ozaki_planes(const int8_t* wres, const double* rowscale, int nmod, int kbits, int64_t n,
                              const double* alpha, const double* xtr, int64_t ntr, int64_t ntr_pad, const double* xg,
                              int64_t m, const gp2d_kernel_t* k, int var_mode, double noise, const int8_t* bres,
                              int nmod_b, int kbits_b, double* mean, double* var, const int64_t* out_order, int64_t chunk, void* work,
                              size_t work_bytes, void* stream) {
  const OzakiWork lay(n, chunk, nmod, false);
  const int rc = predict_ozaki_args(k, n, ntr_pad, chunk, var_mode, alpha != nullptr && bres != nullptr, m, nmod,
                                    kbits, lay, work, work_bytes);
  if (rc != 0) return rc < 0 ? rc : 0;
  if (nmod > nmod_b || ozaki_kbits(kbits) != ozaki_kbits(kbits_b)) {
    set_error("ozaki_planes: the fit needs more moduli, or another K* precision, than the planes carry");
    return -3;
  }
  const KstarBuf buf(n, chunk, nmod_b);
  return predict_ozaki_impl(wres, rowscale, nmod, kbits, n, alpha, xtr, ntr, ntr_pad, xg, m, k, var_mode, noise, 1, mean,
                            var, out_order, chunk, lay, work, &buf, bres, S(stream));
}

int gp2d_morton_codes(const double* pts, int64_t n, int dim, double* bbox, int64_t* codes, void* stream) {
  GP2D_REQUIRE(pts && bbox && codes && n > 0 && (dim == 2 || dim == 3), "morton_codes: bad arguments");
  hipStream_t s = S(stream);
  morton_bbox_kernel<<<1, 1024, 0, s>>>(pts, n, dim, bbox);
  GP2D_CHECK(check_launch("morton_bbox_kernel"));
  morton_code_kernel<<<(unsigned)((n + 255) / 256), 256, 0, s>>>(pts, n, dim, bbox, codes);
  return check_launch("morton_code_kernel");
}

// ---- Morton order on the device (order.hpp): codes → stable radix sort → gathered points
static int64_t rs_tiles(int64_t n) { return (n + RS_TILE - 1) / RS_TILE; }
static size_t rs_hist_bytes(int64_t n) { return (size_t)round_up((int64_t)RS_BINS * rs_tiles(n) * 4, 256); }

size_t gp2d_morton_sort_workspace(int64_t n) {
  if (n <= 0) return 0;
  // bbox | codes ×2 | index ping-pong buffer | per-tile digit counts
  return 256 + 3 * (size_t)round_up(n * 8, 256) + rs_hist_bytes(n);
}

int gp2d_morton_sort(const double* pts, int64_t n, int dim, double* sorted, int64_t* order, void* work,
                     size_t work_bytes, void* stream) {
  GP2D_REQUIRE(pts && order && n > 0 && (dim == 2 || dim == 3), "morton_sort: bad arguments");
  GP2D_REQUIRE(n < (int64_t)1 << 31, "morton_sort: at most 2^31 − 1 points");
  GP2D_REQUIRE(work != nullptr && work_bytes >= gp2d_morton_sort_workspace(n), "morton_sort: workspace too small");
  hipStream_t s = S(stream);
  char* w = static_cast<char*>(work);
  double* bbox = reinterpret_cast<double*>(w);
  const size_t nb8 = (size_t)round_up(n * 8, 256);
  uint64_t* ka = reinterpret_cast<uint64_t*>(w + 256);
  uint64_t* kb = reinterpret_cast<uint64_t*>(w + 256 + nb8);
  int64_t* vb = reinterpret_cast<int64_t*>(w + 256 + 2 * nb8);
  uint32_t* hist = reinterpret_cast<uint32_t*>(w + 256 + 3 * nb8);
  GP2D_CHECK(gp2d_morton_codes(pts, n, dim, bbox, reinterpret_cast<int64_t*>(ka), stream));
  // 21 bits per coordinate: 6 digit passes in 2-D, 8 in 3-D — an even count, so the indices of
  // the last pass land in `order` (pass p writes the ping-pong buffer of its parity)
  const int passes = (21 * dim + RS_BITS - 1) / RS_BITS;
  const unsigned tiles = (unsigned)rs_tiles(n);
  for (int p = 0; p < passes; ++p) {
    const uint64_t* kin = (p & 1) ? kb : ka;
    uint64_t* kout = (p & 1) ? ka : kb;
    const int64_t* vin = p == 0 ? nullptr : ((p & 1) ? vb : order);
    int64_t* vout = (p & 1) ? order : vb;
    radix_hist_kernel<<<tiles, RS_THREADS, 0, s>>>(kin, n, RS_BITS * p, hist);
    GP2D_CHECK(check_launch("radix_hist_kernel"));
    radix_scan_kernel<<<1, 1024, 0, s>>>(hist, (int64_t)RS_BINS * tiles);
    GP2D_CHECK(check_launch("radix_scan_kernel"));
    radix_scatter_kernel<<<tiles, RS_THREADS, 0, s>>>(kin, vin, n, RS_BITS * p, hist, kout, vout);
    GP2D_CHECK(check_launch("radix_scatter_kernel"));
  }
  static_assert((((21 * 2 + RS_BITS - 1) / RS_BITS) & 1) == 0 && (((21 * 3 + RS_BITS - 1) / RS_BITS) & 1) == 0,
                "an even number of digit passes");
  if (sorted == nullptr) return 0;
  return gp2d_gather_rows(pts, order, n, dim, sorted, stream);
}

int gp2d_gather_rows(const double* src, const int64_t* order, int64_t n, int64_t dim, double* dst, void* stream) {
  GP2D_REQUIRE(src && order && dst && n >= 0 && dim >= 1, "gather_rows: bad arguments");
  GP2D_REQUIRE(src != dst, "gather_rows: src and dst must not alias");
  GP2D_REQUIRE(n * dim < ((int64_t)1 << 40), "gather_rows: too many elements");
  if (n == 0) return 0;
  gather_rows_kernel<<<(unsigned)((n * dim + 255) / 256), 256, 0, S(stream)>>>(src, order, n, dim, dst);
  return check_launch("gather_rows_kernel");
}

int gp2d_obs_pad(const double* y, int64_t ntr, int64_t npad, int bd, const int64_t* perm, double* out,
                 void* stream) {
  GP2D_REQUIRE(y && out && ntr >= 0 && npad >= ntr && npad > 0 && (bd == 1 || bd == 2), "obs_pad: bad arguments");
  const int64_t t = (int64_t)bd * npad;
  obs_pad_kernel<<<(unsigned)((t + 255) / 256), 256, 0, S(stream)>>>(y, ntr, npad, bd, perm, out);
  return check_launch("obs_pad_kernel");
}

int gp2d_status_flip(int* status, int count, void* stream) {
  GP2D_REQUIRE(status && count >= 0, "status_flip: bad arguments");
  if (count == 0) return 0;
  status_flip_kernel<<<(unsigned)((count + 63) / 64), 64, 0, S(stream)>>>(status, count);
  return check_launch("status_flip_kernel");
}

// ------------------------------------------------- LOG MARGINAL LIKELIHOOD (§8f.1)
int gp2d_lml(const double* W, int64_t n, int64_t ldw, const double* alpha, const double* y, int64_t nobs,
             double* lml_dev, void* stream) {
  GP2D_REQUIRE(W && alpha && y && lml_dev, "lml: NULL argument");
  GP2D_REQUIRE(n > 0 && nobs >= 0 && nobs <= n, "lml: bad sizes");
  GP2D_REQUIRE(ldw >= n, "lml: ldw must be >= n");
  hipStream_t s = S(stream);
  lml_terms_kernel<<<1, 256, 0, s>>>(W, n, ldw, alpha, y, nobs, lml_dev);
  return check_launch("lml_terms_kernel");
}

int gp2d_lml_trend(const double* W, int64_t n, int64_t wld, const double* alpha, const double* y, int64_t nobs,
                   const gp2d_trend_t* trend, const double* block, double* lml_dev, void* stream) {
  GP2D_CHECK(validate_trend(trend, block, "lml_trend"));
  GP2D_REQUIRE(W && alpha && y && lml_dev, "lml_trend: NULL argument");
  GP2D_REQUIRE(n > 0 && nobs >= 0 && nobs <= n, "lml_trend: bad sizes");
  GP2D_REQUIRE(wld >= n, "lml_trend: wld must be >= n");
  hipStream_t s = S(stream);
  lml_terms_kernel<<<1, 256, 0, s>>>(W, n, wld, alpha, y, nobs, lml_dev);
  GP2D_CHECK(check_launch("lml_terms_kernel"));
  lml_trend_terms_kernel<<<1, 64, 0, s>>>(lml_dev, block, trend_q(trend->order));
  return check_launch("lml_trend_terms_kernel");
}

int gp2d_lml_grad_count(const gp2d_kernel_t* k) {
  if (validate_kernel(k) != 0) return -2;
  if (is_sum_family(k))   // per term its weight and its own entries without noise, then noise
    return k->nterms * (sum_term(k, 0)->family == GP2D_FAMILY_VECTOR_ST ? 6 : 4) + 1;
  if (k->family == GP2D_FAMILY_VECTOR2D) return 4;
  if (k->family == GP2D_FAMILY_VECTOR_ST) return 6;
  return k->nterms * (1 + k->dim) + 1;
}

int gp2d_kernel_grad_count(const gp2d_kernel_t* k) {
  const int n = gp2d_lml_grad_count(k);
  return n < 0 ? n : n - 1;
}

}  // extern "C"

namespace {
// Output order → accumulator slots (lml.hpp): GPy param_array order, noise last.
SlotMap grad_slots(const gp2d_kernel_t* k, bool with_noise) {
  SlotMap m{};
  m.ng = 0;
  if (k->family == GP2D_FAMILY_VECTOR2D || k->family == GP2D_FAMILY_VECTOR_ST) {
    for (int a = 0; a < 3; ++a) m.slot[m.ng++] = a;
    if (k->family == GP2D_FAMILY_VECTOR_ST) { m.slot[m.ng++] = 4; m.slot[m.ng++] = 5; }
    if (with_noise) m.slot[m.ng++] = 3;
  } else {
    for (int t = 0; t < k->nterms; ++t) {
      m.slot[m.ng++] = t * 4;
      for (int d = 0; d < k->dim; ++d) m.slot[m.ng++] = t * 4 + 1 + d;
    }
    if (with_noise) m.slot[m.ng++] = 8;
  }
  return m;
}

// One term of a sum: its weight, then the term's own entries in its family's order; the noise
// (the last term's launch only) after them.
SlotMap sum_term_slots(const gp2d_kernel_t* kt, bool with_noise) {
  SlotMap m = grad_slots(kt, with_noise);
  for (int g = m.ng; g > 0; --g) m.slot[g] = m.slot[g - 1];
  m.slot[0] = SumVecFamily::WEIGHT;
  ++m.ng;
  return m;
}

// A pair gradient (lml.hpp): weights ⊙ ∂K/∂θ summed over the pairs of the na row points xa and the
// nb column points xb (ncols_pad: nb padded to whole tiles) into `partial`, then out[g] = scale ·
// the blocks' sum of output g's slot.
template <class Weights>
int launch_pair_grad(const gp2d_kernel_t* k, const double* xa, int64_t na, const double* xb, int64_t nb,
                     int64_t ncols_pad, const Weights& weights, double* partial, double scale, bool with_noise,
                     double* out, hipStream_t s) {
  const dim3 grid((unsigned)(ncols_pad / PT_TILE), (unsigned)((na + LML_ROWS - 1) / LML_ROWS));
  if (is_sum_family(k)) {
    // one launch per term into the same partials (stream order keeps them apart), each term's
    // outputs at its offset; the noise slot, equal in every launch, is taken from the last one
    for (int t = 0; t < k->nterms; ++t) {
      const gp2d_kernel_t* kt = sum_term(k, t);
      const SumVecFamily fam{{make_vec_params(kt), kt->l_df, kt->l_cf, kt->ls[0][0]}, sum_weight(k, t)};
      pair_grad_kernel<<<grid, 256, 0, s>>>(xa, na, xb, nb, fam, weights, partial);
      GP2D_CHECK(check_launch("pair_grad_kernel"));
      const SlotMap sm = sum_term_slots(kt, with_noise && t == k->nterms - 1);
      grad_sum_kernel<<<sm.ng, 256, 0, s>>>(partial, grad_blocks(ncols_pad, na), sm, scale, out);
      GP2D_CHECK(check_launch("grad_sum_kernel"));
      out += sm.ng;
    }
    return 0;
  }
  if (is_vector_family(k)) {
    const VecFamily fam{{make_vec_params(k), k->l_df, k->l_cf, k->ls[0][0]}};
    pair_grad_kernel<<<grid, 256, 0, s>>>(xa, na, xb, nb, fam, weights, partial);
  } else {
    const ArdFamily fam{make_ard_params(k)};
    pair_grad_kernel<<<grid, 256, 0, s>>>(xa, na, xb, nb, fam, weights, partial);
  }
  GP2D_CHECK(check_launch("pair_grad_kernel"));
  const SlotMap sm = grad_slots(k, with_noise);
  grad_sum_kernel<<<sm.ng, 256, 0, s>>>(partial, grad_blocks(ncols_pad, na), sm, scale, out);
  return check_launch("grad_sum_kernel");
}
}  // namespace

extern "C" {

size_t gp2d_lml_grad_workspace(int64_t n) { return LmlGradWork(n).total; }

// gp2d_lml_grad, and with a trend (order, block) gp2d_lml_grad_trend: the rank-q update of C between
// the product and the pair loop
static int lml_grad_impl(const double* W, int64_t n, int64_t ldw, const double* alpha, const double* xtr, int64_t ntr,
                         int64_t ntr_pad, const gp2d_kernel_t* k, double* grad_dev, void* work, size_t work_bytes,
                         void* stream, int order, const double* block) {
  GP2D_CHECK(validate_kernel(k));
  GP2D_REQUIRE(W && alpha && xtr && grad_dev, "lml_grad: NULL argument");
  const int bd = gp2d_block_dim(k);
  GP2D_REQUIRE(n == bd * ntr_pad && ntr_pad % PT_TILE == 0, "lml_grad: n must equal block_dim × ntr_pad");
  GP2D_REQUIRE(n % NB == 0, "lml_grad: n must be a multiple of 128");
  GP2D_REQUIRE(ntr >= 1 && ntr <= ntr_pad, "lml_grad: bad sizes");
  GP2D_REQUIRE(block == nullptr || bd == 2, "lml_grad_trend: k must be a vector kernel (two components per point)");
  GP2D_REQUIRE(ld_even(ldw, n),
               block ? "lml_grad_trend: wld must be >= n and even" : "lml_grad: ldw must be >= n and even");
  GP2D_REQUIRE(work != nullptr && work_bytes >= gp2d_lml_grad_workspace(n), "lml_grad: workspace too small");
  GP2D_REQUIRE(aligned16(W), "lml_grad: W must be 16-byte aligned");
  // (the two checks above cover both operands of the TN product below: as A and as B, W is read in
  // 16-byte pieces at W + k·ldw + i0 + 2·j)
  hipStream_t s = S(stream);
  const auto [C, partial] = LmlGradWork(n).at(work);
  // C = WᵀW = K_y⁻¹, lower tiles only: W is read K-major on both sides, op(A) = Wᵀ is upper
  GemmParams p = gemm_params();
  p.A = W; p.lda = ldw;
  p.B = W; p.ldb = ldw;
  p.C = C; p.ldc = n;
  p.M = (int)n; p.N = (int)n; p.K = (int)n;
  p.a_upper = 1; p.c_lower = 1;
  GP2D_CHECK((launch_gemm<false, EPI_STORE, true>(p, 1, s)));
  if (block) {   // C ← K_y⁻¹ − B0·A⁻¹·B0ᵀ on the stored triangle
    const dim3 grid((unsigned)n, (unsigned)((n + 255) / 256));
    if (order == 0) trend_rank_update_kernel<2><<<grid, 256, 0, s>>>(C, n, block);
    else trend_rank_update_kernel<TREND_QMAX><<<grid, 256, 0, s>>>(C, n, block);
    GP2D_CHECK(check_launch("trend_rank_update_kernel"));
  }
  return launch_pair_grad(k, xtr, ntr, xtr, ntr, ntr_pad, TraceWeights{C, n, alpha, ntr_pad}, partial, 0.5, true,
                          grad_dev, s);
}

int gp2d_lml_grad(const double* W, int64_t n, int64_t ldw, const double* alpha, const double* xtr, int64_t ntr,
                  int64_t ntr_pad, const gp2d_kernel_t* k, double* grad_dev, void* work, size_t work_bytes,
                  void* stream) {
  return lml_grad_impl(W, n, ldw, alpha, xtr, ntr, ntr_pad, k, grad_dev, work, work_bytes, stream, 0, nullptr);
}

size_t gp2d_lml_grad_trend_workspace(int64_t n) { return gp2d_lml_grad_workspace(n); }

int gp2d_lml_grad_trend(const double* W, int64_t n, int64_t wld, const double* alpha, const double* xtr, int64_t ntr,
                        int64_t ntr_pad, const gp2d_kernel_t* k, const gp2d_trend_t* trend, const double* block,
                        double* grad_dev, void* work, size_t work_bytes, void* stream) {
  GP2D_CHECK(validate_trend(trend, block, "lml_grad_trend"));
  return lml_grad_impl(W, n, wld, alpha, xtr, ntr, ntr_pad, k, grad_dev, work, work_bytes, stream, trend->order,
                       block);
}

size_t gp2d_kernel_grad_workspace(int64_t na, int64_t nb) { return KernelGradWork(na, nb).total; }

int gp2d_kernel_grad(const double* xa, int64_t na, const double* xb, int64_t nb, const gp2d_kernel_t* k,
                     const double* dL_dK, int64_t ld, double* grad_dev, void* work, size_t work_bytes,
                     void* stream) {
  GP2D_CHECK(validate_kernel(k));
  GP2D_REQUIRE(xa && xb && dL_dK && grad_dev, "kernel_grad: NULL argument");
  GP2D_REQUIRE(na >= 1 && nb >= 1, "kernel_grad: empty point set");
  const int bd = gp2d_block_dim(k);
  GP2D_REQUIRE(ld >= bd * nb, "kernel_grad: ld too small");
  GP2D_REQUIRE(work != nullptr && work_bytes >= gp2d_kernel_grad_workspace(na, nb), "kernel_grad: workspace too small");
  return launch_pair_grad(k, xa, na, xb, nb, round_up(nb, PT_TILE), DenseWeights{dL_dK, ld, na, nb},
                          KernelGradWork(na, nb).at(work).partial, 1.0, false, grad_dev, S(stream));
}

// ------------------------------------------------- leave-one-out density and gradient (loo.hpp)
size_t gp2d_loo_grad_workspace(int64_t n) { return (n > 0 && n % NB == 0) ? LooGradWork(n).total : 0; }

int gp2d_loo_grad(const double* W, int64_t n, int64_t wld, const double* alpha, const double* y, const double* xtr,
                  int64_t ntr, int64_t ntr_pad, const gp2d_kernel_t* k, double* value_dev, double* grad_dev,
                  int* info_dev, void* work, size_t work_bytes, void* stream) {
  GP2D_CHECK(validate_kernel(k));
  GP2D_REQUIRE(W && alpha && y && xtr && value_dev && info_dev, "loo_grad: NULL argument");
  const int bd = gp2d_block_dim(k);
  GP2D_REQUIRE(ntr_pad > 0 && n == bd * ntr_pad && ntr_pad % PT_TILE == 0,
               "loo_grad: n must equal block_dim × ntr_pad");
  GP2D_REQUIRE(n % NB == 0, "loo_grad: n must be a multiple of 128");
  GP2D_REQUIRE(ntr >= 1 && ntr <= ntr_pad, "loo_grad: ntr must be 1..ntr_pad");
  GP2D_REQUIRE(ld_even(wld, n), "loo_grad: wld must be >= n and even");
  GP2D_REQUIRE(aligned16(W), "loo_grad: W must be 16-byte aligned");
  GP2D_REQUIRE(work != nullptr && work_bytes >= gp2d_loo_grad_workspace(n), "loo_grad: workspace too small");
  GP2D_REQUIRE(aligned16(work), "loo_grad: workspace must be 16-byte aligned");
  hipStream_t s = S(stream);
  const LooGradWork lay(n);
  const auto w = lay.at(work, n);
  // P = WᵀW = K_y⁻¹, lower tiles only, as gp2d_lml_grad forms it
  GemmParams p = gemm_params();
  p.A = W; p.lda = wld;
  p.B = W; p.ldb = wld;
  p.C = w.P; p.ldc = n;
  p.M = (int)n; p.N = (int)n; p.K = (int)n;
  p.a_upper = 1; p.c_lower = 1;
  GP2D_CHECK((launch_gemm<false, EPI_STORE, true>(p, 1, s)));
  // (α = P·y is the fit's; y enters the objective through it alone)
  loo_point_kernel<<<1, LOO_POINT_THREADS, 0, s>>>(w.P, n, ntr_pad, ntr, bd, alpha, w.r, w.c11, w.c21, w.c22,
                                                   value_dev, info_dev);
  GP2D_CHECK(check_launch("loo_point_kernel"));
  if (grad_dev == nullptr) return 0;
  GP2D_CHECK(gp2d_potrs_inv(W, n, wld, w.r, w.s, w.potrs, PotrsWork(n).total, stream));   // s = Wᵀ(W·r)
  const dim3 grid((unsigned)(ntr_pad / 64), (unsigned)(n / 64));
  if (bd == 2) loo_scale_kernel<2><<<grid, 256, 0, s>>>(w.P, n, ntr_pad, w.c11, w.c21, w.c22, w.B);
  else loo_scale_kernel<1><<<grid, 256, 0, s>>>(w.P, n, ntr_pad, w.c11, w.c21, w.c22, w.B);
  GP2D_CHECK(check_launch("loo_scale_kernel"));
  GemmParams m = gemm_params();   // M = B·Bᵀ = P·D·P, lower tiles, over P (s and B are formed)
  m.A = m.B = w.B; m.lda = m.ldb = n;
  m.C = w.P; m.ldc = n;
  m.M = m.N = m.K = (int)n;
  m.c_lower = 1;
  GP2D_CHECK((launch_gemm<true, EPI_STORE>(m, 1, s)));
  return launch_pair_grad(k, xtr, ntr, xtr, ntr, ntr_pad, LooWeights{w.P, n, alpha, w.s, ntr_pad}, w.partial, 0.5,
                          true, grad_dev, s);
}

// ------------------------------------------------------------------ cross-validation (cv.hpp)
size_t gp2d_cv_points_workspace(int64_t n) { return (n > 0 && n % PT_TILE == 0) ? cv_points_bytes(n) : 0; }

int gp2d_cv_points(const double* W, int64_t n, int64_t ldw, const double* alpha, const double* y, int64_t ntr,
                   int64_t npad, int bd, const int64_t* out_order, double* mean, double* var, double* cuv,
                   double* lpd, double* summary, void* work, size_t work_bytes, void* stream) {
  GP2D_REQUIRE(bd == 1 || bd == 2, "cv_points: bd must be 1 or 2");
  GP2D_REQUIRE(npad > 0 && npad % PT_TILE == 0 && n == bd * npad,
               "cv_points: n must be bd·npad with npad a positive multiple of 64");
  GP2D_REQUIRE(ldw >= n, "cv_points: ldw below n");
  GP2D_REQUIRE(ntr >= 1 && ntr <= npad, "cv_points: ntr must be 1..npad");
  GP2D_REQUIRE(bd == 2 || cuv == nullptr, "cv_points: cuv must be NULL for bd = 1 (one component has no cross term)");
  GP2D_REQUIRE(W && alpha && y && mean && var && lpd && summary, "cv_points: NULL argument");
  GP2D_REQUIRE(work != nullptr && work_bytes >= gp2d_cv_points_workspace(n), "cv_points: workspace too small");
  hipStream_t s = S(stream);
  const int64_t nseg = (n + CV_RSEG - 1) / CV_RSEG;
  double* part = static_cast<double*>(work);
  cv_point_partial_kernel<<<dim3((unsigned)((npad + 255) / 256), (unsigned)nseg), 256, 0, s>>>(W, ldw, n, npad, bd,
                                                                                            part);
  GP2D_CHECK(check_launch("cv_point_partial_kernel"));
  cv_point_finish_kernel<<<1, 1024, 0, s>>>(part, nseg, npad, ntr, bd, alpha, y, out_order, mean, var, cuv, lpd,
                                            summary);
  return check_launch("cv_point_finish_kernel");
}

size_t gp2d_cv_groups_workspace(int64_t n, int64_t qpad, int ngroups) {
  if (n <= 0 || n % PT_TILE || qpad <= 0 || qpad % NB || qpad > CV_MAX_Q || ngroups < 1) return 0;
  return CvGroupWork(n, qpad, cv_groups_batch(n, qpad, ngroups)).total;
}

int gp2d_cv_groups(const double* W, int64_t n, int64_t ldw, const double* alpha, const double* y, int64_t ntr,
                   int64_t npad, int bd, const int64_t* gstart, const int64_t* gidx, int ngroups,
                   const int64_t* out_order, double* mean, double* var, double* lpd_group, int* info_group,
                   void* work, size_t work_bytes, void* stream) {
  GP2D_REQUIRE(bd == 1 || bd == 2, "cv_groups: bd must be 1 or 2");
  GP2D_REQUIRE(npad > 0 && npad % PT_TILE == 0 && n == bd * npad,
               "cv_groups: n must be bd·npad with npad a positive multiple of 64");
  GP2D_REQUIRE(ldw >= n, "cv_groups: ldw below n");
  GP2D_REQUIRE(ntr >= 1 && ntr <= npad, "cv_groups: ntr must be 1..npad");
  GP2D_REQUIRE(gstart != nullptr && ngroups >= 1, "cv_groups: no groups");
  int64_t qmax = 0;
  for (int g = 0; g < ngroups; ++g) {   // gstart is a host array: it sizes every launch
    const int64_t cnt = gstart[g + 1] - gstart[g];
    GP2D_REQUIRE(gstart[g] >= 0 && cnt >= 0, "cv_groups: gstart must start at 0 or above and not decrease");
    if (bd * cnt > CV_MAX_Q) {
      set_error("cv_groups: group " + std::to_string(g) + " has " + std::to_string(bd * cnt) +
                " components, over GP2D_CV_MAX_Q = " + std::to_string(CV_MAX_Q));
      return -2;
    }
    qmax = std::max(qmax, bd * cnt);
  }
  GP2D_REQUIRE(W && alpha && y && gidx && mean && var && lpd_group && info_group, "cv_groups: NULL argument");
  const int64_t qpad = round_up(std::max<int64_t>(qmax, 1), NB);
  int nb = std::min(CV_MAX_BATCH, ngroups);
  while (nb >= 1 && (work == nullptr || CvGroupWork(n, qpad, nb).total > work_bytes)) --nb;
  GP2D_REQUIRE(nb >= 1, "cv_groups: workspace too small for one group (gp2d_cv_groups_workspace)");
  GP2D_REQUIRE(reinterpret_cast<uintptr_t>(work) % 16 == 0, "cv_groups: workspace must be 16-byte aligned");
  hipStream_t s = S(stream);
  const CvGroupWork lay(n, qpad, nb);
  double* gram = work_at(work, lay.gram);
  double* fac = work_at(work, lay.fac);
  double* dinv = work_at(work, lay.dinv);
  double* panel = work_at(work, lay.panel);
  const int64_t blk = qpad * qpad;
  const double nan = std::numeric_limits<double>::quiet_NaN();
  for (double* out : {mean, var}) {   // points in no group keep NaN
    cv_fill_kernel<<<(unsigned)((bd * ntr + 255) / 256), 256, 0, s>>>(out, bd * ntr, nan);
    GP2D_CHECK(check_launch("cv_fill_kernel"));
  }
  for (int g0 = 0; g0 < ngroups; g0 += nb) {
    const int cnt = std::min(nb, ngroups - g0);
    CvBatch bt;
    for (int b = 0; b <= CV_MAX_BATCH; ++b) bt.start[b] = gstart[g0 + std::min(b, cnt)];
    cv_gather_t_kernel<<<dim3((unsigned)(n / 64), (unsigned)(qpad / 64), (unsigned)cnt), 256, 0, s>>>(
        W, ldw, n, npad, ntr, bd, gidx, bt, (int)qpad, panel);
    GP2D_CHECK(check_launch("cv_gather_t_kernel"));
    GemmParams p = gemm_params();   // the lower tiles of panel·panelᵀ, one batch entry per group
    p.A = p.B = panel; p.lda = p.ldb = n; p.sA = p.sB = qpad * n;
    p.C = gram; p.ldc = qpad; p.sC = blk;
    p.M = p.N = (int)qpad; p.K = (int)n;
    p.c_lower = 1;
    GP2D_CHECK((launch_gemm<true, EPI_STORE>(p, cnt, s)));
    cv_gram_finish_kernel<<<dim3((unsigned)(qpad / 16), (unsigned)(qpad / 16), (unsigned)cnt), 256, 0, s>>>(
        gram, fac, bt, bd, (int)qpad);
    GP2D_CHECK(check_launch("cv_gram_finish_kernel"));
    GP2D_CHECK(gp2d_potrf_batched(fac, qpad, qpad, blk, cnt, dinv, info_group + g0, stream));
    GP2D_CHECK(gp2d_trtri_batched(fac, qpad, qpad, blk, cnt, dinv, work_at(work, lay.trtri),
                                  TrtriWork(qpad, cnt, false).total, stream));
    cv_group_solve_kernel<<<(unsigned)cnt, 256, 0, s>>>(fac, bt, bd, (int)qpad, npad, ntr, gidx, alpha, y, out_order,
                                                        mean, var, lpd_group + g0);
    GP2D_CHECK(check_launch("cv_group_solve_kernel"));
  }
  return 0;
}

// ------------------------------------------------------------------ instrumentation
// ---- dense helpers of the GP_scripts functional API (getMean / getCov on explicit matrices)
int gp2d_gemm(int transb, int64_t m, int64_t n, int64_t k, double alpha, const double* A, int64_t lda,
              const double* B, int64_t ldb, double beta, double* C, int64_t ldc, void* stream) {
  GP2D_REQUIRE(A && B && C, "gemm: NULL argument");
  GP2D_REQUIRE(m % NB == 0 && n % NB == 0 && k % 16 == 0 && m >= 0 && n >= 0 && k >= 0,
               "gemm: m, n must be multiples of 128 and k of 16");
  GP2D_REQUIRE(ld_even(lda, k), "gemm: lda must be >= k and even");
  GP2D_REQUIRE(ld_even(ldb, transb ? k : n), "gemm: ldb must be >= B's row length (n, or k with transb) and even");
  GP2D_REQUIRE(ldc >= n, "gemm: ldc must be >= n");
  GP2D_REQUIRE(m <= INT32_MAX && n <= INT32_MAX && k <= INT32_MAX, "gemm: sizes exceed int32");
  GP2D_REQUIRE(aligned16(A) && aligned16(B), "gemm: A and B must be 16-byte aligned");
  GemmParams p = gemm_params();
  p.A = A; p.lda = lda;
  p.B = B; p.ldb = ldb;
  p.C = C; p.ldc = ldc;
  p.M = (int)m; p.N = (int)n; p.K = (int)k;
  p.alpha = alpha; p.beta = beta;   // k = 0: C = beta·C (the K loop runs no slab)
  return transb ? launch_gemm<true, EPI_STORE>(p, 1, S(stream)) : launch_gemm<false, EPI_STORE>(p, 1, S(stream));
}

int gp2d_transpose(const double* A, int64_t n, int64_t lda, double* At, void* stream) {
  GP2D_REQUIRE(A && At, "transpose: NULL argument");
  GP2D_REQUIRE(n % 64 == 0 && n >= 0 && lda >= n, "transpose: n must be a multiple of 64, lda >= n");
  if (n == 0) return 0;
  transpose_kernel<<<dim3((unsigned)(n / 64), (unsigned)(n / 64)), 256, 0, S(stream)>>>(A, n, lda, At);
  return check_launch("transpose_kernel");
}

// ------------------------------------------------------------- RCCL (the library's communicator)
// The multi-GPU data path — a job's packed factor, the distributed factor's panels, its W column
// all-gather, the status all-reduce — runs on an RCCL communicator the library itself creates
// (gp2d_comm_init from an ncclUniqueId the caller exchanges over any host channel; the Python
// layer uses torch.distributed's TCP store) and drives on the caller's HIP stream.  RCCL is
// resolved at first use from the copy the process already has loaded (dlsym(RTLD_DEFAULT), then an
// RTLD_NOLOAD librccl.so.1 — torch's bundled RCCL carries that soname), else librccl.so.1 from the
// ROCm install: no link-time dependency, so the engine loads where RCCL is absent.  A communicator
// must be used with the RCCL instance that made it (gp2d_bcast with a foreign ncclComm_t: the
// same rule).
}  // extern "C"
namespace {
struct RcclUniqueId { char internal[128]; };   // ncclUniqueId (NCCL_UNIQUE_ID_BYTES)
typedef int (*rccl_bcast_fn)(const void*, void*, size_t, int, int, void*, hipStream_t);
typedef int (*rccl_allgather_fn)(const void*, void*, size_t, int, void*, hipStream_t);
typedef int (*rccl_allreduce_fn)(const void*, void*, size_t, int, int, void*, hipStream_t);
typedef int (*rccl_p2p_fn)(const void*, size_t, int, int, void*, hipStream_t);   // ncclSend / ncclRecv
typedef int (*rccl_void_fn)(void);                                             // ncclGroupStart / End
typedef int (*rccl_uid_fn)(RcclUniqueId*);
typedef int (*rccl_init_fn)(void**, int, RcclUniqueId, int);
typedef int (*rccl_comm_fn)(void*);
typedef int (*rccl_count_fn)(void*, int*);
typedef const char* (*rccl_errstr_fn)(int);
struct RcclSyms {
  rccl_bcast_fn bcast = nullptr;
  rccl_allgather_fn allgather = nullptr;
  rccl_allreduce_fn allreduce = nullptr;
  rccl_p2p_fn send = nullptr, recv = nullptr;
  rccl_void_fn group_start = nullptr, group_end = nullptr;
  rccl_uid_fn unique_id = nullptr;
  rccl_init_fn init_rank = nullptr;
  rccl_comm_fn destroy = nullptr;
  rccl_count_fn count = nullptr, user_rank = nullptr;
  rccl_errstr_fn errstr = nullptr;
};
template <class F> void rccl_sym(void* h, const char* name, F& out) {
  out = reinterpret_cast<F>(h ? dlsym(h, name) : dlsym(RTLD_DEFAULT, name));
}
const RcclSyms& rccl_syms() {
  static const RcclSyms r = [] {
    // 1. whatever RCCL the process already resolves globally; 2. an already loaded librccl.so.1
    //    (torch's); 3. the ROCm install's copy
    void* h = nullptr;
    if (!dlsym(RTLD_DEFAULT, "ncclBroadcast")) {
      h = dlopen("librccl.so.1", RTLD_NOW | RTLD_NOLOAD);
      if (!h) h = dlopen("librccl.so.1", RTLD_NOW | RTLD_LOCAL);
    }
    RcclSyms x;
    if (!h && !dlsym(RTLD_DEFAULT, "ncclBroadcast")) return x;
    rccl_sym(h, "ncclBroadcast", x.bcast);
    rccl_sym(h, "ncclAllGather", x.allgather);
    rccl_sym(h, "ncclAllReduce", x.allreduce);
    rccl_sym(h, "ncclSend", x.send);
    rccl_sym(h, "ncclRecv", x.recv);
    rccl_sym(h, "ncclGroupStart", x.group_start);
    rccl_sym(h, "ncclGroupEnd", x.group_end);
    rccl_sym(h, "ncclGetUniqueId", x.unique_id);
    rccl_sym(h, "ncclCommInitRank", x.init_rank);
    rccl_sym(h, "ncclCommDestroy", x.destroy);
    rccl_sym(h, "ncclCommCount", x.count);
    rccl_sym(h, "ncclCommUserRank", x.user_rank);
    rccl_sym(h, "ncclGetErrorString", x.errstr);
    return x;
  }();
  return r;
}
constexpr int kRcclUint8 = 1, kRcclInt32 = 2, kRcclFloat64 = 8;   // ncclDataType_t
int rccl_fail(const char* what, int rc) {
  const RcclSyms& r = rccl_syms();
  set_error(std::string(what) + " failed: " + (r.errstr ? r.errstr(rc) : "unknown RCCL error"));
  return -100 - rc;
}
#define GP2D_RCCL(sym, what)                                                                   \
  const RcclSyms& r = rccl_syms();                                                            \
  GP2D_REQUIRE(r.sym != nullptr, what ": RCCL (librccl.so.1) not found")
}  // namespace
extern "C" {

size_t gp2d_comm_id_bytes(void) { return sizeof(RcclUniqueId); }

int gp2d_comm_unique_id(void* id) {
  GP2D_REQUIRE(id != nullptr, "comm_unique_id: NULL id");
  GP2D_RCCL(unique_id, "comm_unique_id");
  const int rc = r.unique_id(static_cast<RcclUniqueId*>(id));
  return rc ? rccl_fail("ncclGetUniqueId", rc) : 0;
}

int gp2d_comm_init(void** comm, int nranks, const void* id, int rank, int device) {
  GP2D_REQUIRE(comm != nullptr && id != nullptr, "comm_init: NULL argument");
  GP2D_REQUIRE(nranks >= 1 && rank >= 0 && rank < nranks, "comm_init: need 0 <= rank < nranks");
  GP2D_RCCL(init_rank, "comm_init");
  if (device >= 0 && hipSetDevice(device) != hipSuccess) { set_error("comm_init: hipSetDevice failed"); return -1; }
  RcclUniqueId uid;
  std::memcpy(&uid, id, sizeof(uid));
  *comm = nullptr;
  const int rc = r.init_rank(comm, nranks, uid, rank);
  return rc ? rccl_fail("ncclCommInitRank", rc) : 0;
}

int gp2d_comm_destroy(void* comm) {
  if (comm == nullptr) return 0;
  GP2D_RCCL(destroy, "comm_destroy");
  const int rc = r.destroy(comm);
  return rc ? rccl_fail("ncclCommDestroy", rc) : 0;
}

int gp2d_comm_size(void* comm, int* nranks, int* rank) {
  GP2D_REQUIRE(comm != nullptr && nranks != nullptr && rank != nullptr, "comm_size: NULL argument");
  GP2D_RCCL(count, "comm_size");
  GP2D_REQUIRE(r.user_rank != nullptr, "comm_size: ncclCommUserRank not found");
  int rc = r.count(comm, nranks);
  if (rc) return rccl_fail("ncclCommCount", rc);
  rc = r.user_rank(comm, rank);
  return rc ? rccl_fail("ncclCommUserRank", rc) : 0;
}

int gp2d_bcast(void* buf, size_t bytes, int root, void* comm, void* stream) {
  GP2D_REQUIRE(root >= 0, "bcast: root must be >= 0");
  if (bytes == 0) return 0;
  GP2D_REQUIRE(buf != nullptr && comm != nullptr, "bcast: NULL buffer or communicator");
  GP2D_RCCL(bcast, "bcast");
  const int rc = r.bcast(buf, buf, bytes, kRcclUint8, root, comm, S(stream));
  return rc ? rccl_fail("bcast: ncclBroadcast", rc) : 0;
}

int gp2d_allgather(const void* send, void* recv, size_t bytes_per_rank, void* comm, void* stream) {
  if (bytes_per_rank == 0) return 0;
  GP2D_REQUIRE(send != nullptr && recv != nullptr && comm != nullptr, "allgather: NULL argument");
  GP2D_RCCL(allgather, "allgather");
  const int rc = r.allgather(send, recv, bytes_per_rank, kRcclUint8, comm, S(stream));
  return rc ? rccl_fail("allgather: ncclAllGather", rc) : 0;
}

int gp2d_allreduce(void* buf, size_t count, int dtype, int op, void* comm, void* stream) {
  GP2D_REQUIRE(dtype == GP2D_COMM_INT32 || dtype == GP2D_COMM_FLOAT64, "allreduce: dtype must be INT32 or FLOAT64");
  GP2D_REQUIRE(op >= GP2D_COMM_SUM && op <= GP2D_COMM_MIN, "allreduce: op must be SUM, MAX or MIN");
  if (count == 0) return 0;
  GP2D_REQUIRE(buf != nullptr && comm != nullptr, "allreduce: NULL argument");
  GP2D_RCCL(allreduce, "allreduce");
  const int nccl_op = op == GP2D_COMM_SUM ? 0 : (op == GP2D_COMM_MAX ? 2 : 3);   // ncclSum / ncclMax / ncclMin
  const int rc = r.allreduce(buf, buf, count, dtype == GP2D_COMM_INT32 ? kRcclInt32 : kRcclFloat64, nccl_op, comm,
                             S(stream));
  return rc ? rccl_fail("allreduce: ncclAllReduce", rc) : 0;
}

int gp2d_sendrecv(const void* send, int send_peer, void* recv, int recv_peer, size_t bytes, void* comm,
                  void* stream) {
  if (bytes == 0) return 0;
  GP2D_REQUIRE(comm != nullptr && (send != nullptr || recv != nullptr), "sendrecv: NULL argument");
  GP2D_RCCL(send, "sendrecv");
  GP2D_REQUIRE(r.recv && r.group_start && r.group_end, "sendrecv: ncclRecv / ncclGroupStart not found");
  int rc = r.group_start();
  if (rc) return rccl_fail("ncclGroupStart", rc);
  int rs = 0, rr = 0;
  if (send != nullptr) rs = r.send(send, bytes, kRcclUint8, send_peer, comm, S(stream));
  if (recv != nullptr) rr = r.recv(recv, bytes, kRcclUint8, recv_peer, comm, S(stream));
  rc = r.group_end();
  if (rs) return rccl_fail("sendrecv: ncclSend", rs);
  if (rr) return rccl_fail("sendrecv: ncclRecv", rr);
  return rc ? rccl_fail("ncclGroupEnd", rc) : 0;
}

int gp2d_stream_create_cumask(int first, int count, void** stream) {
  // A HIP stream whose kernels may use only the CUs of mask bits [first, first + count).  The
  // driver deals the mask's bits over the XCDs (bit i → XCD i mod 8), so a range of 8k bits is k
  // CUs of every XCD.
  GP2D_REQUIRE(stream != nullptr, "stream_create_cumask: NULL stream");
  int dev = 0;
  hipDeviceProp_t prop;
  if (hipGetDevice(&dev) != hipSuccess || hipGetDeviceProperties(&prop, dev) != hipSuccess) {
    set_error("stream_create_cumask: cannot query the device");
    return -1;
  }
  const int ncu = prop.multiProcessorCount;
  GP2D_REQUIRE(first >= 0 && count >= 1 && first + count <= ncu,
               "stream_create_cumask: need 0 <= first, 1 <= count, first + count <= CU count");
  std::vector<uint32_t> mask((ncu + 31) / 32, 0u);
  for (int c = first; c < first + count; ++c) mask[c / 32] |= 1u << (c % 32);
  hipStream_t s = nullptr;
  if (hipExtStreamCreateWithCUMask(&s, (uint32_t)mask.size(), mask.data()) != hipSuccess) {
    set_error("stream_create_cumask: hipExtStreamCreateWithCUMask failed");
    return -1;
  }
  *stream = s;
  return 0;
}

int gp2d_stream_destroy(void* stream) {
  if (stream == nullptr) return 0;
  if (hipStreamDestroy(S(stream)) != hipSuccess) { set_error("stream_destroy: hipStreamDestroy failed"); return -1; }
  return 0;
}

// An empty kernel whose dispatch marks a point of the stream in a rocprofv3 kernel trace (bench.py
// brackets its timed region with tags 1 and 2; tools/timed_kernels.py lists what ran between).
__global__ void trace_mark_kernel(int) {}

int gp2d_trace_mark(int tag, void* stream) {
  trace_mark_kernel<<<1, 64, 0, S(stream)>>>(tag);
  return check_launch("trace_mark_kernel");
}

void gp2d_timing_enable(int on) {
  std::lock_guard<std::mutex> lk(g_timing.mu);
  g_timing.on = (on != 0);
}

int gp2d_timing_read(double* total_ms, int64_t* launches, double* flops) {
  std::lock_guard<std::mutex> lk(g_timing.mu);
  double ms = 0.0, fl = 0.0;
  for (size_t i = 0; i < g_timing.ev.size(); ++i) {
    auto& pr = g_timing.ev[i];
    if (hipEventSynchronize(pr.second) != hipSuccess) { set_error("timing: event sync failed"); return -1; }
    float t = 0.f;
    hipEventElapsedTime(&t, pr.first, pr.second);
    ms += t;
    fl += g_timing.flops[i];
    g_timing.pool.push_back(pr.first);
    g_timing.pool.push_back(pr.second);
  }
  if (total_ms) *total_ms = ms;
  if (launches) *launches = (int64_t)g_timing.ev.size();
  if (flops) *flops = fl;
  g_timing.ev.clear();
  g_timing.flops.clear();
  return 0;
}

}  // extern "C"
