// The int8 NT GEMM of ozaki.hpp in isolation on random residues (dev tool): time per
// IGEMM_N × IGEMM_NC × IGEMM_N lower-triangular launch (defaults 8192 × 16384), outputs checked
// against a CPU dot product: all of them when there are at most 2^20, else 4096 samples.
// Every variant launches the product kernel, igemm_nt_mod_kernel<IG_TBN, IG_NST, PROBE>: FULL
// with the library's IgemmNoProbe, the ablation and stamp variants with a policy of
// igemm_probes.hpp (-DPROBE=...).
// IGEMM_ADD=1: a second product after the plain one, same operands, adding the first one's
// residues (add_col0 = its columns) into columns of its own (c_col0 = IGEMM_NC) — the shape P2
// has in OzakiProducts; checked against (prior + Σ) mod m.
#include "igemm_probes.hpp"
#include <cstdio>
#include <random>
#include <vector>
#include <climits>
#include <cstdlib>
#include <type_traits>
namespace gp2d { void set_error(const std::string&) {} }
using namespace gp2d;
#ifndef IG_TBN
#define IG_TBN 256
#endif
#ifndef IG_NST
#define IG_NST 4
#endif
#ifndef PROBE
#define PROBE IgemmNoProbe
#endif
constexpr bool kStamps = std::is_same<PROBE, IgemmStamps>::value;
static int env_int(const char* name, int dflt) { return getenv(name) ? atoi(getenv(name)) : dflt; }
// per-wave segment sums of the last launch (IgemmStamps) → shares and per-step cycles
static void report_stamps(const char* what, int blocks) {
  std::vector<unsigned long long> st((size_t)IG_STAMP_BLOCKS * 8 * 8);
  (void)hipMemcpyFromSymbol(st.data(), HIP_SYMBOL(ig_stamp), st.size() * 8);
  double seg[6] = {0}, steps = 0, waves = 0;
  unsigned long long smin = ~0ull, smax = 0;
  for (int b = 0; b < blocks; ++b)
    for (int w = 0; w < IG_TBN / 32; ++w) {
      const unsigned long long* o = st.data() + ((size_t)b * 8 + w) * 8;
      for (int q = 0; q < 6; ++q) seg[q] += (double)o[q];
      steps += (double)o[6];
      smin = o[6] < smin ? o[6] : smin;
      smax = o[6] > smax ? o[6] : smax;
      waves += 1;
    }
  const char* nm[6] = {"work (reads, h1+h0 MFMAs, DMA issue)", "vmcnt wait (own DMA of next slab)", "s_barrier wait",
                       "ring tail", "epilogue", "prologue"};
  double tot = 0;
  for (int q = 0; q < 6; ++q) tot += seg[q];
  printf("stamps %s: %.0f waves, stamped steps per wave mean %.3f min %llu max %llu, %.0f wave-cycles per wave\n", what,
         waves, steps / waves, smin, smax, tot / waves);
  for (int q = 0; q < 6; ++q)
    printf("  %s seg %d %-40s share %.4f  per wave %.0f  per step %.1f\n", what, q, nm[q], seg[q] / tot, seg[q] / waves,
           q < 3 && steps > 0 ? seg[q] / steps : 0.0);
}
int main() {
  const int n = env_int("IGEMM_N", 8192), nc = env_int("IGEMM_NC", 16384), mod = 251;
  const bool add = env_int("IGEMM_ADD", 0) != 0;
  if (n < IBM || n % IBM || nc < IBN || nc % IBN || n >= 131072) {
    printf("IGEMM_N and IGEMM_NC are positive multiples of 256, IGEMM_N below 131072\n");
    return 2;
  }
  std::mt19937 rng(17);
  std::vector<int8_t> A((size_t)n * n), B((size_t)nc * n), Ab(A.size()), Bb(B.size());
  for (int i = 0; i < n; ++i)
    for (int k = 0; k < n; ++k) A[(size_t)i * n + k] = (k <= i) ? (int8_t)(rng() & 0xff) : 0;
  for (auto& v : B) v = (int8_t)(rng() & 0xff);
  if (getenv("IGEMM_ZERO")) { for (auto& v : A) v = 0; for (auto& v : B) v = 0; }
  for (int i = 0; i < n; ++i)
    for (int k = 0; k < n; ++k) Ab[slab_offset(i, k, n)] = A[(size_t)i * n + k];
  for (int j = 0; j < nc; ++j)
    for (int k = 0; k < n; ++k) Bb[slab_offset(j, k, n)] = B[(size_t)j * n + k];
  // C: column-major, the plain product's nc columns, then the add product's
  const size_t plane = (size_t)n * nc;
  int8_t *dA, *dB; uint8_t* dC;
  if (hipMalloc(&dA, A.size()) != hipSuccess || hipMalloc(&dB, B.size()) != hipSuccess ||
      hipMalloc(&dC, 2 * plane) != hipSuccess) {
    printf("hipMalloc failed\n");
    return 1;
  }
  (void)hipMemcpy(dA, Ab.data(), A.size(), hipMemcpyHostToDevice);
  (void)hipMemcpy(dB, Bb.data(), B.size(), hipMemcpyHostToDevice);
  hipEvent_t e0, e1; (void)hipEventCreate(&e0); (void)hipEventCreate(&e1);
  const dim3 g(nc / IG_TBN, n / IBM);
  // IGEMM_K=k: dense (not triangular) launches with K = k on the same planes — per-tile vs
  // per-slab cost (time = tiles·a + slabs·b); the check then does not apply
  const int kx = getenv("IGEMM_K") ? atoi(getenv("IGEMM_K")) : n, low = getenv("IGEMM_K") ? 0 : 1;
#ifdef IGEMM_GRID
  const dim3 gl(IGEMM_GRID);
#else
  const dim3 gl = g;
#endif
  if (kx < IBK || kx % IBK || kx > n || (kStamps && (int)(gl.x * gl.y) > IG_STAMP_BLOCKS)) {
    printf("IGEMM_K is a multiple of 64 up to IGEMM_N; the stamp build holds %d tiles\n", IG_STAMP_BLOCKS);
    return 2;
  }
  // one product, dense K loop (no slab list), one modulus; returns ms per launch, < 0 on a HIP error
  auto time_launches = [&](const IgemmProd& p) -> float {
    auto launch = [&]() {
      igemm_nt_mod_kernel<IG_TBN, IG_NST, PROBE><<<gl, 2 * IG_TBN>>>(dA, dB, dC, n, n / IBK, mod, p, nullptr, nullptr,
                                                                     IgemmZ{});
    };
    for (int w = 0; w < 3; ++w) launch();
    if (hipDeviceSynchronize() != hipSuccess) return -1.f;
    (void)hipEventRecord(e0);
    for (int r = 0; r < 20; ++r) launch();
    (void)hipEventRecord(e1);
    float ms;
    if (hipEventSynchronize(e1) != hipSuccess || hipEventElapsedTime(&ms, e0, e1) != hipSuccess) return -1.f;
    return ms / 20;
  };
  IgemmProd plain = IgemmProd::plain(kx, low != 0), added = plain;
  added.c_col0 = nc;
  added.add_col0 = 0;
  const float ms = time_launches(plain);
  if (ms < 0) { printf("%s: HIP error: %s\n", VARIANT, hipGetErrorString(hipGetLastError())); return 1; }
  const double ops = 2.0 * ((double)n * n / 2 + n * 128.0) * nc;
  if (!low) {
    printf("%s: K=%d dense: %.4f ms/launch\n", VARIANT, kx, ms);
    return 0;
  }
  printf("%s: %.3f ms/launch, %.0f TOPs\n", VARIANT, ms, ops / ms / 1e9);
  if (kStamps) report_stamps("plain", (int)(gl.x * gl.y));
  if (add) {
    const float ms2 = time_launches(added);
    if (ms2 < 0) { printf("%s: HIP error: %s\n", VARIANT, hipGetErrorString(hipGetLastError())); return 1; }
    printf("%s: add product: %.3f ms/launch, %.0f TOPs\n", VARIANT, ms2, ops / ms2 / 1e9);
    if (kStamps) report_stamps("add", (int)(gl.x * gl.y));
  }
  std::vector<uint8_t> C(2 * plane);
  if (hipMemcpy(C.data(), dC, (add ? 2 : 1) * plane, hipMemcpyDeviceToHost) != hipSuccess) {
    printf("%s: HIP error: %s\n", VARIANT, hipGetErrorString(hipGetLastError()));
    return 1;
  }
  const bool all = plane <= (size_t)1 << 20;
  const size_t checks = all ? plane : 4096;
  size_t bad = 0, bad2 = 0;
  for (size_t t = 0; t < checks; ++t) {
    const int i = all ? (int)(t % n) : (int)(rng() % n), j = all ? (int)(t / n) : (int)(rng() % nc);
    long long sacc = 0;
    for (int k = 0; k <= i; ++k) sacc += (long long)A[(size_t)i * n + k] * B[(size_t)j * n + k];
    const int want = (int)(((sacc % mod) + mod) % mod);
    bad += C[(size_t)j * n + i] != want;
    bad2 += add && C[plane + (size_t)j * n + i] != (want + want) % mod;   // (prior + Σ) mod m
  }
  const char* kind = all ? "" : "sampled ";
  printf("%s: plain product: %zu of %zu %soutputs differ from the CPU dot product\n", VARIANT, bad, checks, kind);
  if (add) printf("%s: add product: %zu of %zu %soutputs differ from (prior + sum) mod m\n", VARIANT, bad2, checks, kind);
  return 0;
}
