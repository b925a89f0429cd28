// igemm_probes.hpp — the probe policies of ozaki.hpp's igemm_nt_mod_kernel<TBN, NST, Probe>
// (tools/microbench only; the library instantiates IgemmNoProbe alone).  The kernel has one
// text: a policy switches parts of it off or reads the clock at its hook points.
#pragma once
#include "../../2d-gp_amd/csrc/ozaki.hpp"
namespace gp2d {
// Ablations: the outputs are meaningless by design, read the time per launch.
//   DMA off      no global→LDS DMA (MFMAs on stale LDS)
//   BARRIER off  (with DMA off) no vmcnt wait / barrier per slab
//   LDSREAD off  no fragment reads (MFMAs on constant registers)
//   MFMA off     no MFMAs (one xor per half step keeps the loads live)
//   KLOOP off    no K loop at all (prologue-free: epilogue and stores only)
template <bool DMA, bool BARRIER, bool LDSREAD, bool MFMA, bool KLOOP>
struct IgemmAblate : IgemmNoProbe {
  static_assert(BARRIER || !DMA, "without the vmcnt wait the DMA's slabs are read before they land");
  static constexpr bool kDma = DMA, kBarrier = BARRIER, kLdsRead = LDSREAD, kMfma = MFMA, kKLoop = KLOOP;
};
using IgemmNoDma = IgemmAblate<false, true, true, true, true>;
using IgemmNoDmaNoBar = IgemmAblate<false, false, true, true, true>;
using IgemmMfmaOnly = IgemmAblate<false, false, false, true, true>;
using IgemmNoLdsRead = IgemmAblate<true, true, false, true, true>;
using IgemmNoMfma = IgemmAblate<true, true, true, false, true>;
using IgemmEpiOnly = IgemmAblate<true, true, true, true, false>;

// Stamps: s_memtime at the hook points (read the SHARES, not the run time: every stamp drains
// lgkmcnt, so the build cannot overlap what the product kernel overlaps there).
// Per wave, 64-bit scalar sums of the cycles between consecutive stamps:
//   seg 0  work: after a barrier → the next FULL step's vmcnt wait, or the ring tail (fragment
//          reads, h1 and h0 MFMAs, DMA issue)
//   seg 1  waiting for the wave's own LDS-DMA pieces of the next slab (s_waitcnt vmcnt, taken
//          here ahead of the kernel's own, which then finds them landed)
//   seg 2  waiting at the per-slab s_barrier for the other waves
//   seg 3  the ring tail (NST − 1 steps without stamps)
//   seg 4  epilogue (prior residues, mod m, LDS transpose, stores issued)
//   seg 5  prologue (launch → first fragments)
// Stored once per wave by lane 0 (vector store) into ig_stamp[block][wave][8]:
// slots 0-5 = segment sums, 6 = FULL steps, 7 = tile start time.  One modulus (grid.z = 1).
constexpr int IG_STAMP_BLOCKS = 2048;
__device__ unsigned long long ig_stamp[IG_STAMP_BLOCKS * 8 * 8];
struct IgemmStamps : IgemmNoProbe {
  unsigned long long sum[6] = {0, 0, 0, 0, 0, 0}, steps = 0, t0, last;
  __device__ __forceinline__ static unsigned long long now() {
    unsigned long long t;
    __builtin_amdgcn_sched_barrier(0);
    asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t)::"memory");
    __builtin_amdgcn_sched_barrier(0);
    return t;
  }
  __device__ __forceinline__ void seg(int i) {
    const unsigned long long t = now();
    sum[i] += t - last;
    last = t;
  }
  __device__ __forceinline__ void tile_start() { t0 = last = now(); }
  __device__ __forceinline__ void ring_filled() { seg(5); }
  template <int VM>
  __device__ __forceinline__ void before_wait() {
    seg(0);   // lgkmcnt(0) inside: a1 landed, as the barrier requires
    asm volatile("s_waitcnt vmcnt(%0)" ::"n"(VM) : "memory");
    seg(1);
  }
  __device__ __forceinline__ void after_barrier() {
    seg(2);
    ++steps;
  }
  __device__ __forceinline__ void ring_tail() { seg(0); }
  __device__ __forceinline__ void before_epilogue() { seg(3); }
  __device__ __forceinline__ void after_store() {
    seg(4);
    const unsigned blk = blockIdx.y * gridDim.x + blockIdx.x;
    if ((threadIdx.x & 63) == 0 && blk < IG_STAMP_BLOCKS) {
      unsigned long long* o = ig_stamp + ((size_t)blk * 8 + (threadIdx.x >> 6)) * 8;
      for (int q = 0; q < 6; ++q) o[q] = sum[q];
      o[6] = steps;
      o[7] = t0;
    }
  }
};
}  // namespace gp2d
