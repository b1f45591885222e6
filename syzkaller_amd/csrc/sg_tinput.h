// sg_tinput.h -- the per-input kernels of triageInput's signal math, shared by
// sg_tinput.hip (ready-made lists, a call per step) and sg_triage_runs.hip (the
// whole loop from raw buffers).  Not installed.
#pragma once

#include "sg_internal.h"

#include <algorithm>

namespace sg {
namespace tin {

constexpr uint32_t kSentT = 0xFFFFFFFFu;  // cover.go:17
constexpr int kTB = 256;                  // threads per input
constexpr uint32_t kCap = kTinChunk;      // a values per LDS chunk (32 KiB)

// Order-preserving compaction of one round of kTB flags inside a workgroup:
// returns this thread's rank among the kept ones; *total = kept in the round.
__device__ __forceinline__ uint32_t block_rank(bool keep, uint32_t* wsum, uint32_t* total) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const uint64_t m = __ballot(keep);
  const uint32_t below = __popcll(m & (lane ? (~0ull >> (64 - lane)) : 0ull));
  if (lane == 0) wsum[w] = __popcll(m);
  __syncthreads();
  uint32_t base = 0, t = 0;
#pragma unroll
  for (int k = 0; k < kTB / 64; k++) {
    const uint32_t c = wsum[k];
    base += k < w ? c : 0u;
    t += c;
  }
  __syncthreads();
  *total = t;
  return base + below;
}

// SignalDiff (cover.go:169-176) per segment: count, then write in order.
template <bool kWrite>
__global__ __launch_bounds__(kTB) void k_tin_diff(const uint32_t* __restrict__ words, const uint32_t* __restrict__ v,
                                                  const uint64_t* __restrict__ off, uint32_t* __restrict__ cnt,
                                                  const uint64_t* __restrict__ dst_off, uint32_t* __restrict__ dst) {
  __shared__ uint32_t wsum[kTB / 64];
  const uint64_t k = blockIdx.x, b = off[k], e = off[k + 1];
  uint64_t pos = kWrite ? dst_off[k] : 0;
  uint32_t n = 0;
  for (uint64_t base = b; base < e; base += kTB) {
    const uint64_t i = base + threadIdx.x;
    uint32_t s = 0;
    bool miss = false;
    if (i < e) {
      s = v[i];
      miss = !sgd::test_bit(words, s);
    }
    uint32_t tot;
    const uint32_t r = block_rank(miss, wsum, &tot);
    if (kWrite && miss) dst[pos + r] = s;
    pos += tot;
    n += tot;
  }
  if (!kWrite && threadIdx.x == 0) cnt[k] = n;
}

// The LDS of one workgroup of tin_intersect
struct IntersectLds {
  uint32_t av[kCap];
  uint32_t found[kCap / 32];
  uint32_t wsum[kTB / 64];
};

// Intersection(a, Canonicalize(r)) for a sorted a = a[a0 .. a1) and any r =
// r[r0 .. r1) (sg_tinput.hip's header), by the kTB threads of one workgroup:
// returns the number of kept values; kIntersect writes them at a's own start.
template <bool kIntersect>
__device__ __forceinline__ uint64_t tin_intersect(uint32_t* __restrict__ a, uint64_t a0, uint64_t a1,
                                                  const uint32_t* __restrict__ r, uint64_t r0, uint64_t r1,
                                                  IntersectLds& s) {
  uint64_t kept = 0;
  for (uint64_t c0 = a0; c0 < a1; c0 += kCap) {
    const uint32_t m = (uint32_t)std::min<uint64_t>(kCap, a1 - c0);
    __syncthreads();  // the previous chunk is written out
    for (uint32_t j = threadIdx.x; j < m; j += kTB) s.av[j] = a[c0 + j];
    for (uint32_t j = threadIdx.x; j < kCap / 32; j += kTB) s.found[j] = 0;
    __syncthreads();
    for (uint64_t i = r0 + threadIdx.x; i < r1; i += kTB) {
      const uint32_t x = r[i];
      uint32_t lo = 0, hi = m;  // first j with av[j] >= x
      while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (s.av[mid] < x)
          lo = mid + 1;
        else
          hi = mid;
      }
      if (lo < m && s.av[lo] == x) atomicOr(&s.found[lo >> 5], 1u << (lo & 31));
    }
    __syncthreads();
    // c0 > a0: the value before the chunk decides whether its first element is a first copy
    const uint32_t before = c0 > a0 ? a[c0 - 1] : 0u;
    for (uint32_t j0 = 0; j0 < m; j0 += kTB) {
      const uint32_t j = j0 + threadIdx.x;
      bool keep = false;
      uint32_t x = 0;
      if (j < m) {
        x = s.av[j];
        const bool first = j ? s.av[j - 1] != x : (c0 == a0 || before != x);
        keep = ((s.found[j >> 5] >> (j & 31)) & 1u) && first && x != kSentT;
      }
      uint32_t tot;
      const uint32_t rk = block_rank(keep, s.wsum, &tot);
      if (kIntersect && keep) a[a0 + kept + rk] = x;  // never past the chunk: kept + rk <= c0 - a0 + j
      kept += tot;
    }
  }
  return kept;
}

}  // namespace tin
}  // namespace sg
