// sg_plan.h -- layout arithmetic of the context's device buffers (the
// workspace and the host forms' staging buffer) and launch arithmetic that a
// test has to reach without a device (band_plan).  Plain C++: no HIP, so a host
// compiler builds it alone (tests/cpp/plan_test.cc).
#pragma once

#include <cstddef>
#include <cstdint>

namespace sg {

constexpr size_t align256(size_t b) { return (b + 255) & ~size_t(255); }

// Bump-allocated regions of one buffer, each 256-B aligned: add returns the
// region's offset and total is the bytes to reserve.  off[] records the first
// kMaxRegions offsets in order (sg_part.h indexes it); a region past them is
// still laid out, and overflow makes ws_reserve / dstage_reserve refuse the
// plan.
struct WsPlan {
  static constexpr int kMaxRegions = 48;
  size_t off[kMaxRegions];
  int n = 0;
  size_t total = 0;
  bool overflow = false;
  size_t add(size_t bytes) {
    const size_t o = total;
    if (n < kMaxRegions)
      off[n++] = o;
    else
      overflow = true;
    total += align256(bytes);
    return o;
  }
};

// The capacity a grow-only buffer of `cap` elements takes to hold `need`:
// unchanged while it fits, else max(2 * cap, floor) doubled until it does.
// ("cap, or the floor when cap is 0, doubled while too small" is the same
// function: growth is only entered with need > cap, where the first doubling
// of cap always happens, and a buffer that exists is never below its floor.)
inline size_t grow_cap(size_t cap, size_t need, size_t floor) {
  if (need <= cap) return cap;
  size_t nc = 2 * cap > floor ? 2 * cap : floor;
  while (nc < need) nc *= 2;
  return nc;
}

// A mask covering 0 .. n - 1, for the radix sort's `vary` over keys below n: 0
// for n <= 1, else the smallest 2^k - 1 that is >= n - 1.
inline uint64_t bits_below(uint64_t n) {
  uint64_t m = 0;
  while (n > 1 && m < n - 1) m = (m << 1) | 1;  // (ends: all ones is >= any n - 1)
  return m;
}

// The launch of k_prio_band (sg_call_prios.hip) for a matrix of ncalls rows and
// nids >= 1 places of entries: a band of `rows` rows whose u32 cells fit
// band_cells, nbands of them (grid x); the places cut into gridy parts (grid y)
// of `part` places each, a multiple of band_threads and at most part_max:
// parts enough for about 2048 workgroups (1024 measured slower), a part worth
// a workgroup (4 * band_threads places), none longer than part_max.  Computed
// in 64 bits; with ncalls <= 2^13 and nids < 2^32 every value fits 32 bits but
// part, which reaches part_max (tests/cpp/plan_test.cc sweeps it).
struct BandPlan {
  uint32_t rows, nbands;
  uint64_t nparts, part;
  uint32_t gridy;
};
inline BandPlan band_plan(uint32_t ncalls, uint64_t nids, uint32_t band_cells, uint32_t band_threads, uint64_t part_max) {
  const auto up = [](uint64_t a, uint64_t b) { return (a + b - 1) / b; };
  const auto lo = [](uint64_t a, uint64_t b) { return a < b ? a : b; };
  BandPlan p;
  const uint64_t fit = lo(band_cells / ncalls, ncalls);
  p.rows = (uint32_t)(fit ? fit : 1);
  p.nbands = (uint32_t)up(ncalls, p.rows);
  p.nparts = lo(up(2048, p.nbands), up(nids, 4 * (uint64_t)band_threads));
  if (p.nparts < up(nids, part_max)) p.nparts = up(nids, part_max);
  p.part = up(up(nids, p.nparts), band_threads) * band_threads;
  p.gridy = (uint32_t)up(nids, p.part);
  return p;
}

// CSR offsets of n lists: off[0] == 0 and non-decreasing up to off[n].
inline bool offsets_ok(const uint64_t* off, size_t n) {
  if (off[0] != 0) return false;
  for (size_t i = 0; i < n; i++)
    if (off[i + 1] < off[i]) return false;
  return true;
}

}  // namespace sg
