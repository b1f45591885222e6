// sg_linewalk.h -- the line walk of the text scans, the 64-line store group they
// write through and the whole-wave searches inside one line.  k_cs_scan of
// sg_call_set.hip runs on the walk and the group; k_ci_scan of
// sg_cover_ingest.hip still walks in a copy of its own and keeps its own
// searches (profiles/README.md has why); the searches here serve
// sg_crash_report.hip.
// Device code only; pinned at its own edges by tests/test_stages.py through
// sgt_walk_lines.
//
// The walk.  A text segment [a0, a1) -- a program of a batch, or a whole tool
// output -- is cut into tiles; a wave takes a tile [tb, te) and owns the lines
// that START in it: at a0 for the head tile (tb == a0, which reads nothing in
// front of a0), else behind a '\n' at tb - 1 .. te - 2.  It walks kWalkStep
// bytes a step, a lane a byte (kWalkLoad steps' loads in flight), ballots '\n'
// and the caller's byte classes into 64-bit masks and moves from line to line
// with scalar bit operations on them.  The state it carries from step to step:
// in a line or not, the line's start, and per class whether it was met and
// where first.  A line that leaves the tile is walked to its end by its owner
// (the next tile's wave skips it: it starts at the first '\n' at or after its
// tile's last-but-one byte), so no wave waits for another and nothing is
// carried between waves.  A walk is cut max_line bytes into a line: a line open
// at the end of a step and already that long there is handed out once, with
// that step's end as its end, and what follows it up to the next '\n' is no
// line.  A line that ends at a1 without '\n' is a line; nothing follows a final
// '\n'.
//
// A byte past a1 is read as 0x100, which equals no byte: a class byte may be 0.
// Every load is checked against a1, and every loop is bounded by the tile's
// end, the segment's end or the line limit.
#pragma once

#include <cstdint>

namespace sgd {

constexpr uint32_t kWalkStep = 64;  // bytes of a step
constexpr uint32_t kWalkLoad = 4;   // steps loaded at a time
constexpr uint32_t kLineGroup = 64;  // kept lines held before a store

// cls(c, m): c is this lane's byte of a step (0x100: none); it fills
// m[0 .. kClasses) with the ballots of its classes (kClasses: 0, 1 or 2).  line(s, e, have, first): a line [s, e) of this tile (e: its '\n',
// a1, or the step's end of a line cut at the limit); have[k] says class k was
// met in it, first[k] where first.  All 64 lanes, the same arguments.
template <uint32_t kClasses, typename Cls, typename Line>
__device__ __forceinline__ void walk_lines(const uint8_t* text, uint64_t a0, uint64_t a1, uint64_t tb, uint64_t te,
                                           uint64_t max_line, uint32_t lane, Cls cls, Line line) {
  constexpr uint32_t kN = kClasses ? kClasses : 1;
  bool in_line = tb == a0;
  uint32_t done = 0;  // (a word: as a bool it leaves the unrolled steps as a lane mask, and k_cs_scan then needs
                      // more SGPRs than 8 waves a SIMD have)
  bool have[kN] = {};
  uint64_t first[kN] = {};
  uint64_t s = a0;
  uint64_t cb = tb == a0 ? a0 : tb - 1;
  auto line_end = [&](uint64_t e) {
    in_line = false;
    line(s, e, have, first);
  };
  while (!done) {
    uint32_t c[kWalkLoad];
#pragma unroll
    for (uint32_t k = 0; k < kWalkLoad; k++) {
      const uint64_t pos = cb + kWalkStep * k + lane;
      c[k] = pos < a1 ? text[pos] : 0x100u;  // (no byte)
    }
#pragma unroll
    for (uint32_t k = 0; k < kWalkLoad; k++) {
      if (done) break;
      const uint64_t base = cb + kWalkStep * k;
      if (base >= a1) {  // (an open line always ends in the step that holds the segment's end)
        if (in_line) line_end(a1);
        done = 1;
        break;
      }
      const uint64_t nl = __ballot(c[k] == '\n');
      uint64_t m[kN] = {};
      cls(c[k], m);
      uint32_t bit = 0;
      while (true) {
        if (!in_line) {  // the next '\n' that a line of this tile starts behind
          if (bit >= 64) break;
          const uint64_t nlm = nl & (~0ull << bit);
          if (!nlm) break;
          const uint32_t i = (uint32_t)__builtin_ctzll(nlm);
          if (base + i + 1 >= te) {
            done = 1;
            break;
          }
          s = base + i + 1;
          in_line = true;
#pragma unroll
          for (uint32_t j = 0; j < kClasses; j++) have[j] = false;
          bit = i + 1;
        }
        if (bit >= 64) break;
        const uint64_t from = ~0ull << bit, nlm = nl & from;
        const uint32_t endi = nlm ? (uint32_t)__builtin_ctzll(nlm) : 64u;
        const uint64_t reg = endi < 64 ? from & ((1ull << endi) - 1) : from;
#pragma unroll
        for (uint32_t j = 0; j < kClasses; j++)
          if (!have[j] && (m[j] & reg)) {
            first[j] = base + (uint32_t)__builtin_ctzll(m[j] & reg);
            have[j] = true;
          }
        if (endi < 64) {
          line_end(base + endi);
          bit = endi;  // (that '\n' may start the next line)
          continue;
        }
        if (base + kWalkStep >= a1) {
          line_end(a1);
          done = 1;
        } else if (base + kWalkStep - s >= max_line) {
          line_end(base + kWalkStep);  // too long already, wherever it ends
        }
        break;
      }
      if (!in_line && base + kWalkStep + 1 >= te) done = 1;
    }
    cb += kWalkLoad * kWalkStep;
  }
}

// The kept lines of a tile, written kLineGroup to a store: lane n & 63 keeps
// the n-th kept line's payload, the 64th stores all of them, the tile's end the
// rest.  store(i0, payload): this lane's payload is the tile's (i0 + lane)-th
// kept line's; where that goes, and whether it is in bounds, is the caller's.
// (i0 is the same in all lanes and the lane is added by the caller, behind its
// own uniform base: a count that meets the lane in 32-bit arithmetic here is
// moved to a VGPR as a whole, and every test of it then goes through exec.)  A
// pass that only counts calls count().
template <typename T>
struct LineGroup {
  uint32_t n = 0;
  T mine{};
  __device__ __forceinline__ void count() { n++; }
  template <typename Store>
  __device__ __forceinline__ void add(uint32_t lane, const T& v, Store store) {
    if (lane == (n & (kLineGroup - 1))) mine = v;
    if ((n & (kLineGroup - 1)) == kLineGroup - 1) store(n - (kLineGroup - 1), mine);
    n++;
  }
  template <typename Store>
  __device__ __forceinline__ void flush(uint32_t lane, Store store) {
    const uint32_t held = n & (kLineGroup - 1);
    if (lane < held) store(n - held, mine);
  }
};

// ---- the whole wave on one line: all 64 lanes, the same arguments --------------
__device__ __forceinline__ uint64_t wave_bcast64(uint64_t v, uint32_t src) {
  return (uint64_t)__shfl((unsigned long long)v, (int)src);
}

// Does the needle (its bytes b[], len of them) stand at p, inside [p, to)?  (a lane's own question)
template <typename Needle>
__device__ __forceinline__ bool needle_at(const uint8_t* text, const Needle& n, uint64_t p, uint64_t to) {
  const uint32_t len = n.len;
  if (p > to || to - p < len) return false;
  for (uint32_t k = 0; k < len && k < sizeof(n.b); k++)
    if (text[p + k] != (uint8_t)n.b[k]) return false;
  return true;
}

// The leftmost place of the needle in [from, to), or `to`.  64 places a step.
template <typename Needle>
__device__ __forceinline__ uint64_t wave_find_needle(const uint8_t* text, const Needle& n, uint64_t from, uint64_t to,
                                                     uint32_t lane) {
  const uint32_t len = n.len;
  for (uint64_t p0 = from; p0 < to && to - p0 >= len; p0 += 64) {
    const uint64_t m = __ballot(needle_at(text, n, p0 + lane, to));
    if (m) return p0 + (uint32_t)__builtin_ctzll(m);
  }
  return to;
}

}  // namespace sgd
