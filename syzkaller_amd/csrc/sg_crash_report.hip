// sg_crash_report.hip -- pkg/report over a batch of console logs: the header
// search of report.ContainsCrash (pkg/report/report.go:369-387) and matchOops
// (:515-531), everything of report.Parse before extractDescription (:393-465)
// and report.ExtractConsoleOutput (:492-513), each over a CSR of logs in one
// call.  The oops table (:29-345) is fixed below, in the reference's order.
//
// Nothing walks a log.  Every stage is a launch over the batch's bytes, its
// lines or its logs:
//
//   k_cr_mark    a thread a log: one bit at the first byte of every log that
//                has bytes, so that a line never runs on into the next log.
//   k_cr_starts  a workgroup a tile of SG_CRASH_TILE bytes, a thread 16 of
//                them: a line starts at byte 0, at a marked byte and behind
//                every '\n'.  Counted, scanned (sg_scan.hip), run again to
//                write: the line table lstart, ascending, lstart[nlines] the
//                batch's end.  Lines tile the batch, so a line's content ends
//                at the next line's start, less its '\n' where it has one.
//   k_cr_flags   a workgroup a tile, held in LDS with a halo of
//                SG_CRASH_MAX_LITERAL - 1 bytes behind it: every byte asks a
//                256-entry table which of the 24 literals start with it, and
//                compares those in LDS.  A literal that stands there finds its
//                line by a search of lstart, is dropped when it runs past the
//                next line's start (no literal holds a '\n', so that is a
//                log's end), and ORs its bit into the line's word.  The one
//                literal that is an anchor, " ? ", walks the rest of
//                questionableRe from there (each class run is closed by a byte
//                outside the class, so the walk is the regexp) and ORs another
//                bit.  Lines hold literals seldom; the atomics are rare and
//                idempotent.
//   k_cr_line    a thread a line: the suppressions from the bits, the ignore
//                list, consoleOutputRe's prefix read from the line's start.
//                The two-part NMI suppression needs places, not bits: a line
//                with "INFO:" and both halves is taken by the whole wave, 64
//                places a step (leftmost first half, then any second half at
//                or behind its end).  With first/last, the logs' first and
//                last record line by atomicMin / atomicMax.
//   then counts over the lines and their scans: records (sg_crash_scan),
//   console lines (the ranks that the text's window and cut are stated in)
//   and text bytes; k_cr_records / k_cr_logs find a header's leftmost place
//   with the whole wave on the few lines that have one; k_cr_copy writes the
//   bodies, a wave 64 lines, a lane a byte of their output per step.
//
// Every index is checked before it is an address: byte positions against the
// batch's end, line indices against nlines, records and text bytes against
// cap, the device forms' offsets through csr_range.  Every loop is bounded by
// a line's length or halves an interval.
#include "sg_internal.h"
#include "sg_linewalk.h"
#include "sg_rank.h"

#include <algorithm>
#include <cstring>

namespace sg {
namespace {

constexpr uint32_t kCrTile = SG_CRASH_TILE;
constexpr uint32_t kCrBlock = 256;
constexpr uint32_t kCrPer = kCrTile / kCrBlock;  // bytes of a thread of k_cr_starts
constexpr uint32_t kCrHalo = SG_CRASH_MAX_LITERAL - 1;
constexpr uint64_t kCrMaxBytes = 1ull << 32;
constexpr uint32_t kCrPrefix = 5, kCrPanicRank = 40;  // report.go:426, :442
static_assert(kCrPer == 16 && kCrTile % 4 == 0, "k_cr_starts reads one 16-bit half of a mark word per thread");

// The literals.  0..12 are the oops headers in table order; a literal's index is its bit in a line's word.
#define CR_LITS(X)                                                                                               \
  X("BUG:") X("WARNING:") X("INFO:") X("Unable to handle kernel paging request") X("general protection fault:") \
  X("Kernel panic") X("kernel BUG") X("Kernel BUG") X("BUG kmalloc-") X("divide error:") X("invalid opcode:")    \
  X("unreferenced object") X("UBSAN:")                                                                           \
  X("Boot_DEBUG:") X("WARNING: /etc/ssh/moduli does not exist, using fixed modulus")                             \
  X("INFO: lockdep is turned off") X("INFO: Stall ended before state dump start") X("_INFO::")                   \
  X("INFO: NMI handler ") X(" took too long to run")                                                             \
  X("<EOI>") X("Disabling lock debugging due to kernel taint") X("Kernel panic - not syncing") X(" ? ")
enum : uint32_t {
  kLitBoot = 13, kLitModuli, kLitLockdep, kLitStall, kLitInfo2, kLitNmiA, kLitNmiB, kLitEoi, kLitTaint, kLitPanic,
  kLitAnchor, kCrLits,
  kBitQuestion = kCrLits,  // questionableRe matches somewhere in the line
};
constexpr uint32_t kOopsMask = (1u << SG_CRASH_OOPSES) - 1;
// a line's word after k_cr_line: the live oopses, then
constexpr uint32_t kLnConsole = 1u << 16, kLnTaint = 1u << 17, kLnPanic = 1u << 18;

struct CrLit {
  uint32_t len;
  char b[64];
};
#define CR_X(s) {(uint32_t)sizeof(s) - 1, s},
__constant__ CrLit d_lits[kCrLits] = {CR_LITS(CR_X)};
constexpr CrLit h_lits[] = {CR_LITS(CR_X)};
#undef CR_X
constexpr uint32_t cr_longest() {
  uint32_t m = 0;
  for (const CrLit& l : h_lits) m = l.len > m ? l.len : m;
  return m;
}
static_assert(sizeof(h_lits) / sizeof(h_lits[0]) == kCrLits && kCrLits <= 24, "a literal's index is a bit below 24");
static_assert(SG_CRASH_OOPSES == 13 && cr_longest() == SG_CRASH_MAX_LITERAL, "the header states the table");

struct CrArgs {
  const uint8_t* text;
  const uint64_t* off;  // [nlogs + 1]
  uint64_t nlogs;
  uint64_t nbytes;  // the caller's; the batch ends at min(off[nlogs], nbytes)
  uint64_t ntiles;
  uint32_t* marks;
  uint32_t* tcnt;        // [ntiles] line starts of each tile
  const uint64_t* tpos;  // [ntiles + 1] its scan
  // from here on: after the line count
  uint64_t nlines;
  uint64_t* lstart;  // [nlines + 1]
  uint32_t* word;    // [nlines]
  uint32_t* pfx;     // [nlines] a console line's prefix length
  uint32_t* cnt;     // [nlines] what is scanned next
  uint64_t* pos;     // [nlines + 1] records, then console lines
  uint64_t* opos;    // [nlines + 1] output bytes
  const uint64_t* ign_off;
  const uint64_t* ign_pos;
  uint64_t nign;
  unsigned long long* first;  // [nlogs] each log's first record line, ~0 none
  unsigned long long* last;   // [nlogs] ... last record line + 1, 0 none
  unsigned long long* cut;    // [nlogs] the cut, ~0 none
};

__device__ __forceinline__ uint64_t cr_end(const CrArgs& a) { return min(a.off[a.nlogs], a.nbytes); }
__device__ __forceinline__ bool cr_digit(uint32_t c) { return c - '0' < 10u; }
__device__ __forceinline__ bool cr_hex(uint32_t c) { return c - '0' < 10u || c - 'a' < 6u; }
__device__ __forceinline__ bool cr_word(uint32_t c) {
  return c - '0' < 10u || (c | 0x20u) - 'a' < 26u || c == '_' || c == '.';
}
// a line's content is [lstart[li], cr_content(...))
__device__ __forceinline__ uint64_t cr_content(const uint8_t* t, uint64_t s, uint64_t nx) {
  return nx > s && t[nx - 1] == '\n' ? nx - 1 : nx;
}
__device__ __forceinline__ uint64_t cr_log_of(const CrArgs& a, uint64_t s) { return sgd::seg_search(a.off, 0, a.nlogs - 1, s); }

__global__ void k_cr_mark(CrArgs a) {
  const uint64_t l = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (l >= a.nlogs) return;
  uint64_t r0, r1;
  sgd::csr_range(a.off, l, cr_end(a), r0, r1);
  if (r1 > r0) atomicOr(&a.marks[r0 >> 5], 1u << (r0 & 31));
}

// Does a line start at p (p < n)?
__device__ __forceinline__ bool cr_starts(const CrArgs& a, uint64_t p, uint32_t mark_bits, uint32_t prev) {
  return p == 0 || ((mark_bits >> (p & 31)) & 1u) || prev == '\n';
}

template <bool kEmit>
__global__ __launch_bounds__(kCrBlock) void k_cr_starts(CrArgs a) {
  __shared__ uint32_t s_wave[kCrBlock / 64];
  const uint64_t n = cr_end(a);
  const uint64_t tb = (uint64_t)blockIdx.x * kCrTile;
  const uint64_t p0 = tb + (uint64_t)threadIdx.x * kCrPer;
  uint32_t mine = 0;  // bit k: a line starts at p0 + k
  if (p0 < n) {
    const uint32_t mb = a.marks[p0 >> 5];
    uint32_t prev = p0 ? a.text[p0 - 1] : 0u;
    for (uint32_t k = 0; k < kCrPer && p0 + k < n; k++) {
      if (cr_starts(a, p0 + k, mb, prev)) mine |= 1u << k;
      prev = a.text[p0 + k];
    }
  }
  const uint32_t c = (uint32_t)__popc(mine);
  const uint32_t incl = sgd::wave_incl_add(c);
  const uint32_t lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  if (lane == 63) s_wave[w] = incl;
  __syncthreads();
  uint32_t before = 0, total = 0;
  for (uint32_t k = 0; k < kCrBlock / 64; k++) {
    if (k < w) before += s_wave[k];
    total += s_wave[k];
  }
  if (!kEmit) {
    if (threadIdx.x == 0) a.tcnt[blockIdx.x] = total;
    return;
  }
  uint64_t o = a.tpos[blockIdx.x] + before + (incl - c);
  for (uint32_t m = mine; m; m &= m - 1, o++)
    if (o < a.nlines) a.lstart[o] = p0 + (uint32_t)__builtin_ctz(m);
  if (blockIdx.x == 0 && threadIdx.x == 0) a.lstart[a.nlines] = n;
}

// The line of byte p: the last one that starts at or before it (line 0 starts at 0).
__device__ __forceinline__ uint64_t cr_line_of(const CrArgs& a, uint64_t p) {
  const uint64_t j = sgd::ub64(a.lstart, a.nlines, p);
  return j ? j - 1 : 0;
}

// questionableRe from its " ? " at p, inside [p, nx): ` \? +[a-zA-Z0-9_.]+\+0x[0-9a-f]+/[0-9a-f]+`.  The optional
// group in front of it changes no answer.  Each run ends at the first byte outside its class, and what must follow
// is outside it too, so there is one way to read it.
__device__ bool cr_question(const uint8_t* t, uint64_t p, uint64_t nx) {
  uint64_t q = p + 2;
  while (q < nx && t[q] == ' ') q++;
  const uint64_t w0 = q;
  while (q < nx && cr_word(t[q])) q++;
  if (q == w0 || nx - q < 3 || t[q] != '+' || t[q + 1] != '0' || t[q + 2] != 'x') return false;
  q += 3;
  const uint64_t h0 = q;
  while (q < nx && cr_hex(t[q])) q++;
  if (q == h0 || nx - q < 2 || t[q] != '/') return false;
  return cr_hex(t[q + 1]);
}

__global__ __launch_bounds__(kCrBlock) void k_cr_flags(CrArgs a) {
  __shared__ uint32_t s_first[256];
  __shared__ uint8_t s_t[kCrTile + kCrHalo + 1];
  const uint64_t n = cr_end(a);
  const uint64_t tb = (uint64_t)blockIdx.x * kCrTile;
  {
    uint32_t m = 0;
    for (uint32_t j = 0; j < kCrLits; j++)
      if ((uint8_t)d_lits[j].b[0] == threadIdx.x) m |= 1u << j;
    s_first[threadIdx.x] = m;
  }
  if (tb >= n) return;  // (the whole workgroup)
  for (uint32_t i = threadIdx.x; i < kCrTile + kCrHalo; i += kCrBlock) s_t[i] = tb + i < n ? a.text[tb + i] : 0;
  __syncthreads();
  const uint32_t have = (uint32_t)min((uint64_t)kCrTile, n - tb);
  for (uint32_t i = threadIdx.x; i < have; i += kCrBlock) {
    uint32_t m = s_first[s_t[i]];
    for (; m; m &= m - 1) {
      const uint32_t j = (uint32_t)__builtin_ctz(m);
      const uint32_t len = d_lits[j].len;
      const uint64_t p = tb + i;
      if (n - p < len) continue;
      bool same = true;
      for (uint32_t k = 1; k < len && k <= kCrHalo; k++)
        if (s_t[i + k] != (uint8_t)d_lits[j].b[k]) {
          same = false;
          break;
        }
      if (!same) continue;
      const uint64_t li = cr_line_of(a, p);
      const uint64_t nx = min(a.lstart[li + 1], n);
      if (nx < p || nx - p < len) continue;  // it runs into the next log
      if (j == kLitAnchor) {
        if (cr_question(a.text, p, nx)) atomicOr(&a.word[li], 1u << kBitQuestion);
      } else {
        atomicOr(&a.word[li], 1u << j);
      }
    }
  }
}

// consoleOutputRe at a line's start: `^(?:<[0-9]+>)?\[ *[0-9]+\.[0-9]+\] `; *body the place behind it
__device__ bool cr_prefix(const uint8_t* t, uint64_t s, uint64_t e, uint64_t* body) {
  uint64_t q = s;
  if (q < e && t[q] == '<') {
    uint64_t d = q + 1;
    while (d < e && cr_digit(t[d])) d++;
    if (d == q + 1 || d >= e || t[d] != '>') return false;
    q = d + 1;
  }
  if (q >= e || t[q] != '[') return false;
  q++;
  while (q < e && t[q] == ' ') q++;
  uint64_t d = q;
  while (q < e && cr_digit(t[q])) q++;
  if (q == d || q >= e || t[q] != '.') return false;
  d = ++q;
  while (q < e && cr_digit(t[q])) q++;
  if (q == d || e - q < 2 || t[q] != ']' || t[q + 1] != ' ') return false;
  *body = q + 2;
  return true;
}

// Is rel among log l's ignored line starts?
__device__ bool cr_ignored(const CrArgs& a, uint64_t l, uint64_t rel) {
  if (!a.ign_off) return false;
  uint64_t r0, r1;
  sgd::csr_range(a.ign_off, l, a.nign, r0, r1);
  const uint64_t j = r0 + sgd::lb64(a.ign_pos + r0, r1 - r0, rel);
  return j < r1 && a.ign_pos[j] == rel;
}

template <bool kBounds>
__global__ __launch_bounds__(kCrBlock) void k_cr_line(CrArgs a) {
  const uint64_t li = (uint64_t)blockIdx.x * kCrBlock + threadIdx.x;
  const uint32_t lane = threadIdx.x & 63;
  const bool in = li < a.nlines;
  uint64_t s = 0, e = 0;
  uint32_t f = 0;
  if (in) {
    s = a.lstart[li];
    e = cr_content(a.text, s, a.lstart[li + 1]);
    f = a.word[li];
  }
  uint32_t live = f & kOopsMask;
  if (f & (1u << kLitBoot)) live &= ~1u;
  if (f & (1u << kLitModuli)) live &= ~2u;
  if (f & ((1u << kLitLockdep) | (1u << kLitStall) | (1u << kLitInfo2))) live &= ~4u;
  // "INFO: NMI handler .* took too long to run": the whole wave, a line at a time (every lane stays to the end)
  bool nmi = (live & 4u) && (f & (1u << kLitNmiA)) && (f & (1u << kLitNmiB));
  for (uint64_t m = __ballot(nmi); m; m &= m - 1) {
    const uint32_t src = (uint32_t)__builtin_ctzll(m);
    const uint64_t ls = sgd::wave_bcast64(s, src), le = sgd::wave_bcast64(e, src);
    const uint64_t at = sgd::wave_find_needle(a.text, d_lits[kLitNmiA], ls, le, lane);
    bool supp = false;
    if (at < le) supp = sgd::wave_find_needle(a.text, d_lits[kLitNmiB], at + d_lits[kLitNmiA].len, le, lane) < le;
    if (lane == src && supp) live &= ~4u;
  }
  uint64_t l = 0;
  if (live) {
    l = cr_log_of(a, s);
    if (cr_ignored(a, l, s - a.off[l])) live = 0;
  }
  uint32_t out = live, pfx = 0;
  if (in) {
    uint64_t body = 0;
    if (cr_prefix(a.text, s, e, &body) && (!(f & (1u << kBitQuestion)) || (f & (1u << kLitEoi)))) {
      out |= kLnConsole;
      pfx = (uint32_t)(body - s);
    }
    if (f & (1u << kLitTaint)) out |= kLnTaint;
    if (f & (1u << kLitPanic)) out |= kLnPanic;
    a.word[li] = out;
    a.pfx[li] = pfx;
    if (kBounds && live) {
      atomicMin(&a.first[l], (unsigned long long)li);
      atomicMax(&a.last[l], (unsigned long long)li + 1);
    }
  }
}

// a console line's body: [s + pfx, its content's end less one '\r')
__device__ __forceinline__ uint64_t cr_body_end(const uint8_t* t, uint64_t s, uint64_t nx) {
  const uint64_t e = cr_content(t, s, nx);
  return e > s && t[e - 1] == '\r' ? e - 1 : e;
}

enum : int { kCntRecords = 0, kCntConsole = 1, kCntOutput = 2, kCntText = 3 };
template <int kWhat>
__global__ __launch_bounds__(kCrBlock) void k_cr_cnt(CrArgs a) {
  const uint64_t li = (uint64_t)blockIdx.x * kCrBlock + threadIdx.x;
  if (li >= a.nlines) return;
  const uint32_t w = a.word[li];
  uint32_t c = 0;
  if (kWhat == kCntRecords) c = (uint32_t)__popc(w & kOopsMask);
  if (kWhat == kCntConsole) c = w & kLnConsole ? 1u : 0u;
  if (kWhat == kCntOutput || kWhat == kCntText) {
    bool take = w & kLnConsole;
    if (kWhat == kCntText && take) {
      // report.go:417-459 without its state: the window of five before the first record line, the lines from
      // it on that are no taint line, all of it only up to the cut and only when a console line follows
      const uint64_t l = cr_log_of(a, a.lstart[li]);
      const uint64_t l0 = a.first[l];
      take = l0 < a.nlines && li < a.cut[l];
      if (take && li >= l0) take = !(w & kLnTaint);  // (:440 is asked only once there is an oops)
      if (take && li < l0) {
        uint64_t r0, r1;
        sgd::csr_range(a.off, l, cr_end(a), r0, r1);
        const uint64_t lend = sgd::lb64(a.lstart, a.nlines, r1);  // the log's lines end here
        take = a.pos[l0] - a.pos[li] <= kCrPrefix && a.pos[min(max(lend, l0), a.nlines)] > a.pos[l0];
      }
    }
    if (take) {
      const uint64_t s = a.lstart[li];
      c = (uint32_t)(cr_body_end(a.text, s, a.lstart[li + 1]) - (s + a.pfx[li])) + 1;
    }
  }
  a.cnt[li] = c;
}

// the cut (report.go:442): the first console line from the first record line on, above rank 40, with the panic
// sentence and without the taint sentence
__global__ __launch_bounds__(kCrBlock) void k_cr_cut(CrArgs a) {
  const uint64_t li = (uint64_t)blockIdx.x * kCrBlock + threadIdx.x;
  if (li >= a.nlines) return;
  const uint32_t w = a.word[li];
  if (!(w & kLnConsole) || !(w & kLnPanic) || (w & kLnTaint)) return;
  const uint64_t l = cr_log_of(a, a.lstart[li]);
  const uint64_t l0 = a.first[l];
  if (l0 >= a.nlines || li < l0) return;
  if (a.pos[li] - a.pos[l0] + 1 > kCrPanicRank) atomicMin(&a.cut[l], (unsigned long long)li);
}

struct CrRecs {
  uint8_t* contains;
  uint32_t* log;
  uint64_t* start;
  uint64_t* end;
  uint32_t* oops;
  uint64_t* match;
  uint64_t cap;
  uint64_t* nrec;
};

// One record per (line, live oops), at pos[li] + its rank among the line's: the wave finds each header's
// leftmost place, a line at a time.
__global__ __launch_bounds__(kCrBlock) void k_cr_records(CrArgs a, CrRecs r) {
  const uint64_t li = (uint64_t)blockIdx.x * kCrBlock + threadIdx.x;
  const uint32_t lane = threadIdx.x & 63;
  const uint64_t total = a.pos[a.nlines];
  if (blockIdx.x == 0 && threadIdx.x == 0) *r.nrec = total;
  uint64_t s = 0, e = 0, o = 0;
  uint32_t live = 0;
  if (li < a.nlines) {
    live = a.word[li] & kOopsMask;
    s = a.lstart[li];
    e = cr_content(a.text, s, a.lstart[li + 1]);
    o = a.pos[li];
  }
  for (uint64_t m = __ballot(live != 0); m; m &= m - 1) {
    const uint32_t src = (uint32_t)__builtin_ctzll(m);
    const uint64_t ls = sgd::wave_bcast64(s, src), le = sgd::wave_bcast64(e, src);
    uint64_t at = sgd::wave_bcast64(o, src);
    const uint64_t l = cr_log_of(a, ls);
    const uint64_t base = a.off[l];
    if (lane == 0) r.contains[l] = 1;
    for (uint32_t lv = (uint32_t)__shfl((int)live, (int)src); lv; lv &= lv - 1, at++) {
      const uint32_t j = (uint32_t)__builtin_ctz(lv);
      const uint64_t p = sgd::wave_find_needle(a.text, d_lits[j], ls, le, lane);
      if (lane != 0 || total > r.cap || at >= r.cap) continue;
      r.log[at] = (uint32_t)l;
      r.start[at] = ls - base;
      r.end[at] = le - base;
      r.oops[at] = j;
      r.match[at] = p - ls;
    }
  }
}

struct CrLogs {
  int32_t* oops;
  uint64_t* start;
  uint64_t* end;
  uint64_t* desc_pos;
  uint64_t* desc_len;
  uint64_t* text_off;  // [nlogs + 1]
};

// A thread a log: its bounds, and where its bytes of the output start.  The description's place is the leftmost
// header of the first live oops of the first record line: the wave, a log at a time.
template <bool kBounds>
__global__ __launch_bounds__(kCrBlock) void k_cr_logs(CrArgs a, CrLogs r) {
  const uint64_t l = (uint64_t)blockIdx.x * kCrBlock + threadIdx.x;
  const uint32_t lane = threadIdx.x & 63;
  const bool in = l < a.nlogs;
  uint64_t l0 = ~0ull;
  if (in) {
    uint64_t r0, r1;
    sgd::csr_range(a.off, l, cr_end(a), r0, r1);
    r.text_off[l] = a.nlines ? a.opos[min(sgd::lb64(a.lstart, a.nlines, r0), a.nlines)] : 0;
    if (l == 0) r.text_off[a.nlogs] = a.nlines ? a.opos[a.nlines] : 0;
    if (kBounds && a.nlines) l0 = a.first[l];
    if (kBounds && l0 >= a.nlines) {
      r.oops[l] = -1;
      r.start[l] = r.end[l] = r.desc_pos[l] = r.desc_len[l] = 0;
    }
  }
  if (!kBounds) return;
  for (uint64_t m = __ballot(in && l0 < a.nlines); m; m &= m - 1) {
    const uint32_t src = (uint32_t)__builtin_ctzll(m);
    const uint64_t gl = sgd::wave_bcast64(l, src), fl = sgd::wave_bcast64(l0, src);
    const uint64_t ls = a.lstart[fl], le = cr_content(a.text, ls, a.lstart[fl + 1]);
    const uint32_t lv = a.word[fl] & kOopsMask;
    const uint32_t j = lv ? (uint32_t)__builtin_ctz(lv) : 0u;  // (a first record line has a live oops)
    const uint64_t p = sgd::wave_find_needle(a.text, d_lits[j], ls, le, lane);
    if (lane != 0) continue;
    const uint64_t base = a.off[gl];
    const uint64_t ll = min((uint64_t)a.last[gl], a.nlines);
    r.oops[gl] = (int32_t)j;
    r.start[gl] = ls - base;
    r.end[gl] = (ll ? cr_content(a.text, a.lstart[ll - 1], a.lstart[ll]) : le) - base;
    r.desc_pos[gl] = p - base;
    r.desc_len[gl] = le - p;
  }
}

// The bodies: a wave takes 64 lines, whose output is one run of bytes, and writes it 64 bytes a step; a lane
// finds its byte's line among the 64 offsets the wave holds in LDS.
__global__ __launch_bounds__(kCrBlock) void k_cr_copy(CrArgs a, uint8_t* out, uint64_t cap) {
  __shared__ uint64_t s_o[kCrBlock / 64][65];
  const uint32_t lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const uint64_t base = ((uint64_t)blockIdx.x * (kCrBlock / 64) + w) * 64;
  const bool run = base < a.nlines && a.opos[a.nlines] <= cap;  // (the whole wave)
  const uint64_t cnt = run ? min((uint64_t)64, a.nlines - base) : 0;
  uint64_t src = 0, len = 0;
  if (lane < cnt) {
    const uint64_t li = base + lane;
    len = a.opos[li + 1] - a.opos[li];
    src = a.lstart[li] + a.pfx[li];
  }
  if (run) s_o[w][lane] = lane < cnt ? a.opos[base + lane] : a.opos[base + cnt];
  if (run && lane == 0) s_o[w][64] = a.opos[base + cnt];
  __syncthreads();
  if (!run) return;
  const uint64_t o0 = s_o[w][0], o1 = s_o[w][64];
  const uint64_t n = cr_end(a);
  for (uint64_t ob = o0; ob < o1; ob += 64) {
    const uint64_t o = ob + lane;
    // the last of the 64 lines that starts at or before o
    uint32_t lo = 0, hi = 63;
    while (lo < hi) {
      const uint32_t mid = (lo + hi + 1) >> 1;
      if (s_o[w][mid] <= o)
        lo = mid;
      else
        hi = mid - 1;
    }
    const uint64_t lsrc = sgd::wave_bcast64(src, lo), llen = sgd::wave_bcast64(len, lo), lo0 = s_o[w][lo];
    if (o >= o1 || o >= cap) continue;
    const uint64_t k = o - lo0;
    const uint64_t p = lsrc + k;
    out[o] = k + 1 >= llen || p >= n ? '\n' : a.text[p];
  }
}

// nothing to scan: every log is empty (or there is none)
__global__ void k_cr_none(uint64_t nlogs, CrRecs r, CrLogs g, bool recs, bool bounds) {
  const uint64_t l = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (l == 0 && recs) *r.nrec = 0;
  if (l == 0 && !recs) g.text_off[nlogs] = 0;
  if (l >= nlogs) return;
  if (recs) {
    r.contains[l] = 0;
    return;
  }
  g.text_off[l] = 0;
  if (bounds) {
    g.oops[l] = -1;
    g.start[l] = g.end[l] = g.desc_pos[l] = g.desc_len[l] = 0;
  }
}

__global__ void k_cr_stats(CrArgs a, uint64_t* stats, const uint64_t* console, const uint64_t* records) {
  stats[0] = a.nlines;
  stats[1] = console ? console[a.nlines] : 0;
  stats[2] = records ? records[a.nlines] : 0;
}

// ---- host ------------------------------------------------------------------------------------------------------
enum : int { kScan = 0, kParse = 1, kConsole = 2 };

struct CrPlan {
  WsPlan p;
  size_t o_marks, o_tcnt, o_tpos, o_scan;
  uint64_t ntiles;
  CrPlan(uint64_t nbytes) {
    ntiles = (nbytes + kCrTile - 1) / kCrTile;
    o_marks = p.add((nbytes / 32 + 2) * 4);
    o_tcnt = p.add(ntiles * 4 + 4);
    o_tpos = p.add((ntiles + 1) * 8);
    o_scan = p.add(scan_ws_bytes(std::max<uint64_t>(ntiles, 1)));
  }
};

int cr_count_lines(sg_ctx* ctx, const CrPlan& pl, CrArgs& a, uint64_t* nlines) {
  a.marks = (uint32_t*)ws_at(ctx, pl.o_marks);
  a.tcnt = (uint32_t*)ws_at(ctx, pl.o_tcnt);
  a.tpos = (const uint64_t*)ws_at(ctx, pl.o_tpos);
  SG_HIP(hipMemsetAsync(a.marks, 0, (a.nbytes / 32 + 2) * 4, ctx->stream));
  {
    ScopedTimer tm(ctx, "crash_lines");
    hipLaunchKernelGGL(k_cr_mark, dim3(div_up(a.nlogs, 256)), dim3(256), 0, ctx->stream, a);
    hipLaunchKernelGGL(k_cr_starts<false>, dim3((uint32_t)pl.ntiles), dim3(kCrBlock), 0, ctx->stream, a);
    SG_HIP(hipGetLastError());
  }
  int rc = scan_counts(ctx, a.tcnt, (uint64_t*)ws_at(ctx, pl.o_tpos), pl.ntiles, pl.o_scan);
  if (rc) return rc;
  SG_HIP(hipMemcpyAsync(nlines, a.tpos + pl.ntiles, 8, hipMemcpyDeviceToHost, ctx->stream));
  SG_HIP(hipStreamSynchronize(ctx->stream));
  return SG_OK;
}

// The three calls' body (ctx lock held, the device ensured): every pointer is device memory.
int crash_body(sg_ctx* ctx, int what, const uint8_t* d_bytes, const uint64_t* d_off, uint64_t nlogs, uint64_t nbytes,
               const uint64_t* d_ign_off, const uint64_t* d_ign_pos, uint64_t nign, const CrRecs& recs, const CrLogs& logs,
               uint8_t* d_out, uint64_t cap, uint64_t* d_stats) {
  if (nlogs == 0 || nbytes == 0) {
    hipLaunchKernelGGL(k_cr_none, dim3(div_up(std::max<uint64_t>(nlogs, 1), 256)), dim3(256), 0, ctx->stream, nlogs, recs,
                       logs, what == kScan, what == kParse);
    SG_HIP(hipGetLastError());
    if (d_stats) SG_HIP(hipMemsetAsync(d_stats, 0, SG_CRASH_NSTATS * 8, ctx->stream));
    return SG_OK;
  }
  const CrPlan pl(nbytes);
  int rc = ws_reserve(ctx, pl.p);
  if (rc) return rc;
  CrArgs a{};
  a.text = d_bytes;
  a.off = d_off;
  a.nlogs = nlogs;
  a.nbytes = nbytes;
  a.ntiles = pl.ntiles;
  a.ign_off = d_ign_off && d_ign_pos && nign ? d_ign_off : nullptr;
  a.ign_pos = d_ign_pos;
  a.nign = nign;
  uint64_t nlines = 0;
  if ((rc = cr_count_lines(ctx, pl, a, &nlines))) return rc;
  if (nlines == 0 || nlines > nbytes) {  // (offsets that leave the batch no bytes; never more lines than bytes)
    hipLaunchKernelGGL(k_cr_none, dim3(div_up(nlogs, 256)), dim3(256), 0, ctx->stream, nlogs, recs, logs, what == kScan,
                       what == kParse);
    SG_HIP(hipGetLastError());
    if (d_stats) SG_HIP(hipMemsetAsync(d_stats, 0, SG_CRASH_NSTATS * 8, ctx->stream));
    return SG_OK;
  }
  WsPlan p = pl.p;
  const size_t o_lstart = p.add((nlines + 1) * 8), o_word = p.add(nlines * 4), o_pfx = p.add(nlines * 4);
  const size_t o_cnt = p.add(nlines * 4), o_pos = p.add((nlines + 1) * 8), o_opos = p.add((nlines + 1) * 8);
  const size_t o_logs = p.add(nlogs * 24), o_scan = p.add(scan_ws_bytes(nlines));
  // (growing drops the tiles' counts: count again, into the workspace that has room for the rest)
  rc = ws_reserve_redo(ctx, p.total, [&] {
    uint64_t again = 0;
    const int r = cr_count_lines(ctx, pl, a, &again);
    return r ? r : again == nlines ? SG_OK : SG_EHIP;
  });
  if (rc) return rc;
  a.nlines = nlines;
  a.lstart = (uint64_t*)ws_at(ctx, o_lstart);
  a.word = (uint32_t*)ws_at(ctx, o_word);
  a.pfx = (uint32_t*)ws_at(ctx, o_pfx);
  a.cnt = (uint32_t*)ws_at(ctx, o_cnt);
  a.pos = (uint64_t*)ws_at(ctx, o_pos);
  a.opos = (uint64_t*)ws_at(ctx, o_opos);
  a.first = (unsigned long long*)ws_at(ctx, o_logs);
  a.cut = a.first + nlogs;
  a.last = a.cut + nlogs;
  const dim3 lgrid(div_up(nlines, kCrBlock)), tgrid((uint32_t)pl.ntiles), blk(kCrBlock);
  SG_HIP(hipMemsetAsync(a.word, 0, nlines * 4, ctx->stream));
  SG_HIP(hipMemsetAsync(a.first, 0xFF, nlogs * 16, ctx->stream));  // (first and cut)
  SG_HIP(hipMemsetAsync(a.last, 0, nlogs * 8, ctx->stream));
  {
    ScopedTimer tm(ctx, "crash_lines");
    hipLaunchKernelGGL(k_cr_starts<true>, tgrid, blk, 0, ctx->stream, a);
  }
  {
    ScopedTimer tm(ctx, "crash_flags");
    hipLaunchKernelGGL(k_cr_flags, tgrid, blk, 0, ctx->stream, a);
  }
  {
    ScopedTimer tm(ctx, "crash_line");
    if (what == kParse)
      hipLaunchKernelGGL(k_cr_line<true>, lgrid, blk, 0, ctx->stream, a);
    else
      hipLaunchKernelGGL(k_cr_line<false>, lgrid, blk, 0, ctx->stream, a);
  }
  SG_HIP(hipGetLastError());
  const uint64_t *d_console = nullptr, *d_records = nullptr;
  if (what == kScan) {
    hipLaunchKernelGGL(k_cr_cnt<kCntRecords>, lgrid, blk, 0, ctx->stream, a);
    if ((rc = scan_counts(ctx, a.cnt, a.pos, nlines, o_scan))) return rc;
    SG_HIP(hipMemsetAsync(recs.contains, 0, nlogs, ctx->stream));
    ScopedTimer tm(ctx, "crash_records");
    hipLaunchKernelGGL(k_cr_records, lgrid, blk, 0, ctx->stream, a, recs);
    d_records = a.pos;
  } else {
    if (what == kParse) {
      hipLaunchKernelGGL(k_cr_cnt<kCntConsole>, lgrid, blk, 0, ctx->stream, a);
      if ((rc = scan_counts(ctx, a.cnt, a.pos, nlines, o_scan))) return rc;
      hipLaunchKernelGGL(k_cr_cut, lgrid, blk, 0, ctx->stream, a);
      hipLaunchKernelGGL(k_cr_cnt<kCntText>, lgrid, blk, 0, ctx->stream, a);
      d_console = a.pos;
    } else {
      hipLaunchKernelGGL(k_cr_cnt<kCntOutput>, lgrid, blk, 0, ctx->stream, a);
    }
    if ((rc = scan_counts(ctx, a.cnt, a.opos, nlines, o_scan))) return rc;
    {
      ScopedTimer tm(ctx, "crash_logs");
      if (what == kParse)
        hipLaunchKernelGGL(k_cr_logs<true>, dim3(div_up(nlogs, kCrBlock)), blk, 0, ctx->stream, a, logs);
      else
        hipLaunchKernelGGL(k_cr_logs<false>, dim3(div_up(nlogs, kCrBlock)), blk, 0, ctx->stream, a, logs);
    }
    if (cap) {
      ScopedTimer tm(ctx, "crash_copy");
      hipLaunchKernelGGL(k_cr_copy, dim3(div_up(nlines, kCrBlock)), blk, 0, ctx->stream, a, d_out, cap);
    }
  }
  if (d_stats) hipLaunchKernelGGL(k_cr_stats, dim3(1), dim3(1), 0, ctx->stream, a, d_stats, d_console, d_records);
  SG_HIP(hipGetLastError());
  return SG_OK;
}

int cr_limits(const char* fn, uint64_t nlogs, uint64_t nbytes) {
  if (nlogs >= (1ull << 32) || nbytes >= kCrMaxBytes) {
    set_error("%s: %llu logs of %llu bytes (the limits are 2^32 - 1 each)", fn, (unsigned long long)nlogs,
              (unsigned long long)nbytes);
    return SG_EINVAL;
  }
  return SG_OK;
}

int cr_invalid(const char* fn) {
  set_error("%s: invalid argument", fn);
  return SG_EINVAL;
}

// what the host forms reject of the ignore list: offsets as a CSR's, each log's places ascending and inside it
int cr_ignores_ok(const char* fn, const uint64_t* off, size_t nlogs, const uint64_t* ign_off, const uint64_t* ign_pos) {
  if (!ign_off) return SG_OK;
  if (!offsets_ok(ign_off, nlogs) || (ign_off[nlogs] && !ign_pos)) {
    set_error("%s: the ignore list's offsets start at 0 and do not decrease", fn);
    return SG_EINVAL;
  }
  for (size_t l = 0; l < nlogs; l++)
    for (uint64_t k = ign_off[l]; k < ign_off[l + 1]; k++)
      if (ign_pos[k] >= off[l + 1] - off[l] || (k > ign_off[l] && ign_pos[k] <= ign_pos[k - 1])) {
        set_error("%s: log %zu's ignored line starts ascend and lie inside the log", fn, l);
        return SG_EINVAL;
      }
  return SG_OK;
}

// The host forms' inputs in the staging buffer, behind `outs` bytes planned by the caller.
struct CrStage {
  WsPlan p;
  size_t o_bytes, o_off, o_ioff = 0, o_ipos = 0, o_stats;
  uint64_t nbytes, nign = 0;
};
CrStage cr_stage_plan(const uint64_t* off, size_t nlogs, const uint64_t* ign_off) {
  CrStage s;
  s.nbytes = off[nlogs];
  s.o_bytes = s.p.add(s.nbytes + 4);
  s.o_off = s.p.add((nlogs + 1) * 8);
  if (ign_off) {
    s.nign = ign_off[nlogs];
    s.o_ioff = s.p.add((nlogs + 1) * 8);
    s.o_ipos = s.p.add(s.nign * 8 + 8);
  }
  s.o_stats = s.p.add(SG_CRASH_NSTATS * 8);
  return s;
}
int cr_stage_up(sg_ctx* ctx, const CrStage& s, const uint8_t* bytes, const uint64_t* off, size_t nlogs,
                const uint64_t* ign_off, const uint64_t* ign_pos) {
  int rc = upload(ctx, dstage_at<uint8_t>(ctx, s.o_bytes), bytes, s.nbytes);
  if (rc || (rc = upload(ctx, dstage_at<uint64_t>(ctx, s.o_off), off, (nlogs + 1) * 8))) return rc;
  if (ign_off) {
    if ((rc = upload(ctx, dstage_at<uint64_t>(ctx, s.o_ioff), ign_off, (nlogs + 1) * 8))) return rc;
    if ((rc = upload(ctx, dstage_at<uint64_t>(ctx, s.o_ipos), ign_pos, s.nign * 8))) return rc;
  }
  return SG_OK;
}
int cr_down(sg_ctx* ctx, void* dst, const void* src, size_t bytes) {
  if (dst && bytes) SG_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, ctx->stream));
  return SG_OK;
}

// sg_crash_parse and sg_console_output, host forms
int cr_text_host(sg_ctx* ctx, const char* fn, int what, const uint8_t* bytes, const uint64_t* off, size_t nlogs,
                 const uint64_t* ign_off, const uint64_t* ign_pos, int32_t* oops, uint64_t* start, uint64_t* end,
                 uint64_t* desc_pos, uint64_t* desc_len, uint64_t* text_off, uint8_t* text, size_t cap, size_t* ntext,
                 uint64_t* stats) {
  int rc = prog_texts_ok(fn, bytes, off, nlogs);
  if (rc || (rc = cr_limits(fn, nlogs, off[nlogs])) || (rc = cr_ignores_ok(fn, off, nlogs, ign_off, ign_pos))) return rc;
  std::lock_guard<std::mutex> g(ctx->mu);
  if ((rc = ensure_device(ctx))) return rc;
  CrStage s = cr_stage_plan(off, nlogs, ign_off);
  const uint64_t ocap = std::min<uint64_t>(cap, s.nbytes);  // (a body and its '\n' are never longer than the line)
  const size_t o_log = s.p.add(nlogs * 40 + 8), o_toff = s.p.add((nlogs + 1) * 8), o_text = s.p.add(ocap + 1);
  if ((rc = dstage_reserve(ctx, s.p)) || (rc = cr_stage_up(ctx, s, bytes, off, nlogs, ign_off, ign_pos))) return rc;
  CrLogs lg{};
  uint64_t* w = dstage_at<uint64_t>(ctx, o_log);
  lg.start = w;
  lg.end = w + nlogs;
  lg.desc_pos = w + 2 * nlogs;
  lg.desc_len = w + 3 * nlogs;
  lg.oops = (int32_t*)(w + 4 * nlogs);
  lg.text_off = dstage_at<uint64_t>(ctx, o_toff);
  uint64_t* d_stats = stats ? dstage_at<uint64_t>(ctx, s.o_stats) : nullptr;
  rc = crash_body(ctx, what, dstage_at<uint8_t>(ctx, s.o_bytes), dstage_at<uint64_t>(ctx, s.o_off), nlogs, s.nbytes,
                  ign_off ? dstage_at<uint64_t>(ctx, s.o_ioff) : nullptr,
                  ign_off ? dstage_at<uint64_t>(ctx, s.o_ipos) : nullptr, s.nign, CrRecs{}, lg,
                  dstage_at<uint8_t>(ctx, o_text), ocap, d_stats);
  if (rc) return rc;
  if (what == kParse) {
    if ((rc = cr_down(ctx, oops, lg.oops, nlogs * 4)) || (rc = cr_down(ctx, start, lg.start, nlogs * 8)) ||
        (rc = cr_down(ctx, end, lg.end, nlogs * 8)) || (rc = cr_down(ctx, desc_pos, lg.desc_pos, nlogs * 8)) ||
        (rc = cr_down(ctx, desc_len, lg.desc_len, nlogs * 8)))
      return rc;
  }
  if ((rc = cr_down(ctx, stats, d_stats, SG_CRASH_NSTATS * 8))) return rc;
  // (a total above ocap is above cap: the output is never longer than the batch)
  if ((rc = csr_download(ctx, text_off, lg.text_off, nlogs, text, dstage_at<uint8_t>(ctx, o_text), 1, ocap))) return rc;
  *ntext = text_off[nlogs];
  return SG_OK;
}

int cr_text_dev(sg_ctx* ctx, const char* fn, int what, const uint8_t* d_bytes, const uint64_t* d_off, uint64_t nlogs,
                uint64_t nbytes, const uint64_t* d_ign_off, const uint64_t* d_ign_pos, uint64_t nign, const CrLogs& lg,
                uint8_t* d_text, uint64_t cap, uint64_t* d_stats) {
  int rc = cr_limits(fn, nlogs, nbytes);
  if (rc) return rc;
  std::lock_guard<std::mutex> g(ctx->mu);
  if ((rc = ensure_device(ctx))) return rc;
  return crash_body(ctx, what, d_bytes, d_off, nlogs, nbytes, d_ign_off, d_ign_pos, nign, CrRecs{}, lg, d_text, cap,
                    d_stats);
}

}  // namespace
}  // namespace sg

using namespace sg;

extern "C" {

int sg_crash_scan_dev(sg_ctx* ctx, const uint8_t* d_bytes, const uint64_t* d_off, uint64_t nlogs, uint64_t nbytes,
                      uint8_t* d_contains, uint32_t* d_rec_log, uint64_t* d_rec_start, uint64_t* d_rec_end,
                      uint32_t* d_rec_oops, uint64_t* d_rec_match, uint64_t cap, uint64_t* d_nrec, uint64_t* d_stats) {
  const char* fn = "sg_crash_scan_dev";
  if (!ctx || !d_off || !d_nrec || (nbytes && !d_bytes) || (nlogs && !d_contains) ||
      (cap && (!d_rec_log || !d_rec_start || !d_rec_end || !d_rec_oops || !d_rec_match)))
    return cr_invalid(fn);
  int rc = cr_limits(fn, nlogs, nbytes);
  if (rc) return rc;
  std::lock_guard<std::mutex> g(ctx->mu);
  if ((rc = ensure_device(ctx))) return rc;
  const CrRecs r{d_contains, d_rec_log, d_rec_start, d_rec_end, d_rec_oops, d_rec_match, cap, d_nrec};
  return crash_body(ctx, kScan, d_bytes, d_off, nlogs, nbytes, nullptr, nullptr, 0, r, CrLogs{}, nullptr, 0, d_stats);
}

int sg_crash_scan(sg_ctx* ctx, const uint8_t* bytes, const uint64_t* off, size_t nlogs, uint8_t* contains,
                  uint32_t* rec_log, uint64_t* rec_start, uint64_t* rec_end, uint32_t* rec_oops, uint64_t* rec_match,
                  size_t cap, size_t* nrec, uint64_t* stats) {
  const char* fn = "sg_crash_scan";
  if (!ctx || !nrec || (nlogs && !contains) || (cap && (!rec_log || !rec_start || !rec_end || !rec_oops || !rec_match)))
    return cr_invalid(fn);
  int rc = prog_texts_ok(fn, bytes, off, nlogs);
  if (rc || (rc = cr_limits(fn, nlogs, off[nlogs]))) return rc;
  std::lock_guard<std::mutex> g(ctx->mu);
  if ((rc = ensure_device(ctx))) return rc;
  CrStage s = cr_stage_plan(off, nlogs, nullptr);
  const uint64_t rcap = std::min<uint64_t>(cap, s.nbytes);  // (no two headers start at one byte)
  const size_t o_cont = s.p.add(nlogs + 1), o_n = s.p.add(8), o_r64 = s.p.add(rcap * 24 + 8), o_r32 = s.p.add(rcap * 8 + 8);
  if ((rc = dstage_reserve(ctx, s.p)) || (rc = cr_stage_up(ctx, s, bytes, off, nlogs, nullptr, nullptr))) return rc;
  uint64_t* r64 = dstage_at<uint64_t>(ctx, o_r64);
  uint32_t* r32 = dstage_at<uint32_t>(ctx, o_r32);
  const CrRecs r{dstage_at<uint8_t>(ctx, o_cont), r32, r64, r64 + rcap, r32 + rcap, r64 + 2 * rcap, rcap,
                 dstage_at<uint64_t>(ctx, o_n)};
  uint64_t* d_stats = stats ? dstage_at<uint64_t>(ctx, s.o_stats) : nullptr;
  rc = crash_body(ctx, kScan, dstage_at<uint8_t>(ctx, s.o_bytes), dstage_at<uint64_t>(ctx, s.o_off), nlogs, s.nbytes,
                  nullptr, nullptr, 0, r, CrLogs{}, nullptr, 0, d_stats);
  if (rc) return rc;
  uint64_t n = 0;
  SG_HIP(hipMemcpyAsync(&n, r.nrec, 8, hipMemcpyDeviceToHost, ctx->stream));
  if ((rc = cr_down(ctx, contains, r.contains, nlogs)) || (rc = cr_down(ctx, stats, d_stats, SG_CRASH_NSTATS * 8)))
    return rc;
  SG_HIP(hipStreamSynchronize(ctx->stream));
  *nrec = n;
  if (n == 0 || n > cap) return SG_OK;  // (n <= nbytes, so n <= cap is n <= rcap)
  if ((rc = cr_down(ctx, rec_log, r.log, n * 4)) || (rc = cr_down(ctx, rec_start, r.start, n * 8)) ||
      (rc = cr_down(ctx, rec_end, r.end, n * 8)) || (rc = cr_down(ctx, rec_oops, r.oops, n * 4)) ||
      (rc = cr_down(ctx, rec_match, r.match, n * 8)))
    return rc;
  SG_HIP(hipStreamSynchronize(ctx->stream));
  return SG_OK;
}

int sg_crash_parse_dev(sg_ctx* ctx, const uint8_t* d_bytes, const uint64_t* d_off, uint64_t nlogs, uint64_t nbytes,
                       const uint64_t* d_ign_off, const uint64_t* d_ign_pos, uint64_t nign, int32_t* d_oops,
                       uint64_t* d_start, uint64_t* d_end, uint64_t* d_desc_pos, uint64_t* d_desc_len,
                       uint64_t* d_text_off, uint8_t* d_text, uint64_t cap, uint64_t* d_stats) {
  const char* fn = "sg_crash_parse_dev";
  if (!ctx || !d_off || !d_text_off || (nbytes && !d_bytes) || (cap && !d_text) || (nign && (!d_ign_off || !d_ign_pos)) ||
      (nlogs && (!d_oops || !d_start || !d_end || !d_desc_pos || !d_desc_len)))
    return cr_invalid(fn);
  const CrLogs lg{d_oops, d_start, d_end, d_desc_pos, d_desc_len, d_text_off};
  return cr_text_dev(ctx, fn, kParse, d_bytes, d_off, nlogs, nbytes, d_ign_off, d_ign_pos, nign, lg, d_text, cap, d_stats);
}

int sg_crash_parse(sg_ctx* ctx, const uint8_t* bytes, const uint64_t* off, size_t nlogs, const uint64_t* ign_off,
                   const uint64_t* ign_pos, int32_t* oops, uint64_t* start, uint64_t* end, uint64_t* desc_pos,
                   uint64_t* desc_len, uint64_t* text_off, uint8_t* text, size_t cap, size_t* ntext, uint64_t* stats) {
  const char* fn = "sg_crash_parse";
  if (!ctx || !text_off || !ntext || (cap && !text) || (nlogs && (!oops || !start || !end || !desc_pos || !desc_len)))
    return cr_invalid(fn);
  return cr_text_host(ctx, fn, kParse, bytes, off, nlogs, ign_off, ign_pos, oops, start, end, desc_pos, desc_len, text_off,
                      text, cap, ntext, stats);
}

int sg_console_output_dev(sg_ctx* ctx, const uint8_t* d_bytes, const uint64_t* d_off, uint64_t nlogs, uint64_t nbytes,
                          uint64_t* d_out_off, uint8_t* d_out, uint64_t cap, uint64_t* d_stats) {
  const char* fn = "sg_console_output_dev";
  if (!ctx || !d_off || !d_out_off || (nbytes && !d_bytes) || (cap && !d_out)) return cr_invalid(fn);
  const CrLogs lg{nullptr, nullptr, nullptr, nullptr, nullptr, d_out_off};
  return cr_text_dev(ctx, fn, kConsole, d_bytes, d_off, nlogs, nbytes, nullptr, nullptr, 0, lg, d_out, cap, d_stats);
}

int sg_console_output(sg_ctx* ctx, const uint8_t* bytes, const uint64_t* off, size_t nlogs, uint64_t* out_off,
                      uint8_t* out, size_t cap, size_t* nout, uint64_t* stats) {
  const char* fn = "sg_console_output";
  if (!ctx || !out_off || !nout || (cap && !out)) return cr_invalid(fn);
  return cr_text_host(ctx, fn, kConsole, bytes, off, nlogs, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                      out_off, out, cap, nout, stats);
}

}  // extern "C"
