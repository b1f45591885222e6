// sg_call_set.hip -- prog.CallSet (prog/encoding.go:559-592, over bufio.Scanner /
// ScanLines) for a whole batch of program texts, and the name dictionary that
// turns each call line's name into a dense id.  The hub runs CallSet on every
// record of its corpus for every manager's every sync (syz-hub/state/state.go:
// 265-308), on every input (:326-336) and on the whole database at start-up
// (:83-110).
//
// The scan.  A program is cut into tiles of kCsTile << shift bytes; a wave
// takes a tile and walks the lines that start in it with sgd::walk_lines
// (sg_linewalk.h), the classes '(' and '=', the limit SG_CALLSET_MAX_LINE.
// Tiles, not programs, are the unit of work, so a 1 MiB program is 4096 waves'
// work and an empty one nobody's.  shift is 0 for offsets that do not decrease;
// the device form's garbage offsets may make programs overlap, and then the
// least shift is taken at which the batch has at most nbytes / kCsTile + nprogs
// tiles, which is what the workspace holds (k_cs_lens adds up the tile counts
// of the 33 shifts, k_cs_ntiles picks; the host forms have checked their
// offsets and skip k_cs_lens).
//
// Output positions come from counting first: k_cs_scan<false> counts each tile's
// call lines and atomicMin's a program's first failure, by text position, into
// perr[program]; scan_counts; k_cs_status gives each program its status and its
// lines; scan_counts again gives line_off; k_cs_scan<true> walks the tiles again
// and writes the spans, 64 lines a store (sgd::LineGroup); k_nt_lookup, a lane
// per line, hashes the name (FNV-1a, 64 bits), probes the dictionary, compares
// the stored hash and then always the bytes.  The text is read twice (plus,
// per line, its first and last byte and the walk past the tile's end).  The
// only atomics are the min on perr and the adds of k_cs_lens; no output cursor.
//
// Every index is checked before it is used as an address, every probe loop is
// bounded by the slot count, and each program's range is clamped to the buffer
// as sg_prog_hashes_dev clamps it.
#include "sg_internal.h"
#include "sg_linewalk.h"

#include <algorithm>
#include <cstring>
#include <vector>

struct sg_nametab {
  sg_ctx* ctx = nullptr;
  // the host's table: names' bytes, offsets, hashes; slots hold ids
  std::vector<uint8_t> bytes;
  std::vector<uint64_t> off{0};
  std::vector<uint64_t> hash;
  std::vector<uint32_t> slots;
  // the device mirror, one allocation: [bytes | off | hash | slots], uploaded after every add
  sg::DevBuf<uint8_t> d_mirror;  // (64 KiB, then doubling)
  size_t o_off = 0, o_hash = 0, o_slots = 0;
};

namespace sg {
namespace {

constexpr uint32_t kCsTileLog = 8;
constexpr uint32_t kCsTile = 1u << kCsTileLog;  // bytes of a tile at shift 0
constexpr uint32_t kCsShifts = 33;              // shifts 0..32: at 32 a tile is longer than any batch
constexpr uint32_t kCsShift = kCsShifts;         // the slot of sums[] behind the totals: the shift taken
constexpr uint32_t kCsBlock = 256;              // four waves, each on tiles of its own
constexpr uint32_t kCsMaxWaves = 1u << 16;
constexpr uint64_t kCsMaxBytes = 1ull << 33;
constexpr unsigned long long kNoErr = ~0ull;
constexpr uint32_t kNoId = SG_NAME_UNKNOWN;

enum : uint32_t { kLnSkip = 0, kLnBracket = 1, kLnEmpty = 2, kLnLong = 3, kLnCall = 8 };

__host__ __device__ __forceinline__ uint64_t fnv1a(const uint8_t* p, uint64_t n) {
  uint64_t h = SG_FNV64_OFFSET;
  for (uint64_t i = 0; i < n; i++) h = (h ^ p[i]) * SG_FNV64_PRIME;
  return h;
}

struct NtView {
  const uint8_t* bytes;
  const uint64_t* off;
  const uint64_t* hash;
  const uint32_t* slots;  // null: no dictionary
  uint32_t mask, n;
  uint64_t nbytes;
};

struct CsArgs {
  const uint8_t* bytes;
  uint64_t nbytes;
  const uint64_t* off;
  uint64_t nprogs;
  const uint64_t* tile_off;  // [nprogs + 1]
  const unsigned long long* sums;  // [kCsShifts] tile totals, then the shift taken
  uint64_t tile_bound;
  uint32_t nwaves;
  uint32_t* cnt;             // [tile_bound] call lines of each tile
  unsigned long long* perr;  // [nprogs] (position in the program << 3) | failure of its first failing line
  // the second walk
  const uint64_t* cpos;  // [tile_bound + 1] cnt's scan
  const uint8_t* status;
  const uint64_t* line_off;
  uint64_t cap;
  uint64_t* name_pos;
  uint32_t* name_len;
};

// sums[k]: the batch's tiles at shift k beyond one per non-empty program.  That is zero for every program of at
// most kCsTile << k bytes, so a wave of short programs adds to a few shifts only (each add is an atomic on one
// address: with all 33 sums added by every wave this kernel took 1.6 ms at 500k programs).  The tiles are at
// most sums[k] + nprogs.
__global__ __launch_bounds__(256) void k_cs_lens(const uint64_t* __restrict__ off, uint64_t nprogs, uint64_t nbytes,
                                                  unsigned long long* __restrict__ sums) {
  const uint64_t p = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  uint64_t len = 0;
  if (p < nprogs) {
    uint64_t a0, a1;
    sgd::csr_range(off, p, nbytes, a0, a1);
    len = a1 - a0;
  }
  uint64_t longest = len;
  for (int d = 32; d; d >>= 1) longest = max(longest, (uint64_t)__shfl_xor((unsigned long long)longest, d));
  const bool lead = (threadIdx.x & 63) == 0;
#pragma unroll 1
  for (uint32_t k = 0; k < kCsShifts && (longest >> (kCsTileLog + k)) != 0; k++) {
    const uint32_t sh = kCsTileLog + k;
    uint32_t v = (uint32_t)((len + ((1ull << sh) - 1)) >> sh);  // (a batch is below 2^33 bytes: 2^25 tiles at most)
    v = v ? v - 1 : 0;
    for (int d = 32; d; d >>= 1) v += (uint32_t)__shfl_xor((int)v, d);
    if (lead && v) atomicAdd(&sums[k], (unsigned long long)v);
  }
}

__device__ __forceinline__ uint32_t pick_shift(const unsigned long long* sums, uint64_t nprogs, uint64_t bound) {
  uint32_t k = 0;
  while (k + 1 < kCsShifts && sums[k] + nprogs > bound) k++;
  return k;
}

__global__ __launch_bounds__(256) void k_cs_ntiles(const uint64_t* __restrict__ off, uint64_t nprogs, uint64_t nbytes,
                                                    unsigned long long* __restrict__ sums, uint64_t bound,
                                                    uint32_t* __restrict__ ntile) {
  const uint64_t p = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  const uint32_t sh = kCsTileLog + pick_shift(sums, nprogs, bound);
  if (p == 0) sums[kCsShift] = sh;  // (read by the later launches)
  if (p >= nprogs) return;
  uint64_t a0, a1;
  sgd::csr_range(off, p, nbytes, a0, a1);
  ntile[p] = (uint32_t)((a1 - a0 + ((1ull << sh) - 1)) >> sh);
}

// What a line [s, e) is (e: its '\n' or the program's end), given the first '(' and the first '=' in it.
// (Reading the line's first and last byte and the blanks from ballots of three more classes instead of from
// memory was tried and was slower: the walk is bound by scalar instructions, not by these loads.)
__device__ __forceinline__ uint32_t cs_classify(const uint8_t* bytes, uint64_t s, uint64_t e, bool have_b, uint64_t b,
                                                bool have_q, uint64_t q, uint64_t& np, uint32_t& nlen) {
  if (e - s >= SG_CALLSET_MAX_LINE) return kLnLong;  // (the scanner fails before it hands the line out)
  if (e > s && bytes[e - 1] == '\r') e--;
  if (e == s || bytes[s] == '#') return kLnSkip;
  if (!have_b) return kLnBracket;
  uint64_t ns = s;
  if (have_q && q < b) {
    ns = q + 1;
    while (ns < b && bytes[ns] == ' ') ns++;
  }
  if (ns == b) return kLnEmpty;
  np = ns;
  nlen = (uint32_t)(b - ns);
  return kLnCall;
}

// what a call line gives: its name's span
struct CsName {
  uint64_t pos;
  uint32_t len;
};

template <bool kEmit>
__global__ __launch_bounds__(kCsBlock) void k_cs_scan(CsArgs a) {
  const uint32_t lane = threadIdx.x & 63;
  const uint64_t wave = (uint64_t)blockIdx.x * (kCsBlock / 64) + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const uint64_t total = min((uint64_t)a.tile_off[a.nprogs], a.tile_bound);
  const uint64_t per = (total + a.nwaves - 1) / a.nwaves;
  uint64_t g = wave * per;
  const uint64_t gend = min(total, g + per);
  if (g >= gend) return;
  if (kEmit && a.line_off[a.nprogs] > a.cap) return;
  const uint32_t sh = (uint32_t)min((unsigned long long)a.sums[kCsShift], (unsigned long long)(kCsTileLog + kCsShifts - 1));
  uint64_t p = sgd::seg_search(a.tile_off, (uint64_t)0, a.nprogs - 1, g);
  for (; g < gend; g++) {
    while (p + 1 < a.nprogs && a.tile_off[p + 1] <= g) p++;
    uint64_t a0, a1;
    sgd::csr_range(a.off, p, a.nbytes, a0, a1);
    const uint64_t t = g - a.tile_off[p];
    const uint64_t tb = a0 + (t << sh);
    if (kEmit && a.status[p] != 0) continue;
    if (tb >= a1 || t > (a.nbytes >> sh)) {  // (never for a tile count made from the same offsets)
      if (!kEmit && lane == 0) a.cnt[g] = 0;
      continue;
    }
    const uint64_t te = min(a1, tb + (1ull << sh));
    // the second walk: where this tile's lines go
    uint64_t obase = 0, oend = 0;
    if (kEmit) {
      obase = a.line_off[p] + (a.cpos[g] - a.cpos[min((uint64_t)a.tile_off[p], a.tile_bound)]);
      oend = min((uint64_t)a.line_off[p + 1], a.cap);
    }
    sgd::LineGroup<CsName> calls;
    auto store = [&](uint32_t i0, const CsName& nm) {
      const uint64_t o = obase + i0 + lane;
      if (o < oend) {
        a.name_pos[o] = nm.pos;
        a.name_len[o] = nm.len;
      }
    };
    sgd::walk_lines<2>(
        a.bytes, a0, a1, tb, te, SG_CALLSET_MAX_LINE, lane,
        [](uint32_t c, uint64_t* m) {
          m[0] = __ballot(c == '(');
          m[1] = __ballot(c == '=');
        },
        [&](uint64_t s, uint64_t e, const bool* have, const uint64_t* first) {
          CsName nm{};
          const uint32_t kind = cs_classify(a.bytes, s, e, have[0], first[0], have[1], first[1], nm.pos, nm.len);
          if (kind == kLnCall) {
            if (kEmit)
              calls.add(lane, nm, store);
            else
              calls.count();
          } else if (!kEmit && kind != kLnSkip && lane == 0) {
            atomicMin(&a.perr[p], (unsigned long long)(((s - a0) << 3) | kind));
          }
        });
    if (kEmit)
      calls.flush(lane, store);
    else if (lane == 0)
      a.cnt[g] = calls.n;
  }
}

__global__ __launch_bounds__(256) void k_cs_status(const uint64_t* __restrict__ tile_off, uint64_t nprogs, uint64_t bound,
                                                    const uint64_t* __restrict__ cpos,
                                                    const unsigned long long* __restrict__ perr,
                                                    uint8_t* __restrict__ status, uint32_t* __restrict__ keep) {
  const uint64_t p = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (p >= nprogs) return;
  const uint64_t t0 = min(tile_off[p], bound), t1 = min(tile_off[p + 1], bound);
  const uint64_t nc = t1 >= t0 ? cpos[t1] - cpos[t0] : 0;
  const unsigned long long e = perr[p];
  const uint32_t st = e != kNoErr ? (uint32_t)(e & 7) : nc == 0 ? SG_CALLSET_NO_CALLS : SG_CALLSET_OK;
  status[p] = (uint8_t)st;
  keep[p] = st == SG_CALLSET_OK ? (uint32_t)min(nc, (uint64_t)0xFFFFFFFFull) : 0u;
}

// name_id of each call line: a lane per line
__global__ __launch_bounds__(256) void k_nt_lookup(NtView t, const uint8_t* __restrict__ text, uint64_t nbytes,
                                                    const uint64_t* __restrict__ nlines, uint64_t cap,
                                                    const uint64_t* __restrict__ name_pos,
                                                    const uint32_t* __restrict__ name_len, uint32_t* __restrict__ name_id) {
  const uint64_t nl = *nlines;
  if (nl > cap) return;
  const uint64_t stride = (uint64_t)gridDim.x * 256;
  for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < nl; i += stride) {
    uint32_t id = kNoId;
    const uint64_t p = name_pos[i];
    const uint64_t len = name_len[i];
    if (t.slots && p <= nbytes && len <= nbytes - p) {
      const uint64_t h = fnv1a(text + p, len);
      uint32_t s = (uint32_t)h & t.mask;
      for (uint32_t probe = 0; probe <= t.mask; probe++, s = (s + 1) & t.mask) {
        const uint32_t c = t.slots[s];
        if (c == kNoId) break;
        if (c >= t.n || t.hash[c] != h) continue;
        const uint64_t o0 = t.off[c], o1 = t.off[c + 1];
        if (o1 < o0 || o1 > t.nbytes || o1 - o0 != len) continue;
        bool eq = true;
        for (uint64_t j = 0; j < len && eq; j++) eq = t.bytes[o0 + j] == text[p + j];
        if (eq) {
          id = c;
          break;
        }
      }
    }
    name_id[i] = id;
  }
}

uint64_t tile_bound(uint64_t nprogs, uint64_t nbytes) { return nbytes / kCsTile + 1 + nprogs; }

struct CsPlan {
  size_t o_sums, o_ntile, o_tile_off, o_cnt, o_cpos, o_perr, o_keep, o_scan, total;
  uint64_t bound;
  CsPlan(size_t base, uint64_t nprogs, uint64_t nbytes) {
    bound = tile_bound(nprogs, nbytes);
    o_sums = base;
    o_ntile = o_sums + align256((kCsShifts + 2) * 8);
    o_tile_off = o_ntile + align256(nprogs * 4);
    o_cnt = o_tile_off + align256((nprogs + 1) * 8);
    o_cpos = o_cnt + align256(bound * 4);
    o_perr = o_cpos + align256((bound + 1) * 8);
    o_keep = o_perr + align256(nprogs * 8);
    o_scan = o_keep + align256(nprogs * 4);
    total = o_scan + scan_ws_bytes(std::max(bound, nprogs));
  }
};

CsArgs cs_args(sg_ctx* ctx, const CsPlan& pl, const uint8_t* d_bytes, const uint64_t* d_off, uint64_t nprogs,
               uint64_t nbytes) {
  CsArgs a{};
  a.bytes = d_bytes;
  a.nbytes = nbytes;
  a.off = d_off;
  a.nprogs = nprogs;
  a.tile_off = (const uint64_t*)ws_at(ctx, pl.o_tile_off);
  a.sums = (const unsigned long long*)ws_at(ctx, pl.o_sums);
  a.tile_bound = pl.bound;
  a.nwaves = (uint32_t)std::min<uint64_t>((pl.bound + 3) & ~3ull, kCsMaxWaves);
  a.cnt = (uint32_t*)ws_at(ctx, pl.o_cnt);
  a.perr = (unsigned long long*)ws_at(ctx, pl.o_perr);
  a.cpos = (const uint64_t*)ws_at(ctx, pl.o_cpos);
  return a;
}

NtView nt_view(const sg_nametab* t) {
  NtView v{};
  if (!t || !t->d_mirror.p || t->hash.empty()) return v;
  const uint8_t* m = t->d_mirror.p;
  v.bytes = m;
  v.off = (const uint64_t*)(m + t->o_off);
  v.hash = (const uint64_t*)(m + t->o_hash);
  v.slots = (const uint32_t*)(m + t->o_slots);
  v.mask = (uint32_t)t->slots.size() - 1;
  v.n = (uint32_t)t->hash.size();
  v.nbytes = t->bytes.size();
  return v;
}

// the id of a name in the host's table, or kNoId
uint32_t nt_find(const sg_nametab* t, const uint8_t* p, uint64_t len, uint64_t h) {
  if (t->slots.empty()) return kNoId;
  const uint32_t mask = (uint32_t)t->slots.size() - 1;
  uint32_t s = (uint32_t)h & mask;
  for (uint32_t probe = 0; probe <= mask; probe++, s = (s + 1) & mask) {
    const uint32_t c = t->slots[s];
    if (c == kNoId) return kNoId;
    if (t->hash[c] != h || t->off[c + 1] - t->off[c] != len) continue;
    if (!memcmp(t->bytes.data() + t->off[c], p, len)) return c;
  }
  return kNoId;
}

void nt_place(sg_nametab* t, uint32_t id) {
  const uint32_t mask = (uint32_t)t->slots.size() - 1;
  uint32_t s = (uint32_t)t->hash[id] & mask;
  while (t->slots[s] != kNoId) s = (s + 1) & mask;  // (at most half the slots are used)
  t->slots[s] = id;
}

int nt_upload(sg_nametab* t) {
  sg_ctx* ctx = t->ctx;
  const size_t nb = align256(t->bytes.size() + 1), no = align256(t->off.size() * 8), nh = align256(t->hash.size() * 8 + 8),
               ns = align256(t->slots.size() * 4 + 4);
  SG_HIP(hipStreamSynchronize(ctx->stream));  // (no lookup in flight reads the old mirror)
  const int rc = t->d_mirror.grow_drop(grow_cap(t->d_mirror.cap, nb + no + nh + ns, 1 << 16), ctx->stream);
  if (rc) return rc;
  uint8_t* m = t->d_mirror.p;
  t->o_off = nb;
  t->o_hash = nb + no;
  t->o_slots = nb + no + nh;
  if (!t->bytes.empty()) SG_HIP(hipMemcpy(m, t->bytes.data(), t->bytes.size(), hipMemcpyHostToDevice));
  SG_HIP(hipMemcpy(m + t->o_off, t->off.data(), t->off.size() * 8, hipMemcpyHostToDevice));
  if (!t->hash.empty())
    SG_HIP(hipMemcpy(m + t->o_hash, t->hash.data(), t->hash.size() * 8, hipMemcpyHostToDevice));
  if (!t->slots.empty())
    SG_HIP(hipMemcpy(m + t->o_slots, t->slots.data(), t->slots.size() * 4, hipMemcpyHostToDevice));
  return SG_OK;
}

}  // namespace

sg_ctx* nametab_ctx(const sg_nametab* tab) { return tab->ctx; }
uint64_t nametab_names(const sg_nametab* tab) { return tab->hash.size(); }

size_t call_sets_ws(uint64_t nprogs, uint64_t nbytes) { return CsPlan(0, nprogs, nbytes).total; }

int call_sets_limits(const char* fn, uint64_t nprogs, uint64_t nbytes) {
  if (nprogs >= (1ull << 32)) {
    set_error("%s: %llu programs (the limit is 2^32 - 1)", fn, (unsigned long long)nprogs);
    return SG_EINVAL;
  }
  if (nbytes >= kCsMaxBytes) {
    set_error("%s: %llu bytes of text (the limit is 2^33 - 1)", fn, (unsigned long long)nbytes);
    return SG_EINVAL;
  }
  return SG_OK;
}

int call_sets_count(sg_ctx* ctx, const uint8_t* d_bytes, const uint64_t* d_off, uint64_t nprogs, uint64_t nbytes,
                    uint8_t* d_status, uint64_t* d_line_off, size_t ws_used, bool offsets_checked) {
  if (nprogs == 0) {
    SG_HIP(hipMemsetAsync(d_line_off, 0, 8, ctx->stream));
    return SG_OK;
  }
  const CsPlan pl(ws_used, nprogs, nbytes);
  const CsArgs a = cs_args(ctx, pl, d_bytes, d_off, nprogs, nbytes);
  unsigned long long* sums = (unsigned long long*)ws_at(ctx, pl.o_sums);
  uint32_t* ntile = (uint32_t*)ws_at(ctx, pl.o_ntile);
  uint64_t* tile_off = (uint64_t*)ws_at(ctx, pl.o_tile_off);
  uint64_t* cpos = (uint64_t*)ws_at(ctx, pl.o_cpos);
  uint32_t* keep = (uint32_t*)ws_at(ctx, pl.o_keep);
  SG_HIP(hipMemsetAsync(sums, 0, (kCsShifts + 2) * 8, ctx->stream));
  SG_HIP(hipMemsetAsync(a.cnt, 0, pl.bound * 4, ctx->stream));
  SG_HIP(hipMemsetAsync(a.perr, 0xFF, nprogs * 8, ctx->stream));
  {
    ScopedTimer tm(ctx, "call_set_tiles");
    // (offsets the host has checked do not decrease: shift 0 fits, which is what all-zero sums say)
    if (!offsets_checked)
      hipLaunchKernelGGL(k_cs_lens, dim3(div_up(nprogs, 256)), dim3(256), 0, ctx->stream, d_off, nprogs, nbytes, sums);
    hipLaunchKernelGGL(k_cs_ntiles, dim3(div_up(nprogs, 256)), dim3(256), 0, ctx->stream, d_off, nprogs, nbytes, sums,
                       pl.bound, ntile);
  }
  SG_HIP(hipGetLastError());
  int rc = scan_counts(ctx, ntile, tile_off, nprogs, pl.o_scan);
  if (rc) return rc;
  {
    ScopedTimer tm(ctx, "call_set_scan");
    hipLaunchKernelGGL(k_cs_scan<false>, dim3(a.nwaves / 4), dim3(kCsBlock), 0, ctx->stream, a);
  }
  SG_HIP(hipGetLastError());
  if ((rc = scan_counts(ctx, a.cnt, cpos, pl.bound, pl.o_scan))) return rc;
  {
    ScopedTimer tm(ctx, "call_set_status");
    hipLaunchKernelGGL(k_cs_status, dim3(div_up(nprogs, 256)), dim3(256), 0, ctx->stream, (const uint64_t*)tile_off,
                       nprogs, pl.bound, (const uint64_t*)cpos, (const unsigned long long*)a.perr, d_status, keep);
  }
  SG_HIP(hipGetLastError());
  return scan_counts(ctx, keep, d_line_off, nprogs, pl.o_scan);
}

int call_sets_emit(sg_ctx* ctx, sg_nametab* tab, const uint8_t* d_bytes, const uint64_t* d_off, uint64_t nprogs,
                   uint64_t nbytes, const uint8_t* d_status, const uint64_t* d_line_off, uint64_t* d_name_pos,
                   uint32_t* d_name_len, uint32_t* d_name_id, uint64_t cap, size_t ws_used) {
  if (nprogs == 0 || cap == 0) return SG_OK;
  const CsPlan pl(ws_used, nprogs, nbytes);
  CsArgs a = cs_args(ctx, pl, d_bytes, d_off, nprogs, nbytes);
  a.status = d_status;
  a.line_off = d_line_off;
  a.cap = cap;
  a.name_pos = d_name_pos;
  a.name_len = d_name_len;
  {
    ScopedTimer tm(ctx, "call_set_emit");
    hipLaunchKernelGGL(k_cs_scan<true>, dim3(a.nwaves / 4), dim3(kCsBlock), 0, ctx->stream, a);
  }
  SG_HIP(hipGetLastError());
  if (d_name_id) {
    ScopedTimer tm(ctx, "name_lookup");
    const uint32_t grid = (uint32_t)std::min<uint64_t>(div_up(cap, 256), 1u << 16);
    hipLaunchKernelGGL(k_nt_lookup, dim3(grid), dim3(256), 0, ctx->stream, nt_view(tab), d_bytes, nbytes,
                       d_line_off + nprogs, cap, (const uint64_t*)d_name_pos, (const uint32_t*)d_name_len, d_name_id);
  }
  SG_HIP(hipGetLastError());
  return SG_OK;
}

}  // namespace sg

using namespace sg;

extern "C" {

int sg_nametab_create(sg_ctx* ctx, sg_nametab** out) {
  if (!ctx || !out) {
    set_error("sg_nametab_create: invalid argument");
    return SG_EINVAL;
  }
  *out = nullptr;
  std::lock_guard<std::mutex> g(ctx->mu);
  int rc = ensure_device(ctx);
  if (rc) return rc;
  sg_nametab* t = new sg_nametab();
  t->ctx = ctx;
  t->slots.assign(64, kNoId);
  if ((rc = nt_upload(t))) {
    delete t;
    return rc;
  }
  *out = t;
  return SG_OK;
}

void sg_nametab_destroy(sg_nametab* t) {
  if (!t) return;
  {
    std::lock_guard<std::mutex> g(t->ctx->mu);
    hipSetDevice(t->ctx->device);
    hipStreamSynchronize(t->ctx->stream);
  }
  delete t;
}

int sg_nametab_count(sg_nametab* t, uint64_t* out) {
  if (!t || !out) {
    set_error("sg_nametab_count: invalid argument");
    return SG_EINVAL;
  }
  std::lock_guard<std::mutex> g(t->ctx->mu);
  *out = t->hash.size();
  return SG_OK;
}

int sg_nametab_add(sg_nametab* t, const uint8_t* bytes, const uint64_t* off, size_t n, uint32_t* ids) {
  const char* fn = "sg_nametab_add";
  if (!t || (n && !ids)) {
    set_error("%s: invalid argument", fn);
    return SG_EINVAL;
  }
  int rc = prog_texts_ok(fn, bytes, off, n);
  if (rc) return rc;
  for (size_t k = 0; k < n; k++)
    if (off[k + 1] == off[k]) {
      set_error("%s: name %llu is empty", fn, (unsigned long long)k);
      return SG_EINVAL;
    }
  sg_ctx* ctx = t->ctx;
  std::lock_guard<std::mutex> g(ctx->mu);
  rc = ensure_device(ctx);
  if (rc) return rc;
  if (t->hash.size() + n >= (1ull << 31)) {
    set_error("%s: the table would reach 2^31 names", fn);
    return SG_EINVAL;
  }
  bool grown = false;
  for (size_t k = 0; k < n; k++) {
    const uint8_t* p = bytes + off[k];
    const uint64_t len = off[k + 1] - off[k], h = fnv1a(p, len);
    uint32_t id = nt_find(t, p, len, h);
    if (id == kNoId) {
      id = (uint32_t)t->hash.size();
      t->bytes.insert(t->bytes.end(), p, p + len);
      t->off.push_back(t->bytes.size());
      t->hash.push_back(h);
      if (2 * t->hash.size() > t->slots.size()) {  // at most half used: twice the slots, every id placed again
        t->slots.assign(t->slots.size() * 2, kNoId);
        for (uint32_t i = 0; i < id; i++) nt_place(t, i);
      }
      nt_place(t, id);
      grown = true;
    }
    ids[k] = id;
  }
  return grown ? nt_upload(t) : SG_OK;
}

static int call_sets_args(const char* fn, sg_ctx* ctx, sg_nametab* tab) {
  if (!ctx) {
    set_error("%s: invalid argument", fn);
    return SG_EINVAL;
  }
  if (tab && tab->ctx != ctx) {
    set_error("%s: the name table belongs to another context", fn);
    return SG_EINVAL;
  }
  return SG_OK;
}

int sg_call_sets_dev(sg_ctx* ctx, sg_nametab* tab, const uint8_t* d_bytes, const uint64_t* d_off, uint64_t nprogs,
                     uint64_t nbytes, uint8_t* d_status, uint64_t* d_line_off, uint64_t* d_name_pos,
                     uint32_t* d_name_len, uint32_t* d_name_id, uint64_t cap) {
  const char* fn = "sg_call_sets_dev";
  int rc = call_sets_args(fn, ctx, tab);
  if (rc) return rc;
  if (!d_line_off || (nprogs && (!d_off || !d_status)) || (nbytes && !d_bytes) || (cap && (!d_name_pos || !d_name_len))) {
    set_error("%s: invalid argument", fn);
    return SG_EINVAL;
  }
  if ((rc = call_sets_limits(fn, nprogs, nbytes))) return rc;
  std::lock_guard<std::mutex> g(ctx->mu);
  rc = ensure_device(ctx);
  if (rc) return rc;
  if ((rc = ws_reserve(ctx, call_sets_ws(nprogs, nbytes)))) return rc;
  if ((rc = call_sets_count(ctx, d_bytes, d_off, nprogs, nbytes, d_status, d_line_off, 0, false))) return rc;
  return call_sets_emit(ctx, tab, d_bytes, d_off, nprogs, nbytes, d_status, d_line_off, d_name_pos, d_name_len,
                        d_name_id, cap, 0);
}

int sg_call_sets(sg_ctx* ctx, sg_nametab* tab, const uint8_t* bytes, const uint64_t* off, size_t nprogs, uint8_t* status,
                 uint64_t* line_off, uint64_t* name_pos, uint32_t* name_len, uint32_t* name_id, size_t cap,
                 size_t* nlines) {
  const char* fn = "sg_call_sets";
  int rc = call_sets_args(fn, ctx, tab);
  if (rc) return rc;
  if (!line_off || !nlines || (nprogs && !status) || (cap && (!name_pos || !name_len))) {
    set_error("%s: invalid argument", fn);
    return SG_EINVAL;
  }
  if ((rc = prog_texts_ok(fn, bytes, off, nprogs))) return rc;
  if ((rc = call_sets_limits(fn, nprogs, off[nprogs]))) return rc;
  std::lock_guard<std::mutex> g(ctx->mu);
  rc = ensure_device(ctx);
  if (rc) return rc;
  line_off[0] = 0;
  *nlines = 0;
  if (nprogs == 0) return SG_OK;
  const uint64_t nbytes = off[nprogs];
  const uint64_t lcap = std::min<uint64_t>(cap, nbytes / 2 + 1);  // (a call line and its '\n' are three bytes or more)
  WsPlan plan;
  const size_t o_bytes = plan.add(nbytes + 4), o_off = plan.add((nprogs + 1) * 8), o_status = plan.add(nprogs),
               o_line = plan.add((nprogs + 1) * 8), o_pos = plan.add(lcap * 8 + 8), o_len = plan.add(lcap * 4 + 4),
               o_id = plan.add(lcap * 4 + 4);
  if ((rc = dstage_reserve(ctx, plan))) return rc;
  if ((rc = ws_reserve(ctx, call_sets_ws(nprogs, nbytes)))) return rc;
  uint8_t* dbytes = dstage_at<uint8_t>(ctx, o_bytes);
  uint64_t* doff = dstage_at<uint64_t>(ctx, o_off);
  uint8_t* dstatus = dstage_at<uint8_t>(ctx, o_status);
  uint64_t* dline = dstage_at<uint64_t>(ctx, o_line);
  uint64_t* dpos = dstage_at<uint64_t>(ctx, o_pos);
  uint32_t* dlen = dstage_at<uint32_t>(ctx, o_len);
  uint32_t* did = dstage_at<uint32_t>(ctx, o_id);
  if ((rc = upload(ctx, dbytes, bytes, nbytes))) return rc;
  if ((rc = upload(ctx, doff, off, (nprogs + 1) * 8))) return rc;
  if ((rc = call_sets_count(ctx, dbytes, doff, nprogs, nbytes, dstatus, dline, 0, true))) return rc;
  if ((rc = call_sets_emit(ctx, tab, dbytes, doff, nprogs, nbytes, dstatus, dline, dpos, dlen, name_id ? did : nullptr,
                           lcap, 0)))
    return rc;
  SG_HIP(hipMemcpyAsync(status, dstatus, nprogs, hipMemcpyDeviceToHost, ctx->stream));
  SG_HIP(hipMemcpyAsync(line_off, dline, (nprogs + 1) * 8, hipMemcpyDeviceToHost, ctx->stream));
  SG_HIP(hipStreamSynchronize(ctx->stream));
  const uint64_t nl = line_off[nprogs];
  *nlines = nl;
  if (nl && nl <= cap) {
    SG_HIP(hipMemcpyAsync(name_pos, dpos, nl * 8, hipMemcpyDeviceToHost, ctx->stream));
    SG_HIP(hipMemcpyAsync(name_len, dlen, nl * 4, hipMemcpyDeviceToHost, ctx->stream));
    if (name_id) SG_HIP(hipMemcpyAsync(name_id, did, nl * 4, hipMemcpyDeviceToHost, ctx->stream));
    SG_HIP(hipStreamSynchronize(ctx->stream));
  }
  return SG_OK;
}

}  // extern "C"
