// sg_cover_ingest.hip -- the text side of the cover report: coveredPCs
// (syz-manager/cover.go:310-347, sorted at :78) over `objdump -d` output,
// symbolizer.ReadSymbols (pkg/symbolizer/nm.go:19-69, flattened and sorted at
// cover.go:262-268) over `nm -nS` output, and symbolize / parse
// (pkg/symbolizer/symbolizer.go:95-191) over `addr2line -afi` output with the
// interning of its names (further down), each the whole text in one call;
// and sg_cover_table_from_text, which hands the parsed frames to the table
// build of sg_cover_lines.hip where they lie, on the device.
//
// The scan is sg_call_set.hip's (now sgd::walk_lines of sg_linewalk.h), over one
// text, in a copy of its own: on the shared walk a2l_lines measured a quarter
// slower (profiles/README.md).  The text is cut into tiles of
// kCiTile bytes; a wave takes a share of consecutive tiles and owns the lines
// that START in each: it walks 64 bytes a step (four steps' loads in flight),
// ballots '\n' and the one byte class its parser is keyed on into 64-bit masks
// and moves from line to line with scalar bit operations on them.  A line that
// leaves the tile is walked to its end by its owner (the next tile's wave skips
// it: it starts at the first '\n' at or after its tile's last-but-one byte), so
// nothing is carried between waves.  A walk stops SG_INGEST_MAX_LINE bytes into
// a line: that line is too long whatever follows.
//
// objdump: the class is "the call needle starts here" -- the ballot of the
// needle's first byte, its few candidates verified against the text by their
// own lanes -- so the common line, which has no call in it, ends on the masks
// alone.  A line with a call match is parsed by the whole wave: the trace
// needle searched in ln[pos:] 64 places a step, the first ':' likewise, the hex
// field's digits a lane each.  nm: the class is ' ', the first blank of the
// line; the second blank, the type letter and the two hex fields are read per
// line in the same way.  Needles and fields are always read from the text at
// their own positions, never from a step's registers, so a step or tile
// boundary inside one changes nothing.
//
// Output positions come from counting first: k_ci_scan<.., false> counts each
// tile's kept lines and atomicMin's the first too-long line's start into perr;
// scan_counts; the host reads {total, perr} (the one wait: the total sizes the
// sort); k_ci_scan<.., true> walks the tiles again and writes, 64 lines a
// store.  The text is read twice (plus, per kept line, the bytes of its parse
// and the walk past the tile's end).  The only atomic is the min on perr; no
// output cursor.  The PCs are then sorted (sg_sort.hip); the symbols are ranked
// by start (sg_rank.h) and sorted as rank << 32 | text index, which is the
// pinned (start, text order).
//
// Every index is checked before it is used as an address and every loop is
// bounded: a step loop by the tile's end or the line limit, a per-line loop by
// the line's length (below SG_INGEST_MAX_LINE).
#include "sg_internal.h"
#include "sg_cover_lines.h"
#include "sg_rank.h"

#include <algorithm>
#include <cstring>
#include <vector>

namespace sg {
namespace {

constexpr uint32_t kCiTileLog = 10;
constexpr uint32_t kCiTile = 1u << kCiTileLog;  // bytes of a tile
constexpr uint32_t kCiBlock = 256;              // four waves, each on tiles of its own
constexpr uint32_t kCiMaxWaves = 1u << 13;       // (every CU's 32 waves: more only queue)
constexpr uint64_t kCiMaxBytes = 1ull << 33;
constexpr unsigned long long kNoErr = ~0ull;

enum : int { kObjdump = 0, kNm = 1, kLines = 2 };  // (kLines: every line's start, for addr2line)

struct CiNeedle {
  uint8_t b[SG_INGEST_MAX_NEEDLE];
  uint32_t len;
};

struct CiArgs {
  const uint8_t* text;
  uint64_t nbytes;
  uint64_t ntiles;
  uint32_t nwaves;
  CiNeedle call, func;       // objdump
  uint32_t* cnt;             // [ntiles] kept lines of each tile
  unsigned long long* perr;  // the start of the first too-long line
  // the second walk
  const uint64_t* cpos;  // [ntiles + 1] cnt's scan
  uint64_t cap;
  uint64_t* o_val;  // objdump: the PCs; nm: addr
  int64_t* o_size;
  uint64_t* o_npos;
  uint32_t* o_nlen;
};

// what a kept line gives
struct CiLine {
  uint64_t val;
  int64_t size;
  uint64_t npos;
  uint32_t nlen;
};

__device__ __forceinline__ uint64_t wave_or(uint64_t v) {
  for (int d = 32; d; d >>= 1) v |= (uint64_t)__shfl_xor((unsigned long long)v, d);
  return v;
}

// does the needle stand at p, inside [p, to)?  (a lane's own question)
__device__ __forceinline__ bool needle_at(const uint8_t* text, const CiNeedle& n, uint64_t p, uint64_t to) {
  if (p > to || to - p < n.len) return false;
  for (uint32_t k = 0; k < n.len && k < SG_INGEST_MAX_NEEDLE; k++)
    if (text[p + k] != n.b[k]) return false;
  return true;
}

// The whole wave: is the needle anywhere in [from, to)?  64 places a step.
__device__ __forceinline__ bool wave_has_needle(const uint8_t* text, const CiNeedle& n, uint64_t from, uint64_t to,
                                                uint32_t lane) {
  for (uint64_t p0 = from; p0 < to && to - p0 >= n.len; p0 += 64)
    if (__ballot(needle_at(text, n, p0 + lane, to))) return true;
  return false;
}

// The whole wave: the first byte c in [from, to), or `to`.
__device__ __forceinline__ uint64_t wave_find_byte(const uint8_t* text, uint32_t c, uint64_t from, uint64_t to,
                                                   uint32_t lane) {
  for (uint64_t p0 = from; p0 < to; p0 += 64) {
    const uint64_t p = p0 + lane;
    const uint64_t m = __ballot(p < to && text[p] == c);
    if (m) return p0 + (uint32_t)__builtin_ctzll(m);
  }
  return to;
}

// The whole wave: strconv.ParseUint(text[a:b], 16, 64).  The last 16 bytes are
// the value's digits, a lane each; every byte before them must be '0'.
__device__ __forceinline__ bool wave_parse_hex(const uint8_t* text, uint64_t a, uint64_t b, uint32_t lane, uint64_t& out) {
  if (b <= a) return false;
  const uint64_t n = b - a;
  uint64_t v = 0;
  bool bad = false;
  for (uint64_t o = 0; o < n; o += 64) {
    const uint64_t i = o + lane;
    if (i >= n) continue;
    const uint32_t c = text[a + i];
    const uint32_t d = c - '0' < 10u ? c - '0' : (c | 0x20u) - 'a' < 6u ? (c | 0x20u) - 'a' + 10 : 255u;
    const uint64_t r = n - 1 - i;  // the digit's place from the end
    if (d == 255u || (r >= 16 && d != 0))
      bad = true;
    else if (r < 16)
      v |= (uint64_t)d << (4 * r);
  }
  if (__ballot(bad)) return false;
  out = wave_or(v);
  return true;
}

// A line [s, e) (e: past its content, the '\r' dropped) whose first position of the kernel's class is f.
template <int kKind>
__device__ __forceinline__ bool ci_parse(const CiArgs& a, uint64_t s, uint64_t e, uint64_t f, uint32_t lane, CiLine& out) {
  const uint8_t* t = a.text;
  if (kKind == kObjdump) {
    // f: the first place the call needle stands at.  A match that runs past e (a needle that ends in the
    // dropped '\r') is no match, and then no later one fits either.
    if (f > e || e - f < a.call.len) return false;
    if (!wave_has_needle(t, a.func, f, e, lane)) return false;
    const uint64_t colon = wave_find_byte(t, ':', s, e, lane);
    if (colon == e) return false;
    return wave_parse_hex(t, s, colon, lane, out.val);
  }
  // f: the first blank
  if (f >= e) return false;
  const uint64_t sp2 = wave_find_byte(t, ' ', f + 1, e, lane);
  if (e - sp2 < 3) return false;  // (also sp2 == e: no second blank)
  if ((t[sp2 + 1] != 't' && t[sp2 + 1] != 'T') || t[sp2 + 2] != ' ') return false;
  uint64_t size = 0;
  if (!wave_parse_hex(t, s, f, lane, out.val) || !wave_parse_hex(t, f + 1, sp2, lane, size)) return false;
  out.size = (int64_t)(size + 15) / 16 * 16;
  out.npos = sp2 + 3;
  out.nlen = (uint32_t)(e - (sp2 + 3));  // (a line's content is below SG_INGEST_MAX_LINE)
  return true;
}

template <int kKind, bool kEmit>
__global__ __launch_bounds__(kCiBlock) void k_ci_scan(CiArgs a) {
  const uint32_t lane = threadIdx.x & 63;
  const uint64_t wave = (uint64_t)blockIdx.x * (kCiBlock / 64) + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const uint64_t per = (a.ntiles + a.nwaves - 1) / a.nwaves;
  uint64_t g = wave * per;
  const uint64_t gend = min(a.ntiles, g + per);
  const uint64_t n = a.nbytes;
  const uint32_t key = kKind == kObjdump ? a.call.b[0] : kKind == kNm ? ' ' : 0x200u;  // (kLines: no class)
  for (; g < gend; g++) {
    const uint64_t tb = g << kCiTileLog;
    if (tb >= n) {  // (never for a tile count made from nbytes)
      if (!kEmit && lane == 0) a.cnt[g] = 0;
      continue;
    }
    const uint64_t te = min(n, tb + kCiTile);
    // the lines that start in [tb, te): at 0, or behind a '\n' at tb - 1 .. te - 2
    bool in_line = g == 0, have_f = false, done = false;
    uint64_t s = 0, f = 0;
    uint64_t cb = g == 0 ? 0 : tb - 1;
    uint32_t nkeep = 0;
    // the second walk: where this tile's lines go, and up to 64 of them held a lane each
    const uint64_t obase = kEmit ? a.cpos[g] : 0;
    CiLine mine{};
    auto store = [&](uint64_t o) {
      if (o >= a.cap) return;
      a.o_val[o] = mine.val;
      if (kKind == kNm) {
        a.o_size[o] = mine.size;
        a.o_npos[o] = mine.npos;
        a.o_nlen[o] = mine.nlen;
      }
    };
    auto line_end = [&](uint64_t e) {
      in_line = false;
      CiLine ln{};
      if (kKind == kLines) {
        ln.val = s;  // (the too-long ones too: addr2line's reader fails only on a line it reaches)
      } else {
        if (e - s >= SG_INGEST_MAX_LINE) {  // (the scanner fails before it hands the line out)
          if (!kEmit && lane == 0) atomicMin(a.perr, (unsigned long long)s);
          return;
        }
        if (!have_f) return;
        if (e > s && a.text[e - 1] == '\r') e--;
        if (!ci_parse<kKind>(a, s, e, f, lane, ln)) return;
      }
      if (kEmit) {
        if (lane == (nkeep & 63)) mine = ln;
        if ((nkeep & 63) == 63) store(obase + (nkeep - 63) + lane);  // 64 lines held: one store
      }
      nkeep++;
    };
    while (!done) {
      uint32_t c[4];
#pragma unroll
      for (uint32_t k = 0; k < 4; k++) {
        const uint64_t pos = cb + 64 * k + lane;
        c[k] = pos < n ? a.text[pos] : 0x100u;  // (no byte)
      }
#pragma unroll
      for (uint32_t k = 0; k < 4; k++) {
        if (done) break;
        const uint64_t base = cb + 64 * k;
        if (base >= n) {  // (an open line always ends in the step that holds the text's end)
          if (in_line) line_end(n);
          done = true;
          break;
        }
        const uint64_t nl = __ballot(c[k] == '\n');
        bool hit = c[k] == key;
        if (kKind == kObjdump && hit) hit = needle_at(a.text, a.call, base + lane, n);
        const uint64_t fm = __ballot(hit);
        uint32_t bit = 0;
        while (true) {
          if (!in_line) {  // the next '\n' that a line of this tile starts behind
            if (bit >= 64) break;
            const uint64_t m = nl & (~0ull << bit);
            if (!m) break;
            const uint32_t i = (uint32_t)__builtin_ctzll(m);
            if (base + i + 1 >= te) {
              done = true;
              break;
            }
            s = base + i + 1;
            in_line = true;
            have_f = false;
            bit = i + 1;
          }
          if (bit >= 64) break;
          const uint64_t from = ~0ull << bit, nlm = nl & from;
          const uint32_t endi = nlm ? (uint32_t)__builtin_ctzll(nlm) : 64u;
          const uint64_t reg = endi < 64 ? from & ((1ull << endi) - 1) : from;
          if (!have_f && (fm & reg)) {
            f = base + (uint32_t)__builtin_ctzll(fm & reg);
            have_f = true;
          }
          if (endi < 64) {
            line_end(base + endi);
            bit = endi;  // (that '\n' may start the next line)
            continue;
          }
          if (base + 64 >= n) {
            line_end(n);
            done = true;
          } else if (base + 64 - s >= SG_INGEST_MAX_LINE) {
            line_end(base + 64);  // too long already, wherever it ends
          }
          break;
        }
        if (!in_line && base + 65 >= te) done = true;
      }
      cb += 256;
    }
    if (kEmit) {
      const uint32_t held = nkeep & 63;
      if (lane < held) store(obase + (nkeep - held) + lane);
    } else if (lane == 0) {
      a.cnt[g] = nkeep;
    }
  }
}

// keys[i] = rank[i] << 32 | i
__global__ void k_ci_pack(const uint32_t* __restrict__ rank, uint64_t n, uint64_t* __restrict__ keys) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) keys[i] = ((uint64_t)rank[i] << 32) | i;
}
// sorted place j holds text-order symbol (u32)keys[j]
__global__ void k_ci_gather(const uint64_t* __restrict__ keys, uint64_t n, const uint64_t* __restrict__ addr,
                            const int64_t* __restrict__ size, uint64_t* __restrict__ start, uint64_t* __restrict__ end,
                            uint32_t* __restrict__ order) {
  const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n) return;
  const uint64_t i = min(keys[j] & 0xFFFFFFFFull, n - 1);
  start[j] = addr[i];
  end[j] = addr[i] + (uint64_t)size[i];
  order[j] = (uint32_t)i;
}

uint64_t ci_tiles(uint64_t nbytes) { return (nbytes + kCiTile - 1) >> kCiTileLog; }

// The count pass's regions, the same at the front of every plan of a call.
struct CiPlan {
  WsPlan p;
  size_t o_cnt, o_cpos, o_perr, o_scan;
  uint64_t ntiles;
  explicit CiPlan(uint64_t nbytes) {
    ntiles = ci_tiles(nbytes);
    o_cnt = p.add(ntiles * 4 + 4);
    o_cpos = p.add((ntiles + 1) * 8);
    o_perr = p.add(8);
    o_scan = p.add(scan_ws_bytes(std::max<uint64_t>(ntiles, 1)));
  }
};

CiArgs ci_args(sg_ctx* ctx, const CiPlan& pl, const uint8_t* d_text, uint64_t nbytes) {
  CiArgs a{};
  a.text = d_text;
  a.nbytes = nbytes;
  a.ntiles = pl.ntiles;
  a.nwaves = (uint32_t)std::min<uint64_t>((pl.ntiles + 3) & ~3ull, kCiMaxWaves);
  a.cnt = (uint32_t*)ws_at(ctx, pl.o_cnt);
  a.perr = (unsigned long long*)ws_at(ctx, pl.o_perr);
  a.cpos = (const uint64_t*)ws_at(ctx, pl.o_cpos);
  return a;
}

template <int kKind, bool kEmit>
int ci_launch(sg_ctx* ctx, const CiArgs& a, const char* name) {
  ScopedTimer tm(ctx, name);
  hipLaunchKernelGGL((k_ci_scan<kKind, kEmit>), dim3(a.nwaves / 4), dim3(kCiBlock), 0, ctx->stream, a);
  SG_HIP(hipGetLastError());
  return SG_OK;
}

// The count pass and its one wait: *total kept lines, *err the first too-long line's start or kNoErr.
template <int kKind>
int ci_count(sg_ctx* ctx, const CiPlan& pl, const CiArgs& a, uint64_t* total, unsigned long long* err) {
  SG_HIP(hipMemsetAsync(a.perr, 0xFF, 8, ctx->stream));
  int rc = ci_launch<kKind, false>(ctx, a, kKind == kObjdump ? "objdump_scan" : kKind == kNm ? "nm_scan" : "a2l_lines");
  if (rc) return rc;
  if ((rc = scan_counts(ctx, a.cnt, (uint64_t*)ws_at(ctx, pl.o_cpos), pl.ntiles, pl.o_scan))) return rc;
  SG_HIP(hipMemcpyAsync(total, a.cpos + pl.ntiles, 8, hipMemcpyDeviceToHost, ctx->stream));
  SG_HIP(hipMemcpyAsync(err, a.perr, 8, hipMemcpyDeviceToHost, ctx->stream));
  SG_HIP(hipStreamSynchronize(ctx->stream));
  return SG_OK;
}

int ci_text_ok(const char* fn, uint64_t nbytes) {
  if (nbytes >= kCiMaxBytes) {
    set_error("%s: %llu bytes of text (the limit is 2^33 - 1)", fn, (unsigned long long)nbytes);
    return SG_EINVAL;
  }
  return SG_OK;
}

int ci_needle(const char* fn, const char* what, const uint8_t* p, size_t len, CiNeedle* out) {
  if (!p || len < 1 || len > SG_INGEST_MAX_NEEDLE) {
    set_error("%s: the %s needle must be 1..%d bytes", fn, what, SG_INGEST_MAX_NEEDLE);
    return SG_EINVAL;
  }
  memset(out, 0, sizeof(*out));
  memcpy(out->b, p, len);
  out->len = (uint32_t)len;
  return SG_OK;
}

// {count, status, err_pos} of a call
struct CiInfo {
  uint64_t count = 0, status = SG_INGEST_OK, err_pos = 0;
};

// device -> where the caller wants it: device memory (dev) or host memory, on ctx->stream
int ci_out(sg_ctx* ctx, void* dst, const void* src, size_t bytes, bool dev) {
  if (dst && bytes)
    SG_HIP(hipMemcpyAsync(dst, src, bytes, dev ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, ctx->stream));
  return SG_OK;
}

// sg_objdump_pcs*'s body (ctx lock held, the device ensured): the sorted PCs to `pcs` when they fit cap.
int objdump_pcs(sg_ctx* ctx, const uint8_t* d_text, uint64_t nbytes, const CiNeedle& call, const CiNeedle& func,
                uint64_t* pcs, uint64_t cap, bool dev, CiInfo* info) {
  *info = CiInfo();
  if (nbytes == 0) return SG_OK;
  const CiPlan pl(nbytes);
  int rc = ws_reserve(ctx, pl.p);
  if (rc) return rc;
  CiArgs a = ci_args(ctx, pl, d_text, nbytes);
  a.call = call;
  a.func = func;
  uint64_t total = 0;
  unsigned long long err = kNoErr;
  if ((rc = ci_count<kObjdump>(ctx, pl, a, &total, &err))) return rc;
  if (err != kNoErr) {
    info->status = SG_INGEST_TOO_LONG;
    info->err_pos = err;
    return SG_OK;
  }
  info->count = total;
  if (total == 0 || total > cap) return SG_OK;
  WsPlan p = pl.p;
  const size_t o_a = p.add(total * 8), o_b = p.add(total * 8), o_sort = p.add(radix_sort_ws(total));
  // (growing drops the tile positions: count again, into the workspace that has room for the rest)
  rc = ws_reserve_redo(ctx, p.total, [&] {
    a = ci_args(ctx, pl, d_text, nbytes);
    a.call = call;
    a.func = func;
    uint64_t again = 0;
    const int r = ci_count<kObjdump>(ctx, pl, a, &again, &err);
    return r ? r : again == total ? SG_OK : SG_EHIP;
  });
  if (rc) return rc;
  a.cap = total;
  a.o_val = (uint64_t*)ws_at(ctx, o_a);
  if ((rc = ci_launch<kObjdump, true>(ctx, a, "objdump_emit"))) return rc;
  uint64_t* sorted = nullptr;
  {
    ScopedTimer tm(ctx, "objdump_sort");
    if ((rc = radix_sort_u64(ctx, a.o_val, (uint64_t*)ws_at(ctx, o_b), total, o_sort, &sorted, 0))) return rc;
  }
  return ci_out(ctx, pcs, sorted, total * 8, dev);
}

struct NmOut {
  uint64_t* addr;
  int64_t* size;
  uint64_t* name_pos;
  uint32_t* name_len;
  uint64_t* sym_start;
  uint64_t* sym_end;
  uint32_t* order;
};

// sg_nm_symbols*'s body, likewise
int nm_symbols(sg_ctx* ctx, const char* fn, const uint8_t* d_text, uint64_t nbytes, const NmOut& out, uint64_t cap,
               bool dev, CiInfo* info) {
  *info = CiInfo();
  if (nbytes == 0) return SG_OK;
  const CiPlan pl(nbytes);
  int rc = ws_reserve(ctx, pl.p);
  if (rc) return rc;
  CiArgs a = ci_args(ctx, pl, d_text, nbytes);
  uint64_t total = 0;
  unsigned long long err = kNoErr;
  if ((rc = ci_count<kNm>(ctx, pl, a, &total, &err))) return rc;
  if (err != kNoErr) {
    info->status = SG_INGEST_TOO_LONG;
    info->err_pos = err;
    return SG_OK;
  }
  if (total >= 0xFFFFFFFFull) {
    set_error("%s: %llu symbols (the limit is 2^32 - 2)", fn, (unsigned long long)total);
    return SG_EINVAL;
  }
  info->count = total;
  if (total == 0 || total > cap) return SG_OK;
  WsPlan p = pl.p;
  const size_t o_size = p.add(total * 8), o_npos = p.add(total * 8), o_nlen = p.add(total * 4), o_u = p.add(total * 8),
               o_rank = p.add(total * 4), o_start = p.add(total * 8), o_end = p.add(total * 8),
               o_order = p.add(total * 4);
  const size_t rank_at = p.total;
  const size_t need = rank_at + rank_ws_bytes(total);
  rc = ws_reserve_redo(ctx, need, [&] {
    a = ci_args(ctx, pl, d_text, nbytes);
    uint64_t again = 0;
    const int r = ci_count<kNm>(ctx, pl, a, &again, &err);
    return r ? r : again == total ? SG_OK : SG_EHIP;
  });
  if (rc) return rc;
  const RankWs g = rank_ws(ctx, p, total);  // (g.v: the symbols' addr, in text order)
  a.cap = total;
  a.o_val = g.v;
  a.o_size = (int64_t*)ws_at(ctx, o_size);
  a.o_npos = (uint64_t*)ws_at(ctx, o_npos);
  a.o_nlen = (uint32_t*)ws_at(ctx, o_nlen);
  if ((rc = ci_launch<kNm, true>(ctx, a, "nm_emit"))) return rc;
  SG_HIP(hipMemcpyAsync(g.ka, g.v, total * 8, hipMemcpyDeviceToDevice, ctx->stream));
  uint32_t* rank = (uint32_t*)ws_at(ctx, o_rank);
  uint64_t* start = (uint64_t*)ws_at(ctx, o_start);
  uint64_t* end = (uint64_t*)ws_at(ctx, o_end);
  uint32_t* order = (uint32_t*)ws_at(ctx, o_order);
  {
    ScopedTimer tm(ctx, "nm_order");
    if ((rc = rank_values(ctx, g, ~0ull, (uint64_t*)ws_at(ctx, o_u), rank))) return rc;
    hipLaunchKernelGGL(k_ci_pack, dim3(div_up(total, 256)), dim3(256), 0, ctx->stream, (const uint32_t*)rank, total, g.ka);
    uint64_t* sorted = nullptr;
    const uint64_t vary = bits_below(total) << 32;
    if ((rc = radix_sort_u64(ctx, g.ka, g.kb, total, g.tail, &sorted, vary ? vary : 1))) return rc;
    hipLaunchKernelGGL(k_ci_gather, dim3(div_up(total, 256)), dim3(256), 0, ctx->stream, (const uint64_t*)sorted, total,
                       (const uint64_t*)g.v, (const int64_t*)a.o_size, start, end, order);
    SG_HIP(hipGetLastError());
  }
  if ((rc = ci_out(ctx, out.addr, g.v, total * 8, dev))) return rc;
  if ((rc = ci_out(ctx, out.size, a.o_size, total * 8, dev))) return rc;
  if ((rc = ci_out(ctx, out.name_pos, a.o_npos, total * 8, dev))) return rc;
  if ((rc = ci_out(ctx, out.name_len, a.o_nlen, total * 4, dev))) return rc;
  if ((rc = ci_out(ctx, out.sym_start, start, total * 8, dev))) return rc;
  if ((rc = ci_out(ctx, out.sym_end, end, total * 8, dev))) return rc;
  return ci_out(ctx, out.order, order, total * 4, dev);
}

int ci_info_dev(sg_ctx* ctx, uint64_t* d_info, const CiInfo& info) {
  const uint64_t w[3] = {info.count, info.status, info.err_pos};
  SG_HIP(hipMemcpyAsync(d_info, w, sizeof(w), hipMemcpyHostToDevice, ctx->stream));
  SG_HIP(hipStreamSynchronize(ctx->stream));  // (w leaves scope)
  return SG_OK;
}

// the host forms' text, in the device staging buffer
int ci_stage_text(sg_ctx* ctx, const uint8_t* text, uint64_t nbytes, const uint8_t** d_text) {
  *d_text = nullptr;
  if (nbytes == 0) return SG_OK;
  WsPlan plan;
  const size_t o_text = plan.add(nbytes + 4);
  int rc = dstage_reserve(ctx, plan);
  if (rc) return rc;
  uint8_t* d = dstage_at<uint8_t>(ctx, o_text);
  if ((rc = upload(ctx, d, text, nbytes))) return rc;
  *d_text = d;
  return SG_OK;
}

// ---- addr2line: symbolize + parse (pkg/symbolizer/symbolizer.go:95-191) ------------------------------------
// k_ci_scan<kLines> gives every line's start (count, scan, write, as above).  From there a thread owns a line:
// k_al_class notes its shape and last ':' and flags the record starts (line 0; a "0x" line without ':'), a scan of
// the flags gives each line its record, k_al_rline each record its first line, and k_al_term where the last record
// ends early.  k_al_check then knows a line's place in its record: place 0 is the PC line, odd places are function
// lines, even ones file lines, and what does not fit is a failure, the first by position winning (the one atomic:
// the min on perr).  A function line's thread owns the frame of its pair; kept frames are counted, scanned, written.
// The names of a column (File or Func) are interned by k_in_*: hash, rank the hashes, sort rank << 32 | frame so
// that a hash's frames stand together in frame order, compare every frame with its hash's first BY BYTES, and when
// all agree number the firsts in frame order.  When any differs the column is hashed again under another seed,
// unmasked: a name's id never depends on a hash being unique.
enum : uint32_t { kAlLong = 1, kAlShaped = 2, kAlStart = 4 };
constexpr uint32_t kAlNoColon = 0xFFFFFFFFu;
constexpr uint32_t kInternRounds = 4;

struct AlArgs {
  const uint8_t* text;
  uint64_t nbytes, nlines, nrec;
  const uint64_t* lstart;  // [nlines]
  uint8_t* cls;            // [nlines]
  uint32_t* lcolon;        // [nlines] the last ':' of a line, from its start
  uint32_t* sflag;         // [nlines] the line starts a record
  const uint64_t* spos;    // [nlines + 1] sflag's scan
  uint32_t* rline;         // [nlines + 1] a record's first line; rline[records] = nlines
  uint32_t* term;          // the line the last record ends before
  unsigned long long* perr;  // (position << 3) | status of the first failure
  uint64_t* rec_pc;        // [min(nrec, nlines)]
  uint32_t* keep;          // [nlines] the frame of this function line is kept
  const uint64_t* fpos;    // [nlines + 1] keep's scan
  uint64_t cap;
  uint64_t *fn_pos, *fl_pos;  // [cap] the kept frames' names
  uint32_t *fn_len, *fl_len;
  int64_t* line;
};

// line i: content [s, e), the '\r' dropped unless the line is too long
__device__ __forceinline__ void al_line(const AlArgs& a, uint64_t i, uint64_t& s, uint64_t& e, bool& lng) {
  const uint64_t n = a.nbytes;
  s = min(a.lstart[i], n);
  if (i + 1 < a.nlines)
    e = min(max(a.lstart[i + 1], s + 1), n) - 1;  // its '\n'
  else
    e = (n > s && a.text[n - 1] == '\n') ? n - 1 : n;
  lng = e - s >= SG_INGEST_MAX_LINE;
  if (!lng && e > s && a.text[e - 1] == '\r') e--;
}

__device__ __forceinline__ uint32_t al_lower(uint32_t c) { return c | 0x20u; }

// strconv.underscoreOK
__device__ bool al_underscore_ok(const uint8_t* t, uint64_t q, uint64_t e) {
  uint32_t last = '^';
  if (q < e && (t[q] == '-' || t[q] == '+')) q++;
  bool hex = false;
  if (e - q >= 2 && t[q] == '0' && (al_lower(t[q + 1]) == 'b' || al_lower(t[q + 1]) == 'o' || al_lower(t[q + 1]) == 'x')) {
    last = '0';
    hex = al_lower(t[q + 1]) == 'x';
    q += 2;
  }
  for (; q < e; q++) {
    const uint32_t c = t[q];
    if (c - '0' < 10u || (hex && al_lower(c) - 'a' < 6u)) {
      last = '0';
    } else if (c == '_') {
      if (last != '0') return false;
      last = '_';
    } else {
      if (last == '_') return false;
      last = '!';
    }
  }
  return last != '_';
}

// strconv.ParseUint(text[s:e], 0, 64)
__device__ bool al_parse_pc(const uint8_t* t, uint64_t s, uint64_t e, uint64_t& out) {
  if (e <= s) return false;
  uint64_t p = s;
  uint32_t base = 10;
  if (t[s] == '0') {
    const uint32_t c1 = e - s >= 3 ? al_lower(t[s + 1]) : 0;
    if (c1 == 'b' || c1 == 'o' || c1 == 'x') {
      base = c1 == 'b' ? 2 : c1 == 'o' ? 8 : 16;
      p = s + 2;
    } else {
      base = 8;
      p = s + 1;
    }
  }
  const uint64_t cutoff = ~0ull / base + 1;
  uint64_t v = 0;
  bool us = false;
  for (; p < e; p++) {
    const uint32_t c = t[p];
    uint32_t d;
    if (c == '_') {
      us = true;
      continue;
    } else if (c - '0' < 10u) {
      d = c - '0';
    } else if (al_lower(c) - 'a' < 26u) {
      d = al_lower(c) - 'a' + 10;
    } else {
      return false;
    }
    if (d >= base || v >= cutoff) return false;
    v *= base;
    if (v + d < v) return false;
    v += d;
  }
  if (us && !al_underscore_ok(t, s, e)) return false;
  out = v;
  return true;
}

__device__ __forceinline__ bool al_is_qq(const uint8_t* t, uint64_t s, uint64_t e) {
  return e == s || (e - s == 2 && t[s] == '?' && t[s + 1] == '?');
}

// the frame of function line [s1, e1) and file line [s2, e2) with its last ':' at colon: kept?
__device__ bool al_frame(const uint8_t* t, uint64_t s1, uint64_t e1, uint64_t s2, uint64_t colon, uint64_t e2,
                         int64_t& line) {
  uint64_t p = colon + 1;
  while (p < e2 && t[p] == '0') p++;  // (leading zeros: Atoi goes by value)
  const bool any = p > colon + 1;
  uint64_t v = 0;
  uint32_t sig = 0;
  for (; p < e2 && t[p] - '0' < 10u; p++, sig++)
    if (sig < 19) v = v * 10 + (t[p] - '0');
  if ((!any && sig == 0) || sig > 19 || v > 0x7FFFFFFFFFFFFFFFull || v == 0) return false;
  if (al_is_qq(t, s1, e1) || al_is_qq(t, s2, colon)) return false;
  line = (int64_t)v;
  return true;
}

__global__ __launch_bounds__(256) void k_al_class(AlArgs a) {
  const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= a.nlines) return;
  uint64_t s, e;
  bool lng;
  al_line(a, i, s, e, lng);
  uint32_t c = lng ? kAlLong : 0, colon = kAlNoColon;
  if (!lng) {
    if (e - s > 3 && a.text[s] == '0' && a.text[s + 1] == 'x') c |= kAlShaped;
    for (uint64_t p = e; p > s; p--)
      if (a.text[p - 1] == ':') {
        colon = (uint32_t)(p - 1 - s);
        break;
      }
  }
  const bool start = i == 0 || ((c & kAlShaped) && colon == kAlNoColon);
  a.cls[i] = (uint8_t)(c | (start ? kAlStart : 0));
  a.lcolon[i] = colon;
  a.sflag[i] = start;
}

__global__ __launch_bounds__(256) void k_al_rline(AlArgs a) {
  const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= a.nlines) return;
  if (a.sflag[i]) a.rline[min(a.spos[i], a.nlines)] = (uint32_t)i;
  if (i == 0) a.rline[min(a.spos[a.nlines], a.nlines)] = (uint32_t)a.nlines;
}

// One workgroup: the last record parsed, nrec - 1, also ends before the first "0x" line (it has a ':', or it would
// start a record) at a function place, where the reference leaves parse() for the last time.
__global__ __launch_bounds__(256) void k_al_term(AlArgs a) {
  __shared__ uint32_t best;
  if (threadIdx.x == 0) best = (uint32_t)a.nlines;
  __syncthreads();
  const uint64_t nr = min(a.spos[a.nlines], a.nlines);
  if (a.nrec >= 1 && a.nrec <= nr) {
    const uint64_t b = a.rline[a.nrec - 1], end = min((uint64_t)a.rline[a.nrec], a.nlines);
    uint32_t mine = (uint32_t)end;
    for (uint64_t i = b + 1 + 2 * (uint64_t)threadIdx.x; i < end; i += 512)
      if (a.cls[i] & kAlShaped) {
        mine = (uint32_t)i;
        break;
      }
    atomicMin(&best, mine);  // (LDS)
  }
  __syncthreads();
  if (threadIdx.x == 0) *a.term = best;
}

template <bool kEmit>
__global__ __launch_bounds__(256) void k_al_check(AlArgs a) {
  const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= a.nlines) return;
  const uint64_t L = a.nlines, nr = min(a.spos[L], L);
  auto fail = [&](uint32_t status, uint64_t pos) {
    if (!kEmit) atomicMin(a.perr, (unsigned long long)((pos << 3) | status));
  };
  if (i == 0 && nr < a.nrec) fail(SG_A2L_TOO_FEW, a.nbytes);
  uint64_t s, e;
  bool lng;
  al_line(a, i, s, e, lng);
  if (a.nrec == 0) {  // (the reference reads one line before it looks at len(pcs))
    if (i == 0 && lng) fail(SG_A2L_TOO_LONG, s);
    return;
  }
  const uint64_t sp = a.spos[i + 1];
  const uint64_t r = (sp ? min(sp, L) : 1) - 1;  // (line 0 starts record 0: sp >= 1)
  const uint32_t c = a.cls[i];
  const uint64_t term = *a.term;
  // a start met where the record before it expects a file line
  if ((c & kAlStart) && r >= 1 && r <= a.nrec && (r < a.nrec || term == i)) {
    const uint64_t body = i - a.rline[r - 1] - 1;
    if (body & 1) {  // (read as a file line, it is never parsed as a PC)
      fail(SG_A2L_NO_COLON, s);
      return;
    }
  }
  if (r >= a.nrec || (r == a.nrec - 1 && i >= term)) return;  // behind the last record: never read
  if (lng) {
    fail(SG_A2L_TOO_LONG, s);
    return;
  }
  const uint64_t place = i - a.rline[r];
  if (place == 0) {
    uint64_t pc = 0;
    if (!al_parse_pc(a.text, s, e, pc))
      fail(SG_A2L_BAD_PC, s);
    else if (!kEmit && r < L)
      a.rec_pc[r] = pc;
    return;
  }
  if (!(place & 1)) {  // a file line
    if (a.lcolon[i] == kAlNoColon) fail(SG_A2L_NO_COLON, s);
    return;
  }
  if (c & kAlShaped) {  // parse() ends here and the next parse() takes this line for a PC: it has a ':'
    fail(SG_A2L_BAD_PC, s);
    return;
  }
  uint64_t rend = min((uint64_t)a.rline[r + 1], L);
  if (r == a.nrec - 1) rend = min(rend, term);
  if (i + 1 >= rend) {  // no file line: the text ends here, or a start follows (its thread says so)
    if (i + 1 == L) fail(SG_A2L_NO_FILE_LINE, s);
    return;
  }
  uint64_t s2, e2;
  bool lng2;
  al_line(a, i + 1, s2, e2, lng2);
  const uint32_t colon = a.lcolon[i + 1];
  if (lng2 || colon == kAlNoColon) return;  // (the file line's thread fails the call)
  int64_t line = 0;
  if (!al_frame(a.text, s, e, s2, s2 + colon, e2, line)) return;
  if (!kEmit) {
    a.keep[i] = 1;
    return;
  }
  const uint64_t f = a.fpos[i];
  if (f >= a.cap) return;
  a.fn_pos[f] = s;
  a.fn_len[f] = (uint32_t)(e - s);
  a.fl_pos[f] = s2;
  a.fl_len[f] = colon;
  a.line[f] = line;
}

__global__ void k_al_frame_off(AlArgs a, uint64_t* __restrict__ frame_off) {
  const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (r > a.nrec) return;
  const uint64_t nr = min(a.spos[a.nlines], a.nlines);
  frame_off[r] = a.fpos[min((uint64_t)a.rline[min(r, nr)], a.nlines)];
}

// -- interning one column of names: frame i's is text[pos[i] .. + len[i])
struct InArgs {
  const uint8_t* text;
  uint64_t nbytes, n;
  const uint64_t* pos;
  const uint32_t* len;
  uint64_t seed, mask;
  const uint32_t* rank;  // [n] the place of a frame's hash among the distinct hashes
  uint32_t* head;        // [n] per hash: its first frame
  uint32_t* ishead;      // [n]
  const uint64_t* hpos;  // [n + 1] ishead's scan
  uint32_t* impure;
  uint32_t* id;      // [n]
  uint64_t* id_pos;  // [n] per id
  uint32_t* id_len;
};

__device__ __forceinline__ void in_span(const InArgs& a, uint64_t i, uint64_t& p, uint64_t& l) {
  p = min(a.pos[i], a.nbytes);
  l = min((uint64_t)a.len[i], a.nbytes - p);
}

__global__ void k_in_hash(InArgs a, uint64_t* __restrict__ v, uint64_t* __restrict__ ka) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= a.n) return;
  uint64_t p, l;
  in_span(a, i, p, l);
  uint64_t h = a.seed;
  for (uint64_t k = 0; k < l; k++) h = (h ^ a.text[p + k]) * SG_FNV64_PRIME;
  v[i] = ka[i] = h & a.mask;
}
// sorted: rank << 32 | frame.  A hash's first frame.
__global__ void k_in_heads(InArgs a, const uint64_t* __restrict__ sorted) {
  const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= a.n) return;
  const uint64_t c = sorted[j] >> 32;
  if (c < a.n && (j == 0 || (sorted[j - 1] >> 32) != c)) a.head[c] = (uint32_t)min(sorted[j] & 0xFFFFFFFFull, a.n - 1);
}
__global__ void k_in_verify(InArgs a) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= a.n) return;
  const uint64_t h = min((uint64_t)a.head[min((uint64_t)a.rank[i], a.n - 1)], a.n - 1);
  a.ishead[i] = h == i;
  if (h == i) return;
  uint64_t p, l, hp, hl;
  in_span(a, i, p, l);
  in_span(a, h, hp, hl);
  bool same = l == hl;
  for (uint64_t k = 0; same && k < l; k++) same = a.text[p + k] == a.text[hp + k];
  if (!same) *a.impure = 1;  // (every writer writes the same word)
}
__global__ void k_in_ids(InArgs a) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= a.n) return;
  const uint64_t h = min((uint64_t)a.head[min((uint64_t)a.rank[i], a.n - 1)], a.n - 1);
  const uint64_t id = min(a.hpos[h], a.n - 1);
  a.id[i] = (uint32_t)id;
  if (h == i) {
    a.id_pos[id] = a.pos[i];
    a.id_len[id] = a.len[i];
  }
}

// the workspace, kept across its growth (a phase's sizes come from the phase before)
int ws_grow_keep(sg_ctx* ctx, size_t bytes, size_t keep) {
  return ctx->ws.grow_keep(grow_cap(ctx->ws.cap, bytes, (size_t)64 << 20), keep, ctx->stream);
}

// One column: ids and the names' spans from the frames' spans.  The scratch from `scratch` on is free; *nids and
// *rounds (added to) are read back.
int intern_column(sg_ctx* ctx, const uint8_t* d_text, uint64_t nbytes, uint64_t n, const uint64_t* pos,
                  const uint32_t* len, uint32_t hash_bits, uint32_t* id, uint64_t* id_pos, uint32_t* id_len, WsPlan p,
                  uint64_t* nids, uint64_t* rounds) {
  const size_t o_u = p.add(n * 8), o_rank = p.add(n * 4), o_head = p.add(n * 4), o_ishead = p.add(n * 4),
               o_hpos = p.add((n + 1) * 8), o_flag = p.add(8);
  const RankWs g = rank_ws(ctx, p, n);
  InArgs a{};
  a.text = d_text;
  a.nbytes = nbytes;
  a.n = n;
  a.pos = pos;
  a.len = len;
  a.rank = (const uint32_t*)ws_at(ctx, o_rank);
  a.head = (uint32_t*)ws_at(ctx, o_head);
  a.ishead = (uint32_t*)ws_at(ctx, o_ishead);
  a.hpos = (const uint64_t*)ws_at(ctx, o_hpos);
  a.impure = (uint32_t*)ws_at(ctx, o_flag);
  a.id = id;
  a.id_pos = id_pos;
  a.id_len = id_len;
  const dim3 grid(div_up(n, 256)), b(256);
  for (uint32_t round = 0;; round++) {
    if (round == kInternRounds) {
      set_error("interning: %u rounds of 64-bit hashes left different names together", kInternRounds);
      return SG_EHIP;
    }
    a.seed = SG_FNV64_OFFSET ^ (0x9E3779B97F4A7C15ull * round);
    a.mask = round == 0 && hash_bits < 64 ? (1ull << hash_bits) - 1 : ~0ull;
    SG_HIP(hipMemsetAsync(a.impure, 0, 8, ctx->stream));
    SG_HIP(hipMemsetAsync(a.head, 0, n * 4, ctx->stream));
    hipLaunchKernelGGL(k_in_hash, grid, b, 0, ctx->stream, a, g.v, g.ka);
    int rc = rank_values(ctx, g, ~0ull, (uint64_t*)ws_at(ctx, o_u), (uint32_t*)ws_at(ctx, o_rank));
    if (rc) return rc;
    hipLaunchKernelGGL(k_ci_pack, grid, b, 0, ctx->stream, a.rank, n, g.ka);
    uint64_t* sorted = nullptr;
    const uint64_t vary = bits_below(n) << 32;
    if ((rc = radix_sort_u64(ctx, g.ka, g.kb, n, g.tail, &sorted, vary ? vary : 1))) return rc;
    hipLaunchKernelGGL(k_in_heads, grid, b, 0, ctx->stream, a, (const uint64_t*)sorted);
    hipLaunchKernelGGL(k_in_verify, grid, b, 0, ctx->stream, a);
    SG_HIP(hipGetLastError());
    uint32_t impure = 0;
    SG_HIP(hipMemcpyAsync(&impure, a.impure, 4, hipMemcpyDeviceToHost, ctx->stream));
    SG_HIP(hipStreamSynchronize(ctx->stream));
    if (!impure) break;
    ++*rounds;
  }
  int rc = scan_counts(ctx, a.ishead, (uint64_t*)ws_at(ctx, o_hpos), n, g.tail);
  if (rc) return rc;
  hipLaunchKernelGGL(k_in_ids, grid, b, 0, ctx->stream, a);
  SG_HIP(hipGetLastError());
  SG_HIP(hipMemcpyAsync(nids, a.hpos + n, 8, hipMemcpyDeviceToHost, ctx->stream));
  SG_HIP(hipStreamSynchronize(ctx->stream));
  return SG_OK;
}
size_t intern_ws(uint64_t n) { return align256(n * 8) + 3 * align256(n * 4) + align256((n + 1) * 8) + 256 + rank_ws_bytes(n); }

struct A2lOut {
  uint64_t* rec_pc;
  uint64_t* frame_off;
  uint32_t* frame_file;
  int64_t* frame_line;
  uint32_t* frame_func;
  uint64_t* file_pos;
  uint32_t* file_len;
  uint64_t* func_pos;
  uint32_t* func_len;
};

// sg_addr2line_frames*'s body (ctx lock held, the device ensured).  info: {frames, nfiles, nfuncs, status, err_pos,
// extra rounds}.
// With `kept` the records' PCs and the frame arrays are left in the workspace (nothing before kept->ws_end is touched
// until the next reserve, and cover_table_build_ws(frames) bytes behind it are there).
struct A2lKept {
  size_t o_pc = 0, o_foff = 0, o_file = 0, o_line = 0, o_func = 0, ws_end = 0;
};
int addr2line_frames(sg_ctx* ctx, const char* fn, const uint8_t* d_text, uint64_t nbytes, uint64_t nrec, const A2lOut& out,
                     uint64_t cap, uint32_t hash_bits, bool dev, uint64_t info[6], A2lKept* kept = nullptr) {
  for (int k = 0; k < 6; k++) info[k] = 0;
  if (nbytes == 0) {
    info[3] = SG_A2L_EMPTY;
    return SG_OK;
  }
  // phase 1: the lines
  const CiPlan pl(nbytes);
  int rc = ws_reserve(ctx, pl.p);
  if (rc) return rc;
  CiArgs ca = ci_args(ctx, pl, d_text, nbytes);
  uint64_t L = 0;
  unsigned long long err = kNoErr;
  if ((rc = ci_count<kLines>(ctx, pl, ca, &L, &err))) return rc;
  if (L >= 0xFFFFFFFFull) {
    set_error("%s: %llu lines (the limit is 2^32 - 2)", fn, (unsigned long long)L);
    return SG_EINVAL;
  }
  WsPlan p = pl.p;
  const uint64_t npc = std::min<uint64_t>(nrec, L);
  const size_t o_lstart = p.add(L * 8), o_cls = p.add(L), o_lcolon = p.add(L * 4), o_sflag = p.add(L * 4),
               o_spos = p.add((L + 1) * 8), o_rline = p.add((L + 2) * 4), o_word = p.add(16), o_pc = p.add(npc * 8 + 8),
               o_keep = p.add(L * 4), o_fpos = p.add((L + 1) * 8), o_foff = p.add((npc + 2) * 8),
               o_scan = p.add(scan_ws_bytes(L));
  if ((rc = ws_grow_keep(ctx, p.total, pl.p.total))) return rc;
  ca = ci_args(ctx, pl, d_text, nbytes);
  ca.cap = L;
  ca.o_val = (uint64_t*)ws_at(ctx, o_lstart);
  if ((rc = ci_launch<kLines, true>(ctx, ca, "a2l_lines"))) return rc;
  // phase 2: records, failures, kept frames
  AlArgs a{};
  a.text = d_text;
  a.nbytes = nbytes;
  a.nlines = L;
  a.nrec = nrec;
  auto bind = [&] {
    a.lstart = (const uint64_t*)ws_at(ctx, o_lstart);
    a.cls = (uint8_t*)ws_at(ctx, o_cls);
    a.lcolon = (uint32_t*)ws_at(ctx, o_lcolon);
    a.sflag = (uint32_t*)ws_at(ctx, o_sflag);
    a.spos = (const uint64_t*)ws_at(ctx, o_spos);
    a.rline = (uint32_t*)ws_at(ctx, o_rline);
    a.perr = (unsigned long long*)ws_at(ctx, o_word);
    a.term = (uint32_t*)ws_at(ctx, o_word + 8);
    a.rec_pc = (uint64_t*)ws_at(ctx, o_pc);
    a.keep = (uint32_t*)ws_at(ctx, o_keep);
    a.fpos = (const uint64_t*)ws_at(ctx, o_fpos);
  };
  bind();
  const dim3 lgrid(div_up(L, 256)), b(256);
  uint64_t nframes = 0;
  {
    ScopedTimer tm(ctx, "a2l_records");
    SG_HIP(hipMemsetAsync(a.perr, 0xFF, 8, ctx->stream));
    SG_HIP(hipMemsetAsync(a.keep, 0, L * 4, ctx->stream));
    hipLaunchKernelGGL(k_al_class, lgrid, b, 0, ctx->stream, a);
    if ((rc = scan_counts(ctx, a.sflag, (uint64_t*)ws_at(ctx, o_spos), L, o_scan))) return rc;
    hipLaunchKernelGGL(k_al_rline, lgrid, b, 0, ctx->stream, a);
    hipLaunchKernelGGL(k_al_term, dim3(1), b, 0, ctx->stream, a);
    hipLaunchKernelGGL(k_al_check<false>, lgrid, b, 0, ctx->stream, a);
    if ((rc = scan_counts(ctx, a.keep, (uint64_t*)ws_at(ctx, o_fpos), L, o_scan))) return rc;
    SG_HIP(hipGetLastError());
    SG_HIP(hipMemcpyAsync(&err, a.perr, 8, hipMemcpyDeviceToHost, ctx->stream));
    SG_HIP(hipMemcpyAsync(&nframes, a.fpos + L, 8, hipMemcpyDeviceToHost, ctx->stream));
    SG_HIP(hipStreamSynchronize(ctx->stream));
  }
  if (err != kNoErr) {
    info[3] = err & 7;
    info[4] = err >> 3;
    return SG_OK;
  }
  info[0] = nframes;
  uint64_t* frame_off = (uint64_t*)ws_at(ctx, o_foff);
  // (no failure: the text holds nrec records, so nrec <= L and the regions sized by min(nrec, L) hold them)
  hipLaunchKernelGGL(k_al_frame_off, dim3(div_up(nrec + 1, 256)), b, 0, ctx->stream, a, frame_off);
  SG_HIP(hipGetLastError());
  if ((rc = ci_out(ctx, out.rec_pc, a.rec_pc, nrec * 8, dev))) return rc;
  if ((rc = ci_out(ctx, out.frame_off, frame_off, (nrec + 1) * 8, dev))) return rc;
  if (kept) *kept = A2lKept{o_pc, o_foff, 0, 0, 0, p.total};
  if (nframes == 0 || nframes > cap) return SG_OK;
  // phase 3: the frames and their names' ids
  const uint64_t F = nframes;
  const size_t keep2 = p.total;
  const size_t o_fnp = p.add(F * 8), o_fnl = p.add(F * 4), o_flp = p.add(F * 8), o_fll = p.add(F * 4), o_line = p.add(F * 8),
               o_fid = p.add(F * 4), o_uid = p.add(F * 4), o_idp = p.add(F * 8), o_idl = p.add(F * 4), o_idp2 = p.add(F * 8),
               o_idl2 = p.add(F * 4);
  if ((rc = ws_grow_keep(ctx, p.total + std::max(intern_ws(F), kept ? cover_table_build_ws(F) : 0), keep2))) return rc;
  if (kept) *kept = A2lKept{o_pc, o_foff, o_fid, o_line, o_uid, p.total};
  bind();
  frame_off = (uint64_t*)ws_at(ctx, o_foff);
  a.cap = F;
  a.fn_pos = (uint64_t*)ws_at(ctx, o_fnp);
  a.fn_len = (uint32_t*)ws_at(ctx, o_fnl);
  a.fl_pos = (uint64_t*)ws_at(ctx, o_flp);
  a.fl_len = (uint32_t*)ws_at(ctx, o_fll);
  a.line = (int64_t*)ws_at(ctx, o_line);
  {
    ScopedTimer tm(ctx, "a2l_frames");
    hipLaunchKernelGGL(k_al_check<true>, lgrid, b, 0, ctx->stream, a);
    SG_HIP(hipGetLastError());
  }
  uint32_t* fid = (uint32_t*)ws_at(ctx, o_fid);
  uint32_t* uid = (uint32_t*)ws_at(ctx, o_uid);
  {
    ScopedTimer tm(ctx, "a2l_intern");
    if ((rc = intern_column(ctx, d_text, nbytes, F, a.fl_pos, a.fl_len, hash_bits, fid, (uint64_t*)ws_at(ctx, o_idp),
                            (uint32_t*)ws_at(ctx, o_idl), p, &info[1], &info[5])))
      return rc;
    if ((rc = intern_column(ctx, d_text, nbytes, F, a.fn_pos, a.fn_len, hash_bits, uid, (uint64_t*)ws_at(ctx, o_idp2),
                            (uint32_t*)ws_at(ctx, o_idl2), p, &info[2], &info[5])))
      return rc;
  }
  if ((rc = ci_out(ctx, out.frame_file, fid, F * 4, dev))) return rc;
  if ((rc = ci_out(ctx, out.frame_line, a.line, F * 8, dev))) return rc;
  if ((rc = ci_out(ctx, out.frame_func, uid, F * 4, dev))) return rc;
  if ((rc = ci_out(ctx, out.file_pos, ws_at(ctx, o_idp), info[1] * 8, dev))) return rc;
  if ((rc = ci_out(ctx, out.file_len, ws_at(ctx, o_idl), info[1] * 4, dev))) return rc;
  if ((rc = ci_out(ctx, out.func_pos, ws_at(ctx, o_idp2), info[2] * 8, dev))) return rc;
  return ci_out(ctx, out.func_len, ws_at(ctx, o_idl2), info[2] * 4, dev);
}

int a2l_args(const char* fn, sg_ctx* ctx, const uint8_t* text, uint64_t nbytes, uint64_t nrec, const A2lOut& o, uint64_t cap,
             uint32_t hash_bits, const uint64_t* info) {
  if (!ctx || !info || (nbytes && !text) || !o.rec_pc || !o.frame_off ||
      (cap && (!o.frame_file || !o.frame_line || !o.frame_func || !o.file_pos || !o.file_len || !o.func_pos || !o.func_len))) {
    set_error("%s: invalid argument", fn);
    return SG_EINVAL;
  }
  if (nrec >= 0xFFFFFFFFull) {
    set_error("%s: %llu records (the limit is 2^32 - 2)", fn, (unsigned long long)nrec);
    return SG_EINVAL;
  }
  if (hash_bits < 1 || hash_bits > 64) {
    set_error("%s: hash_bits %u (1..64)", fn, hash_bits);
    return SG_EINVAL;
  }
  return ci_text_ok(fn, nbytes);
}

}  // namespace
}  // namespace sg

using namespace sg;

extern "C" {

int sg_objdump_pcs_dev(sg_ctx* ctx, const uint8_t* d_text, uint64_t nbytes, const uint8_t* call, size_t call_len,
                       const uint8_t* func, size_t func_len, uint64_t* d_pcs, uint64_t cap, uint64_t* d_info) {
  const char* fn = "sg_objdump_pcs_dev";
  if (!ctx || !d_info || (nbytes && !d_text) || (cap && !d_pcs)) {
    set_error("%s: invalid argument", fn);
    return SG_EINVAL;
  }
  CiNeedle nc, nf;
  int rc = ci_needle(fn, "call", call, call_len, &nc);
  if (rc || (rc = ci_needle(fn, "function", func, func_len, &nf)) || (rc = ci_text_ok(fn, nbytes))) return rc;
  std::lock_guard<std::mutex> g(ctx->mu);
  if ((rc = ensure_device(ctx))) return rc;
  CiInfo info;
  if ((rc = objdump_pcs(ctx, d_text, nbytes, nc, nf, d_pcs, cap, true, &info))) return rc;
  return ci_info_dev(ctx, d_info, info);
}

int sg_objdump_pcs(sg_ctx* ctx, const uint8_t* text, size_t nbytes, const uint8_t* call, size_t call_len,
                   const uint8_t* func, size_t func_len, uint64_t* pcs, size_t cap, size_t* npcs, uint32_t* status,
                   uint64_t* err_pos) {
  const char* fn = "sg_objdump_pcs";
  if (!ctx || !npcs || !status || !err_pos || (nbytes && !text) || (cap && !pcs)) {
    set_error("%s: invalid argument", fn);
    return SG_EINVAL;
  }
  CiNeedle nc, nf;
  int rc = ci_needle(fn, "call", call, call_len, &nc);
  if (rc || (rc = ci_needle(fn, "function", func, func_len, &nf)) || (rc = ci_text_ok(fn, nbytes))) return rc;
  std::lock_guard<std::mutex> g(ctx->mu);
  if ((rc = ensure_device(ctx))) return rc;
  const uint8_t* d_text = nullptr;
  if ((rc = ci_stage_text(ctx, text, nbytes, &d_text))) return rc;
  CiInfo info;
  if ((rc = objdump_pcs(ctx, d_text, nbytes, nc, nf, pcs, cap, false, &info))) return rc;
  SG_HIP(hipStreamSynchronize(ctx->stream));
  *npcs = info.count;
  *status = (uint32_t)info.status;
  *err_pos = info.err_pos;
  return SG_OK;
}

int sg_nm_symbols_dev(sg_ctx* ctx, const uint8_t* d_text, uint64_t nbytes, uint64_t* d_addr, int64_t* d_size,
                      uint64_t* d_name_pos, uint32_t* d_name_len, uint64_t* d_sym_start, uint64_t* d_sym_end,
                      uint32_t* d_order, uint64_t cap, uint64_t* d_info) {
  const char* fn = "sg_nm_symbols_dev";
  if (!ctx || !d_info || (nbytes && !d_text)) {
    set_error("%s: invalid argument", fn);
    return SG_EINVAL;
  }
  int rc = ci_text_ok(fn, nbytes);
  if (rc) return rc;
  std::lock_guard<std::mutex> g(ctx->mu);
  if ((rc = ensure_device(ctx))) return rc;
  CiInfo info;
  const NmOut out{d_addr, d_size, d_name_pos, d_name_len, d_sym_start, d_sym_end, d_order};
  if ((rc = nm_symbols(ctx, fn, d_text, nbytes, out, cap, true, &info))) return rc;
  return ci_info_dev(ctx, d_info, info);
}

int sg_nm_symbols(sg_ctx* ctx, const uint8_t* text, size_t nbytes, uint64_t* addr, int64_t* size, uint64_t* name_pos,
                  uint32_t* name_len, uint64_t* sym_start, uint64_t* sym_end, uint32_t* order, size_t cap, size_t* nsyms,
                  uint32_t* status, uint64_t* err_pos) {
  const char* fn = "sg_nm_symbols";
  if (!ctx || !nsyms || !status || !err_pos || (nbytes && !text)) {
    set_error("%s: invalid argument", fn);
    return SG_EINVAL;
  }
  int rc = ci_text_ok(fn, nbytes);
  if (rc) return rc;
  std::lock_guard<std::mutex> g(ctx->mu);
  if ((rc = ensure_device(ctx))) return rc;
  const uint8_t* d_text = nullptr;
  if ((rc = ci_stage_text(ctx, text, nbytes, &d_text))) return rc;
  CiInfo info;
  const NmOut out{addr, size, name_pos, name_len, sym_start, sym_end, order};
  if ((rc = nm_symbols(ctx, fn, d_text, nbytes, out, cap, false, &info))) return rc;
  SG_HIP(hipStreamSynchronize(ctx->stream));
  *nsyms = info.count;
  *status = (uint32_t)info.status;
  *err_pos = info.err_pos;
  return SG_OK;
}

int sg_addr2line_frames_dev(sg_ctx* ctx, const uint8_t* d_text, uint64_t nbytes, uint64_t nrec, uint64_t* d_rec_pc,
                            uint64_t* d_frame_off, uint32_t* d_frame_file, int64_t* d_frame_line, uint32_t* d_frame_func,
                            uint64_t cap, uint64_t* d_file_pos, uint32_t* d_file_len, uint64_t* d_func_pos,
                            uint32_t* d_func_len, uint32_t hash_bits, uint64_t* d_info) {
  const char* fn = "sg_addr2line_frames_dev";
  const A2lOut out{d_rec_pc, d_frame_off, d_frame_file, d_frame_line, d_frame_func, d_file_pos, d_file_len, d_func_pos,
                   d_func_len};
  int rc = a2l_args(fn, ctx, d_text, nbytes, nrec, out, cap, hash_bits, d_info);
  if (rc) return rc;
  std::lock_guard<std::mutex> g(ctx->mu);
  if ((rc = ensure_device(ctx))) return rc;
  uint64_t info[6];
  if ((rc = addr2line_frames(ctx, fn, d_text, nbytes, nrec, out, cap, hash_bits, true, info))) return rc;
  SG_HIP(hipMemcpyAsync(d_info, info, sizeof(info), hipMemcpyHostToDevice, ctx->stream));
  SG_HIP(hipStreamSynchronize(ctx->stream));  // (info leaves scope)
  return SG_OK;
}

int sg_addr2line_frames(sg_ctx* ctx, const uint8_t* text, size_t nbytes, size_t nrec, uint64_t* rec_pc,
                        uint64_t* frame_off, uint32_t* frame_file, int64_t* frame_line, uint32_t* frame_func, size_t cap,
                        uint64_t* file_pos, uint32_t* file_len, uint64_t* func_pos, uint32_t* func_len, uint32_t hash_bits,
                        uint64_t* info) {
  const char* fn = "sg_addr2line_frames";
  const A2lOut out{rec_pc, frame_off, frame_file, frame_line, frame_func, file_pos, file_len, func_pos, func_len};
  int rc = a2l_args(fn, ctx, text, nbytes, nrec, out, cap, hash_bits, info);
  if (rc) return rc;
  std::lock_guard<std::mutex> g(ctx->mu);
  if ((rc = ensure_device(ctx))) return rc;
  const uint8_t* d_text = nullptr;
  if ((rc = ci_stage_text(ctx, text, nbytes, &d_text))) return rc;
  uint64_t got[6];
  if ((rc = addr2line_frames(ctx, fn, d_text, nbytes, nrec, out, cap, hash_bits, false, got))) return rc;
  SG_HIP(hipStreamSynchronize(ctx->stream));
  for (int k = 0; k < 6; k++) info[k] = got[k];
  return SG_OK;
}

int sg_cover_table_from_text(sg_ctx* ctx, const uint8_t* nm_text, size_t nm_bytes, const uint64_t* all_pcs, size_t nall,
                             const uint8_t* a2l_text, size_t a2l_bytes, size_t nrec, uint32_t hash_bits, uint64_t* file_pos,
                             uint32_t* file_len, uint64_t* func_pos, uint32_t* func_len, size_t names_cap, uint64_t* info,
                             sg_cover_table** out) {
  const char* fn = "sg_cover_table_from_text";
  if (!ctx || !out || !info || (nm_bytes && !nm_text) || (a2l_bytes && !a2l_text) || (nall && !all_pcs) ||
      (names_cap && (!file_pos || !file_len || !func_pos || !func_len))) {
    set_error("%s: invalid argument", fn);
    return SG_EINVAL;
  }
  *out = nullptr;
  if (nrec >= 0xFFFFFFFFull || hash_bits < 1 || hash_bits > 64) {
    set_error("%s: nrec must be below 2^32 - 1 and hash_bits in 1..64", fn);
    return SG_EINVAL;
  }
  int rc = ci_text_ok(fn, nm_bytes);
  if (rc || (rc = ci_text_ok(fn, a2l_bytes))) return rc;
  for (int k = 0; k < 8; k++) info[k] = 0;
  std::lock_guard<std::mutex> g(ctx->mu);
  if ((rc = ensure_device(ctx))) return rc;
  // the symbols: a few MB of text, and the table's plan reads them on the host
  const uint8_t* d_text = nullptr;
  if ((rc = ci_stage_text(ctx, nm_text, nm_bytes, &d_text))) return rc;
  const uint64_t scap = nm_bytes / 6 + 1;
  std::vector<uint64_t> ss(scap), se(scap);
  CiInfo ni;
  const NmOut nmo{nullptr, nullptr, nullptr, nullptr, ss.data(), se.data(), nullptr};
  if ((rc = nm_symbols(ctx, fn, d_text, nm_bytes, nmo, scap, false, &ni))) return rc;
  SG_HIP(hipStreamSynchronize(ctx->stream));
  if (ni.status) {
    info[6] = ni.status;
    info[7] = ni.err_pos;
    return SG_OK;
  }
  if ((rc = table_syms_ok(fn, ss.data(), se.data(), ni.count, all_pcs, nall))) return rc;
  // the frames: parsed and interned on the device, and left there
  if ((rc = ci_stage_text(ctx, a2l_text, a2l_bytes, &d_text))) return rc;
  const A2lOut ao{nullptr, nullptr, nullptr, nullptr, nullptr, file_pos, file_len, func_pos, func_len};
  A2lKept kept;
  uint64_t got[6];
  // (names never outnumber frames: with more frames than names_cap nothing is written and the count comes back)
  if ((rc = addr2line_frames(ctx, fn, d_text, a2l_bytes, nrec, ao, names_cap, hash_bits, false, got, &kept))) return rc;
  SG_HIP(hipStreamSynchronize(ctx->stream));
  for (int k = 0; k < 6; k++) info[k] = got[k];
  if (got[3] || got[0] > names_cap) return SG_OK;
  const uint64_t nfr = got[0];
  if (nfr >= 0xFFFFFFFFull) {
    set_error("%s: too many frames for one table", fn);
    return SG_EINVAL;
  }
  uint64_t ends[2] = {0, 0};
  const uint64_t* d_pc = (const uint64_t*)ws_at(ctx, kept.o_pc);
  if (nrec) {
    SG_HIP(hipMemcpyAsync(&ends[0], d_pc, 8, hipMemcpyDeviceToHost, ctx->stream));
    SG_HIP(hipMemcpyAsync(&ends[1], d_pc + (nrec - 1), 8, hipMemcpyDeviceToHost, ctx->stream));
    SG_HIP(hipStreamSynchronize(ctx->stream));
  }
  if ((rc = ws_grow_keep(ctx, kept.ws_end + cover_table_build_ws(nfr), kept.ws_end))) return rc;
  d_pc = (const uint64_t*)ws_at(ctx, kept.o_pc);
  const CoverTableDev dv{d_pc, (const uint64_t*)ws_at(ctx, kept.o_foff), (const uint32_t*)ws_at(ctx, kept.o_file),
                         (const int64_t*)ws_at(ctx, kept.o_line), (const uint32_t*)ws_at(ctx, kept.o_func), kept.ws_end};
  const TableSrc src{nullptr, nullptr, nullptr, nullptr, nullptr, &dv, (bits_below(got[1]) << 32) | 0xFFFFFFFFull};
  return table_build(ctx, fn, ss.data(), se.data(), ni.count, all_pcs, nall, nrec, ends[0], ends[1], nfr, (uint32_t)got[1],
                     (uint32_t)got[2], src, out);
}

}  // extern "C"
