// sg_cover_pages.hip -- the /cover page's file bodies: fileSet -> templateFile.
//
// Reference: syz-manager/cover.go:122-156 (generateCoverHtml's loop over
// fileSet's map: parseFile, then every line written into a bytes.Buffer, a
// listed line between one of two pairs of literals) and cover.go:198-217
// (parseFile: the file split at '\n', every line through a four-way
// strings.Replacer, what follows the last '\n' appended raw), all of it under
// mgr.mu (httpCover, syz-manager/html.go:169-194) and per request.
//
// The sources depend on the tree alone, so parseFile runs once, into a table
// that stays on the device (sg_src_table): the escaped text of every file,
// each line followed by '\n' (the raw last fragment too: the render loop
// appends one to every line), the line offsets, each file's line range.  A
// file's stored text is its body when nothing is listed.
//
//   k_sp_last    per 16 raw bytes: atomicMax of each file's last '\n' (what
//                lies behind it is the raw fragment)
//   k_sp_count   per 16 raw bytes: stored bytes and lines; two scans
//   k_sp_write   per 16 raw bytes: the stored text, a line offset behind every
//                stored '\n', each file's first line
//
// A report is sg_cover_lines' pipeline (cover_lines_body, sg_cover_lines.h)
// with a tail that works on the line tables where they lie:
//
//   k_pg_marks   per listed line: its file, and the bytes it inserts (38
//                covered, 28 uncovered, 0 when it lies past the file's end)
//   scan         of the inserted bytes
//   k_pg_files   per file: the listed lines inside it (a search: they ascend),
//                Coverage from the inserted bytes, the stored length and the
//                records it will hold; the lowest unreadable file
//   k_pg_scan    one workgroup: stored bytes and records before each file
//   k_pg_off     body_off; a record for each file's start
//   k_pg_emit    a record per listed line inside its file: where its prefix
//                starts in the bodies, its text and its length
//   -- the report's one wait, which brings back body_off, Coverage and the
//      record count with the counts --
//   k_pg_tiles   per tile of the bodies: the record its first byte is under
//   k_pg_copy    a workgroup per tile, a lane per aligned 16 bytes: the record
//                by search inside the tile's range, then run by run (text at
//                a constant shift, or a literal) one unaligned 16-byte load
//                merged under a byte mask; one aligned 16-byte store
//
// The records ascend by position: a body is its file's record, then its
// listed lines'.  The only tie is a file's record with a listed first line.
#include "sg_cover_lines.h"

#include <algorithm>
#include <cstring>
#include <vector>

namespace sg {
namespace {

// cover.go:133-140, as rows of 64 bytes with the literal at byte 16: a run of
// a literal is loaded as the 16 bytes of its lane's chunk, which start up to
// 15 bytes before the literal and end up to 15 behind it.
constexpr uint32_t kLitRow = 64, kLitAt = 16, kLitBytes = 4 * kLitRow;
const char* const kLits[4] = {"<span id='covered'>", "</span> /*covered*/\n", "<span id='uncovered'>", "</span>\n"};
constexpr uint32_t kPreCov = 19, kSufCov = 20, kPreUnc = 21, kSufUnc = 8;
constexpr uint32_t kInsCov = kPreCov + kSufCov - 1, kInsUnc = kPreUnc + kSufUnc - 1;  // (the suffix carries the '\n')
constexpr uint32_t kTextPad = 16;  // bytes kept in front of and behind the stored text, for the same reason
enum : uint8_t { kRecFile = 0, kRecUnc = 1, kRecCov = 2 };

}  // namespace
}  // namespace sg

struct sg_src_table {
  sg_ctx* ctx = nullptr;
  sg::DevBuf<char> mem;  // the one device block everything below lives in
  uint32_t nfiles = 0;
  uint64_t nlines = 0, stored = 0, raw = 0;
  const uint8_t* lit = nullptr;  // [kLitBytes]
  uint8_t* text = nullptr;       // [stored], kTextPad bytes on either side
  uint32_t* line_off = nullptr;  // [nlines + 1]
  uint32_t* file_line = nullptr; // [nfiles + 1]
  uint8_t* have = nullptr;       // [nfiles]
  std::vector<uint32_t> h_file_line;
};

namespace sg {
namespace {

// ---- the source table ---------------------------------------------------------
struct SrcArgs {
  const uint8_t* raw;   // [nraw], padded to whole chunks
  const uint32_t* off;  // [nfiles + 1]
  uint32_t* esc_end;    // [nfiles] the end of what the replacer sees: behind the last '\n', else the file's start
  uint64_t nraw;
  uint32_t nfiles;
  uint32_t *cl, *cn;       // [chunks] stored bytes, lines
  const uint64_t *sl, *sn; // their scans
  uint8_t* text;
  uint32_t *line_off, *file_line;
};

// the file of raw byte p < nraw: the last f with off[f] <= p (the empty files at p come before it)
__device__ __forceinline__ uint32_t file_of(const uint32_t* off, uint32_t nfiles, uint64_t p) {
  uint32_t lo = 0, hi = nfiles;
  while (lo < hi) {
    const uint32_t mid = (lo + hi) >> 1;
    if (off[mid] <= p)
      lo = mid + 1;
    else
      hi = mid;
  }
  return lo - 1;  // (off[0] == 0 <= p)
}

// fn(p, f, file start, file end, esc_end, byte) for the raw bytes of chunk c
template <typename F>
__device__ __forceinline__ void walk_chunk(const SrcArgs& a, uint64_t c, F&& fn) {
  const uint64_t p0 = c * 16;
  const uint4 v = *reinterpret_cast<const uint4*>(a.raw + p0);
  const uint32_t w[4] = {v.x, v.y, v.z, v.w};
  uint32_t f = file_of(a.off, a.nfiles, p0);
  uint64_t fbeg = a.off[f], fend = a.off[f + 1], esc = a.esc_end[f];
#pragma unroll
  for (int i = 0; i < 16; i++) {
    const uint64_t p = p0 + i;
    if (p < a.nraw) {
      while (p >= fend) {  // (p < nraw == off[nfiles]: ends at a file)
        f++;
        fbeg = fend;
        fend = a.off[f + 1];
        esc = a.esc_end[f];
      }
      fn(p, f, fbeg, fend, esc, (uint8_t)(w[i >> 2] >> (8 * (i & 3))));
    }
  }
}

__global__ __launch_bounds__(256) void k_sp_last(SrcArgs a, uint64_t nch) {
  const uint64_t c = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= nch) return;
  walk_chunk(a, c, [&](uint64_t p, uint32_t f, uint64_t, uint64_t, uint64_t, uint8_t b) {
    if (b == '\n' && a.esc_end[f] < p + 1) atomicMax(&a.esc_end[f], (uint32_t)(p + 1));
  });
}

// cover.go:203: what a byte in front of the file's last '\n' is stored as
__device__ __forceinline__ uint32_t esc_len(uint8_t b) {
  return b == '>' || b == '<' ? 4u : b == '&' ? 5u : b == '\t' ? 8u : 1u;
}

__global__ __launch_bounds__(256) void k_sp_count(SrcArgs a, uint64_t nch) {
  const uint64_t c = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= nch) return;
  uint32_t len = 0, ln = 0;
  walk_chunk(a, c, [&](uint64_t p, uint32_t, uint64_t, uint64_t fend, uint64_t esc, uint8_t b) {
    if (p < esc) {
      len += esc_len(b);
      ln += b == '\n';
    } else {  // the raw fragment; its last byte brings the '\n' the render loop appends
      len += 1 + (p + 1 == fend);
      ln += p + 1 == fend;
    }
  });
  a.cl[c] = len;
  a.cn[c] = ln;
}

__global__ __launch_bounds__(256) void k_sp_write(SrcArgs a, uint64_t nch) {
  const uint64_t c = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= nch) return;
  uint64_t w = a.sl[c], n = a.sn[c];
  walk_chunk(a, c, [&](uint64_t p, uint32_t f, uint64_t fbeg, uint64_t fend, uint64_t esc, uint8_t b) {
    if (p == fbeg)  // a file's first byte: its first line, and that of the empty files in front of it
      for (uint32_t g = f;; g--) {
        a.file_line[g] = (uint32_t)n;
        if (g == 0 || a.off[g - 1] != p) break;
      }
    bool eol = false;
    if (p >= esc) {
      a.text[w++] = b;
      eol = p + 1 == fend;
      if (eol) a.text[w++] = '\n';
    } else if (b == '\n') {
      a.text[w++] = '\n';
      eol = true;
    } else if (b == '\t') {
      for (int k = 0; k < 8; k++) a.text[w++] = ' ';
    } else if (b == '>' || b == '<' || b == '&') {
      a.text[w++] = '&';
      if (b == '&') {
        a.text[w++] = 'a';
        a.text[w++] = 'm';
        a.text[w++] = 'p';
      } else {
        a.text[w++] = b == '>' ? 'g' : 'l';
        a.text[w++] = 't';
      }
      a.text[w++] = ';';
    } else {
      a.text[w++] = b;
    }
    if (eol) a.line_off[++n] = (uint32_t)w;
  });
}

// the files that start at the end of the raw bytes (none of whose bytes a chunk holds), and entry nfiles
__global__ void k_sp_tail(SrcArgs a, uint32_t nlines) {
  const uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (g <= a.nfiles && a.off[g] == a.nraw) a.file_line[g] = nlines;
}

// ---- the report's tail --------------------------------------------------------------
struct PagesHead {
  uint32_t bad;  // the lowest file of the report that could not be read, else UINT32_MAX
  uint32_t pad;
  uint64_t nrec;
};

struct PagesArgs {
  LinesDev d;
  uint64_t nslots;
  uint32_t nfiles;
  const uint8_t *lit, *text;
  const uint32_t *line_off, *file_line;
  const uint8_t* have;
  uint32_t* ins;     // [nslots] bytes a listed line inserts
  uint64_t* inscan;  // [nslots + 1]
  uint32_t* mfile;   // [nslots] its file
  uint64_t* flen;    // [nfiles + 1] stored bytes of a file of the report; scanned in place
  uint64_t* frec;    // [nfiles + 1] its records; scanned in place
  uint64_t* body_off;  // [nfiles + 1]
  uint32_t* coverage;  // [nfiles]
  PagesHead* head;
  uint64_t* rec_pos;  // [nslots + nfiles + 1] where a record starts in the bodies; [nrec] = their end
  uint32_t* rec_src;  // ... its text in the table
  uint32_t* rec_len;  // ... a listed line's length without its '\n'
  uint8_t* rec_kind;
};

__global__ __launch_bounds__(256) void k_pg_marks(PagesArgs a) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= a.nslots) return;
  uint32_t ins = 0;
  if (i < a.d.file_off[a.nfiles]) {
    const uint32_t f = (uint32_t)(sgd::ub64(a.d.file_off, (uint64_t)a.nfiles + 1, i) - 1);
    const uint32_t nl = a.have[f] ? a.file_line[f + 1] - a.file_line[f] : 0;
    a.mfile[i] = f;
    if (a.d.lines[i] <= nl) ins = a.d.cov[i] ? kInsCov : kInsUnc;  // (lines are > 0; one past the end is dropped)
  }
  a.ins[i] = ins;
}

__global__ __launch_bounds__(256) void k_pg_files(PagesArgs a) {
  const uint64_t f = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (f > a.nfiles) return;
  uint64_t stored = 0, rec = 0;
  if (f < a.nfiles) {
    const uint64_t m0 = a.d.file_off[f], m1 = a.d.file_off[f + 1];
    uint32_t cov = 0;
    if (m1 > m0) {
      if (!a.have[f]) {
        atomicMin(&a.head->bad, (uint32_t)f);
      } else {
        const uint32_t l0 = a.file_line[f], nl = a.file_line[f + 1] - l0;
        uint64_t lo = m0, hi = m1;  // the listed lines <= nl: they ascend
        while (lo < hi) {
          const uint64_t mid = (lo + hi) >> 1;
          if (a.d.lines[mid] <= nl)
            lo = mid + 1;
          else
            hi = mid;
        }
        const uint64_t inside = lo - m0;
        cov = (uint32_t)((a.inscan[m1] - a.inscan[m0] - kInsUnc * inside) / (kInsCov - kInsUnc));
        stored = a.line_off[l0 + nl] - a.line_off[l0];
        rec = nl ? 1 + inside : 0;
      }
    }
    a.coverage[f] = cov;
  }
  a.flen[f] = stored;
  a.frec[f] = rec;
}

// exclusive scans of flen and frec in place, n = nfiles + 1 entries (the last ones zero: they become the totals)
__global__ __launch_bounds__(1024) void k_pg_scan(PagesArgs a) {
  __shared__ uint64_t sa[1024], sb[1024];
  const uint32_t t = threadIdx.x;
  const uint64_t n = (uint64_t)a.nfiles + 1;
  uint64_t ca = 0, cb = 0;
  for (uint64_t base = 0; base < n; base += 1024) {
    const uint64_t i = base + t;
    const uint64_t va = i < n ? a.flen[i] : 0, vb = i < n ? a.frec[i] : 0;
    sa[t] = va;
    sb[t] = vb;
    __syncthreads();
    for (uint32_t d = 1; d < 1024; d <<= 1) {
      const uint64_t xa = t >= d ? sa[t - d] : 0, xb = t >= d ? sb[t - d] : 0;
      __syncthreads();
      sa[t] += xa;
      sb[t] += xb;
      __syncthreads();
    }
    if (i < n) {
      a.flen[i] = ca + sa[t] - va;
      a.frec[i] = cb + sb[t] - vb;
    }
    ca += sa[1023];
    cb += sb[1023];
    __syncthreads();
  }
  if (t == 0) a.head->nrec = cb;
}

__global__ __launch_bounds__(256) void k_pg_off(PagesArgs a) {
  const uint64_t f = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (f > a.nfiles) return;
  if (a.head->bad != 0xFFFFFFFFu) {  // nothing is rendered
    a.body_off[f] = 0;
    if (f < a.nfiles) a.coverage[f] = 0;
    return;
  }
  const uint64_t at = a.flen[f] + a.inscan[a.d.file_off[f]];
  a.body_off[f] = at;
  const uint64_t r = a.frec[f];
  if (f == a.nfiles) {
    a.rec_pos[r] = at;
  } else if (a.frec[f + 1] > r) {
    a.rec_pos[r] = at;
    a.rec_src[r] = a.line_off[a.file_line[f]];
    a.rec_len[r] = 0;
    a.rec_kind[r] = kRecFile;
  }
}

__global__ __launch_bounds__(256) void k_pg_emit(PagesArgs a) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= a.nslots || a.ins[i] == 0 || a.head->bad != 0xFFFFFFFFu) return;
  const uint32_t f = a.mfile[i];
  const uint64_t m0 = a.d.file_off[f];
  const uint64_t r = a.frec[f] + 1 + (i - m0);  // (the lines inside the file are the first of its list)
  const uint32_t l0 = a.file_line[f], ln = a.d.lines[i];
  const uint32_t beg = a.line_off[l0 + ln - 1], end = a.line_off[l0 + ln] - 1;
  a.rec_pos[r] = a.body_off[f] + (beg - a.line_off[l0]) + (a.inscan[i] - a.inscan[m0]);
  a.rec_src[r] = beg;
  a.rec_len[r] = end - beg;
  a.rec_kind[r] = a.d.cov[i] ? kRecCov : kRecUnc;
}

// ---- the copy -------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_pg_tiles(const uint64_t* __restrict__ rec_pos, uint64_t nrec, uint64_t ntiles,
                                                  uint64_t* __restrict__ tile_rec) {
  const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t > ntiles) return;
  // (record 0 starts at byte 0 of the bodies: every byte is under one)
  tile_rec[t] = t < ntiles ? sgd::ub64(rec_pos, nrec, t * kPagesTile) - 1 : nrec - 1;
}

__device__ __forceinline__ uint4 load16u(const uint8_t* p) {
  uint4 v;
  __builtin_memcpy(&v, p, 16);
  return v;
}

// the bytes [a, b) of a chunk, as the mask of its dword j
__device__ __forceinline__ uint32_t run_mask(uint32_t a, uint32_t b, uint32_t j) {
  const uint32_t lo = a > 4 * j ? min(a - 4 * j, 4u) : 0u, hi = b > 4 * j ? min(b - 4 * j, 4u) : 0u;
  const uint32_t below_hi = hi >= 4 ? 0xFFFFFFFFu : (1u << (8 * hi)) - 1;
  const uint32_t below_lo = lo >= 4 ? 0xFFFFFFFFu : (1u << (8 * lo)) - 1;
  return below_hi & ~below_lo;
}

__global__ __launch_bounds__(256) void k_pg_copy(const uint8_t* __restrict__ lit, const uint8_t* __restrict__ text,
                                                 const uint64_t* __restrict__ rec_pos,
                                                 const uint32_t* __restrict__ rec_src,
                                                 const uint32_t* __restrict__ rec_len,
                                                 const uint8_t* __restrict__ rec_kind,
                                                 const uint64_t* __restrict__ tile_rec, uint64_t nbytes,
                                                 uint8_t* __restrict__ out) {
  const uint64_t o0 = (uint64_t)blockIdx.x * kPagesTile + (uint64_t)threadIdx.x * 16;
  if (o0 >= nbytes) return;
  const uint64_t end = min(o0 + 16, nbytes);
  uint64_t r = sgd::seg_search(rec_pos, tile_rec[blockIdx.x], tile_rec[blockIdx.x + 1], o0);
  uint64_t next = rec_pos[r + 1];  // (rec_pos[nrec] == nbytes > o: the walk ends at a record)
  uint32_t w0 = 0, w1 = 0, w2 = 0, w3 = 0;
  for (uint64_t o = o0; o < end;) {
    while (next <= o) next = rec_pos[++r + 1];
    const uint64_t pos = rec_pos[r], d = o - pos;
    const uint64_t src = rec_src[r], len = rec_len[r];
    const uint32_t kind = rec_kind[r];
    const uint32_t pre = kind == kRecFile ? 0 : kind == kRecCov ? kPreCov : kPreUnc;
    const uint32_t suf = kind == kRecFile ? 0 : kind == kRecCov ? kSufCov : kSufUnc;
    const uint32_t row = kind == kRecCov ? 0 : 2 * kLitRow;  // the prefix's row; the suffix's follows it
    const uint8_t* from;
    uint64_t stop = next;
    if (kind == kRecFile) {
      from = text + src + d;
    } else if (d < pre) {
      from = lit + row + kLitAt + d;
      stop = pos + pre;
    } else if (d < pre + len) {
      from = text + src + (d - pre);
      stop = pos + pre + len;
    } else if (d < pre + len + suf) {
      from = lit + row + kLitRow + kLitAt + (d - pre - len);
      stop = pos + pre + len + suf;
    } else {  // behind the listed line, up to the next record
      from = text + src + len + 1 + (d - pre - len - suf);
    }
    stop = min(stop, min(next, end));
    const uint32_t ra = (uint32_t)(o - o0), rb = (uint32_t)(stop - o0);
    const uint4 v = load16u(from - ra);
    const uint32_t m0 = run_mask(ra, rb, 0), m1 = run_mask(ra, rb, 1), m2 = run_mask(ra, rb, 2),
                   m3 = run_mask(ra, rb, 3);
    w0 = (w0 & ~m0) | (v.x & m0);
    w1 = (w1 & ~m1) | (v.y & m1);
    w2 = (w2 & ~m2) | (v.z & m2);
    w3 = (w3 & ~m3) | (v.w & m3);
    o = stop;
  }
  *reinterpret_cast<uint4*>(out + o0) = make_uint4(w0, w1, w2, w3);  // (the buffer holds whole chunks)
}

// What sg_cover_pages hangs on the report (sg_cover_lines.h).
struct PagesTail final : LinesTail {
  sg_cover_table* t;
  sg_src_table* src;
  uint64_t* body_off;
  uint32_t* coverage;
  uint8_t* bodies;
  size_t cap;
  size_t* nbytes;
  uint32_t* bad_file;
  PagesHead head{};
  PagesArgs a{};
  WsPlan p;
  size_t o_ins, o_scan, o_mf, o_fl, o_fr, o_bo, o_cv, o_hd, o_rp, o_rs, o_rl, o_rk, o_tail;

  PagesTail(sg_cover_table* t_, sg_src_table* s_) : t(t_), src(s_) {
    const uint64_t ns = t->nslots, nf = t->nfiles, nr = ns + nf + 1;
    o_ins = p.add(ns * 4), o_scan = p.add((ns + 1) * 8), o_mf = p.add(ns * 4), o_fl = p.add((nf + 1) * 8);
    o_fr = p.add((nf + 1) * 8), o_bo = p.add((nf + 1) * 8), o_cv = p.add(nf * 4), o_hd = p.add(sizeof(PagesHead));
    o_rp = p.add(nr * 8), o_rs = p.add(nr * 4), o_rl = p.add(nr * 4), o_rk = p.add(nr);
    o_tail = p.total;
    ws_bytes = p.total + scan_ws_bytes(ns);
  }

  int queued(const LinesDev& d, size_t ws_off) override {
    sg_ctx* ctx = t->ctx;
    const uint64_t ns = t->nslots, nf = t->nfiles;
    char* w = (char*)ws_at(ctx, ws_off);
    a.d = d;
    a.nslots = ns;
    a.nfiles = t->nfiles;
    a.lit = src->lit;
    a.text = src->text;
    a.line_off = src->line_off;
    a.file_line = src->file_line;
    a.have = src->have;
    a.ins = (uint32_t*)(w + o_ins);
    a.inscan = (uint64_t*)(w + o_scan);
    a.mfile = (uint32_t*)(w + o_mf);
    a.flen = (uint64_t*)(w + o_fl);
    a.frec = (uint64_t*)(w + o_fr);
    a.body_off = (uint64_t*)(w + o_bo);
    a.coverage = (uint32_t*)(w + o_cv);
    a.head = (PagesHead*)(w + o_hd);
    a.rec_pos = (uint64_t*)(w + o_rp);
    a.rec_src = (uint32_t*)(w + o_rs);
    a.rec_len = (uint32_t*)(w + o_rl);
    a.rec_kind = (uint8_t*)(w + o_rk);
    {
      ScopedTimer tm(ctx, "pages_marks");
      SG_HIP(hipMemsetAsync(a.head, 0xFF, 4, ctx->stream));
      if (ns) hipLaunchKernelGGL(k_pg_marks, dim3(div_up(ns, 256)), dim3(256), 0, ctx->stream, a);
      const int rc = scan_counts(ctx, a.ins, a.inscan, ns, ws_off + o_tail);
      if (rc) return rc;
      const dim3 fgrid(div_up(nf + 1, 256));
      hipLaunchKernelGGL(k_pg_files, fgrid, dim3(256), 0, ctx->stream, a);
      hipLaunchKernelGGL(k_pg_scan, dim3(1), dim3(1024), 0, ctx->stream, a);
      hipLaunchKernelGGL(k_pg_off, fgrid, dim3(256), 0, ctx->stream, a);
      if (ns) hipLaunchKernelGGL(k_pg_emit, dim3(div_up(ns, 256)), dim3(256), 0, ctx->stream, a);
    }
    SG_HIP(hipGetLastError());
    SG_HIP(hipMemcpyAsync(&head, a.head, sizeof(head), hipMemcpyDeviceToHost, ctx->stream));
    SG_HIP(hipMemcpyAsync(body_off, a.body_off, (nf + 1) * 8, hipMemcpyDeviceToHost, ctx->stream));
    if (nf) SG_HIP(hipMemcpyAsync(coverage, a.coverage, nf * 4, hipMemcpyDeviceToHost, ctx->stream));
    return SG_OK;
  }

  int counted(bool* more) override {
    sg_ctx* ctx = t->ctx;
    *bad_file = head.bad;
    const uint64_t total = body_off[t->nfiles];  // (0 when a file could not be read)
    *nbytes = (size_t)total;
    if (total == 0 || total > cap) return SG_OK;
    // the bodies in whole chunks, then the tiles' records
    const uint64_t ntiles = (total + kPagesTile - 1) / kPagesTile;
    const size_t o_tiles = align256(ntiles * kPagesTile);
    const size_t need = o_tiles + (ntiles + 1) * 8;
    int rc = ctx->inflate_out.grow_drop(grow_cap(ctx->inflate_out.cap, need, 16u << 20), ctx->stream);
    if (rc) return rc;
    uint8_t* out = ctx->inflate_out.p;
    uint64_t* tile_rec = (uint64_t*)(out + o_tiles);
    {
      ScopedTimer tm(ctx, "pages_tiles");
      hipLaunchKernelGGL(k_pg_tiles, dim3(div_up(ntiles + 1, 256)), dim3(256), 0, ctx->stream, a.rec_pos, head.nrec,
                         ntiles, tile_rec);
    }
    {
      ScopedTimer tm(ctx, "pages_copy");
      hipLaunchKernelGGL(k_pg_copy, dim3((uint32_t)ntiles), dim3(256), 0, ctx->stream, a.lit, a.text, a.rec_pos,
                         a.rec_src, a.rec_len, a.rec_kind, tile_rec, total, out);
    }
    SG_HIP(hipGetLastError());
    SG_HIP(hipMemcpyAsync(bodies, out, total, hipMemcpyDeviceToHost, ctx->stream));
    *more = true;
    return SG_OK;
  }
};

int pages_args_ok(const char* fn, sg_cover_table* t, sg_src_table* src, uint64_t* body_off, uint32_t* coverage,
                  uint8_t* bodies, size_t cap, size_t* nbytes, uint32_t* bad_file) {
  if (!src || !body_off || !coverage || !nbytes || !bad_file) {
    set_error("%s: a null source table or output", fn);
    return SG_EINVAL;
  }
  if (cap && !bodies) {
    set_error("%s: null bodies with a capacity of %zu", fn, cap);
    return SG_EINVAL;
  }
  if (!t->ctx || src->ctx != t->ctx) {
    set_error("%s: the source table belongs to another context", fn);
    return SG_EINVAL;
  }
  if (src->nfiles != t->nfiles) {
    set_error("%s: %u source files for a table of %u", fn, src->nfiles, t->nfiles);
    return SG_EINVAL;
  }
  std::fill(body_off, body_off + (size_t)t->nfiles + 1, 0ull);
  std::fill(coverage, coverage + t->nfiles, 0u);
  *nbytes = 0;
  *bad_file = 0xFFFFFFFFu;
  return SG_OK;
}

int pages_body(sg_cover_table* t, sg_src_table* src, const uint32_t* d_cov, uint64_t ncov, uint32_t base,
               uint64_t* file_off, uint32_t* lines, uint8_t* covered, uint8_t* file_seen, uint64_t* ncovered_frames,
               uint64_t* missing, size_t* nmissing, uint64_t* body_off, uint32_t* coverage, uint8_t* bodies, size_t cap,
               size_t* nbytes, uint32_t* bad_file) {
  PagesTail tail(t, src);
  if (tail.p.overflow) {
    set_error("sg_cover_pages: a buffer plan of more than %d regions", WsPlan::kMaxRegions);
    return SG_EINVAL;
  }
  tail.body_off = body_off;
  tail.coverage = coverage;
  tail.bodies = bodies;
  tail.cap = cap;
  tail.nbytes = nbytes;
  tail.bad_file = bad_file;
  return cover_lines_body(t, d_cov, ncov, base, file_off, lines, covered, file_seen, ncovered_frames, missing, nmissing,
                          &tail);
}

}  // namespace
}  // namespace sg

using namespace sg;

extern "C" {

int sg_src_table_create(sg_ctx* ctx, const uint8_t* have, const uint8_t* bytes, const uint64_t* off, uint32_t nfiles,
                        sg_src_table** out) {
  const char* fn = "sg_src_table_create";
  if (!ctx || !out || !off || (nfiles && !have)) {
    set_error("%s: a null argument", fn);
    return SG_EINVAL;
  }
  *out = nullptr;
  if (off[0] != 0) {
    set_error("%s: off must start at 0", fn);
    return SG_EINVAL;
  }
  for (uint32_t f = 0; f < nfiles; f++) {
    if (off[f + 1] < off[f]) {
      set_error("%s: off must not decrease (file %u)", fn, f);
      return SG_EINVAL;
    }
    if (!have[f] && off[f + 1] != off[f]) {
      set_error("%s: file %u could not be read and has bytes", fn, f);
      return SG_EINVAL;
    }
  }
  const uint64_t nraw = off[nfiles];
  if (nraw >= 1ull << 32) {
    set_error("%s: %llu bytes of sources, at most 2^32 - 1 fit one table", fn, (unsigned long long)nraw);
    return SG_EINVAL;
  }
  if (nraw && !bytes) {
    set_error("%s: null bytes", fn);
    return SG_EINVAL;
  }
  std::vector<uint32_t> off32((size_t)nfiles + 1);
  for (size_t f = 0; f <= nfiles; f++) off32[f] = (uint32_t)off[f];
  uint8_t lits[kLitBytes] = {};
  for (int k = 0; k < 4; k++) memcpy(lits + k * kLitRow + kLitAt, kLits[k], strlen(kLits[k]));

  std::lock_guard<std::mutex> g(ctx->mu);
  int rc = ensure_device(ctx);
  if (rc) return rc;
  sg_src_table* t = new sg_src_table();
  t->ctx = ctx;
  t->nfiles = nfiles;
  t->raw = nraw;
  auto build = [&]() -> int {
    ScopedTimer tm(ctx, "src_table_build");
    const uint64_t nch = (nraw + 15) / 16;
    WsPlan p;
    const size_t o_raw = p.add(nch * 16), o_off = p.add(((uint64_t)nfiles + 1) * 4),
                 o_esc = p.add((uint64_t)nfiles * 4), o_cl = p.add(nch * 4), o_cn = p.add(nch * 4),
                 o_sl = p.add((nch + 1) * 8), o_sn = p.add((nch + 1) * 8);
    int rc = ws_reserve(ctx, p.total + scan_ws_bytes(nch));
    if (rc) return rc;
    SrcArgs a{};
    uint8_t* d_raw = (uint8_t*)ws_at(ctx, o_raw);
    uint32_t* d_off = (uint32_t*)ws_at(ctx, o_off);
    a.raw = d_raw;
    a.off = d_off;
    a.esc_end = (uint32_t*)ws_at(ctx, o_esc);
    a.nraw = nraw;
    a.nfiles = nfiles;
    a.cl = (uint32_t*)ws_at(ctx, o_cl);
    a.cn = (uint32_t*)ws_at(ctx, o_cn);
    a.sl = (uint64_t*)ws_at(ctx, o_sl);
    a.sn = (uint64_t*)ws_at(ctx, o_sn);
    if ((rc = upload(ctx, d_raw, bytes, nraw))) return rc;
    if ((rc = upload(ctx, d_off, off32.data(), off32.size() * 4))) return rc;
    if ((rc = upload(ctx, a.esc_end, off32.data(), (size_t)nfiles * 4))) return rc;
    uint64_t tot[2] = {0, 0};  // stored bytes, lines
    const dim3 grid(div_up(nch, 256));
    if (nch) {
      hipLaunchKernelGGL(k_sp_last, grid, dim3(256), 0, ctx->stream, a, nch);
      hipLaunchKernelGGL(k_sp_count, grid, dim3(256), 0, ctx->stream, a, nch);
      if ((rc = scan_counts(ctx, a.cl, (uint64_t*)a.sl, nch, p.total))) return rc;
      if ((rc = scan_counts(ctx, a.cn, (uint64_t*)a.sn, nch, p.total))) return rc;
      SG_HIP(hipGetLastError());
      SG_HIP(hipMemcpyAsync(&tot[0], a.sl + nch, 8, hipMemcpyDeviceToHost, ctx->stream));
      SG_HIP(hipMemcpyAsync(&tot[1], a.sn + nch, 8, hipMemcpyDeviceToHost, ctx->stream));
    }
    SG_HIP(hipStreamSynchronize(ctx->stream));  // (the host arrays are the caller's again)
    if (tot[0] >= 1ull << 32) {
      set_error("%s: %llu bytes of escaped text, at most 2^32 - 1 fit one table", fn, (unsigned long long)tot[0]);
      return SG_EINVAL;
    }
    t->stored = tot[0];
    t->nlines = tot[1];
    WsPlan bp;
    const size_t o_lit = bp.add(kLitBytes), o_text = bp.add(kTextPad + t->stored + kTextPad),
                 o_lo = bp.add((t->nlines + 1) * 4), o_fl = bp.add(((uint64_t)nfiles + 1) * 4), o_hv = bp.add(nfiles);
    if ((rc = t->mem.grow_drop(bp.total, nullptr))) return rc;
    char* b = t->mem.p;
    t->lit = (const uint8_t*)(b + o_lit);
    t->text = (uint8_t*)(b + o_text + kTextPad);
    t->line_off = (uint32_t*)(b + o_lo);
    t->file_line = (uint32_t*)(b + o_fl);
    t->have = (uint8_t*)(b + o_hv);
    a.text = t->text;
    a.line_off = t->line_off;
    a.file_line = t->file_line;
    if ((rc = upload(ctx, b + o_lit, lits, kLitBytes))) return rc;
    if ((rc = upload(ctx, t->have, have, nfiles))) return rc;
    SG_HIP(hipMemsetAsync(b + o_text, 0, kTextPad, ctx->stream));
    SG_HIP(hipMemsetAsync(t->text + t->stored, 0, kTextPad, ctx->stream));
    SG_HIP(hipMemsetAsync(t->line_off, 0, 4, ctx->stream));
    if (nch) hipLaunchKernelGGL(k_sp_write, grid, dim3(256), 0, ctx->stream, a, nch);
    hipLaunchKernelGGL(k_sp_tail, dim3(div_up((uint64_t)nfiles + 1, 256)), dim3(256), 0, ctx->stream, a,
                       (uint32_t)t->nlines);
    SG_HIP(hipGetLastError());
    t->h_file_line.resize((size_t)nfiles + 1);
    SG_HIP(hipMemcpyAsync(t->h_file_line.data(), t->file_line, ((size_t)nfiles + 1) * 4, hipMemcpyDeviceToHost,
                          ctx->stream));
    SG_HIP(hipStreamSynchronize(ctx->stream));
    return SG_OK;
  };
  rc = build();
  if (rc) {
    (void)hipStreamSynchronize(ctx->stream);
    delete t;
    return rc;
  }
  *out = t;
  return SG_OK;
}

void sg_src_table_destroy(sg_src_table* src) {
  if (!src) return;
  {
    std::lock_guard<std::mutex> g(src->ctx->mu);
    hipSetDevice(src->ctx->device);
    hipStreamSynchronize(src->ctx->stream);
  }
  delete src;
}

int sg_src_table_counts(sg_src_table* src, uint64_t* file_line_off, uint64_t totals[3]) {
  if (!src || !file_line_off || !totals) {
    set_error("sg_src_table_counts: a null argument");
    return SG_EINVAL;
  }
  std::copy(src->h_file_line.begin(), src->h_file_line.end(), file_line_off);
  totals[0] = src->nlines;
  totals[1] = src->stored;
  totals[2] = src->raw;
  return SG_OK;
}

int sg_src_table_export(sg_src_table* src, uint64_t* line_off, uint8_t* text) {
  if (!src || !line_off || (src->stored && !text)) {
    set_error("sg_src_table_export: a null argument");
    return SG_EINVAL;
  }
  sg_ctx* ctx = src->ctx;
  std::lock_guard<std::mutex> g(ctx->mu);
  const int rc = ensure_device(ctx);
  if (rc) return rc;
  std::vector<uint32_t> lo(src->nlines + 1);
  SG_HIP(hipMemcpyAsync(lo.data(), src->line_off, lo.size() * 4, hipMemcpyDeviceToHost, ctx->stream));
  if (src->stored) SG_HIP(hipMemcpyAsync(text, src->text, src->stored, hipMemcpyDeviceToHost, ctx->stream));
  SG_HIP(hipStreamSynchronize(ctx->stream));
  std::copy(lo.begin(), lo.end(), line_off);
  return SG_OK;
}

int sg_cover_pages(sg_cover_table* t, sg_src_table* src, const uint32_t* cov, size_t ncov, uint32_t base,
                   uint64_t* file_off, uint32_t* lines, uint8_t* covered, uint8_t* file_seen, uint64_t* ncovered_frames,
                   uint64_t* missing, size_t* nmissing, uint64_t* body_off, uint32_t* coverage, uint8_t* bodies,
                   size_t cap, size_t* nbytes, uint32_t* bad_file) {
  const char* fn = "sg_cover_pages";
  int rc = lines_args_ok(fn, t, file_off, lines, covered, ncovered_frames, missing, nmissing);
  if (rc) return rc;
  if (ncov && !cov) {
    set_error("%s: null cov", fn);
    return SG_EINVAL;
  }
  if (ncov >= 0xFFFFFFFFull) {
    set_error("%s: too many PCs for one call", fn);
    return SG_EINVAL;
  }
  rc = pages_args_ok(fn, t, src, body_off, coverage, bodies, cap, nbytes, bad_file);
  if (rc) return rc;
  lines_empty(t, file_off, file_seen, ncovered_frames, nmissing);
  if (ncov == 0) return SG_OK;
  sg_ctx* ctx = t->ctx;
  std::lock_guard<std::mutex> g(ctx->mu);
  rc = ensure_device(ctx);
  if (rc) return rc;
  rc = dstage_reserve(ctx, ncov * 4);
  if (rc) return rc;
  uint32_t* dcov = dstage_at<uint32_t>(ctx, 0);
  rc = upload(ctx, dcov, cov, ncov * 4);
  if (rc) return rc;
  return pages_body(t, src, dcov, ncov, base, file_off, lines, covered, file_seen, ncovered_frames, missing, nmissing,
                    body_off, coverage, bodies, cap, nbytes, bad_file);
}

int sg_cover_pages_set(sg_cover_table* t, sg_src_table* src, sg_set* cov, uint32_t base, uint64_t* file_off,
                       uint32_t* lines, uint8_t* covered, uint8_t* file_seen, uint64_t* ncovered_frames,
                       uint64_t* missing, size_t* nmissing, uint64_t* body_off, uint32_t* coverage, uint8_t* bodies,
                       size_t cap, size_t* nbytes, uint32_t* bad_file) {
  const char* fn = "sg_cover_pages_set";
  int rc = lines_args_ok(fn, t, file_off, lines, covered, ncovered_frames, missing, nmissing);
  if (rc) return rc;
  if (!cov) {
    set_error("%s: null set", fn);
    return SG_EINVAL;
  }
  if (!t->ctx || cov->ctx != t->ctx) {
    set_error("%s: the set belongs to another context", fn);
    return SG_EINVAL;
  }
  rc = pages_args_ok(fn, t, src, body_off, coverage, bodies, cap, nbytes, bad_file);
  if (rc) return rc;
  lines_empty(t, file_off, file_seen, ncovered_frames, nmissing);
  sg_ctx* ctx = t->ctx;
  std::lock_guard<std::mutex> g(ctx->mu);
  rc = ensure_device(ctx);
  if (rc) return rc;
  uint64_t total = 0;
  rc = lines_set_cover(fn, ctx, cov, &total);
  if (rc) return rc;
  if (total == 0) return SG_OK;
  return pages_body(t, src, dstage_at<uint32_t>(ctx, 0), total, base, file_off, lines, covered, file_seen,
                    ncovered_frames, missing, nmissing, body_off, coverage, bodies, cap, nbytes, bad_file);
}

}  // extern "C"
