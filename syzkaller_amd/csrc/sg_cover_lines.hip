// sg_cover_lines.hip -- the /cover page's line tables: cover -> fileSet.
//
// Reference: syz-manager/html.go:169-194 (httpCover takes mgr.mu and holds it
// across generateCoverHtml), syz-manager/cover.go:91-120 (generateCoverHtml:
// pcs[i] = RestorePC(cov[i], base) - callLen, uncoveredPcsInFuncs, then two
// symbolize passes over the covered and the uncovered PCs) and cover.go:165-196
// (fileSet):
//
//   for f in coveredFrames:   files[f.File][f.Line] = true; funcs[f.Func] = true
//   for f in uncoveredFrames: if !funcs[f.Func] continue
//                             files[f.File][f.Line] |= false      (true wins)
//   per file: the lines, sorted
//
// The frames of a PC depend on vmlinux alone and the PCs a report can ask
// about are known at start-up (allCoverPCs, cover.go:64-89), so they are
// symbolised once into a frame table that stays on the device
// (sg_cover_table).  Every distinct (file, line) of the table is a slot, the
// slots ordered by file, then line: fileSet's output order.  A report is then
//
//   k_cl_rows     per query: its row of tab_pcs through a radix index; a byte
//                 per covered row, the PCs not found appended to `missing`
//   report_query  sg_report.hip's pipeline on the table's arrays: the per-site
//                 uncovered flag, left on the device
//   k_cl_cov      per covered row, over its frames: OR the func bit, the
//                 slot's covered bit and the file's seen bit 0; count frames
//   k_cl_unc      per uncovered site, over its frames (after k_cl_cov: it
//                 reads funcs): OR seen bit 1 and, when the func bit is set,
//                 the slot's uncovered bit
//   k_cl_count / scan / k_cl_scatter
//                 ordered compaction of the slots with cov | unc set into
//                 lines[] / covered[]: ballot-style masks per chunk of 256
//                 slots (the bitmaps are the masks), a scan of the chunk
//                 counts, a wave per chunk writing its slots in order
//   k_cl_files    per file: file_off[f] = the rank of its first slot; seen byte
//
// No kernel sorts: slot order is output order.  Header lines of inlined
// helpers are hit from thousands of sites, so every OR tests the bit first.
#include "sg_cover_lines.h"
#include "sg_rank.h"

#include <algorithm>
#include <vector>

namespace sg {

constexpr uint32_t kSlotChunk = 256;  // slots per wave of the compaction: four 64-bit mask words
constexpr uint32_t kSlotWaves = 4;    // waves (chunks) per workgroup: a tile of 1024 slots

// ---- table build ----------------------------------------------------------------
__global__ void k_ct_keys(const uint32_t* __restrict__ file, const uint32_t* __restrict__ line, uint64_t n,
                          uint64_t* __restrict__ key) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) key[i] = ((uint64_t)file[i] << 32) | line[i];
}

// the distinct keys, ascending, and each slot's line
__global__ void k_ct_distinct(const uint64_t* __restrict__ sorted, const uint32_t* __restrict__ first,
                              const uint64_t* __restrict__ pos, uint64_t n, uint64_t* __restrict__ dkeys,
                              uint32_t* __restrict__ slot_line) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n && first[i]) {
    dkeys[pos[i]] = sorted[i];
    slot_line[pos[i]] = (uint32_t)sorted[i];
  }
}

// a frame's slot: the rank of its key among the distinct ones (pos[n] of them)
__global__ void k_ct_frame_slot(const uint32_t* __restrict__ file, const uint32_t* __restrict__ line, uint64_t n,
                                const uint64_t* __restrict__ dkeys, const uint64_t* __restrict__ pos,
                                uint32_t* __restrict__ frame_slot) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) frame_slot[i] = (uint32_t)sgd::lb64(dkeys, pos[n], ((uint64_t)file[i] << 32) | line[i]);
}

// file f's slots start at the first key >= f << 32 (f == nfiles: all of them)
__global__ void k_ct_file_off(const uint64_t* __restrict__ dkeys, const uint64_t* __restrict__ pos, uint64_t n,
                              uint32_t nfiles, uint32_t* __restrict__ file_slot_off) {
  const uint64_t f = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (f <= nfiles) file_slot_off[f] = (uint32_t)sgd::lb64(dkeys, pos[n], f << 32);
}

// each call site's row of tab (every site is there: checked on the host)
__global__ void k_ct_site_row(const uint64_t* __restrict__ sites, uint64_t nall, const uint64_t* __restrict__ tab,
                              uint64_t ntab, RadixIdx itab, uint32_t* __restrict__ site_row) {
  const uint64_t s = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (s < nall) site_row[s] = (uint32_t)lb_idx(tab, ntab, itab, sites[s]);
}

// The device-resident sources of a table (cover_table_from_dev): what the host checks of sg_cover_table_create
// for host arrays, here one flag word each, read after the build's one wait.  bad[0]: tab is not strictly
// ascending; bad[1]: a call site is not in tab; bad[2]: a line is 0 or does not fit 32 bits, an id is out of range
// or frame_off decreases or ends elsewhere than at nfr.
__global__ void k_ct_dev_tab(const uint64_t* __restrict__ tab, uint64_t ntab, const uint64_t* __restrict__ sites,
                             uint64_t nall, const uint64_t* __restrict__ off64, uint64_t nfr,
                             uint32_t* __restrict__ off32, uint32_t* __restrict__ bad) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < ntab && i && tab[i] <= tab[i - 1]) bad[0] = 1;
  if (i <= ntab) {
    const uint64_t o = off64[i];
    off32[i] = (uint32_t)min(o, nfr);
    if (o > nfr || (i == 0 && o != 0) || (i == ntab && o != nfr) || (i && o < off64[i - 1])) bad[2] = 1;
  }
  if (i < nall) {
    const uint64_t j = sgd::lb64(tab, ntab, sites[i]);
    if (j >= ntab || tab[j] != sites[i]) bad[1] = 1;
  }
}
__global__ void k_ct_dev_frames(const int64_t* __restrict__ line64, const uint32_t* __restrict__ file,
                                const uint32_t* __restrict__ func, uint64_t nfr, uint32_t nfiles, uint32_t nfuncs,
                                uint32_t* __restrict__ line32, uint32_t* __restrict__ bad) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= nfr) return;
  const int64_t v = line64[i];
  line32[i] = (uint32_t)v;
  if (v <= 0 || v > 0xFFFFFFFFll || file[i] >= nfiles || func[i] >= nfuncs) bad[2] = 1;
}

// ---- the report -------------------------------------------------------------------
struct LinesArgs {
  const uint32_t* cov;
  uint64_t ncov, hi32;
  const uint64_t* tab;
  uint64_t ntab;
  RadixIdx itab;
  const uint32_t *site_row, *frame_off, *frame_slot, *frame_func, *frame_file, *slot_line, *file_slot_off;
  uint64_t nall, nslots;
  uint32_t nfiles, nchunks;
  const uint8_t* flag;  // [nall] uncovered, from report_query
  uint8_t* rowcov;      // [ntab]
  uint32_t* funcs;      // bitmap over func ids
  uint32_t* fseen;      // [nfiles] bit 0 covered, bit 1 uncovered (before the funcs filter)
  uint32_t *covbits, *uncbits;  // bitmaps over slots, 8 words per chunk
  unsigned long long* counters;  // [0] covered frames, [1] missing
  uint64_t* missing;    // [ncov]
  uint32_t* ccnt;       // [nchunks]
  uint64_t* cbase;      // [nchunks + 1]
  uint32_t* out_lines;
  uint8_t* out_cov;
  uint64_t* out_foff;   // [nfiles + 1]
  uint8_t* out_fseen;   // [nfiles]
};

__device__ __forceinline__ void or_bit(uint32_t* words, uint32_t i) {
  const uint32_t b = 1u << (i & 31);
  if (!(words[i >> 5] & b)) atomicOr(&words[i >> 5], b);
}
__device__ __forceinline__ void or_word(uint32_t* w, uint32_t b) {
  if ((*w & b) != b) atomicOr(w, b);
}

// Per query its row of tab: a byte per covered row (same-value stores race
// benignly), a PC not in the table appended to missing (at most one append
// per query: ncov slots suffice).  Grid-stride.
__global__ __launch_bounds__(256) void k_cl_rows(LinesArgs a) {
  const uint64_t S = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < a.ncov; i += S) {
    const uint64_t pc = query_pc(a.hi32, a.cov[i]);
    const uint64_t j = a.ntab ? lb_idx(a.tab, a.ntab, a.itab, pc) : 0;
    if (j < a.ntab && a.tab[j] == pc) {
      if (!a.rowcov[j]) a.rowcov[j] = 1;
    } else {
      a.missing[atomicAdd(&a.counters[1], 1ull)] = pc;
    }
  }
}

// Per covered row, over its frames.  Every lane stays to the end: the frame
// count is summed over the wave and added once.
__global__ __launch_bounds__(256) void k_cl_cov(LinesArgs a) {
  const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  uint32_t nfr = 0;
  if (j < a.ntab && a.rowcov[j]) {
    const uint32_t f0 = a.frame_off[j], f1 = a.frame_off[j + 1];
    nfr = f1 - f0;
    for (uint32_t f = f0; f < f1; f++) {
      or_bit(a.funcs, a.frame_func[f]);
      or_bit(a.covbits, a.frame_slot[f]);
      or_word(&a.fseen[a.frame_file[f]], 1u);
    }
  }
  const uint32_t sum = sgd::wave_incl_add(nfr);
  if ((threadIdx.x & 63) == 63 && sum) atomicAdd(&a.counters[0], (unsigned long long)sum);
}

// Per uncovered site, over its frames; runs after k_cl_cov has completed (a
// later launch on the stream), because it reads funcs.
__global__ __launch_bounds__(256) void k_cl_unc(LinesArgs a) {
  const uint64_t s = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= a.nall || !a.flag[s]) return;
  const uint32_t j = a.site_row[s];
  for (uint32_t f = a.frame_off[j], f1 = a.frame_off[j + 1]; f < f1; f++) {
    or_word(&a.fseen[a.frame_file[f]], 2u);
    const uint32_t fn = a.frame_func[f];
    if ((a.funcs[fn >> 5] >> (fn & 31)) & 1u) or_bit(a.uncbits, a.frame_slot[f]);
  }
}

// chunk c's mask word k (slots 256 c + 64 k ..): the bitmaps are padded to whole chunks
__device__ __forceinline__ uint64_t slot_mask(const LinesArgs& a, uint64_t c, uint32_t k) {
  const uint64_t w = c * 8 + 2 * k;
  return ((uint64_t)(a.covbits[w + 1] | a.uncbits[w + 1]) << 32) | (a.covbits[w] | a.uncbits[w]);
}

__global__ void k_cl_count(LinesArgs a) {
  const uint64_t c = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= a.nchunks) return;
  uint32_t n = 0;
  for (uint32_t k = 0; k < 4; k++) n += __popcll(slot_mask(a, c, k));
  a.ccnt[c] = n;
}

// a wave per chunk: lane l takes slots 64 k + l, k < 4, each written at the
// chunk's base plus the set slots below it
__global__ __launch_bounds__(64 * kSlotWaves) void k_cl_scatter(LinesArgs a) {
  const uint32_t lane = threadIdx.x & 63;
  const uint64_t c = (uint64_t)blockIdx.x * kSlotWaves + (threadIdx.x >> 6);
  if (c >= a.nchunks) return;
  const uint64_t lt = lane ? (~0ull >> (64 - lane)) : 0ull;
  uint64_t at = a.cbase[c];
  for (uint32_t k = 0; k < 4; k++) {
    const uint64_t m = slot_mask(a, c, k);
    if ((m >> lane) & 1ull) {
      const uint64_t slot = c * kSlotChunk + 64 * k + lane;  // (< nslots: no bit is set past it)
      const uint64_t o = at + __popcll(m & lt);
      a.out_lines[o] = a.slot_line[slot];
      a.out_cov[o] = (uint8_t)((a.covbits[slot >> 5] >> (slot & 31)) & 1u);
    }
    at += __popcll(m);
  }
}

// file_off[f] = the set slots below file f's first slot; file_seen
__global__ void k_cl_files(LinesArgs a) {
  const uint64_t f = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (f > a.nfiles) return;
  uint64_t r = 0;
  if (a.nslots) {
    const uint64_t s = a.file_slot_off[f];
    if (s >= a.nslots) {
      r = a.cbase[a.nchunks];
    } else {
      const uint64_t c = s / kSlotChunk;
      const uint32_t in = (uint32_t)(s % kSlotChunk);
      r = a.cbase[c];
      for (uint32_t k = 0; k < 4; k++) {
        const uint64_t m = slot_mask(a, c, k);
        if (in >= 64 * (k + 1))
          r += __popcll(m);
        else if (in > 64 * k)
          r += __popcll(m & (~0ull >> (64 - (in - 64 * k))));
      }
    }
  }
  a.out_foff[f] = r;
  if (f < a.nfiles) a.out_fseen[f] = (uint8_t)a.fseen[f];
}


// (sg_cover_lines.h)
int cover_lines_body(sg_cover_table* t, const uint32_t* d_cov, uint64_t ncov, uint32_t base, uint64_t* file_off,
                     uint32_t* lines, uint8_t* covered, uint8_t* file_seen, uint64_t* ncovered_frames,
                     uint64_t* missing, size_t* nmissing, LinesTail* tail) {
  sg_ctx* ctx = t->ctx;
  const uint64_t nslots = t->nslots, nfiles = t->nfiles;
  const uint32_t nchunks = div_up(nslots, kSlotChunk);
  const bool chunked = t->has_rep && t->rep.chunks && ctx->opt[kOptReportDirect] <= 0;
  WsPlan p;
  RepQueryOff qo{};
  if (t->has_rep) report_query_plan(p, t->rep, ncov, chunked, qo);
  // zeroed per call, as one range: rowcov .. counters
  const size_t o_rc = p.add(t->ntab), o_fn = p.add(((uint64_t)t->nfuncs + 31) / 32 * 4), o_fs = p.add(nfiles * 4),
               o_cb = p.add((uint64_t)nchunks * 32), o_ub = p.add((uint64_t)nchunks * 32), o_ct = p.add(16);
  const size_t o_zend = p.total;
  const size_t o_ms = p.add(ncov * 8), o_cc = p.add((uint64_t)nchunks * 4), o_bs = p.add(((uint64_t)nchunks + 1) * 8),
               o_ol = p.add(nslots * 4), o_oc = p.add(nslots), o_of = p.add((nfiles + 1) * 8), o_os = p.add(nfiles);
  const size_t scan_off = p.total;
  const size_t scan_tail =
      std::max(scan_ws_bytes(nchunks), t->has_rep ? report_query_scan_bytes(t->rep, ncov, chunked) : 0);
  if (p.overflow) {
    set_error("sg_cover_lines: a buffer plan of more than %d regions", WsPlan::kMaxRegions);
    return SG_EINVAL;
  }
  const size_t tail_off = align256(p.total + scan_tail);
  int rc = ws_reserve(ctx, tail ? tail_off + tail->ws_bytes : p.total + scan_tail);
  if (rc) return rc;
  LinesArgs a{};
  a.cov = d_cov;
  a.ncov = ncov;
  a.hi32 = (uint64_t)base << 32;
  a.tab = t->tab;
  a.ntab = t->ntab;
  a.itab = t->itab;
  a.site_row = t->site_row;
  a.frame_off = t->frame_off;
  a.frame_slot = t->frame_slot;
  a.frame_func = t->frame_func;
  a.frame_file = t->frame_file;
  a.slot_line = t->slot_line;
  a.file_slot_off = t->file_slot_off;
  a.nall = t->nall;
  a.nslots = nslots;
  a.nfiles = t->nfiles;
  a.nchunks = nchunks;
  a.rowcov = (uint8_t*)ws_at(ctx, o_rc);
  a.funcs = (uint32_t*)ws_at(ctx, o_fn);
  a.fseen = (uint32_t*)ws_at(ctx, o_fs);
  a.covbits = (uint32_t*)ws_at(ctx, o_cb);
  a.uncbits = (uint32_t*)ws_at(ctx, o_ub);
  a.counters = (unsigned long long*)ws_at(ctx, o_ct);
  a.missing = (uint64_t*)ws_at(ctx, o_ms);
  a.ccnt = (uint32_t*)ws_at(ctx, o_cc);
  a.cbase = (uint64_t*)ws_at(ctx, o_bs);
  a.out_lines = (uint32_t*)ws_at(ctx, o_ol);
  a.out_cov = (uint8_t*)ws_at(ctx, o_oc);
  a.out_foff = (uint64_t*)ws_at(ctx, o_of);
  a.out_fseen = (uint8_t*)ws_at(ctx, o_os);
  SG_HIP(hipMemsetAsync(a.rowcov, 0, o_zend - o_rc, ctx->stream));
  {
    ScopedTimer tm(ctx, "lines_rows");
    hipLaunchKernelGGL(k_cl_rows, dim3(std::min<uint32_t>(div_up(ncov, 256), 8192)), dim3(256), 0, ctx->stream, a);
  }
  if (t->has_rep) {
    uint8_t* flag = nullptr;
    rc = report_query(ctx, t->rep, d_cov, ncov, base, chunked, qo, scan_off, &flag);
    if (rc) return rc;
    a.flag = flag;
  }
  if (t->ntab) {
    ScopedTimer tm(ctx, "lines_cov");
    hipLaunchKernelGGL(k_cl_cov, dim3(div_up(t->ntab, 256)), dim3(256), 0, ctx->stream, a);
  }
  if (t->has_rep) {
    ScopedTimer tm(ctx, "lines_unc");
    hipLaunchKernelGGL(k_cl_unc, dim3(div_up(t->nall, 256)), dim3(256), 0, ctx->stream, a);
  }
  {
    ScopedTimer tm(ctx, "lines_compact");
    if (nchunks) {
      hipLaunchKernelGGL(k_cl_count, dim3(div_up(nchunks, 256)), dim3(256), 0, ctx->stream, a);
      rc = scan_counts(ctx, a.ccnt, a.cbase, nchunks, scan_off);
      if (rc) return rc;
      hipLaunchKernelGGL(k_cl_scatter, dim3(div_up(nchunks, kSlotWaves)), dim3(64 * kSlotWaves), 0, ctx->stream, a);
    }
    hipLaunchKernelGGL(k_cl_files, dim3(div_up(nfiles + 1, 256)), dim3(256), 0, ctx->stream, a);
  }
  SG_HIP(hipGetLastError());
  if (tail && (rc = tail->queued(LinesDev{a.out_foff, a.out_lines, a.out_cov}, tail_off))) return rc;
  // one wait for the counts, then the results
  uint64_t cnt[2] = {0, 0};
  SG_HIP(hipMemcpyAsync(cnt, a.counters, 16, hipMemcpyDeviceToHost, ctx->stream));
  SG_HIP(hipMemcpyAsync(file_off, a.out_foff, (nfiles + 1) * 8, hipMemcpyDeviceToHost, ctx->stream));
  if (file_seen && nfiles) SG_HIP(hipMemcpyAsync(file_seen, a.out_fseen, nfiles, hipMemcpyDeviceToHost, ctx->stream));
  SG_HIP(hipStreamSynchronize(ctx->stream));
  bool more = false;
  if (tail && (rc = tail->counted(&more))) return rc;
  const uint64_t total = file_off[nfiles];
  if (total) {
    SG_HIP(hipMemcpyAsync(lines, a.out_lines, total * 4, hipMemcpyDeviceToHost, ctx->stream));
    SG_HIP(hipMemcpyAsync(covered, a.out_cov, total, hipMemcpyDeviceToHost, ctx->stream));
  }
  std::vector<uint64_t> miss(cnt[1]);  // one entry per query that missed
  if (cnt[1]) SG_HIP(hipMemcpyAsync(miss.data(), a.missing, cnt[1] * 8, hipMemcpyDeviceToHost, ctx->stream));
  if (total || cnt[1] || more) SG_HIP(hipStreamSynchronize(ctx->stream));
  if (cnt[1]) {
    // sorted and de-duplicated only when there are any, on the host: the
    // caller is about to run addr2line over them
    std::sort(miss.begin(), miss.end());
    miss.erase(std::unique(miss.begin(), miss.end()), miss.end());
    std::copy(miss.begin(), miss.end(), missing);
    cnt[1] = miss.size();
  }
  *ncovered_frames = cnt[0];
  *nmissing = (size_t)cnt[1];
  return SG_OK;
}

int lines_args_ok(const char* fn, sg_cover_table* t, uint64_t* file_off, uint32_t* lines, uint8_t* covered,
                  uint64_t* ncovered_frames, uint64_t* missing, size_t* nmissing) {
  if (!t || !file_off || !lines || !covered || !ncovered_frames || !missing || !nmissing) {
    set_error("%s: a null table or output", fn);
    return SG_EINVAL;
  }
  return SG_OK;
}

void lines_empty(sg_cover_table* t, uint64_t* file_off, uint8_t* file_seen, uint64_t* ncovered_frames,
                 size_t* nmissing) {
  std::fill(file_off, file_off + (size_t)t->nfiles + 1, 0ull);
  if (file_seen) std::fill(file_seen, file_seen + t->nfiles, (uint8_t)0);
  *ncovered_frames = 0;
  *nmissing = 0;
}

// (sg_cover_lines.h)
int lines_set_cover(const char* fn, sg_ctx* ctx, sg_set* cov, uint64_t* total) {
  // the members, ascending (the reference's canonical cover order), into the
  // staging buffer: nothing is uploaded.  The member count is a wait of its
  // own; a set that outgrows the buffer is exported a second time.
  int rc = dstage_reserve(ctx, 4);
  if (rc) return rc;
  *total = 0;
  for (int pass = 0; pass < 2; pass++) {
    rc = set_export_dev(cov, dstage_at<uint32_t>(ctx, 0), ctx->dstage.cap / 4, total);
    if (rc) return rc;
    if (*total * 4 <= ctx->dstage.cap) break;
    rc = dstage_reserve(ctx, *total * 4);
    if (rc) return rc;
  }
  if (*total >= 0xFFFFFFFFull) {
    set_error("%s: too many PCs for one call", fn);
    return SG_EINVAL;
  }
  return SG_OK;
}

}  // namespace sg

using namespace sg;

extern "C" {

int sg_cover_table_create(sg_ctx* ctx, const uint64_t* sym_start, const uint64_t* sym_end, size_t nsym,
                          const uint64_t* all_pcs, size_t nall, const uint64_t* tab_pcs, size_t ntab,
                          const uint64_t* frame_off, const uint32_t* frame_file, const uint32_t* frame_line,
                          const uint32_t* frame_func, uint32_t nfiles, uint32_t nfuncs, sg_cover_table** out) {
  const char* fn = "sg_cover_table_create";
  if (!ctx || !out || !frame_off || (nsym && (!sym_start || !sym_end)) || (nall && !all_pcs) || (ntab && !tab_pcs)) {
    set_error("%s: a null argument", fn);
    return SG_EINVAL;
  }
  *out = nullptr;
  const uint64_t lim = 0xFFFFFFFFull;
  if (ntab >= lim || nfiles >= lim || nfuncs >= lim) {
    set_error("%s: too many symbols, call sites, PCs, files or funcs for one table", fn);
    return SG_EINVAL;
  }
  if (int rc0 = table_syms_ok(fn, sym_start, sym_end, nsym, all_pcs, nall)) return rc0;
  for (size_t j = 1; j < ntab; j++)
    if (tab_pcs[j] <= tab_pcs[j - 1]) {
      set_error("%s: table PCs must be sorted and unique", fn);
      return SG_EINVAL;
    }
  if (frame_off[0] != 0) {
    set_error("%s: frame_off must start at 0", fn);
    return SG_EINVAL;
  }
  for (size_t j = 0; j < ntab; j++)
    if (frame_off[j + 1] < frame_off[j]) {
      set_error("%s: frame_off must not decrease", fn);
      return SG_EINVAL;
    }
  const uint64_t nfr = frame_off[ntab];
  if (nfr >= lim) {
    set_error("%s: too many frames for one table", fn);
    return SG_EINVAL;
  }
  if (nfr && (!frame_file || !frame_line || !frame_func)) {
    set_error("%s: a null frame array", fn);
    return SG_EINVAL;
  }
  uint64_t k_and = ~0ull, k_or = 0;
  for (uint64_t f = 0; f < nfr; f++) {
    if (frame_file[f] >= nfiles || frame_func[f] >= nfuncs || frame_line[f] == 0) {
      set_error("%s: frame %llu has a file or func id out of range, or line 0", fn, (unsigned long long)f);
      return SG_EINVAL;
    }
    const uint64_t key = ((uint64_t)frame_file[f] << 32) | frame_line[f];
    k_and &= key;
    k_or |= key;
  }
  for (size_t s = 0, j = 0; s < nall; s++) {  // the table is built by symbolising the call sites
    while (j < ntab && tab_pcs[j] < all_pcs[s]) j++;
    if (j == ntab || tab_pcs[j] != all_pcs[s]) {
      set_error("%s: call site 0x%llx is not in the table", fn, (unsigned long long)all_pcs[s]);
      return SG_EINVAL;
    }
  }
  std::lock_guard<std::mutex> g(ctx->mu);
  int rc = ensure_device(ctx);
  if (rc) return rc;
  const TableSrc src{tab_pcs, frame_off, frame_file, frame_line, frame_func, nullptr, k_and ^ k_or};
  return table_build(ctx, fn, sym_start, sym_end, nsym, all_pcs, nall, ntab, ntab ? tab_pcs[0] : 0,
                     ntab ? tab_pcs[ntab - 1] : 0, nfr, nfiles, nfuncs, src, out);
}

}  // extern "C"

namespace sg {

int table_syms_ok(const char* fn, const uint64_t* sym_start, const uint64_t* sym_end, size_t nsym, const uint64_t* all_pcs,
                  size_t nall) {
  if (nsym >= 0xFFFFFFFFull || nall >= 0xFFFFFFFFull) {
    set_error("%s: too many symbols, call sites, PCs, files or funcs for one table", fn);
    return SG_EINVAL;
  }
  for (size_t s = 1; s < nsym; s++)
    if (sym_start[s] < sym_start[s - 1] || sym_end[s] < sym_end[s - 1]) {
      set_error("%s: symbols must be sorted by start with non-decreasing ends", fn);
      return SG_EINVAL;
    }
  for (size_t j = 1; j < nall; j++)
    if (all_pcs[j] <= all_pcs[j - 1]) {
      set_error("%s: call-site PCs must be sorted and unique", fn);
      return SG_EINVAL;
    }
  return SG_OK;
}

// The table from checked arguments (ctx lock held, the device ensured).  With src.dev the table PCs and the frame
// arrays are device memory and are checked there: SG_EINVAL after the one wait, no table.
int table_build(sg_ctx* ctx, const char* fn, const uint64_t* sym_start, const uint64_t* sym_end, size_t nsym,
                const uint64_t* all_pcs, size_t nall, size_t ntab, uint64_t tab_lo, uint64_t tab_hi, uint64_t nfr,
                uint32_t nfiles, uint32_t nfuncs, const TableSrc& src, sg_cover_table** out) {
  const CoverTableDev* dev = src.dev;
  const uint64_t* tab_pcs = src.tab_pcs;
  const uint64_t* frame_off = src.frame_off;
  const uint32_t *frame_file = src.frame_file, *frame_line = src.frame_line, *frame_func = src.frame_func;
  int rc = SG_OK;
  sg_cover_table* t = new sg_cover_table();
  t->ctx = ctx;
  t->has_rep = nsym && nall;
  t->nsym = nsym;
  t->nall = nall;
  t->ntab = ntab;
  t->nfr = nfr;
  t->nfiles = nfiles;
  t->nfuncs = nfuncs;
  // the block: the report's tables, then the frame table
  WsPlan bp;
  RepTablesOff to{};
  if (t->has_rep) report_tables_plan(bp, sym_start, sym_end, nsym, all_pcs, nall, report_chunkable(nall), t->rep, to);
  if (ntab) radix_index_plan(ntab, tab_lo, tab_hi, t->itab);
  const size_t o_tab = bp.add(ntab * 8), o_it = bp.add(ntab ? ((uint64_t)t->itab.nb + 1) * 4 : 4),
               o_row = bp.add(nall * 4), o_fo = bp.add(((uint64_t)ntab + 1) * 4), o_sl = bp.add(nfr * 4),
               o_fu = bp.add(nfr * 4), o_fi = bp.add(nfr * 4), o_ln = bp.add(nfr * 4),  // (nslots <= nfr)
               o_fso = bp.add(((uint64_t)nfiles + 1) * 4);
  rc = t->mem.grow_drop(bp.total, nullptr);
  if (rc) {
    delete t;
    return rc;
  }
  char* b = t->mem.p;
  if (t->has_rep) report_tables_bind(b, to, t->rep);
  t->tab = (uint64_t*)(b + o_tab);
  t->itab.r = (const uint32_t*)(b + o_it);
  t->site_row = (uint32_t*)(b + o_row);
  t->frame_off = (uint32_t*)(b + o_fo);
  t->frame_slot = (uint32_t*)(b + o_sl);
  t->frame_func = (uint32_t*)(b + o_fu);
  t->frame_file = (uint32_t*)(b + o_fi);
  t->slot_line = (uint32_t*)(b + o_ln);
  t->file_slot_off = (uint32_t*)(b + o_fso);
  std::vector<uint32_t> fo32(dev ? 0 : ntab + 1);  // (< 2^32 - 1 frames)
  for (size_t j = 0; j < fo32.size(); j++) fo32[j] = (uint32_t)frame_off[j];
  uint32_t bad[4] = {0, 0, 0, 0};
  auto build = [&]() -> int {
    ScopedTimer tm(ctx, "cover_table_build");
    int rc = SG_OK;
    if (t->has_rep) {
      if ((rc = upload(ctx, t->rep.sstart, sym_start, nsym * 8))) return rc;
      if ((rc = upload(ctx, t->rep.send, sym_end, nsym * 8))) return rc;
      if ((rc = upload(ctx, t->rep.pcs, all_pcs, nall * 8))) return rc;
      if ((rc = report_tables_build(ctx, t->rep, true))) return rc;
    }
    uint32_t* d_bad = nullptr;
    if (dev) {  // (the sources lie in the workspace behind dev->ws_base, which cover_table_build_ws has made room for)
      d_bad = (uint32_t*)t->site_row;  // (free until k_ct_site_row, or unused without call sites: a word per flag)
      if (!t->has_rep) d_bad = t->file_slot_off;  // (written last)
      SG_HIP(hipMemsetAsync(d_bad, 0, 16, ctx->stream));
      if (ntab) SG_HIP(hipMemcpyAsync(t->tab, dev->tab, ntab * 8, hipMemcpyDeviceToDevice, ctx->stream));
      if (nfr) {
        SG_HIP(hipMemcpyAsync(t->frame_func, dev->frame_func, nfr * 4, hipMemcpyDeviceToDevice, ctx->stream));
        SG_HIP(hipMemcpyAsync(t->frame_file, dev->frame_file, nfr * 4, hipMemcpyDeviceToDevice, ctx->stream));
      }
      hipLaunchKernelGGL(k_ct_dev_tab, dim3(div_up(std::max<uint64_t>(ntab + 1, nall), 256)), dim3(256), 0, ctx->stream,
                         (const uint64_t*)t->tab, (uint64_t)ntab, (const uint64_t*)(t->has_rep ? t->rep.pcs : nullptr),
                         (uint64_t)(t->has_rep ? nall : 0), dev->frame_off, nfr, t->frame_off, d_bad);
      SG_HIP(hipMemcpyAsync(bad, d_bad, 16, hipMemcpyDeviceToHost, ctx->stream));  // (k_ct_dev_frames' flag: below)
    } else {
      if ((rc = upload(ctx, t->tab, tab_pcs, ntab * 8))) return rc;
      if ((rc = upload(ctx, t->frame_off, fo32.data(), (ntab + 1) * 4))) return rc;
      if ((rc = upload(ctx, t->frame_func, frame_func, nfr * 4))) return rc;
      if ((rc = upload(ctx, t->frame_file, frame_file, nfr * 4))) return rc;
    }
    if (ntab && (rc = radix_index_build(ctx, t->tab, ntab, t->itab))) return rc;
    if (t->has_rep)
      hipLaunchKernelGGL(k_ct_site_row, dim3(div_up(nall, 256)), dim3(256), 0, ctx->stream, t->rep.pcs, (uint64_t)nall,
                         t->tab, (uint64_t)ntab, t->itab, t->site_row);
    uint64_t nslots = 0;
    if (nfr) {
      // the slot table: sort the frames' (file << 32 | line) keys, keep the
      // distinct ones, rank every frame and every file's first key among them
      WsPlan p;
      if (dev && dev->ws_base) p.add(dev->ws_base);  // (the sources, kept)
      const size_t o_ka = p.add(nfr * 8), o_kb = p.add(nfr * 8), o_li = p.add(nfr * 4), o_fl = p.add(nfr * 4),
                   o_ps = p.add((nfr + 1) * 8), o_dk = p.add(nfr * 8), o_bad = p.add(16);
      if ((rc = ws_reserve(ctx, p.total + std::max(radix_sort_ws(nfr), scan_ws_bytes(nfr))))) return rc;
      uint64_t *ka = (uint64_t*)ws_at(ctx, o_ka), *kb = (uint64_t*)ws_at(ctx, o_kb), *pos = (uint64_t*)ws_at(ctx, o_ps),
               *dk = (uint64_t*)ws_at(ctx, o_dk), *sorted = nullptr;
      uint32_t *li = (uint32_t*)ws_at(ctx, o_li), *fl = (uint32_t*)ws_at(ctx, o_fl);
      const dim3 fgrid(div_up(nfr, 256));
      uint32_t* d_bad2 = (uint32_t*)ws_at(ctx, o_bad);
      if (dev) {
        SG_HIP(hipMemsetAsync(d_bad2, 0, 16, ctx->stream));
        hipLaunchKernelGGL(k_ct_dev_frames, fgrid, dim3(256), 0, ctx->stream, dev->frame_line, (const uint32_t*)t->frame_file,
                           (const uint32_t*)t->frame_func, nfr, nfiles, nfuncs, li, d_bad2);
        SG_HIP(hipMemcpyAsync(&bad[3], d_bad2 + 2, 4, hipMemcpyDeviceToHost, ctx->stream));
      } else if ((rc = upload(ctx, li, frame_line, nfr * 4))) {
        return rc;
      }
      hipLaunchKernelGGL(k_ct_keys, fgrid, dim3(256), 0, ctx->stream, t->frame_file, li, nfr, ka);
      if (src.vary) {  // (else every key equal: radix_sort_u64 reads vary == 0 as "find them")
        if ((rc = radix_sort_u64(ctx, ka, kb, nfr, p.total, &sorted, src.vary))) return rc;
      } else {
        sorted = ka;
      }
      if ((rc = rank_runs(ctx, sorted, nfr, fl, pos, nullptr, p.total))) return rc;  // (k_ct_distinct writes the keys)
      hipLaunchKernelGGL(k_ct_distinct, fgrid, dim3(256), 0, ctx->stream, sorted, fl, pos, nfr, dk, t->slot_line);
      hipLaunchKernelGGL(k_ct_frame_slot, fgrid, dim3(256), 0, ctx->stream, t->frame_file, li, nfr, dk, pos,
                         t->frame_slot);
      hipLaunchKernelGGL(k_ct_file_off, dim3(div_up((uint64_t)nfiles + 1, 256)), dim3(256), 0, ctx->stream, dk, pos,
                         nfr, nfiles, t->file_slot_off);
      SG_HIP(hipGetLastError());
      SG_HIP(hipMemcpyAsync(&nslots, pos + nfr, 8, hipMemcpyDeviceToHost, ctx->stream));
    } else {
      SG_HIP(hipMemsetAsync(t->file_slot_off, 0, ((uint64_t)nfiles + 1) * 4, ctx->stream));
    }
    SG_HIP(hipGetLastError());
    SG_HIP(hipStreamSynchronize(ctx->stream));  // (the host arrays are the caller's again)
    t->nslots = nslots;
    if (bad[0] || bad[1] || bad[2] || bad[3]) {
      set_error("%s: %s", fn, bad[0] ? "the records' PCs must be sorted and unique"
                              : bad[1] ? "a call site has no record"
                                       : "a frame has a line of 0 or of 2^32 or more, or an id or offset out of range");
      return SG_EINVAL;
    }
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

size_t cover_table_build_ws(uint64_t nfr) {
  return 6 * align256(nfr * 8 + 8) + 256 + std::max(radix_sort_ws(nfr), scan_ws_bytes(nfr));
}

}  // namespace sg

extern "C" {

void sg_cover_table_destroy(sg_cover_table* t) {
  if (!t) return;
  {
    std::lock_guard<std::mutex> g(t->ctx->mu);
    hipSetDevice(t->ctx->device);
    hipStreamSynchronize(t->ctx->stream);
  }
  delete t;
}

int sg_cover_table_slots(sg_cover_table* t, uint64_t* nslots) {
  if (!t || !nslots) return SG_EINVAL;
  *nslots = t->nslots;
  return SG_OK;
}

int sg_cover_lines(sg_cover_table* t, const uint32_t* cov, size_t ncov, uint32_t base, uint64_t* file_off,
                   uint32_t* lines, uint8_t* covered, uint8_t* file_seen, uint64_t* ncovered_frames, uint64_t* missing,
                   size_t* nmissing) {
  const char* fn = "sg_cover_lines";
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
  return cover_lines_body(t, dcov, ncov, base, file_off, lines, covered, file_seen, ncovered_frames, missing, nmissing);
}

int sg_cover_lines_set(sg_cover_table* t, sg_set* cov, uint32_t base, uint64_t* file_off, uint32_t* lines,
                       uint8_t* covered, uint8_t* file_seen, uint64_t* ncovered_frames, uint64_t* missing,
                       size_t* nmissing) {
  const char* fn = "sg_cover_lines_set";
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
  lines_empty(t, file_off, file_seen, ncovered_frames, nmissing);
  sg_ctx* ctx = t->ctx;
  std::lock_guard<std::mutex> g(ctx->mu);
  rc = ensure_device(ctx);
  if (rc) return rc;
  uint64_t total = 0;
  rc = lines_set_cover(fn, ctx, cov, &total);
  if (rc) return rc;
  if (total == 0) return SG_OK;
  return cover_lines_body(t, dstage_at<uint32_t>(ctx, 0), total, base, file_off, lines, covered, file_seen,
                          ncovered_frames, missing, nmissing);
}

}  // extern "C"
