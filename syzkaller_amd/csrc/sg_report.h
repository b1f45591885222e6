// sg_report.h -- the cover report's query pipeline on device-resident arrays
// (sg_report.hip), shared by sg_cover_uncovered and the report table
// (sg_cover_lines.hip).
#pragma once

#include "sg_internal.h"

namespace sg {

// Radix index over a sorted u64 array A[0..n): r[k] = lower_bound(A, lo + (k
// << sh)) for k <= nb (lo = A[0]), so a lower_bound of x only searches
// [r[k], r[k+1]] for x's bucket k (about one entry per bucket): two adjacent
// loads and a short search instead of log2(n) dependent loads (the C5
// queries are 100M random lookups into 5M call sites and 50K symbols).
struct RadixIdx {
  const uint32_t* r;
  uint64_t lo;
  uint32_t sh, nb;
};

__device__ __forceinline__ uint64_t radix_bucket(uint64_t x, uint64_t lo, uint32_t sh, uint32_t nb) {
  if (x < lo) return 0;
  const uint64_t k = (x - lo) >> sh;
  return k < nb ? k : nb;
}

// lower_bound(a, x) through the index
__device__ __forceinline__ uint64_t lb_idx(const uint64_t* a, uint64_t n, const RadixIdx& I, uint64_t x) {
  const uint64_t k = radix_bucket(x, I.lo, I.sh, I.nb);
  uint64_t lo = x < I.lo ? 0 : I.r[k], hi = x < I.lo ? I.r[0] : (k < I.nb ? I.r[k + 1] : n);
  while (lo < hi) {
    const uint64_t mid = (lo + hi) >> 1;
    if (a[mid] < x)
      lo = mid + 1;
    else
      hi = mid;
  }
  return lo;
}

// upper_bound(a, x) = lower_bound(a, x + 1)
__device__ __forceinline__ uint64_t ub_idx(const uint64_t* a, uint64_t n, const RadixIdx& I, uint64_t x) {
  return x == ~0ull ? n : lb_idx(a, n, I, x + 1);
}

__device__ __forceinline__ uint64_t query_pc(uint64_t hi32, uint32_t cov) { return hi32 + (uint64_t)cov - 5; }

// An index's geometry over n >= 1 sorted values spanning [lo, hi]: about one
// entry per bucket, at most 2^20 buckets (4 MiB: one XCD L2).  I.r holds nb + 1
// entries; radix_index_build fills them (ctx lock held, stream-ordered).
void radix_index_plan(uint64_t n, uint64_t lo, uint64_t hi, RadixIdx& I);
int radix_index_build(sg_ctx* ctx, const uint64_t* d_a, uint64_t n, const RadixIdx& I);

// What the query pipeline reads that depends on the symbols and the call sites
// alone: the arrays, their three indexes, the symbol leaders and (up to 16M
// call sites) the chunk tables of the chunked query path.  All device memory,
// laid out in one buffer: the workspace for sg_cover_uncovered, which builds
// them per call, or a report table's own block, built once.
struct RepTables {
  uint64_t *sstart, *send, *pcs;
  uint64_t nsym, npcs;
  RadixIdx iend, ipcs, istart;
  uint32_t* leader;
  bool chunks;      // the chunk tables below are there
  bool cidx_built;  // ... cidx among them (else report_query fills it when the queries are out of PC order)
  uint32_t nch, csh;
  uint64_t* bnd;
  uint16_t* cidx;
  uint2* symr;
  uint32_t* ssh;
  uint16_t* sidx;
  uint32_t* ssym;
};
struct RepTablesOff {
  size_t ss, se, pcs, ie, ip, is, ld, bnd, ci, sr, sh, si, sy;
};
// nsym, nall >= 1.  plan: the regions and the index geometry from the host
// arrays; bind: the pointers inside `buf`; build: the index kernels over
// sstart / send / pcs already in place (ctx lock held, stream-ordered), the
// radix index over the chunk bounds only with chunk_index: tables built for
// one call leave it to the query, which needs it only out of PC order.
bool report_chunkable(uint64_t nall);
void report_tables_plan(WsPlan& p, const uint64_t* sym_start, const uint64_t* sym_end, uint64_t nsym,
                        const uint64_t* all_pcs, uint64_t nall, bool chunks, RepTables& t, RepTablesOff& o);
void report_tables_bind(void* buf, const RepTablesOff& o, RepTables& t);
int report_tables_build(sg_ctx* ctx, RepTables& t, bool chunk_index);

// One query's scratch in the workspace, and the pipeline from the first-query /
// last-delete reductions to k_rep_final: flag[j] = call site j is uncovered,
// left on the device (ctx lock held, stream-ordered but for the sortedness
// check's wait on the chunked path).  chunked needs t.chunks.  scan_off: the
// workspace tail, report_query_scan_bytes of it.
struct RepQueryOff {
  size_t fq, gf, ld, fl, qb, qo, gq, tc, to, jp, js, srt, qc;
};
void report_query_plan(WsPlan& p, const RepTables& t, uint64_t ncov, bool chunked, RepQueryOff& q);
size_t report_query_scan_bytes(const RepTables& t, uint64_t ncov, bool chunked);
int report_query(sg_ctx* ctx, const RepTables& t, const uint32_t* d_cov, uint64_t ncov, uint32_t base, bool chunked,
                 const RepQueryOff& q, size_t scan_off, uint8_t** d_flag);

}  // namespace sg
