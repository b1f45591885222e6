// sg_part_triage.hip -- the partitioned triage's driver (sg_part.h): one
// launch sequence per record slice, the record slices of a batch, and the
// library's entry points over them (bucket_triage, bucket_emit*).
#include "sg_part.h"

namespace sg {

// One launch sequence over a batch of <= kMaxGroups groups (rec_new zeroed).
// With `emit`, the bucket stage writes the distinct candidates instead of
// flagging records and updating the sets (mwords is then only read).  The
// launch's scratch starts at workspace offset ws_base (reserved by the caller
// when ws_base != 0).
int bucket_triage_one(sg_ctx* ctx, uint32_t* mwords, uint32_t* nwords, const uint32_t* d_vals, const uint64_t* d_off,
                      uint64_t n, uint64_t nrec, uint8_t* d_rec_new, const EmitArgs* emit, size_t ws_base, bool trace) {
  if (n == 0) return SG_OK;
  if (nrec == 0) {
    set_error("bucket triage: signal entries without records");
    return SG_EINVAL;
  }
  BucketPlan bp(n, nrec);
  if (emit || ws_base) {
    int rc = partition_one(ctx, d_vals, d_off, ws_base, ws_base != 0, bp, trace);
    if (rc) return rc;
    return buckets_one(ctx, bp, mwords, nwords, d_rec_new, emit);
  }
  // the flags path: with the M0 filter between the two partition passes when
  // its regime tries it (pass 1 then leaves out the pass-2 digit plane: -0.88
  // GB of writes per C2 step; when the survivors overflow, pass 2 makes the
  // plane from the pass-1 entries)
  const bool filter = m0f_try(ctx);
  int rc = partition_pass1(ctx, d_vals, d_off, 0, false, bp, trace, !filter);
  if (rc) return rc;
  if (filter) {
    bool done = false;
    rc = m0_filter(ctx, bp, mwords, nwords, d_rec_new, &done);
    if (rc || done) return rc;
  }
  // a split bucket stage scatters pass 2 around its first launch (P2Late, sg_part.h); not after a filter that
  // overflowed nor for a trace batch, and every other regime runs pass 2 whole
  const int split = buckets_split(ctx, bp, d_rec_new, !filter && !trace);
  if (split == 2) {
    rc = partition_pass2_tables(ctx, bp, true);
    if (!rc) rc = partition_pass2_buckets(ctx, bp);
  } else {
    rc = partition_pass2(ctx, bp, !filter);
  }
  if (!rc) rc = buckets_one(ctx, bp, mwords, nwords, d_rec_new, nullptr, nullptr, split);
  if (!rc) rc = m0f_note_partitioned(ctx, d_rec_new, nrec);
  return rc;
}

__global__ void k_rebase(const uint64_t* __restrict__ off, uint64_t n, uint64_t base, uint64_t* __restrict__ out) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) out[i] = off[i] - base;
}

int rebase_offsets(sg_ctx* ctx, const uint64_t* d_off, uint64_t n, uint64_t base, uint64_t* d_out) {
  hipLaunchKernelGGL(k_rebase, dim3(div_up(n, 256)), dim3(256), 0, ctx->stream, d_off, n, base, d_out);
  SG_HIP(hipGetLastError());
  return SG_OK;
}

// d_off[r], read with a wait (record_slices_host)
static int read_off(sg_ctx* ctx, const uint64_t* d_off, uint64_t r, uint64_t* v) {
  SG_HIP(hipMemcpyAsync(v, d_off + r, 8, hipMemcpyDeviceToHost, ctx->stream));
  SG_HIP(hipStreamSynchronize(ctx->stream));
  return SG_OK;
}

// The cuts by one device thread (a binary search per entry-limited slice):
// out[0] = the number of slices, then {r0, r1, e0, e1} per slice, at most
// kCutCap of them (a count past kCutCap: the host walks them itself).  One
// launch, one small read and one wait per batch, where the host's own search
// waited on the stream ~20 times (each wait an idle GPU between two batches).
constexpr uint32_t kCutCap = 4096;
constexpr uint32_t kCutHead = 64;  // slices read back with the count
__global__ void k_slice_cuts(const uint64_t* __restrict__ off, uint64_t nrec, uint64_t m, uint64_t lim,
                             uint64_t* __restrict__ out) {
  if (threadIdx.x || blockIdx.x) return;
  uint64_t r0 = 0, e0 = off[0], k = 0;
  while (r0 < nrec && k <= kCutCap) {
    uint64_t r1 = nrec - r0 < m ? nrec : r0 + m, e1 = off[r1];
    if (e1 - e0 > lim) {  // largest r1 > r0 with off[r1] - e0 <= lim (at least one record)
      uint64_t lo = r0 + 1, hi = r1;
      while (lo < hi) {
        const uint64_t mid = (lo + hi + 1) / 2;
        if (off[mid] - e0 <= lim)
          lo = mid;
        else
          hi = mid - 1;
      }
      r1 = lo;
      e1 = off[r1];
    }
    if (k < kCutCap) {
      out[1 + 4 * k] = r0;
      out[2 + 4 * k] = r1;
      out[3 + 4 * k] = e0;
      out[4 + 4 * k] = e1;
    }
    k++;
    r0 = r1;
    e0 = e1;
  }
  out[0] = k;
}

static int record_slices_host(sg_ctx* ctx, const uint64_t* d_off, uint64_t nrec, std::vector<RecSlice>& out,
                              uint64_t lim) {
  out.clear();
  const uint64_t m = ctx->max_launch_recs;
  uint64_t e0 = 0;
  int rc = read_off(ctx, d_off, 0, &e0);
  if (rc) return rc;
  for (uint64_t r0 = 0; r0 < nrec;) {
    uint64_t r1 = nrec - r0 < m ? nrec : r0 + m, e1 = 0;
    rc = read_off(ctx, d_off, r1, &e1);
    if (rc) return rc;
    if (e1 - e0 > lim) {
      uint64_t lo = r0 + 1, hi = r1;
      while (lo < hi) {
        const uint64_t mid = (lo + hi + 1) / 2;
        uint64_t em = 0;
        rc = read_off(ctx, d_off, mid, &em);
        if (rc) return rc;
        if (em - e0 <= lim)
          lo = mid;
        else
          hi = mid - 1;
      }
      r1 = lo;
      rc = read_off(ctx, d_off, r1, &e1);
      if (rc) return rc;
    }
    out.push_back({r0, r1, e0, e1});
    r0 = r1;
    e0 = e1;
  }
  return SG_OK;
}

// The record slices of a batch (RecSlice, sg_part.h), entries limited to lim.
int record_slices(sg_ctx* ctx, const uint64_t* d_off, uint64_t nrec, std::vector<RecSlice>& out, uint64_t lim) {
  out.clear();
  if (nrec == 0) return SG_OK;
  const int rc = ctx->slice_cuts.grow_drop(1 + 4 * (size_t)kCutCap, ctx->stream);
  if (rc) return rc;
  hipLaunchKernelGGL(k_slice_cuts, dim3(1), dim3(64), 0, ctx->stream, d_off, nrec, (uint64_t)ctx->max_launch_recs,
                     lim, ctx->slice_cuts.p);
  SG_HIP(hipGetLastError());
  std::vector<uint64_t> h(1 + 4 * (size_t)kCutHead);
  SG_HIP(hipMemcpyAsync(h.data(), ctx->slice_cuts.p, h.size() * 8, hipMemcpyDeviceToHost, ctx->stream));
  SG_HIP(hipStreamSynchronize(ctx->stream));
  const uint64_t k = h[0];
  if (k > kCutCap) return record_slices_host(ctx, d_off, nrec, out, lim);
  if (k > kCutHead) {
    h.resize(1 + 4 * k);
    SG_HIP(hipMemcpy(h.data(), ctx->slice_cuts.p, h.size() * 8, hipMemcpyDeviceToHost));
  }
  for (uint64_t j = 0; j < k; j++) out.push_back({h[1 + 4 * j], h[2 + 4 * j], h[3 + 4 * j], h[4 + 4 * j]});
  return SG_OK;
}

int record_slice_cuts(sg_ctx* ctx, const uint64_t* d_off, uint64_t nrec, uint64_t lim, std::vector<uint64_t>& cuts) {
  std::vector<RecSlice> sl;
  const int rc = record_slices(ctx, d_off, nrec, sl, lim);
  cuts.clear();
  for (const RecSlice& x : sl) cuts.insert(cuts.end(), {x.r0, x.r1, x.e0, x.e1});
  return rc;
}

// Flags-only triage of a device-resident batch (ctx lock held).  Batches of
// more than ctx->max_launch_recs records run as consecutive record slices:
// the sequential loop (fuzzer.go:665) cut between two records sees the same
// maxSignal at every record.  The rebased offsets of a slice live in a
// grow-only context buffer.
int bucket_triage(sg_ctx* ctx, uint32_t* mwords, uint32_t* nwords, const uint32_t* d_vals, const uint64_t* d_off,
                  uint64_t n, uint64_t nrec, uint8_t* d_rec_new, bool trace) {
  if (nrec >= 0xFFFFFFFFull || n >= 0xFFFFFFFFull - 2 * kPT) {
    set_error("bucket triage: a batch holds < 2^32 signal entries and < 2^32 - 1 records");
    return SG_EINVAL;
  }
  if (nrec) SG_HIP(hipMemsetAsync(d_rec_new, 0, nrec, ctx->stream));
  const uint64_t m = ctx->max_launch_recs;
  if (nrec <= m && n <= kSliceEntries)
    return bucket_triage_one(ctx, mwords, nwords, d_vals, d_off, n, nrec, d_rec_new, nullptr, 0, trace);
  std::vector<RecSlice> sl;
  int rc = record_slices(ctx, d_off, nrec, sl);
  if (rc) return rc;
  // every slice's rebased offsets at once (no wait between two slices)
  if ((rc = slice_off_reserve(ctx, nrec + sl.size()))) return rc;
  size_t at = 0;
  for (const RecSlice& x : sl) {
    // the sequential loop (fuzzer.go:665) cut between two records sees the
    // same maxSignal at every record; a slice starts at a record boundary (a
    // trace slice's first entry is a call start)
    const uint64_t nr = x.r1 - x.r0;
    uint64_t* roff = ctx->slice_off.p + at;
    at += nr + 1;
    if (x.e1 == x.e0) continue;  // records without entries (flags cleared above)
    rc = rebase_offsets(ctx, d_off + x.r0, nr + 1, x.e0, roff);
    if (!rc)
      rc = bucket_triage_one(ctx, mwords, nwords, d_vals + x.e0, roff, x.e1 - x.e0, nr, d_rec_new + x.r0, nullptr, 0,
                             trace);
    if (rc) return rc;
  }
  return SG_OK;
}

int bucket_emit(sg_ctx* ctx, const uint32_t* mwords, const uint32_t* d_vals, const uint64_t* d_off, uint64_t n,
                uint64_t nrec, const EmitArgs& emit, size_t ws_base) {
  if (nrec > kMaxLaunchRecords || n >= 0xFFFFFFFFull - 2 * kPT) {
    set_error("bucket emit: a launch holds <= 2^24 records and < 2^32 - 2^15 entries");
    return SG_EINVAL;
  }
  return bucket_triage_one(ctx, const_cast<uint32_t*>(mwords), nullptr, d_vals, d_off, n, nrec, nullptr, &emit,
                           ws_base);
}

int bucket_emit_update(sg_ctx* ctx, uint32_t* mwords, uint32_t* nwords, const uint32_t* d_vals, const uint64_t* d_off,
                       uint64_t n, uint64_t nrec, uint2* pairs, unsigned long long* gcur, size_t ws_base) {
  if (nrec > kMaxLaunchRecords || n >= 0xFFFFFFFFull - 2 * kPT) {
    set_error("bucket emit: a launch holds <= 2^24 records and < 2^32 - 2^15 entries");
    return SG_EINVAL;
  }
  EmitArgs e{};
  e.pairs = pairs;
  e.update = true;
  e.gcur = gcur;
  e.goff = d_off;
  return bucket_triage_one(ctx, mwords, nwords, d_vals, d_off, n, nrec, nullptr, &e, ws_base);
}

}  // namespace sg
