// sg_inflate.hip -- compress/flate's reader on the GPU: every value of a corpus
// database inflated at once (pkg/db/db.go:213-249, through Open :38-52; the
// hub's loadDB, syz-hub/state/state.go:83-110; the manager's start-up,
// syz-manager/manager.go:178-216).
//
// A DEFLATE stream is a serial chain of bits, so the parallelism is across
// streams: a lane per stream, the decoder of sg_inflate.h.
//
//  1. k_inflate_keys: a key per stream, (class << 32) | stream, class = 1024 -
//     compressed bytes / 64, kLongClass for a stream longer than
//     SG_INFLATE_LONG bytes.
//  2. radix_sort_u64 on the 11 class bits (two passes, stable): longest first,
//     the long streams last.  A wave takes 64 neighbours of that order, so its
//     lanes differ by at most 64 compressed bytes and the wave that runs
//     longest starts first -- k_sha1_keys' scheme (sg_prog_hash.hip).
//  3. k_inflate<false>, a wave per 64 keys: the count sink.  Huffman decoding
//     never reads the output, so this pass needs no window: status, consumed
//     and the output's length of every stream.
//  4. scan_counts over the lengths: the outputs' CSR.
//  5. k_inflate<true>: the write sink over the streams whose span is not empty
//     (a caller that wants only some of them zeroes the others' lengths before
//     the scan: sg_db_open does, for the records that are not live).  It runs
//     only when the total fits the caller's buffer, compared on the device.
//  6. k_inflate_long<>, for both passes: a wave per long stream, lane 0
//     decoding (a wave strides over several only when the device form's
//     offsets make long streams overlap and outnumber buffer / 65,537).  It
//     keeps a 1 MiB stream from holding 63 other streams' lanes; it is there
//     for correctness at any length, not for speed.
//  7. k_inflate_nlong: the long streams are the sorted keys' tail; one thread
//     finds where it starts and adds its length to "inflate_long_streams".
//
// Tables.  A lane's Huffman tables are indexed by what it decodes, so they live
// in LDS, never in private arrays: 203 dwords a lane (sg_inflate.h Tab), 51,968
// bytes a wave, three waves a CU.  They are interleaved by dword: logical dword
// w of lane l is LDS dword 64 w + l.  Its bank is l mod 32 whatever w is, so
// the 32 lanes of a ds_read / ds_write group hit 32 different banks at any mix
// of per-lane indices.  (A row per lane with an odd stride is conflict-free
// only when the lanes ask for the same index, which decoders of different
// streams do not.)  The fixed code needs no table: its counts and symbol runs
// are closed forms, the same for the whole wave.
//
// Every stream's range is clamped to the buffer as sg_prog_hashes_dev clamps
// it, and every output span to [0, total]; the decoder's own termination and
// bounds arguments are in sg_inflate.h.  No float; no atomics beyond
// scan_counts'.
#include "sg_internal.h"

#include "sg_inflate.h"

#include <algorithm>

namespace sg {
namespace {

constexpr uint32_t kLongClass = 2047;
constexpr uint32_t kTopClass = kInflateLong >> 6;  // the class field of an empty stream
static_assert(kTopClass < kLongClass, "the class field holds 11 bits");
constexpr uint64_t kClassBits = 0x7FFull << 32;
constexpr uint32_t kIT = 64;  // one wave per workgroup: the LDS columns are its lanes'

struct InfArgs {
  const uint8_t* in;
  uint64_t nbytes;
  const uint64_t* beg;  // stream p is in[beg[p], end[p]), clamped; a CSR passes off and off + 1
  const uint64_t* end;
  uint64_t n;
  const uint64_t* keys;  // sorted
  uint8_t* status;
  // the count pass
  uint64_t* consumed;
  uint32_t* olen;
  // the write pass
  const uint64_t* out_off;  // [n + 1]
  uint8_t* out;
  uint64_t cap;
};

__device__ __forceinline__ void stream_range(const InfArgs& a, uint64_t p, uint64_t& r0, uint64_t& len) {
  r0 = min(a.beg[p], a.nbytes);
  len = min(max(a.end[p], r0), a.nbytes) - r0;
}

__global__ __launch_bounds__(256) void k_inflate_keys(const uint64_t* __restrict__ beg, const uint64_t* __restrict__ end,
                                                       uint64_t n, uint64_t nbytes, uint64_t* __restrict__ keys) {
  const uint64_t p = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (p >= n) return;
  const uint64_t r0 = min(beg[p], nbytes);
  const uint64_t len = min(max(end[p], r0), nbytes) - r0;
  const uint32_t cls = len > kInflateLong ? kLongClass : kTopClass - (uint32_t)(len >> 6);
  keys[p] = ((uint64_t)cls << 32) | p;
}

// One stream by one lane with its tables at `tab`: the count pass, or the write pass into its span.
template <bool kWrite>
__device__ __forceinline__ void inflate_one(const InfArgs& a, uint64_t p, uint64_t r0, uint64_t len, sginf::Tab tab) {
  if (kWrite) {
    if (a.status[p] != SG_INFLATE_OK) return;
    const uint64_t total = a.out_off[a.n];  // (<= cap: the kernel has looked)
    const uint64_t o0 = min(a.out_off[p], total), o1 = min(max(a.out_off[p + 1], o0), total);
    if (o1 == o0) return;
    sginf::WriteSink sink(a.out + o0, o1 - o0);
    uint64_t consumed = 0;
    sginf::inflate(a.in + r0, len, tab, sink, consumed);
  } else {
    sginf::CountSink sink;
    uint64_t consumed = 0;
    const int st = sginf::inflate(a.in + r0, len, tab, sink, consumed);
    a.status[p] = (uint8_t)st;
    a.consumed[p] = st == SG_INFLATE_OK ? consumed : 0;
    a.olen[p] = st == SG_INFLATE_OK ? (uint32_t)sink.n : 0u;  // (below 2^32, or the status is TOO_LARGE)
  }
}

template <bool kWrite>
__global__ __launch_bounds__(kIT) void k_inflate(InfArgs a) {
  __shared__ uint32_t tabs[sginf::kTabDwords * 64];
  const uint32_t lane = threadIdx.x;
  const uint64_t i = (uint64_t)blockIdx.x * 64 + lane;
  if (i >= a.n) return;  // (no barrier below: a lane's column is its own)
  if (kWrite && a.out_off[a.n] > a.cap) return;
  const uint64_t key = a.keys[i];
  const uint64_t p = key & 0xFFFFFFFFull;
  if ((uint32_t)(key >> 32) == kLongClass || p >= a.n) return;
  uint64_t r0, len;
  stream_range(a, p, r0, len);
  if (len > kInflateLong) return;
  inflate_one<kWrite>(a, p, r0, len, sginf::Tab{reinterpret_cast<uint8_t*>(tabs + lane), 64});
}

template <bool kWrite>
__global__ __launch_bounds__(kIT) void k_inflate_long(InfArgs a) {
  __shared__ uint32_t tabs[sginf::kTabDwords];
  if (threadIdx.x != 0) return;
  if (kWrite && a.out_off[a.n] > a.cap) return;
  // The long streams are the sorted keys' tail.  The grid is sized for disjoint streams; the device form's
  // offsets may make long streams overlap and so outnumber it, hence the stride: every long key is somebody's.
  for (uint64_t j = blockIdx.x; j < a.n; j += gridDim.x) {
    const uint64_t key = a.keys[a.n - 1 - j];
    const uint64_t p = key & 0xFFFFFFFFull;
    if ((uint32_t)(key >> 32) != kLongClass || p >= a.n) return;
    uint64_t r0, len;
    stream_range(a, p, r0, len);
    inflate_one<kWrite>(a, p, r0, len, sginf::Tab{reinterpret_cast<uint8_t*>(tabs), 1});
  }
}

__global__ void k_inflate_nlong(const uint64_t* __restrict__ keys, uint64_t n, unsigned long long* __restrict__ ctr) {
  uint64_t lo = 0, hi = n;  // the first key of the long class
  while (lo < hi) {
    const uint64_t mid = lo + (hi - lo) / 2;
    if ((uint32_t)(keys[mid] >> 32) >= kLongClass)
      hi = mid;
    else
      lo = mid + 1;
  }
  *ctr += n - lo;  // (stream-ordered: one thread, one writer)
}

struct InfPlan {
  size_t o_ka, o_kb, o_sort, o_scan, total;
  InfPlan(size_t base, uint64_t n) {
    o_ka = base;
    o_kb = o_ka + align256(n * 8);
    o_sort = o_kb + align256(n * 8);
    o_scan = o_sort + align256(radix_sort_ws(n));
    total = o_scan + scan_ws_bytes(n);
  }
};

uint32_t long_grid(uint64_t n, uint64_t nbytes) {
  return (uint32_t)std::min<uint64_t>(n, nbytes / ((uint64_t)kInflateLong + 1));
}

}  // namespace

size_t inflate_ws(uint64_t n) { return InfPlan(0, n).total; }

int inflate_count(sg_ctx* ctx, const uint8_t* d_in, const uint64_t* d_beg, const uint64_t* d_end, uint64_t n,
                  uint64_t nbytes, uint8_t* d_status, uint64_t* d_consumed, uint32_t* d_olen, size_t ws_used,
                  const uint64_t** d_sorted) {
  *d_sorted = nullptr;
  if (n == 0) return SG_OK;
  const InfPlan pl(ws_used, n);
  uint64_t* ka = (uint64_t*)ws_at(ctx, pl.o_ka);
  uint64_t* kb = (uint64_t*)ws_at(ctx, pl.o_kb);
  {
    ScopedTimer tm(ctx, "inflate_keys");
    hipLaunchKernelGGL(k_inflate_keys, dim3(div_up(n, 256)), dim3(256), 0, ctx->stream, d_beg, d_end, n, nbytes, ka);
  }
  SG_HIP(hipGetLastError());
  uint64_t* sorted = nullptr;
  int rc;
  {
    ScopedTimer tm(ctx, "inflate_sort");  // (its scans are timed as "scan" as well)
    rc = radix_sort_u64(ctx, ka, kb, n, pl.o_sort, &sorted, kClassBits);
  }
  if (rc) return rc;
  InfArgs a{};
  a.in = d_in;
  a.nbytes = nbytes;
  a.beg = d_beg;
  a.end = d_end;
  a.n = n;
  a.keys = sorted;
  a.status = d_status;
  a.consumed = d_consumed;
  a.olen = d_olen;
  {
    ScopedTimer tm(ctx, "inflate_count");
    hipLaunchKernelGGL(k_inflate<false>, dim3(div_up(n, 64)), dim3(kIT), 0, ctx->stream, a);
  }
  SG_HIP(hipGetLastError());
  if (const uint32_t nl = long_grid(n, nbytes)) {
    ScopedTimer tm(ctx, "inflate_long");
    hipLaunchKernelGGL(k_inflate_long<false>, dim3(nl), dim3(kIT), 0, ctx->stream, a);
  }
  hipLaunchKernelGGL(k_inflate_nlong, dim3(1), dim3(1), 0, ctx->stream, (const uint64_t*)sorted, n,
                     (unsigned long long*)&ctx->dev.p->inflate_long_streams);
  SG_HIP(hipGetLastError());
  *d_sorted = sorted;
  return SG_OK;
}

int inflate_offsets(sg_ctx* ctx, const uint32_t* d_olen, uint64_t* d_out_off, uint64_t n, size_t ws_used) {
  return scan_counts(ctx, d_olen, d_out_off, n, InfPlan(ws_used, n).o_scan);
}

int inflate_write(sg_ctx* ctx, const uint8_t* d_in, const uint64_t* d_beg, const uint64_t* d_end, uint64_t n,
                  uint64_t nbytes, const uint64_t* d_sorted, const uint8_t* d_status, const uint64_t* d_out_off,
                  uint8_t* d_out, uint64_t cap) {
  if (n == 0 || cap == 0) return SG_OK;
  InfArgs a{};
  a.in = d_in;
  a.nbytes = nbytes;
  a.beg = d_beg;
  a.end = d_end;
  a.n = n;
  a.keys = d_sorted;
  a.status = const_cast<uint8_t*>(d_status);  // (read only by the write pass)
  a.out_off = d_out_off;
  a.out = d_out;
  a.cap = cap;
  {
    ScopedTimer tm(ctx, "inflate_write");
    hipLaunchKernelGGL(k_inflate<true>, dim3(div_up(n, 64)), dim3(kIT), 0, ctx->stream, a);
  }
  SG_HIP(hipGetLastError());
  if (const uint32_t nl = long_grid(n, nbytes)) {
    ScopedTimer tm(ctx, "inflate_long");
    hipLaunchKernelGGL(k_inflate_long<true>, dim3(nl), dim3(kIT), 0, ctx->stream, a);
  }
  SG_HIP(hipGetLastError());
  return SG_OK;
}

}  // namespace sg

using namespace sg;

extern "C" {

int sg_inflate_batch_dev(sg_ctx* ctx, const uint8_t* d_in, const uint64_t* d_in_off, uint64_t n, uint64_t nbytes,
                         uint8_t* d_status, uint64_t* d_consumed, uint64_t* d_out_off, uint8_t* d_out, uint64_t cap) {
  const char* fn = "sg_inflate_batch_dev";
  if (!ctx || !d_out_off || (n && (!d_in_off || !d_status || !d_consumed)) || (nbytes && !d_in) || (cap && !d_out)) {
    set_error("%s: invalid argument", fn);
    return SG_EINVAL;
  }
  if (n >= (1ull << 32)) {
    set_error("%s: %llu streams (the limit is 2^32 - 1)", fn, (unsigned long long)n);
    return SG_EINVAL;
  }
  std::lock_guard<std::mutex> g(ctx->mu);
  int rc = ensure_device(ctx);
  if (rc) return rc;
  if (n == 0) {
    SG_HIP(hipMemsetAsync(d_out_off, 0, 8, ctx->stream));
    return SG_OK;
  }
  const size_t o_olen = inflate_ws(n);
  if ((rc = ws_reserve(ctx, o_olen + align256(n * 4)))) return rc;
  uint32_t* olen = (uint32_t*)ws_at(ctx, o_olen);
  const uint64_t* sorted = nullptr;
  if ((rc = inflate_count(ctx, d_in, d_in_off, d_in_off + 1, n, nbytes, d_status, d_consumed, olen, 0, &sorted)))
    return rc;
  if ((rc = inflate_offsets(ctx, olen, d_out_off, n, 0))) return rc;
  return inflate_write(ctx, d_in, d_in_off, d_in_off + 1, n, nbytes, sorted, d_status, d_out_off, d_out, cap);
}

int sg_inflate_batch(sg_ctx* ctx, const uint8_t* in, const uint64_t* in_off, size_t n, uint8_t* status,
                     uint64_t* consumed, uint64_t* out_off, uint8_t* out, size_t cap, size_t* nout) {
  const char* fn = "sg_inflate_batch";
  if (!ctx || !out_off || !nout || (n && (!status || !consumed)) || (cap && !out)) {
    set_error("%s: invalid argument", fn);
    return SG_EINVAL;
  }
  int rc = prog_texts_ok(fn, in, in_off, n);
  if (rc) return rc;
  std::lock_guard<std::mutex> g(ctx->mu);
  rc = ensure_device(ctx);
  if (rc) return rc;
  if (n == 0) {
    out_off[0] = 0;
    *nout = 0;
    return SG_OK;
  }
  const uint64_t nbytes = in_off[n];
  WsPlan plan;
  const size_t o_in = plan.add(nbytes + 4), o_off = plan.add((n + 1) * 8), o_status = plan.add(n),
               o_cons = plan.add(n * 8), o_olen = plan.add(n * 4), o_oo = plan.add((n + 1) * 8);
  if ((rc = dstage_reserve(ctx, plan))) return rc;
  if ((rc = ws_reserve(ctx, inflate_ws(n)))) return rc;
  uint8_t* din = dstage_at<uint8_t>(ctx, o_in);
  uint64_t* doff = dstage_at<uint64_t>(ctx, o_off);
  uint8_t* dstatus = dstage_at<uint8_t>(ctx, o_status);
  uint64_t* dcons = dstage_at<uint64_t>(ctx, o_cons);
  uint32_t* dolen = dstage_at<uint32_t>(ctx, o_olen);
  uint64_t* doo = dstage_at<uint64_t>(ctx, o_oo);
  if ((rc = upload(ctx, din, in, nbytes))) return rc;
  if ((rc = upload(ctx, doff, in_off, (n + 1) * 8))) return rc;
  const uint64_t* sorted = nullptr;
  if ((rc = inflate_count(ctx, din, doff, doff + 1, n, nbytes, dstatus, dcons, dolen, 0, &sorted))) return rc;
  if ((rc = inflate_offsets(ctx, dolen, doo, n, 0))) return rc;
  uint64_t total = 0;
  SG_HIP(hipMemcpyAsync(&total, doo + n, 8, hipMemcpyDeviceToHost, ctx->stream));
  SG_HIP(hipStreamSynchronize(ctx->stream));
  if (total >= kInflateMaxOut) {
    set_error("%s: %llu bytes of output (the limit is 2^33 - 1)", fn, (unsigned long long)total);
    return SG_EINVAL;
  }
  const bool fits = total <= cap;
  if (fits && total) {
    if ((rc = ctx->inflate_out.grow_drop(grow_cap(ctx->inflate_out.cap, total, 16u << 20), ctx->stream))) return rc;
    if ((rc = inflate_write(ctx, din, doff, doff + 1, n, nbytes, sorted, dstatus, doo, ctx->inflate_out.p, total)))
      return rc;
    SG_HIP(hipMemcpyAsync(out, ctx->inflate_out.p, total, hipMemcpyDeviceToHost, ctx->stream));
  }
  SG_HIP(hipMemcpyAsync(status, dstatus, n, hipMemcpyDeviceToHost, ctx->stream));
  SG_HIP(hipMemcpyAsync(consumed, dcons, n * 8, hipMemcpyDeviceToHost, ctx->stream));
  SG_HIP(hipMemcpyAsync(out_off, doo, (n + 1) * 8, hipMemcpyDeviceToHost, ctx->stream));
  SG_HIP(hipStreamSynchronize(ctx->stream));
  *nout = total;
  return SG_OK;
}

}  // extern "C"
