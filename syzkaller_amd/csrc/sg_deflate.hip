// sg_deflate.hip -- compress/flate's writer on the GPU: every value of a corpus
// database deflated at once (pkg/db/db.go:137-165 serializeRecord, through
// compact :95-116 and Flush :75-93; the hub's loadDB, addInputs and purgeCorpus,
// syz-hub/state/state.go:106, :310-336, :349-351; minimizeCorpus,
// syz-manager/manager.go:786-795).
//
// An LZ77 parse is a serial chain of decisions, so the parallelism is across
// streams, as in sg_inflate.hip: a lane per stream, the encoder of sg_deflate.h.
//
//  1. k_deflate_keys: a key per stream, (class << 32) | stream, class = 1024 -
//     input bytes / 64, kLongClass for a stream longer than SG_DEFLATE_LONG.
//  2. radix_sort_u64 on the 11 class bits (two passes, stable): longest first,
//     the long streams last, so a wave's lanes differ by at most 64 input bytes.
//  3. k_deflate<false>, a wave per 64 keys: the count phase.  Every stream's
//     exact length and its form (stored 0, fixed 1, dynamic 2).
//  4. scan_counts over the lengths: the outputs' CSR.
//  5. k_deflate<true>: the write phase into each stream's span (a caller that
//     wants only some of them zeroes the others' lengths before the scan:
//     sg_db_serialize does, for deletions and empty values).  It runs only when
//     the total fits the caller's buffer, compared on the device.  It plans
//     again by itself and takes nothing but its span from the count.
//  6. k_deflate_long<>, for both phases: a wave per long stream, lane 0
//     encoding; for correctness at any length, not for speed.
//  7. k_deflate_stats: one workgroup counts the forms of the call
//     ("deflate_stored_streams", "deflate_fixed_streams",
//     "deflate_dynamic_streams") and finds where the sorted keys' long tail
//     starts ("deflate_long_streams").
//
// Tables.  A lane's tables are indexed by what it encodes, so they live in LDS,
// never in private arrays: 620 dwords a lane (sg_deflate.h Tab: 316 counters,
// 316 length nibbles, 16 code counts, 512 hash slots), 158,720 bytes a wave:
// ONE wave a CU.  Two waves a CU would leave 1,280 bytes a lane, of which the
// counters alone take 1,264.  They are interleaved by dword: logical dword w of
// lane l is LDS dword 64 w + l, bank l mod 32 whatever w is, so the 32 lanes of
// a ds_read / ds_write group hit 32 different banks at any mix of per-lane
// indices -- and hash slots and symbol counters are exactly such a mix.
//
// Every stream's range is clamped to the buffer as sg_inflate_batch_dev clamps
// it, and to kDeflateMaxIn bytes so that a length fits 32 bits; every output
// span to [0, cap].  The encoder's own termination, bounds and determinism
// arguments are in sg_deflate.h.
#include "sg_internal.h"

#include "sg_deflate.h"

#include <algorithm>

namespace sg {
namespace {

constexpr uint32_t kLongClass = 2047;
constexpr uint32_t kTopClass = kDeflateLong >> 6;  // the class field of an empty stream
static_assert(kTopClass < kLongClass, "the class field holds 11 bits");
constexpr uint64_t kClassBits = 0x7FFull << 32;
constexpr uint32_t kDT = 64;  // one wave per workgroup: the LDS columns are its lanes'
static_assert(sgdef::kTabDwords * 64 * 4 <= 160 * 1024, "a wave's tables fit the CU's LDS");

struct DefArgs {
  const uint8_t* in;
  uint64_t nbytes;
  const uint64_t* beg;  // stream p is in[beg[p], end[p]), clamped; a CSR passes off and off + 1
  const uint64_t* end;
  uint64_t n;
  const uint64_t* keys;  // sorted
  // the count phase
  uint32_t* olen;
  uint8_t* form;
  // the write phase: stream p's span is out[out_off[p] + shift[p], out_off[p + 1] + shift[p])
  const uint64_t* out_off;  // [n + 1]
  const uint64_t* shift;    // [n], or null for none
  uint64_t extra;           // the bytes of out that are not streams: the call needs out_off[n] + extra
  uint8_t* out;
  uint64_t cap;
};

__device__ __forceinline__ void stream_range(const DefArgs& a, uint64_t p, uint64_t& r0, uint64_t& len) {
  r0 = min(a.beg[p], a.nbytes);
  len = min(min(max(a.end[p], r0), a.nbytes) - r0, kDeflateMaxIn);
}

__global__ __launch_bounds__(256) void k_deflate_keys(const uint64_t* __restrict__ beg, const uint64_t* __restrict__ end,
                                                       uint64_t n, uint64_t nbytes, uint64_t* __restrict__ keys) {
  const uint64_t p = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (p >= n) return;
  const uint64_t r0 = min(beg[p], nbytes);
  const uint64_t len = min(max(end[p], r0), nbytes) - r0;
  const uint32_t cls = len > kDeflateLong ? kLongClass : kTopClass - (uint32_t)(len >> 6);
  keys[p] = ((uint64_t)cls << 32) | p;
}

// One stream by one lane with its tables at `tab`: the count phase, or the write phase into its span.
template <bool kWrite>
__device__ __forceinline__ void deflate_one(const DefArgs& a, uint64_t p, uint64_t r0, uint64_t len, sgdef::Tab tab) {
  if (kWrite) {
    const uint64_t sh = a.shift ? a.shift[p] : 0;
    const uint64_t b0 = a.out_off[p], b1 = max(a.out_off[p + 1], b0);
    if (b1 == b0 || sh > a.cap || b0 > a.cap - sh) return;
    const uint64_t o0 = b0 + sh, o1 = min(b1 - b0, a.cap - o0) + o0;
    sgdef::WriteSink sink(a.out + o0, o1 - o0);
    sgdef::encode(a.in + r0, len, tab, sink);
  } else {
    const sgdef::Plan pl = sgdef::plan(a.in + r0, len, tab);
    a.olen[p] = (uint32_t)pl.bytes;  // (below 2^32: the input is at most kDeflateMaxIn)
    a.form[p] = (uint8_t)pl.form;
  }
}

template <bool kWrite>
__global__ __launch_bounds__(kDT) void k_deflate(DefArgs a) {
  __shared__ uint32_t tabs[sgdef::kTabDwords * 64];
  const uint32_t lane = threadIdx.x;
  const uint64_t i = (uint64_t)blockIdx.x * 64 + lane;
  if (i >= a.n) return;  // (no barrier below: a lane's column is its own)
  if (kWrite && (a.out_off[a.n] > a.cap || a.extra > a.cap - a.out_off[a.n])) return;
  const uint64_t key = a.keys[i];
  const uint64_t p = key & 0xFFFFFFFFull;
  if ((uint32_t)(key >> 32) == kLongClass || p >= a.n) return;
  uint64_t r0, len;
  stream_range(a, p, r0, len);
  if (len > kDeflateLong) return;
  deflate_one<kWrite>(a, p, r0, len, sgdef::Tab{reinterpret_cast<uint8_t*>(tabs + lane), 64});
}

template <bool kWrite>
__global__ __launch_bounds__(kDT) void k_deflate_long(DefArgs a) {
  __shared__ uint32_t tabs[sgdef::kTabDwords];
  if (threadIdx.x != 0) return;
  if (kWrite && (a.out_off[a.n] > a.cap || a.extra > a.cap - a.out_off[a.n])) return;
  // The long streams are the sorted keys' tail.  The grid is sized for disjoint streams; the device form's
  // offsets may make long streams overlap and so outnumber it, hence the stride: every long key is somebody's.
  for (uint64_t j = blockIdx.x; j < a.n; j += gridDim.x) {
    const uint64_t key = a.keys[a.n - 1 - j];
    const uint64_t p = key & 0xFFFFFFFFull;
    if ((uint32_t)(key >> 32) != kLongClass || p >= a.n) return;
    uint64_t r0, len;
    stream_range(a, p, r0, len);
    deflate_one<kWrite>(a, p, r0, len, sgdef::Tab{reinterpret_cast<uint8_t*>(tabs), 1});
  }
}

// The forms of this call's streams, and the first key of the long class (stream-ordered: one workgroup, one writer).
__global__ __launch_bounds__(256) void k_deflate_stats(const uint64_t* __restrict__ keys, const uint8_t* __restrict__ form,
                                                        uint64_t n, CtxDev* __restrict__ dev) {
  __shared__ uint32_t cnt[3][256];
  uint32_t c0 = 0, c1 = 0, c2 = 0;
  for (uint64_t p = threadIdx.x; p < n; p += 256) {
    const uint32_t f = form[p];
    c0 += f == 0;
    c1 += f == 1;
    c2 += f == 2;
  }
  cnt[0][threadIdx.x] = c0;
  cnt[1][threadIdx.x] = c1;
  cnt[2][threadIdx.x] = c2;
  __syncthreads();
  for (uint32_t s = 128; s; s >>= 1) {
    if (threadIdx.x < s)
      for (uint32_t f = 0; f < 3; f++) cnt[f][threadIdx.x] += cnt[f][threadIdx.x + s];
    __syncthreads();
  }
  if (threadIdx.x != 0) return;
  for (uint32_t f = 0; f < 3; f++) dev->deflate_forms[f] = cnt[f][0];
  uint64_t lo = 0, hi = n;
  while (lo < hi) {
    const uint64_t mid = lo + (hi - lo) / 2;
    if ((uint32_t)(keys[mid] >> 32) >= kLongClass)
      hi = mid;
    else
      lo = mid + 1;
  }
  dev->deflate_long_streams += n - lo;
}

struct DefPlan {
  size_t o_ka, o_kb, o_sort, o_scan, total;
  DefPlan(size_t base, uint64_t n) {
    o_ka = base;
    o_kb = o_ka + align256(n * 8);
    o_sort = o_kb + align256(n * 8);
    o_scan = o_sort + align256(radix_sort_ws(n));
    total = o_scan + scan_ws_bytes(n);
  }
};

uint32_t long_grid(uint64_t n, uint64_t nbytes) {
  return (uint32_t)std::min<uint64_t>(n, nbytes / ((uint64_t)kDeflateLong + 1));
}

// the encoder on the host, a stream at a time: lengths, then (with out) the bytes
uint64_t host_count(const uint8_t* in, const uint64_t* in_off, size_t n, uint64_t* out_off, std::vector<uint8_t>& tab) {
  uint64_t total = 0;
  for (size_t k = 0; k < n; k++) {
    out_off[k] = total;
    total += sgdef::plan(in + in_off[k], in_off[k + 1] - in_off[k], sgdef::Tab{tab.data(), 1}).bytes;
  }
  out_off[n] = total;
  return total;
}

}  // namespace

size_t deflate_ws(uint64_t n) { return DefPlan(0, n).total; }

int deflate_count(sg_ctx* ctx, const uint8_t* d_in, const uint64_t* d_beg, const uint64_t* d_end, uint64_t n,
                  uint64_t nbytes, uint32_t* d_olen, uint8_t* d_form, size_t ws_used, const uint64_t** d_sorted) {
  *d_sorted = nullptr;
  if (n == 0) return SG_OK;
  const DefPlan pl(ws_used, n);
  uint64_t* ka = (uint64_t*)ws_at(ctx, pl.o_ka);
  uint64_t* kb = (uint64_t*)ws_at(ctx, pl.o_kb);
  {
    ScopedTimer tm(ctx, "deflate_keys");
    hipLaunchKernelGGL(k_deflate_keys, dim3(div_up(n, 256)), dim3(256), 0, ctx->stream, d_beg, d_end, n, nbytes, ka);
  }
  SG_HIP(hipGetLastError());
  uint64_t* sorted = nullptr;
  int rc;
  {
    ScopedTimer tm(ctx, "deflate_sort");  // (its scans are timed as "scan" as well)
    rc = radix_sort_u64(ctx, ka, kb, n, pl.o_sort, &sorted, kClassBits);
  }
  if (rc) return rc;
  DefArgs a{};
  a.in = d_in;
  a.nbytes = nbytes;
  a.beg = d_beg;
  a.end = d_end;
  a.n = n;
  a.keys = sorted;
  a.olen = d_olen;
  a.form = d_form;
  {
    ScopedTimer tm(ctx, "deflate_count");
    hipLaunchKernelGGL(k_deflate<false>, dim3(div_up(n, 64)), dim3(kDT), 0, ctx->stream, a);
  }
  SG_HIP(hipGetLastError());
  if (const uint32_t nl = long_grid(n, nbytes)) {
    ScopedTimer tm(ctx, "deflate_long");
    hipLaunchKernelGGL(k_deflate_long<false>, dim3(nl), dim3(kDT), 0, ctx->stream, a);
  }
  SG_HIP(hipGetLastError());
  hipLaunchKernelGGL(k_deflate_stats, dim3(1), dim3(256), 0, ctx->stream, (const uint64_t*)sorted,
                     (const uint8_t*)d_form, n, ctx->dev.p);
  SG_HIP(hipGetLastError());
  *d_sorted = sorted;
  return SG_OK;
}

int deflate_offsets(sg_ctx* ctx, const uint32_t* d_olen, uint64_t* d_out_off, uint64_t n, size_t ws_used) {
  return scan_counts(ctx, d_olen, d_out_off, n, DefPlan(ws_used, n).o_scan);
}

int deflate_write(sg_ctx* ctx, const uint8_t* d_in, const uint64_t* d_beg, const uint64_t* d_end, uint64_t n,
                  uint64_t nbytes, const uint64_t* d_sorted, const uint64_t* d_out_off, const uint64_t* d_shift,
                  uint64_t extra, uint8_t* d_out, uint64_t cap) {
  if (n == 0 || cap == 0) return SG_OK;
  DefArgs a{};
  a.in = d_in;
  a.nbytes = nbytes;
  a.beg = d_beg;
  a.end = d_end;
  a.n = n;
  a.keys = d_sorted;
  a.out_off = d_out_off;
  a.shift = d_shift;
  a.extra = extra;
  a.out = d_out;
  a.cap = cap;
  {
    ScopedTimer tm(ctx, "deflate_write");
    hipLaunchKernelGGL(k_deflate<true>, dim3(div_up(n, 64)), dim3(kDT), 0, ctx->stream, a);
  }
  SG_HIP(hipGetLastError());
  if (const uint32_t nl = long_grid(n, nbytes)) {
    ScopedTimer tm(ctx, "deflate_long");
    hipLaunchKernelGGL(k_deflate_long<true>, dim3(nl), dim3(kDT), 0, ctx->stream, a);
  }
  SG_HIP(hipGetLastError());
  return SG_OK;
}

// what the host forms reject of their streams (fn names the caller)
int deflate_texts_ok(const char* fn, const uint8_t* in, const uint64_t* in_off, size_t n) {
  const int rc = prog_texts_ok(fn, in, in_off, n);
  if (rc) return rc;
  for (size_t k = 0; k < n; k++)
    if (in_off[k + 1] - in_off[k] > kDeflateMaxIn) {
      set_error("%s: stream %llu has %llu bytes (the limit is 2^32 - 2^20)", fn, (unsigned long long)k,
                (unsigned long long)(in_off[k + 1] - in_off[k]));
      return SG_EINVAL;
    }
  return SG_OK;
}

}  // namespace sg

using namespace sg;

extern "C" {

size_t sg_deflate_bound(size_t len) { return (size_t)sgdef::stored_bytes(len); }

int sg_deflate_host(const uint8_t* in, const uint64_t* in_off, size_t n, uint64_t* out_off, uint8_t* out, size_t cap,
                    size_t* nout) {
  const char* fn = "sg_deflate_host";
  if (!out_off || !nout || (cap && !out)) {
    set_error("%s: invalid argument", fn);
    return SG_EINVAL;
  }
  const int rc = deflate_texts_ok(fn, in, in_off, n);
  if (rc) return rc;
  std::vector<uint8_t> tab(sgdef::kTabBytes);
  const uint64_t total = host_count(in, in_off, n, out_off, tab);
  *nout = total;
  if (total > cap) return SG_OK;
  for (size_t k = 0; k < n; k++) {
    sgdef::WriteSink sink(out + out_off[k], out_off[k + 1] - out_off[k]);
    sgdef::encode(in + in_off[k], in_off[k + 1] - in_off[k], sgdef::Tab{tab.data(), 1}, sink);
  }
  return SG_OK;
}

int sg_deflate_batch_dev(sg_ctx* ctx, const uint8_t* d_in, const uint64_t* d_in_off, uint64_t n, uint64_t nbytes,
                         uint64_t* d_out_off, uint8_t* d_out, uint64_t cap) {
  const char* fn = "sg_deflate_batch_dev";
  if (!ctx || !d_out_off || (n && !d_in_off) || (nbytes && !d_in) || (cap && !d_out)) {
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
  const size_t o_olen = deflate_ws(n), o_form = o_olen + align256(n * 4);
  if ((rc = ws_reserve(ctx, o_form + align256(n)))) return rc;
  uint32_t* olen = (uint32_t*)ws_at(ctx, o_olen);
  uint8_t* form = (uint8_t*)ws_at(ctx, o_form);
  const uint64_t* sorted = nullptr;
  if ((rc = deflate_count(ctx, d_in, d_in_off, d_in_off + 1, n, nbytes, olen, form, 0, &sorted))) return rc;
  if ((rc = deflate_offsets(ctx, olen, d_out_off, n, 0))) return rc;
  return deflate_write(ctx, d_in, d_in_off, d_in_off + 1, n, nbytes, sorted, d_out_off, nullptr, 0, d_out, cap);
}

int sg_deflate_batch(sg_ctx* ctx, const uint8_t* in, const uint64_t* in_off, size_t n, uint64_t* out_off, uint8_t* out,
                     size_t cap, size_t* nout) {
  const char* fn = "sg_deflate_batch";
  if (!ctx || !out_off || !nout || (cap && !out)) {
    set_error("%s: invalid argument", fn);
    return SG_EINVAL;
  }
  int rc = deflate_texts_ok(fn, in, in_off, n);
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
  const size_t o_in = plan.add(nbytes + 4), o_off = plan.add((n + 1) * 8), o_olen = plan.add(n * 4), o_form = plan.add(n),
               o_oo = plan.add((n + 1) * 8);
  if ((rc = dstage_reserve(ctx, plan))) return rc;
  if ((rc = ws_reserve(ctx, deflate_ws(n)))) return rc;
  uint8_t* din = dstage_at<uint8_t>(ctx, o_in);
  uint64_t* doff = dstage_at<uint64_t>(ctx, o_off);
  uint32_t* dolen = dstage_at<uint32_t>(ctx, o_olen);
  uint8_t* dform = dstage_at<uint8_t>(ctx, o_form);
  uint64_t* doo = dstage_at<uint64_t>(ctx, o_oo);
  if ((rc = upload(ctx, din, in, nbytes))) return rc;
  if ((rc = upload(ctx, doff, in_off, (n + 1) * 8))) return rc;
  const uint64_t* sorted = nullptr;
  if ((rc = deflate_count(ctx, din, doff, doff + 1, n, nbytes, dolen, dform, 0, &sorted))) return rc;
  if ((rc = deflate_offsets(ctx, dolen, doo, n, 0))) return rc;
  uint64_t total = 0;
  SG_HIP(hipMemcpyAsync(&total, doo + n, 8, hipMemcpyDeviceToHost, ctx->stream));
  SG_HIP(hipStreamSynchronize(ctx->stream));
  if (total >= kInflateMaxOut) {
    set_error("%s: %llu bytes of output (the limit is 2^33 - 1)", fn, (unsigned long long)total);
    return SG_EINVAL;
  }
  if (total <= cap) {  // (a stream has at least two bytes, so total > 0)
    if ((rc = ctx->inflate_out.grow_drop(grow_cap(ctx->inflate_out.cap, total, 16u << 20), ctx->stream))) return rc;
    if ((rc = deflate_write(ctx, din, doff, doff + 1, n, nbytes, sorted, doo, nullptr, 0, ctx->inflate_out.p, total)))
      return rc;
    SG_HIP(hipMemcpyAsync(out, ctx->inflate_out.p, total, hipMemcpyDeviceToHost, ctx->stream));
  }
  SG_HIP(hipMemcpyAsync(out_off, doo, (n + 1) * 8, hipMemcpyDeviceToHost, ctx->stream));
  SG_HIP(hipStreamSynchronize(ctx->stream));
  *nout = total;
  return SG_OK;
}

}  // extern "C"
