// sg_tinput.hip -- triageInput's signal math over a batch of inputs.
//
// Reference: syz-fuzzer/fuzzer.go:521-611 triageInput():
//   :526-532  newSignal = Canonicalize(SignalDiff(corpusSignal, inp.signal))
//   :567      newSignal = Intersection(newSignal, Canonicalize(inf.Signal))
//             after each of the 3 re-executions
//   :584-587  the minimisation predicate
//             len(Intersection(newSignal, Canonicalize(inf.Signal))) == len(newSignal)
// A fuzzer runs -procs triage goroutines; these entry points take the inputs
// of all of them (or of a whole batch of triage candidates) at once.  The
// executions in between stay with the caller.
//
// Intersection(a, Canonicalize(r)) for a sorted a (cover.go:72-102): r's
// canonical form holds each value at most once, so the foreach keeps the
// first copy of every value of a that occurs in r, except 0xFFFFFFFF (which
// foreach always drops), in a's order.  No sort of r is needed: one
// workgroup per input holds a (in LDS chunks of kCap values) and every element
// of r marks the first copy of its value in a by a binary search.
#include "sg_tinput.h"

namespace sg {
namespace {

using namespace tin;  // block_rank, k_tin_diff, tin_intersect (sg_tinput.h)

// Intersection(a_k, Canonicalize(r_k)) for every input k (see the header):
// kIntersect writes the kept values at a_k's own start and out_len[k];
// otherwise ok[k] = (kept == len(a_k)).
template <bool kIntersect>
__global__ __launch_bounds__(kTB) void k_tin_intersect(uint32_t* __restrict__ a, const uint64_t* __restrict__ a_off,
                                                       const uint32_t* __restrict__ r,
                                                       const uint64_t* __restrict__ r_off,
                                                       uint64_t* __restrict__ out_len, uint8_t* __restrict__ ok) {
  __shared__ IntersectLds lds;
  const uint64_t k = blockIdx.x, a0 = a_off[k], a1 = a_off[k + 1];
  const uint64_t kept = tin_intersect<kIntersect>(a, a0, a1, r, r_off[k], r_off[k + 1], lds);
  if (threadIdx.x == 0) {
    if (kIntersect)
      out_len[k] = kept;
    else
      ok[k] = kept == a1 - a0 ? 1 : 0;
  }
}

// dst[dst_off[k] ..] = src[src_off[k] .. + len[k]), one wave per segment
__global__ void k_seg_pack(const uint32_t* __restrict__ src, const uint64_t* __restrict__ src_off,
                           const uint64_t* __restrict__ len, const uint64_t* __restrict__ dst_off, uint64_t n,
                           uint32_t* __restrict__ dst) {
  const uint64_t k = (uint64_t)blockIdx.x * (blockDim.x / 64) + (threadIdx.x >> 6);
  if (k >= n) return;
  const uint64_t s = src_off[k], d = dst_off[k], L = len[k];
  for (uint64_t i = threadIdx.x & 63; i < L; i += 64) dst[d + i] = src[s + i];
}

}  // namespace
}  // namespace sg

using namespace sg;

extern "C" {

int sg_triage_newsig(sg_ctx* ctx, sg_set* corpus, const uint32_t* vals, const uint64_t* off, size_t n,
                     uint32_t* new_vals, uint64_t* new_off) {
  if (!ctx || !corpus || corpus->ctx != ctx || !off || !new_off || !offsets_ok(off, n) ||
      (off[n] && (!vals || !new_vals))) {
    set_error("sg_triage_newsig: invalid argument");
    return SG_EINVAL;
  }
  const uint64_t N = off[n];
  if (n == 0 || N == 0) {
    for (size_t k = 0; k <= n; k++) new_off[k] = 0;
    return SG_OK;
  }
  std::lock_guard<std::mutex> g(ctx->mu);
  int rc = ensure_device(ctx);
  if (rc) return rc;
  // staged: S vals | S off | diff vals | diff off | canonical lengths | packed off | packed vals
  WsPlan sp;
  const size_t o_v = sp.add(N * 4), o_off = sp.add((n + 1) * 8), o_diff = sp.add(N * 4), o_doff = sp.add((n + 1) * 8),
               o_len = sp.add((n + 1) * 8), o_poff = sp.add((n + 1) * 8), o_pack = sp.add(N * 4);
  rc = dstage_reserve(ctx, sp);
  if (rc) return rc;
  uint32_t* dv = dstage_at<uint32_t>(ctx, o_v);
  uint64_t* doff = dstage_at<uint64_t>(ctx, o_off);
  uint32_t* ddiff = dstage_at<uint32_t>(ctx, o_diff);
  uint64_t* ddoff = dstage_at<uint64_t>(ctx, o_doff);
  uint64_t* dlen = dstage_at<uint64_t>(ctx, o_len);
  uint64_t* dpoff = dstage_at<uint64_t>(ctx, o_poff);
  uint32_t* dpack = dstage_at<uint32_t>(ctx, o_pack);
  WsPlan p;
  const size_t o_cnt = p.add(n * 4);
  rc = ws_reserve(ctx, p.total + scan_ws_bytes(n));
  if (rc) return rc;
  uint32_t* dcnt = (uint32_t*)ws_at(ctx, o_cnt);
  SG_HIP(hipMemcpyAsync(dv, vals, N * 4, hipMemcpyHostToDevice, ctx->stream));
  SG_HIP(hipMemcpyAsync(doff, off, (n + 1) * 8, hipMemcpyHostToDevice, ctx->stream));
  {
    ScopedTimer tm(ctx, "tinput_diff");
    hipLaunchKernelGGL(k_tin_diff<false>, dim3((uint32_t)n), dim3(kTB), 0, ctx->stream, corpus->words, dv, doff, dcnt,
                       nullptr, nullptr);
    rc = scan_counts(ctx, dcnt, ddoff, n, p.total);
    if (rc) return rc;
    hipLaunchKernelGGL(k_tin_diff<true>, dim3((uint32_t)n), dim3(kTB), 0, ctx->stream, corpus->words, dv, doff, nullptr,
                       ddoff, ddiff);
  }
  SG_HIP(hipGetLastError());
  std::vector<uint64_t> hdoff(n + 1), len(n);
  SG_HIP(hipMemcpyAsync(hdoff.data(), ddoff, (n + 1) * 8, hipMemcpyDeviceToHost, ctx->stream));
  SG_HIP(hipStreamSynchronize(ctx->stream));
  if (hdoff[n] == 0) {
    for (size_t k = 0; k <= n; k++) new_off[k] = 0;
    return SG_OK;
  }
  // Canonicalize (cover.go:28-40) of every diff segment, in place
  rc = canonicalize_dev(ctx, ddiff, hdoff.data(), n, len.data());
  if (rc) return rc;
  new_off[0] = 0;
  for (size_t k = 0; k < n; k++) new_off[k + 1] = new_off[k] + len[k];
  SG_HIP(hipMemcpyAsync(dlen, len.data(), n * 8, hipMemcpyHostToDevice, ctx->stream));
  SG_HIP(hipMemcpyAsync(dpoff, new_off, (n + 1) * 8, hipMemcpyHostToDevice, ctx->stream));
  hipLaunchKernelGGL(k_seg_pack, dim3(div_up(n, 4)), dim3(256), 0, ctx->stream, ddiff, ddoff, dlen, dpoff,
                     (uint64_t)n, dpack);
  SG_HIP(hipGetLastError());
  if (new_off[n]) SG_HIP(hipMemcpyAsync(new_vals, dpack, new_off[n] * 4, hipMemcpyDeviceToHost, ctx->stream));
  SG_HIP(hipStreamSynchronize(ctx->stream));
  return SG_OK;
}

static int tinput_intersect(sg_ctx* ctx, uint32_t* a, const uint64_t* a_off, const uint32_t* r, const uint64_t* r_off,
                            size_t n, uint64_t* out_len, uint8_t* ok) {
  const uint64_t NA = a_off[n], NR = r_off[n];
  std::lock_guard<std::mutex> g(ctx->mu);
  int rc = ensure_device(ctx);
  if (rc) return rc;
  WsPlan p;
  const size_t o_a = p.add(NA * 4), o_r = p.add(NR * 4), o_ao = p.add((n + 1) * 8), o_ro = p.add((n + 1) * 8),
               o_len = p.add((n + 1) * 8), o_ok = p.add(n);
  rc = dstage_reserve(ctx, p);
  if (rc) return rc;
  uint32_t* da = dstage_at<uint32_t>(ctx, o_a);
  uint32_t* dr = dstage_at<uint32_t>(ctx, o_r);
  uint64_t* dao = dstage_at<uint64_t>(ctx, o_ao);
  uint64_t* dro = dstage_at<uint64_t>(ctx, o_ro);
  uint64_t* dlen = dstage_at<uint64_t>(ctx, o_len);
  uint8_t* dok = dstage_at<uint8_t>(ctx, o_ok);
  if ((rc = upload(ctx, da, a, NA * 4))) return rc;
  if ((rc = upload(ctx, dr, r, NR * 4))) return rc;
  if ((rc = upload(ctx, dao, a_off, (n + 1) * 8))) return rc;
  if ((rc = upload(ctx, dro, r_off, (n + 1) * 8))) return rc;
  {
    ScopedTimer tm(ctx, "tinput_intersect");
    if (out_len)
      hipLaunchKernelGGL(k_tin_intersect<true>, dim3((uint32_t)n), dim3(kTB), 0, ctx->stream, da, dao, dr, dro, dlen,
                         nullptr);
    else
      hipLaunchKernelGGL(k_tin_intersect<false>, dim3((uint32_t)n), dim3(kTB), 0, ctx->stream, da, dao, dr, dro,
                         nullptr, dok);
  }
  SG_HIP(hipGetLastError());
  if (out_len) {
    SG_HIP(hipMemcpyAsync(out_len, dlen, n * 8, hipMemcpyDeviceToHost, ctx->stream));
    if (NA) SG_HIP(hipMemcpyAsync(a, da, NA * 4, hipMemcpyDeviceToHost, ctx->stream));
  } else {
    SG_HIP(hipMemcpyAsync(ok, dok, n, hipMemcpyDeviceToHost, ctx->stream));
  }
  SG_HIP(hipStreamSynchronize(ctx->stream));
  return SG_OK;
}

int sg_triage_intersect(sg_ctx* ctx, uint32_t* new_vals, const uint64_t* new_off, const uint32_t* r_vals,
                        const uint64_t* r_off, size_t n, uint64_t* out_len) {
  if (!ctx || !new_off || !r_off || (n && !out_len) || !offsets_ok(new_off, n) || !offsets_ok(r_off, n) ||
      (new_off[n] && !new_vals) || (r_off[n] && !r_vals)) {
    set_error("sg_triage_intersect: invalid argument");
    return SG_EINVAL;
  }
  if (n == 0) return SG_OK;
  if (new_off[n] == 0) {
    for (size_t k = 0; k < n; k++) out_len[k] = 0;
    return SG_OK;
  }
  return tinput_intersect(ctx, new_vals, new_off, r_vals, r_off, n, out_len, nullptr);
}

int sg_triage_subset(sg_ctx* ctx, const uint32_t* new_vals, const uint64_t* new_off, const uint32_t* r_vals,
                     const uint64_t* r_off, size_t n, uint8_t* ok) {
  if (!ctx || !new_off || !r_off || (n && !ok) || !offsets_ok(new_off, n) || !offsets_ok(r_off, n) ||
      (new_off[n] && !new_vals) || (r_off[n] && !r_vals)) {
    set_error("sg_triage_subset: invalid argument");
    return SG_EINVAL;
  }
  if (n == 0) return SG_OK;
  if (new_off[n] == 0) {
    for (size_t k = 0; k < n; k++) ok[k] = 1;  // len(Intersection(nil, x)) == 0 == len(nil)
    return SG_OK;
  }
  return tinput_intersect(ctx, const_cast<uint32_t*>(new_vals), new_off, r_vals, r_off, n, nullptr, ok);
}

}  // extern "C"
