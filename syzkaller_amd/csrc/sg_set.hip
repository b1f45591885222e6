// sg_set.hip -- the signal set (map[uint32]struct{} replacement): its kernels
// and the sg_set_* entry points.
//
// Reference: the Go maps maxSignal / corpusSignal / newSignal
// (syz-fuzzer/fuzzer.go:65-68, syz-manager/manager.go:71-73) and the map
// helpers SignalNew / SignalDiff / SignalAdd (pkg/cover/cover.go:160-182).
// A set is a 2^32-bit bitmap in HBM: membership of s is bit s of word s>>5.
#include "sg_internal.h"

#include <memory>

namespace sg {

__global__ void k_set_add(uint32_t* __restrict__ words, const uint32_t* __restrict__ sig, uint64_t n) {
  uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride)
    sgd::set_bit(words, sig[i]);
}

// kOrU quads of `other` per thread in flight (one at a time left the 512 MiB
// pass latency-bound: 0.28 ms on a nearly empty `other`)
constexpr int kOrU = 4;
__global__ __launch_bounds__(256) void k_set_or(uint32_t* __restrict__ words, const uint32_t* __restrict__ other) {
  constexpr uint64_t q = kSetWords / 4;
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x * kOrU;
  for (uint64_t i0 = (uint64_t)blockIdx.x * blockDim.x * kOrU + threadIdx.x; i0 < q; i0 += stride) {
    uint4 b[kOrU];
#pragma unroll
    for (int u = 0; u < kOrU; u++) b[u] = reinterpret_cast<const uint4*>(other)[i0 + u * blockDim.x];
#pragma unroll
    for (int u = 0; u < kOrU; u++) {
      if (!(b[u].x | b[u].y | b[u].z | b[u].w)) continue;  // (a sparse `other` reads little else)
      uint4* p = reinterpret_cast<uint4*>(words) + i0 + u * blockDim.x;
      uint4 a = *p;
      a.x |= b[u].x;
      a.y |= b[u].y;
      a.z |= b[u].z;
      a.w |= b[u].w;
      *p = a;
    }
  }
}

// words |= other & ~exclude
__global__ __launch_bounds__(256) void k_set_or_new(uint32_t* __restrict__ words, const uint32_t* __restrict__ other,
                                                    const uint32_t* __restrict__ exclude) {
  constexpr uint64_t q = kSetWords / 4;
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x * kOrU;
  for (uint64_t i0 = (uint64_t)blockIdx.x * blockDim.x * kOrU + threadIdx.x; i0 < q; i0 += stride) {
    uint4 b[kOrU];
#pragma unroll
    for (int u = 0; u < kOrU; u++) b[u] = reinterpret_cast<const uint4*>(other)[i0 + u * blockDim.x];
#pragma unroll
    for (int u = 0; u < kOrU; u++) {
      if (!(b[u].x | b[u].y | b[u].z | b[u].w)) continue;
      const uint64_t i = i0 + u * blockDim.x;
      uint4 a = reinterpret_cast<uint4*>(words)[i];
      const uint4 x = reinterpret_cast<const uint4*>(exclude)[i];
      a.x |= b[u].x & ~x.x;
      a.y |= b[u].y & ~x.y;
      a.z |= b[u].z & ~x.z;
      a.w |= b[u].w & ~x.w;
      reinterpret_cast<uint4*>(words)[i] = a;
    }
  }
}

// newsig |= other & ~maxsig; maxsig |= other (newsig nullable)
__global__ __launch_bounds__(256) void k_set_or_new_or(uint32_t* __restrict__ newsig, uint32_t* __restrict__ maxsig,
                                                       const uint32_t* __restrict__ other) {
  constexpr uint64_t q = kSetWords / 4;
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x * kOrU;
  for (uint64_t i0 = (uint64_t)blockIdx.x * blockDim.x * kOrU + threadIdx.x; i0 < q; i0 += stride) {
    uint4 b[kOrU];
#pragma unroll
    for (int u = 0; u < kOrU; u++) b[u] = reinterpret_cast<const uint4*>(other)[i0 + u * blockDim.x];
#pragma unroll
    for (int u = 0; u < kOrU; u++) {
      if (!(b[u].x | b[u].y | b[u].z | b[u].w)) continue;
      const uint64_t i = i0 + u * blockDim.x;
      uint4 m = reinterpret_cast<uint4*>(maxsig)[i];
      if (newsig) {
        uint4 n = reinterpret_cast<uint4*>(newsig)[i];
        n.x |= b[u].x & ~m.x;
        n.y |= b[u].y & ~m.y;
        n.z |= b[u].z & ~m.z;
        n.w |= b[u].w & ~m.w;
        reinterpret_cast<uint4*>(newsig)[i] = n;
      }
      m.x |= b[u].x;
      m.y |= b[u].y;
      m.z |= b[u].z;
      m.w |= b[u].w;
      reinterpret_cast<uint4*>(maxsig)[i] = m;
    }
  }
}

__global__ void k_set_new(const uint32_t* __restrict__ words, const uint32_t* __restrict__ sig, uint64_t n,
                          uint64_t* __restrict__ flag) {
  uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  bool miss = false;
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride)
    miss |= !sgd::test_bit(words, sig[i]);
  if (__any(miss) && (threadIdx.x & 63) == 0) *flag = 1;
}

__global__ void k_count_missing(const uint32_t* __restrict__ words, const uint32_t* __restrict__ v, uint64_t n,
                                unsigned long long* __restrict__ out) {
  uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  uint32_t c = 0;
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride)
    c += !sgd::test_bit(words, v[i]);
  for (int o = 32; o > 0; o >>= 1) c += __shfl_down(c, o);
  if ((threadIdx.x & 63) == 0 && c) atomicAdd(out, (unsigned long long)c);
}

// popcount of the bitmap, per 4096-word tile (for count and export)
__global__ __launch_bounds__(kBlock) void k_set_tile_pop(const uint32_t* __restrict__ words,
                                                         uint32_t* __restrict__ tile_cnt) {
  __shared__ uint32_t red[kBlock / 64];
  // tiles of 4096 words in signal order (sgd::set_word), as the export walks them
  uint32_t c = 0;
#pragma unroll
  for (int j = 0; j < kTile / 4 / kBlock; j++) {
    const uint32_t ws = (uint32_t)blockIdx.x * kTile + (j * kBlock + threadIdx.x) * 4;
    const uint4 v = *reinterpret_cast<const uint4*>(words + sgd::set_word(ws));
    c += __popc(v.x) + __popc(v.y) + __popc(v.z) + __popc(v.w);
  }
  for (int o = 32; o > 0; o >>= 1) c += __shfl_down(c, o);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x / 64] = c;
  __syncthreads();
  if (threadIdx.x == 0) tile_cnt[blockIdx.x] = red[0] + red[1] + red[2] + red[3];
}

// each thread owns 16 consecutive words of the tile; block-scan of their
// popcounts gives each thread's first output slot.
__global__ __launch_bounds__(kBlock) void k_set_export(const uint32_t* __restrict__ words,
                                                       const uint64_t* __restrict__ tile_base,
                                                       uint32_t* __restrict__ out, uint64_t cap) {
  __shared__ uint32_t part[kBlock];
  uint64_t w0 = (uint64_t)blockIdx.x * kTile + (uint64_t)threadIdx.x * 16;
  uint64_t tb = tile_base[blockIdx.x];
  if (tile_base[blockIdx.x + 1] == tb) return;  // empty tile (block-uniform)
  // signal-order words w0 .. w0+15: two runs of 8 consecutive bitmap words
  const uint4* r0 = reinterpret_cast<const uint4*>(words + sgd::set_word((uint32_t)w0));
  const uint4* r1 = reinterpret_cast<const uint4*>(words + sgd::set_word((uint32_t)w0 + 8));
  uint32_t w[16];
  uint32_t c = 0;
#pragma unroll
  for (int j = 0; j < 4; j++) {
    uint4 v = j < 2 ? r0[j] : r1[j - 2];
    w[4 * j] = v.x;
    w[4 * j + 1] = v.y;
    w[4 * j + 2] = v.z;
    w[4 * j + 3] = v.w;
    c += __popc(v.x) + __popc(v.y) + __popc(v.z) + __popc(v.w);
  }
  part[threadIdx.x] = c;
  __syncthreads();
  for (int d = 1; d < kBlock; d <<= 1) {
    uint32_t x = threadIdx.x >= (unsigned)d ? part[threadIdx.x - d] : 0;
    __syncthreads();
    part[threadIdx.x] += x;
    __syncthreads();
  }
  uint64_t pos = tb + part[threadIdx.x] - c;
#pragma unroll
  for (int j = 0; j < 16; j++) {
    uint32_t x = w[j];
    while (x) {
      int b = __ffs(x) - 1;
      x &= x - 1;
      if (pos < cap) out[pos] = (uint32_t)((w0 + j) * 32 + b);
      pos++;
    }
  }
}

}  // namespace sg

using namespace sg;

extern "C" {

int sg_set_create(sg_ctx* ctx, sg_set** out) {
  if (!ctx || !out) return SG_EINVAL;
  std::lock_guard<std::mutex> g(ctx->mu);
  int rc = ensure_device(ctx);
  if (rc) return rc;
  std::unique_ptr<sg_set> s(new sg_set());
  s->ctx = ctx;
  rc = s->mem.grow_drop(kSetWords, nullptr);
  if (rc) return rc;
  SG_HIP(hipMemsetAsync(s->mem.p, 0, kSetBytes, ctx->stream));
  s->words = s->mem.p;
  *out = s.release();
  return SG_OK;
}

void sg_set_destroy(sg_set* set) {
  if (!set) return;
  hipSetDevice(set->ctx->device);
  hipStreamSynchronize(set->ctx->stream);
  delete set;  // (a wrapper's words are the caller's)
}

int sg_set_clear(sg_set* set) {
  if (!set) return SG_EINVAL;
  sg_ctx* ctx = set->ctx;
  std::lock_guard<std::mutex> g(ctx->mu);
  int rc = ensure_device(ctx);
  if (rc) return rc;
  SG_HIP(hipMemsetAsync(set->words, 0, kSetBytes, ctx->stream));
  return SG_OK;
}

void* sg_set_device_words(sg_set* set) { return set ? set->words : nullptr; }

int sg_set_wrap_dev(sg_ctx* ctx, void* d_words, sg_set** out) {
  if (!ctx || !d_words || !out || ((uintptr_t)d_words & 15)) {
    set_error("sg_set_wrap_dev: invalid argument (words must be 16-B aligned device memory)");
    return SG_EINVAL;
  }
  sg_set* s = new sg_set();
  s->ctx = ctx;
  s->words = (uint32_t*)d_words;
  *out = s;
  return SG_OK;
}

int sg_set_copy(sg_set* dst, sg_set* src) {
  if (!dst || !src || dst->ctx != src->ctx) return SG_EINVAL;
  sg_ctx* ctx = dst->ctx;
  std::lock_guard<std::mutex> g(ctx->mu);
  int rc = ensure_device(ctx);
  if (rc) return rc;
  if (dst != src) SG_HIP(hipMemcpyAsync(dst->words, src->words, kSetBytes, hipMemcpyDeviceToDevice, ctx->stream));
  return SG_OK;
}

int sg_set_count_missing_dev(sg_set* set, const uint32_t* d_vals, uint64_t n, uint64_t* out) {
  if (!set || !out || (n && !d_vals)) return SG_EINVAL;
  *out = 0;
  if (n == 0) return SG_OK;
  sg_ctx* ctx = set->ctx;
  std::lock_guard<std::mutex> g(ctx->mu);
  int rc = ensure_device(ctx);
  if (rc) return rc;
  SG_HIP(hipMemsetAsync(&ctx->dev.p->scalar, 0, 8, ctx->stream));
  hipLaunchKernelGGL(k_count_missing, dim3(2048), dim3(256), 0, ctx->stream, set->words, d_vals, n,
                     (unsigned long long*)&ctx->dev.p->scalar);
  SG_HIP(hipGetLastError());
  SG_HIP(hipMemcpyAsync(out, &ctx->dev.p->scalar, 8, hipMemcpyDeviceToHost, ctx->stream));
  SG_HIP(hipStreamSynchronize(ctx->stream));
  return SG_OK;
}

int sg_set_or_dev(sg_set* set, const uint32_t* d_words) {
  if (!set || !d_words) return SG_EINVAL;
  sg_ctx* ctx = set->ctx;
  std::lock_guard<std::mutex> g(ctx->mu);
  int rc = ensure_device(ctx);
  if (rc) return rc;
  ScopedTimer tm(ctx, "set_or");
  hipLaunchKernelGGL(k_set_or, dim3(4096), dim3(256), 0, ctx->stream, set->words, d_words);
  SG_HIP(hipGetLastError());
  return SG_OK;
}

int sg_set_or_new_or_dev(sg_set* newsig, sg_set* maxsig, const uint32_t* d_words) {
  if (!maxsig || !d_words || (newsig && (newsig->ctx != maxsig->ctx || newsig == maxsig ||
                                         d_words == (const uint32_t*)newsig->words)) ||
      d_words == (const uint32_t*)maxsig->words) {
    // k_set_or_new_or takes all three __restrict__: no aliasing
    set_error("sg_set_or_new_or_dev: invalid argument (null, another context's set, or aliasing sets / words)");
    return SG_EINVAL;
  }
  sg_ctx* ctx = maxsig->ctx;
  std::lock_guard<std::mutex> g(ctx->mu);
  int rc = ensure_device(ctx);
  if (rc) return rc;
  ScopedTimer tm(ctx, "set_or_new_or");
  hipLaunchKernelGGL(k_set_or_new_or, dim3(4096), dim3(256), 0, ctx->stream, newsig ? newsig->words : nullptr,
                     maxsig->words, d_words);
  SG_HIP(hipGetLastError());
  return SG_OK;
}

int sg_set_or_new_dev(sg_set* set, const uint32_t* d_words, sg_set* exclude) {
  if (!set || !d_words || !exclude || exclude->ctx != set->ctx || exclude == set ||
      d_words == (const uint32_t*)set->words) {
    // k_set_or_new takes words and exclude __restrict__: no aliasing
    set_error("sg_set_or_new_dev: invalid argument (null, another context's set, or exclude/words aliasing set)");
    return SG_EINVAL;
  }
  sg_ctx* ctx = set->ctx;
  std::lock_guard<std::mutex> g(ctx->mu);
  int rc = ensure_device(ctx);
  if (rc) return rc;
  ScopedTimer tm(ctx, "set_or_new");
  hipLaunchKernelGGL(k_set_or_new, dim3(4096), dim3(256), 0, ctx->stream, set->words, d_words, exclude->words);
  SG_HIP(hipGetLastError());
  return SG_OK;
}

static int set_tile_bases(sg_set* set, uint64_t** bases_out, uint64_t* total) {
  sg_ctx* ctx = set->ctx;
  const uint64_t ntile = kSetWords / kTile;  // 32768
  WsPlan p;
  size_t o_cnt = p.add(ntile * 4);
  size_t o_base = p.add((ntile + 1) * 8);
  int rc = ws_reserve(ctx, p.total + scan_ws_bytes(ntile));
  if (rc) return rc;
  uint32_t* cnt = (uint32_t*)ws_at(ctx, o_cnt);
  uint64_t* base = (uint64_t*)ws_at(ctx, o_base);
  hipLaunchKernelGGL(k_set_tile_pop, dim3((uint32_t)ntile), dim3(kBlock), 0, ctx->stream, set->words, cnt);
  rc = scan_counts(ctx, cnt, base, ntile, p.total);
  if (rc) return rc;
  SG_HIP(hipMemcpyAsync(total, base + ntile, 8, hipMemcpyDeviceToHost, ctx->stream));
  SG_HIP(hipStreamSynchronize(ctx->stream));
  *bases_out = base;
  return SG_OK;
}

int sg_set_count(sg_set* set, uint64_t* out) {
  if (!set || !out) return SG_EINVAL;
  sg_ctx* ctx = set->ctx;
  std::lock_guard<std::mutex> g(ctx->mu);
  int rc = ensure_device(ctx);
  if (rc) return rc;
  uint64_t* bases;
  return set_tile_bases(set, &bases, out);
}

}  // extern "C"

namespace sg {
// The members of `set`, ascending, into device memory d_out (capacity cap);
// *total = count (ctx lock held; syncs).
int set_export_dev(sg_set* set, uint32_t* d_out, uint64_t cap, uint64_t* total) {
  sg_ctx* ctx = set->ctx;
  uint64_t* bases;
  int rc = set_tile_bases(set, &bases, total);
  if (rc) return rc;
  const uint64_t m = *total < cap ? *total : cap;
  if (m == 0) return SG_OK;
  hipLaunchKernelGGL(k_set_export, dim3((uint32_t)(kSetWords / kTile)), dim3(kBlock), 0, ctx->stream, set->words,
                     bases, d_out, m);
  SG_HIP(hipGetLastError());
  return SG_OK;
}

// SignalAdd of n device-resident values (ctx lock held, stream-ordered).
int set_add_dev_locked(sg_set* set, const uint32_t* d_vals, uint64_t n) {
  if (n == 0) return SG_OK;
  ScopedTimer tm(set->ctx, "set_add");
  hipLaunchKernelGGL(k_set_add, dim3(std::min<uint64_t>(div_up(n, 256), 8192)), dim3(256), 0, set->ctx->stream,
                     set->words, d_vals, n);
  SG_HIP(hipGetLastError());
  return SG_OK;
}
}  // namespace sg

extern "C" {

int sg_set_export(sg_set* set, uint32_t* out, size_t cap, size_t* n) {
  if (!set || !n || (cap && !out)) return SG_EINVAL;
  sg_ctx* ctx = set->ctx;
  std::lock_guard<std::mutex> g(ctx->mu);
  int rc = ensure_device(ctx);
  if (rc) return rc;
  uint64_t* bases;
  uint64_t total = 0;
  rc = set_tile_bases(set, &bases, &total);
  if (rc) return rc;
  *n = (size_t)total;
  uint64_t m = total < cap ? total : cap;
  if (m == 0) return SG_OK;
  // output staged in the workspace after the scan area
  size_t used = ((kSetWords / kTile) * 4 + 255) / 256 * 256 + (((kSetWords / kTile) + 1) * 8 + 255) / 256 * 256;
  const size_t o_out = align256(used + scan_ws_bytes(kSetWords / kTile));
  rc = ws_reserve(ctx, o_out + m * 4);
  if (rc) return rc;
  // ws may have been reallocated: recompute the tile bases if so
  rc = set_tile_bases(set, &bases, &total);
  if (rc) return rc;
  uint32_t* dout = (uint32_t*)ws_at(ctx, o_out);
  hipLaunchKernelGGL(k_set_export, dim3((uint32_t)(kSetWords / kTile)), dim3(kBlock), 0, ctx->stream, set->words,
                     bases, dout, (uint64_t)m);
  SG_HIP(hipGetLastError());
  SG_HIP(hipMemcpyAsync(out, dout, m * 4, hipMemcpyDeviceToHost, ctx->stream));
  SG_HIP(hipStreamSynchronize(ctx->stream));
  return SG_OK;
}

int sg_set_add(sg_set* set, const uint32_t* sig, size_t n) {
  if (!set || (n && !sig)) return SG_EINVAL;
  if (n == 0) return SG_OK;
  sg_ctx* ctx = set->ctx;
  std::lock_guard<std::mutex> g(ctx->mu);
  int rc = ensure_device(ctx);
  if (rc) return rc;
  rc = ws_reserve(ctx, n * 4);
  if (rc) return rc;
  uint32_t* d = (uint32_t*)ctx->ws.p;
  SG_HIP(hipMemcpyAsync(d, sig, n * 4, hipMemcpyHostToDevice, ctx->stream));
  {
    ScopedTimer tm(ctx, "set_add");
    hipLaunchKernelGGL(k_set_add, dim3(std::min<uint64_t>(div_up(n, 256), 8192)), dim3(256), 0, ctx->stream,
                       set->words, d, (uint64_t)n);
  }
  SG_HIP(hipGetLastError());
  SG_HIP(hipStreamSynchronize(ctx->stream));
  return SG_OK;
}

int sg_set_new(sg_set* set, const uint32_t* sig, size_t n, int* out) {
  if (!set || !out || (n && !sig)) return SG_EINVAL;
  *out = 0;
  if (n == 0) return SG_OK;
  sg_ctx* ctx = set->ctx;
  std::lock_guard<std::mutex> g(ctx->mu);
  int rc = ensure_device(ctx);
  if (rc) return rc;
  rc = ws_reserve(ctx, n * 4);
  if (rc) return rc;
  uint32_t* d = (uint32_t*)ctx->ws.p;
  SG_HIP(hipMemcpyAsync(d, sig, n * 4, hipMemcpyHostToDevice, ctx->stream));
  SG_HIP(hipMemsetAsync(&ctx->dev.p->scalar, 0, 8, ctx->stream));
  hipLaunchKernelGGL(k_set_new, dim3(std::min<uint64_t>(div_up(n, 256), 8192)), dim3(256), 0, ctx->stream,
                     set->words, d, (uint64_t)n, &ctx->dev.p->scalar);
  SG_HIP(hipGetLastError());
  uint64_t flag = 0;
  SG_HIP(hipMemcpyAsync(&flag, &ctx->dev.p->scalar, 8, hipMemcpyDeviceToHost, ctx->stream));
  SG_HIP(hipStreamSynchronize(ctx->stream));
  *out = flag ? 1 : 0;
  return SG_OK;
}

}  // extern "C"
