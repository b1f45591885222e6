// sg_scan.hip -- the device scan: exclusive prefix of u32 counts into u64
// offsets (scan_counts), used by every stage that sizes its outputs on the device.
#include "sg_internal.h"

namespace sg {

constexpr int kScanItems = 16;
constexpr int kScanTile = kBlock * kScanItems;  // 4096

__global__ __launch_bounds__(kBlock) void k_scan_tile(const uint32_t* __restrict__ in, uint64_t n,
                                                      uint64_t* __restrict__ out, uint64_t* __restrict__ tile_sum) {
  __shared__ uint64_t part[kBlock];
  uint64_t base = (uint64_t)blockIdx.x * kScanTile + (uint64_t)threadIdx.x * kScanItems;
  uint32_t v[kScanItems];
  uint64_t s = 0;
#pragma unroll
  for (int i = 0; i < kScanItems; i++) {
    uint64_t idx = base + i;
    v[i] = idx < n ? in[idx] : 0u;
    s += v[i];
  }
  part[threadIdx.x] = s;
  __syncthreads();
  // Hillis-Steele over 256 partials (inclusive)
  for (int d = 1; d < kBlock; d <<= 1) {
    uint64_t x = threadIdx.x >= (unsigned)d ? part[threadIdx.x - d] : 0;
    __syncthreads();
    part[threadIdx.x] += x;
    __syncthreads();
  }
  uint64_t run = threadIdx.x ? part[threadIdx.x - 1] : 0;
#pragma unroll
  for (int i = 0; i < kScanItems; i++) {
    uint64_t idx = base + i;
    if (idx < n) out[idx] = run;
    run += v[i];
  }
  if (threadIdx.x == kBlock - 1) tile_sum[blockIdx.x] = part[kBlock - 1];
}

__global__ __launch_bounds__(kBlock) void k_scan_u64_tile(uint64_t* __restrict__ data, uint64_t n,
                                                          uint64_t* __restrict__ tile_sum) {
  // in-place exclusive scan of u64 values, per 4096-tile
  __shared__ uint64_t part[kBlock];
  uint64_t base = (uint64_t)blockIdx.x * kScanTile + (uint64_t)threadIdx.x * kScanItems;
  uint64_t v[kScanItems];
  uint64_t s = 0;
#pragma unroll
  for (int i = 0; i < kScanItems; i++) {
    uint64_t idx = base + i;
    v[i] = idx < n ? data[idx] : 0u;
    s += v[i];
  }
  part[threadIdx.x] = s;
  __syncthreads();
  for (int d = 1; d < kBlock; d <<= 1) {
    uint64_t x = threadIdx.x >= (unsigned)d ? part[threadIdx.x - d] : 0;
    __syncthreads();
    part[threadIdx.x] += x;
    __syncthreads();
  }
  uint64_t run = threadIdx.x ? part[threadIdx.x - 1] : 0;
#pragma unroll
  for (int i = 0; i < kScanItems; i++) {
    uint64_t idx = base + i;
    if (idx < n) data[idx] = run;
    run += v[i];
  }
  if (threadIdx.x == kBlock - 1) tile_sum[blockIdx.x] = part[kBlock - 1];
}

__global__ void k_scan_add(uint64_t* __restrict__ out, uint64_t n, const uint64_t* __restrict__ tile_base) {
  uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) out[i] += tile_base[i / kScanTile];
}

__global__ void k_scan_total(uint64_t* out, uint64_t n, const uint64_t* tile_base, const uint64_t* tile_sum,
                             uint64_t ntiles) {
  out[n] = ntiles ? tile_base[ntiles - 1] + tile_sum[ntiles - 1] : 0;
}

size_t scan_ws_bytes(uint64_t n) {
  // (a single count has a level too: its one tile's sum and base, and the sum
  // the scan of that base writes behind them)
  size_t b = 0;
  do {
    uint64_t t = (n + kScanTile - 1) / kScanTile;
    b += 2 * ((t * 8 + 255) & ~255ull);
    n = t;
  } while (n > 1);
  return b + 512;
}

__global__ void k_copy_u64(const uint64_t* __restrict__ in, uint64_t n, uint64_t* __restrict__ out) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) out[i] = in[i];
}

static int scan_u64_inplace(sg_ctx* ctx, uint64_t* data, uint64_t n, char* scratch) {
  // exclusive in-place scan of n u64 values (used for tile sums)
  if (n == 0) return SG_OK;
  uint64_t nt = (n + kScanTile - 1) / kScanTile;
  uint64_t* sums = (uint64_t*)scratch;
  char* next = scratch + ((nt * 8 + 255) & ~255ull);
  hipLaunchKernelGGL(k_scan_u64_tile, dim3((uint32_t)nt), dim3(kBlock), 0, ctx->stream, data, n, sums);
  if (nt > 1) {
    int rc = scan_u64_inplace(ctx, sums, nt, next);
    if (rc) return rc;
    hipLaunchKernelGGL(k_scan_add, dim3(div_up(n, 256)), dim3(256), 0, ctx->stream, data, n, sums);
  }
  return SG_OK;
}

int scan_counts(sg_ctx* ctx, const uint32_t* d_in, uint64_t* d_out, uint64_t n, size_t ws_used) {
  ScopedTimer tm(ctx, "scan");
  char* scratch = ctx->ws.p + ws_used;
  uint64_t nt = n ? (n + kScanTile - 1) / kScanTile : 0;
  uint64_t* sums = (uint64_t*)scratch;
  uint64_t* bases = (uint64_t*)(scratch + ((nt * 8 + 255) & ~255ull));
  char* next = (char*)bases + ((nt * 8 + 255) & ~255ull);
  if (n == 0) {
    SG_HIP(hipMemsetAsync(d_out, 0, 8, ctx->stream));
    return SG_OK;
  }
  hipLaunchKernelGGL(k_scan_tile, dim3((uint32_t)nt), dim3(kBlock), 0, ctx->stream, d_in, n, d_out, sums);
  // (a copy kernel: a device-to-device hipMemcpyAsync between two kernels
  // leaves the stream idle around it)
  hipLaunchKernelGGL(k_copy_u64, dim3(div_up(nt, 256)), dim3(256), 0, ctx->stream, (const uint64_t*)sums, nt, bases);
  int rc = scan_u64_inplace(ctx, bases, nt, next);
  if (rc) return rc;
  if (nt > 1) hipLaunchKernelGGL(k_scan_add, dim3(div_up(n, 256)), dim3(256), 0, ctx->stream, d_out, n, bases);
  hipLaunchKernelGGL(k_scan_total, dim3(1), dim3(1), 0, ctx->stream, d_out, n, bases, sums, nt);
  SG_HIP(hipGetLastError());
  return SG_OK;
}

}  // namespace sg
