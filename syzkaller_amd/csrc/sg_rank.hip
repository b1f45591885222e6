// sg_rank.hip -- the stages every "distinct values, then ranks" path is made
// of (sg_rank.h): sort, mark the run starts, scan, write the distinct values,
// rank by binary search; and for groups (calls) of such values, the sort of
// group << 32 | rank with each group's first place among its first occurrences.
// The general paths of sg_exec_comps.hip and sg_exec_cover.hip are built of
// them, the replacers' sort of sg_hints.hip and the slot table of
// sg_cover_lines.hip of the first.
// Every loop is bounded by a count known on entry (a group's members) or halves
// its interval (sgd::lb64: at most 64 steps).
#include "sg_rank.h"

namespace sg {

__global__ void k_rank_mark(const uint64_t* __restrict__ a, uint64_t n, uint32_t* __restrict__ flags) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) flags[i] = i == 0 || a[i] != a[i - 1];
}
__global__ void k_rank_unique(const uint64_t* __restrict__ a, const uint32_t* __restrict__ flags,
                              const uint64_t* __restrict__ pos, uint64_t n, uint64_t* __restrict__ u) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n && flags[i]) u[pos[i]] = a[i];
}
// rank[i] = the place of v[i] among the nu distinct values u (ascending): v[i] is one of them
__global__ void k_rank_u32(const uint64_t* __restrict__ v, uint64_t n, const uint64_t* __restrict__ u,
                           const uint64_t* __restrict__ nu_at, uint32_t* __restrict__ rank) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) rank[i] = (uint32_t)sgd::lb64(u, min(*nu_at, n), v[i]);
}
__global__ void k_rank_pack(const uint32_t* __restrict__ hi, const uint32_t* __restrict__ lo, uint64_t n,
                            uint64_t* __restrict__ v, uint64_t* __restrict__ ka) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) v[i] = ka[i] = ((uint64_t)hi[i] << 32) | lo[i];
}
// sorted keys group << 32 | rank: the place, among the first occurrences, of each group's first
__global__ void k_rank_first(const uint64_t* __restrict__ keys, const uint64_t* __restrict__ pos, uint64_t n,
                             uint64_t ngroups, uint64_t* __restrict__ first) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint64_t c = keys[i] >> 32;
  if (c < ngroups && (i == 0 || (keys[i - 1] >> 32) != c)) first[c] = pos[i];
}
// a workgroup per group: a flagged group's members get their places
__global__ __launch_bounds__(256) void k_rank_fill(const uint64_t* __restrict__ off, uint64_t total,
                                                   const uint8_t* __restrict__ flag, const uint64_t* __restrict__ gbase,
                                                   uint64_t ng, uint32_t* __restrict__ gidx,
                                                   uint32_t* __restrict__ ggroup) {
  const uint64_t c = blockIdx.x;
  if (!flag[c]) return;
  uint64_t r0, r1;
  sgd::csr_range(off, c, total, r0, r1);
  const uint64_t g0 = gbase[c];
  for (uint64_t k = threadIdx.x; k < r1 - r0; k += 256)
    if (g0 + k < ng) {
      gidx[g0 + k] = (uint32_t)(r0 + k);
      ggroup[g0 + k] = (uint32_t)c;
    }
}
__global__ void k_rank_flag_all(const uint64_t* __restrict__ off, uint64_t ngroups, uint64_t total,
                                const uint8_t* __restrict__ sel, uint8_t* __restrict__ flag, uint64_t* __restrict__ gbase,
                                unsigned long long* __restrict__ scal) {
  const uint64_t c = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= ngroups) return;
  uint64_t r0, r1;
  sgd::csr_range(off, c, total, r0, r1);
  if (!sel) {
    flag[c] = 1;
    gbase[c] = r0;
  } else if (sel[c] && r1 > r0) {
    flag[c] = 1;
    gbase[c] = atomicAdd(&scal[1], (unsigned long long)(r1 - r0));
    atomicAdd(&scal[0], 1ull);
  }
}

int rank_runs(sg_ctx* ctx, const uint64_t* sorted, uint64_t n, uint32_t* flags, uint64_t* pos, uint64_t* u,
              size_t tail) {
  const dim3 grid(div_up(n, 256)), b(256);
  hipLaunchKernelGGL(k_rank_mark, grid, b, 0, ctx->stream, sorted, n, flags);
  const int rc = scan_counts(ctx, flags, pos, n, tail);
  if (rc) return rc;
  if (u)
    hipLaunchKernelGGL(k_rank_unique, grid, b, 0, ctx->stream, sorted, (const uint32_t*)flags, (const uint64_t*)pos, n,
                       u);
  SG_HIP(hipGetLastError());
  return SG_OK;
}

// the regions of a RankWs: one list for the carve and for its size
struct RankOff {
  size_t v, ka, kb, pos, flags;
};
static RankOff rank_regions(WsPlan& p, uint64_t ng) {  // (a braced list is evaluated left to right)
  return RankOff{p.add(ng * 8), p.add(ng * 8), p.add(ng * 8), p.add((ng + 1) * 8), p.add(ng * 4)};
}

RankWs rank_ws(sg_ctx* ctx, WsPlan& p, uint64_t ng) {
  const RankOff o = rank_regions(p, ng);
  RankWs g{};
  g.ng = ng;
  g.v = (uint64_t*)ws_at(ctx, o.v);
  g.ka = (uint64_t*)ws_at(ctx, o.ka);
  g.kb = (uint64_t*)ws_at(ctx, o.kb);
  g.pos = (uint64_t*)ws_at(ctx, o.pos);
  g.flags = (uint32_t*)ws_at(ctx, o.flags);
  g.tail = p.total;
  return g;
}

size_t rank_ws_bytes(uint64_t ng) {
  WsPlan p;
  rank_regions(p, ng);
  return p.total + radix_sort_ws(ng) + scan_ws_bytes(ng);
}

int rank_values(sg_ctx* ctx, const RankWs& g, uint64_t vary, uint64_t* u, uint32_t* rank) {
  uint64_t* sorted = nullptr;
  int rc = radix_sort_u64(ctx, g.ka, g.kb, g.ng, g.tail, &sorted, vary ? vary : 1);
  if (rc) return rc;
  if ((rc = rank_runs(ctx, sorted, g.ng, g.flags, g.pos, u, g.tail))) return rc;
  hipLaunchKernelGGL(k_rank_u32, dim3(div_up(g.ng, 256)), dim3(256), 0, ctx->stream, (const uint64_t*)g.v, g.ng,
                     (const uint64_t*)u, (const uint64_t*)(g.pos + g.ng), rank);
  SG_HIP(hipGetLastError());
  return SG_OK;
}

int rank_pack(sg_ctx* ctx, const RankWs& g, const uint32_t* hi, const uint32_t* lo) {
  hipLaunchKernelGGL(k_rank_pack, dim3(div_up(g.ng, 256)), dim3(256), 0, ctx->stream, hi, lo, g.ng, g.v, g.ka);
  SG_HIP(hipGetLastError());
  return SG_OK;
}

int rank_flag_all(sg_ctx* ctx, const uint64_t* off, uint64_t ngroups, uint64_t total, const uint8_t* sel, uint8_t* flag,
                  uint64_t* gbase, unsigned long long* scal) {
  hipLaunchKernelGGL(k_rank_flag_all, dim3(div_up(ngroups, 256)), dim3(256), 0, ctx->stream, off, ngroups, total, sel, flag,
                     gbase, scal);
  SG_HIP(hipGetLastError());
  return SG_OK;
}

int rank_fill(sg_ctx* ctx, const uint64_t* off, uint64_t ngroups, uint64_t total, const uint8_t* flag,
              const uint64_t* gbase, uint64_t ng, uint32_t* gidx, uint32_t* ggroup) {
  // places never assigned (none, when the counts are consistent) read member 0 of group 0
  SG_HIP(hipMemsetAsync(gidx, 0, ng * 4, ctx->stream));
  SG_HIP(hipMemsetAsync(ggroup, 0, ng * 4, ctx->stream));
  hipLaunchKernelGGL(k_rank_fill, dim3((uint32_t)ngroups), dim3(256), 0, ctx->stream, off, total, flag, gbase, ng, gidx,
                     ggroup);
  SG_HIP(hipGetLastError());
  return SG_OK;
}

int rank_group_first(sg_ctx* ctx, const RankWs& g, const uint32_t* ggroup, const uint32_t* rank, uint64_t ngroups,
                     uint64_t* first, uint64_t** sorted) {
  SG_HIP(hipMemsetAsync(first, 0, ngroups * 8, ctx->stream));
  int rc = rank_pack(ctx, g, ggroup, rank);
  if (rc) return rc;
  const uint64_t kvary = (bits_below(ngroups) << 32) | bits_below(g.ng);
  rc = radix_sort_u64(ctx, g.ka, g.kb, g.ng, g.tail, sorted, kvary ? kvary : 1);
  if (rc) return rc;
  if ((rc = rank_runs(ctx, *sorted, g.ng, g.flags, g.pos, nullptr, g.tail))) return rc;
  hipLaunchKernelGGL(k_rank_first, dim3(div_up(g.ng, 256)), dim3(256), 0, ctx->stream, (const uint64_t*)*sorted,
                     (const uint64_t*)g.pos, g.ng, ngroups, first);
  SG_HIP(hipGetLastError());
  return SG_OK;
}

}  // namespace sg
