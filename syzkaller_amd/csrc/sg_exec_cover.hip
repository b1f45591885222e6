// Executor cover: the flag_collect_cover branch of handle_completion
// (executor/executor.h:402-415) over a batch of raw KCOV buffers, one u64 per
// PC.  Without flag_dedup_cover the call's PCs are truncated in trace order
// (:413-414).  With it: std::sort of the u64 PCs (:408), std::unique (:409),
// and only then the truncation to uint32_t (:411-414, "assuming that they fit
// into 32-bits").  So two PCs that differ only above bit 31 stay two entries,
// in u64 order: a call's u32 list may hold repeats and need not be ascending.
//
// Fast shape (k_xc_call): a workgroup per call.
//  - The call's PCs are streamed once against an LDS open-addressing set whose
//    entries are the u64 keys themselves, claimed with one 64-bit CAS.  The
//    empty marker is the all-ones key; a PC of that value never enters the
//    table and raises a flag of its own instead (it sorts last, so it is
//    appended after the sort).  The new keys of a wave are counted with a
//    ballot and one LDS add.
//  - The table is then compacted in place (a ballot numbers the live entries
//    of each stripe; a stripe's keys never move forward), padded with all-ones
//    keys to a power of two and sorted by a bitonic network.  A key is 8 bytes,
//    so unlike k_ec_call no copy of the keys goes through the workspace and the
//    sort needs no LDS beyond the table: the whole 128 KiB of the large shape
//    is table.
//  - The sorted keys go, truncated, to the workspace: a u32 per PC slot at the
//    call's PC offset (distinct <= PCs), with the call's count.
//  Three instances, each launched over all calls (a workgroup whose call
//  belongs to another leaves at once): calls of at most kXcSmall PCs take 256
//  threads and 4 KiB of LDS, calls of at most kXcMid 512 threads and 32 KiB
//  (four workgroups per CU, by their waves), longer ones 1024 threads and
//  128 KiB of the CU's 160: kXcCap distinct PCs in a table of 2 kXcCap entries.
//  The first two hold any call of theirs.  A call with more distinct PCs than
//  kXcCap (or whose probe walked the whole table) is flagged, not truncated,
//  and takes the
// General path (xc_general), over the flagged calls' PCs only, on the stages of
// sg_rank.hip: the radix sort gives the distinct values U and a binary search
// each PC's rank in U; a sort of call << 32 | rank, its first occurrences and
// their scan give each survivor its place; (uint32_t)U[rank] goes to the same
// workspace slots.  exec_cover() leaves the choice of the calls, the one read of
// their count and the workspace's growth to two_path_first (sg_rank.h).
// scan_counts over the calls' counts gives cov_off; k_xc_emit, a wave per call,
// packs the lists at those offsets and checks the capacity on the device.
// Every loop is bounded by a count known on entry (PCs of the call, table
// entries, sort size).
#include "sg_rank.h"

#include <algorithm>

namespace sg {

constexpr uint32_t kXcSmall = 256;   // PCs of a call of the small shape
constexpr uint32_t kXcMid = 2048;    // ... and of the middle one
constexpr int kXcMidThreads = 512;
constexpr uint32_t kXcCap = SG_EXEC_COVER_FAST_CAP;  // distinct PCs of a call of the large shape
constexpr uint64_t kXcEmpty = ~0ull;                 // the table's empty marker, and the sort's padding
static_assert(2 * kXcCap * 8 + 1024 <= 160 * 1024, "the large shape's table fits the CU's LDS");

struct XcArgs {
  const uint64_t* pcs;
  const uint64_t* call_off;  // [ncalls+1]
  uint64_t ncalls, npcs;
  uint64_t len_lo, len_hi;   // the launch's calls: len_lo < PCs <= len_hi
  const uint8_t* sel;        // [ncalls] or null: only the calls with sel[c] != 0 run
  uint32_t* tmp;             // [npcs] a call's distinct PCs in u64 order, truncated, at its PC offset
  uint32_t* cnt;             // [ncalls] zeroed: the call's cover_size
  uint8_t* flag;             // [ncalls] zeroed: 1 = the general path's
  uint64_t* gbase;           // [ncalls] a flagged call's place among the general path's PCs
  unsigned long long* scal;  // zeroed: {flagged calls, their PCs}
};

__device__ __forceinline__ uint32_t xc_hash(uint64_t pc) {
  uint64_t h = pc * 0x9E3779B97F4A7C15ull;
  h ^= h >> 29;
  h *= 0xC2B2AE3D27D4EB4Full;
  return (uint32_t)(h >> 40);
}

template <int kThreads, uint32_t kCap>
__global__ __launch_bounds__(kThreads) void k_xc_call(XcArgs a) {
  constexpr uint32_t kTab = 2 * kCap;
  static_assert((kCap & (kCap - 1)) == 0 && kTab % kThreads == 0, "a power of two, in whole stripes");
  __shared__ unsigned long long tab[kTab];
  __shared__ uint32_t s_ndist, s_ovf, s_mark;
  __shared__ uint32_t wsum[kThreads / 64];
  const uint64_t c = blockIdx.x;
  const uint32_t tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  uint64_t r0, r1;
  sgd::csr_range(a.call_off, c, a.npcs, r0, r1);
  const uint64_t len = r1 - r0;
  if (len <= a.len_lo || len > a.len_hi) return;  // the other shape's call (or an empty one)
  if (a.sel && !a.sel[c]) return;
  const uint64_t* __restrict__ pc = a.pcs + r0;
  for (uint32_t i = tid; i < kTab; i += kThreads) tab[i] = kXcEmpty;
  if (tid == 0) {
    s_ndist = 0;
    s_ovf = 0;
    s_mark = 0;
  }
  __syncthreads();
  // ---- the distinct PCs ----
  bool over = false;
  for (uint64_t i0 = 0; i0 < len; i0 += kThreads) {
    const uint64_t i = i0 + tid;
    bool fresh = false;
    if (i < len) {
      const unsigned long long x = pc[i];
      if (x == kXcEmpty) {
        atomicOr(&s_mark, 1u);  // the marker's own value: kept by its flag
      } else {
        uint32_t s = xc_hash(x) & (kTab - 1);
        bool placed = false;
        for (uint32_t step = 0; step < kTab; step++) {
          const unsigned long long old = atomicCAS(&tab[s], kXcEmpty, x);
          if (old == kXcEmpty) {
            fresh = placed = true;
            break;
          }
          if (old == x) {
            placed = true;
            break;
          }
          s = (s + 1) & (kTab - 1);
        }
        if (!placed) atomicOr(&s_ovf, 1u);  // the table is full: the call is flagged, the PC is not dropped
      }
    }
    const uint64_t fm = __ballot(fresh);
    if (fm && lane == 0) atomicAdd(&s_ndist, (uint32_t)__popcll(fm));
    if (len > kCap) {  // (uniform) only such a call can pass the capacity
      __syncthreads();
      const bool o = s_ndist + s_mark > kCap || s_ovf;
      __syncthreads();
      if (o) {
        over = true;
        break;
      }
    }
  }
  __syncthreads();  // the probes are done
  if (over || s_ndist + s_mark > kCap || s_ovf) {
    if (tid == 0) {
      a.flag[c] = 1;
      a.gbase[c] = atomicAdd(&a.scal[1], (unsigned long long)len);
      atomicAdd(&a.scal[0], 1ull);
    }
    return;
  }
  // ---- the live entries to the table's front ----
  // Stripe by stripe: every entry of the stripe is read before the barrier in
  // between, and goes to a place at or before its own, so no entry yet to be
  // read is overwritten.
  uint32_t n = 0;
  for (uint32_t j0 = 0; j0 < kTab; j0 += kThreads) {
    const unsigned long long x = tab[j0 + tid];
    const bool live = x != kXcEmpty;
    const uint64_t m = __ballot(live);
    if (lane == 0) wsum[w] = (uint32_t)__popcll(m);
    __syncthreads();
    uint32_t base = 0, tot = 0;
#pragma unroll
    for (int k = 0; k < kThreads / 64; k++) {
      const uint32_t q = wsum[k];
      base += k < (int)w ? q : 0u;
      tot += q;
    }
    __syncthreads();
    if (live) tab[n + base + (uint32_t)__popcll(m & ((1ull << lane) - 1))] = x;
    n += tot;
  }
  // n == s_ndist <= kCap
  uint32_t P = 1;
  while (P < n) P <<= 1;  // <= kCap
  __syncthreads();
  for (uint32_t i = n + tid; i < P; i += kThreads) tab[i] = kXcEmpty;  // sorts last; no real key has its value
  __syncthreads();
  // ---- bitonic sort of P keys ----
  for (uint32_t k = 2; k <= P; k <<= 1)
    for (uint32_t j = k >> 1; j > 0; j >>= 1) {
      for (uint32_t t = tid; t < P / 2; t += kThreads) {
        const uint32_t lo = ((t & ~(j - 1)) << 1) | (t & (j - 1)), hi = lo + j;
        const unsigned long long x = tab[lo], y = tab[hi];
        const bool up = (lo & k) == 0;
        if (up ? y < x : x < y) {
          tab[lo] = y;
          tab[hi] = x;
        }
      }
      __syncthreads();
    }
  // ---- out: the truncated keys (executor.h:413-414), the count ----
  uint32_t* dst = a.tmp + r0;
  for (uint32_t i = tid; i < n; i += kThreads) dst[i] = (uint32_t)tab[i];
  if (tid == 0) {
    const uint32_t mark = s_mark;
    if (mark) dst[n] = (uint32_t)kXcEmpty;  // n + 1 <= len: the marker's value is one of the call's PCs
    a.cnt[c] = n + mark;
  }
}

// ---- the general path's kernels (the shared stages: sg_rank.hip) ----------------
__global__ void k_xc_gather(const uint64_t* __restrict__ pcs, const uint32_t* __restrict__ gidx, uint64_t n,
                            uint64_t* __restrict__ v, uint64_t* __restrict__ ka) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) v[i] = ka[i] = pcs[gidx[i]];
}
// the first occurrences of the sorted keys call << 32 | rank: (uint32_t)U[rank] at the call's next slot
__global__ void k_xc_gwrite(const uint64_t* __restrict__ keys, const uint32_t* __restrict__ flags,
                            const uint64_t* __restrict__ pos, uint64_t n, const uint64_t* __restrict__ u,
                            const uint64_t* __restrict__ first, const uint64_t* __restrict__ call_off, uint64_t ncalls,
                            uint64_t npcs, uint32_t* __restrict__ tmp, uint32_t* __restrict__ cnt) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n || !flags[i]) return;
  const uint64_t c = keys[i] >> 32;
  if (c >= ncalls) return;
  uint64_t r0, r1;
  sgd::csr_range(call_off, c, npcs, r0, r1);
  const uint64_t li = pos[i] - first[c];  // < the call's distinct PCs <= its PCs
  if (li >= r1 - r0) return;
  tmp[r0 + li] = (uint32_t)u[min<uint64_t>((uint32_t)keys[i], n - 1)];  // (a rank is below n: U holds n entries)
  atomicAdd(&cnt[c], 1u);
}

// dedup == 0 (executor.h:413-414): the PCs truncated in place order; cov_off = call_off
__global__ void k_xc_trunc(const uint64_t* __restrict__ pcs, uint64_t npcs, const uint64_t* __restrict__ call_off,
                           uint64_t ncalls, uint64_t* __restrict__ cov_off, uint32_t* __restrict__ cov) {
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  for (uint64_t i = t; i <= ncalls; i += stride) cov_off[i] = min(call_off[i], npcs);
  if (cov)
    for (uint64_t i = t; i < npcs; i += stride) cov[i] = (uint32_t)pcs[i];
}

// a wave per call: the workspace list to cov at the call's offset
__global__ __launch_bounds__(256) void k_xc_emit(const uint64_t* __restrict__ call_off, uint64_t ncalls, uint64_t npcs,
                                                 const uint32_t* __restrict__ tmp,
                                                 const uint64_t* __restrict__ cov_off, uint32_t* __restrict__ cov,
                                                 uint64_t cov_cap) {
  const uint64_t c = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (c >= ncalls || cov_off[ncalls] > cov_cap) return;
  const uint32_t lane = threadIdx.x & 63;
  uint64_t r0, r1;
  sgd::csr_range(call_off, c, npcs, r0, r1);
  const uint64_t o0 = cov_off[c], n = min(cov_off[c + 1] - o0, r1 - r0);
  // four loads per lane in flight before their stores
  for (uint64_t i0 = 0; i0 < n; i0 += 256) {
    uint32_t v[4];
#pragma unroll
    for (int u = 0; u < 4; u++) {
      const uint64_t i = i0 + u * 64 + lane;
      v[u] = i < n ? tmp[r0 + i] : 0u;
    }
#pragma unroll
    for (int u = 0; u < 4; u++) {
      const uint64_t i = i0 + u * 64 + lane;
      if (i < n) cov[o0 + i] = v[u];
    }
  }
}

// xc_general's workspace: three u32 arrays and one u64 array of ng and a u64 per call of its own, then the shared stages'
static size_t xc_general_bytes(uint64_t ng, uint64_t ncalls) {
  return 3 * align256(ng * 4) + align256(ng * 8) + align256(ncalls * 8) + rank_ws_bytes(ng) + 4096;
}

// the flagged calls' ng PCs (places gbase) -> their workspace lists and counts
static int xc_general(sg_ctx* ctx, const XcArgs& a, uint64_t ng, size_t base) {
  ScopedTimer tm(ctx, "exec_cover_general");
  WsPlan p;
  p.total = base;
  const size_t o_gidx = p.add(ng * 4), o_gcall = p.add(ng * 4), o_rank = p.add(ng * 4), o_u = p.add(ng * 8),
               o_first = p.add(a.ncalls * 8);
  const RankWs g = rank_ws(ctx, p, ng);
  uint32_t* gidx = (uint32_t*)ws_at(ctx, o_gidx);
  uint32_t* gcall = (uint32_t*)ws_at(ctx, o_gcall);
  uint32_t* rank = (uint32_t*)ws_at(ctx, o_rank);
  uint64_t* u = (uint64_t*)ws_at(ctx, o_u);
  uint64_t* first = (uint64_t*)ws_at(ctx, o_first);
  const dim3 grid(div_up(ng, 256)), b(256);
  int rc = rank_fill(ctx, a.call_off, a.ncalls, a.npcs, a.flag, a.gbase, ng, gidx, gcall);
  if (rc) return rc;
  // 1. the distinct PCs U and each PC's rank in U
  hipLaunchKernelGGL(k_xc_gather, grid, b, 0, ctx->stream, a.pcs, (const uint32_t*)gidx, ng, g.v, g.ka);
  if ((rc = rank_values(ctx, g, ~0ull, u, rank))) return rc;
  // 2. sort call << 32 | rank; 3. first occurrences and their scan; 4. (uint32_t)U[rank]
  uint64_t* sorted = nullptr;
  if ((rc = rank_group_first(ctx, g, gcall, rank, a.ncalls, first, &sorted))) return rc;
  hipLaunchKernelGGL(k_xc_gwrite, grid, b, 0, ctx->stream, (const uint64_t*)sorted, (const uint32_t*)g.flags,
                     (const uint64_t*)g.pos, ng, (const uint64_t*)u, (const uint64_t*)first, a.call_off, a.ncalls,
                     a.npcs, a.tmp, a.cnt);
  SG_HIP(hipGetLastError());
  return SG_OK;
}

// sg_exec_cover_dev's body; ctx lock held, the device ensured (sg_internal.h)
int exec_cover(sg_ctx* ctx, const uint64_t* d_pcs, const uint64_t* d_call_off, uint64_t ncalls, uint64_t npcs, int dedup,
               uint64_t* d_cov_off, uint32_t* d_cov, uint64_t cov_cap, const uint8_t* sel) {
  ctx->exec_cover_general = 0;
  if (ncalls == 0 || npcs == 0) {
    SG_HIP(hipMemsetAsync(d_cov_off, 0, (ncalls + 1) * 8, ctx->stream));
    return SG_OK;
  }
  if (!dedup) {
    ScopedTimer tm(ctx, "exec_cover_emit");
    const uint64_t work = npcs > ncalls ? npcs : ncalls + 1;
    hipLaunchKernelGGL(k_xc_trunc, dim3(std::min<uint64_t>(div_up(work, 256), 65536)), dim3(256), 0, ctx->stream, d_pcs,
                       npcs, d_call_off, ncalls, d_cov_off, npcs <= cov_cap ? d_cov : nullptr);
    SG_HIP(hipGetLastError());
    return SG_OK;
  }
  const bool all_general = ctx->opt[kOptExecCoverPath] == 0;
  WsPlan p;
  const size_t o_cnt = p.add(ncalls * 4), o_flag = p.add(ncalls), o_scal = p.add(256);
  const size_t zeroed = p.total;
  const size_t o_gbase = p.add(ncalls * 8), o_tmp = p.add(npcs * 4);
  const size_t scan_a = p.total;
  const size_t need_a = p.total + scan_ws_bytes(ncalls);
  XcArgs a{};
  a.pcs = d_pcs;
  a.call_off = d_call_off;
  a.ncalls = ncalls;
  a.npcs = npcs;
  a.sel = sel;
  auto first_pass = [&]() -> int {
    a.cnt = (uint32_t*)ws_at(ctx, o_cnt);
    a.flag = (uint8_t*)ws_at(ctx, o_flag);
    a.scal = (unsigned long long*)ws_at(ctx, o_scal);
    a.gbase = (uint64_t*)ws_at(ctx, o_gbase);
    a.tmp = (uint32_t*)ws_at(ctx, o_tmp);
    SG_HIP(hipMemsetAsync(ws_at(ctx, 0), 0, zeroed, ctx->stream));
    if (all_general) return rank_flag_all(ctx, d_call_off, ncalls, npcs, sel, a.flag, a.gbase, a.scal);
    ScopedTimer tm(ctx, "exec_cover_call");
    a.len_lo = 0;
    a.len_hi = kXcSmall;
    hipLaunchKernelGGL((k_xc_call<256, kXcSmall>), dim3((uint32_t)ncalls), dim3(256), 0, ctx->stream, a);
    if (npcs > kXcSmall) {
      a.len_lo = kXcSmall;
      a.len_hi = kXcMid;
      hipLaunchKernelGGL((k_xc_call<kXcMidThreads, kXcMid>), dim3((uint32_t)ncalls), dim3(kXcMidThreads), 0, ctx->stream,
                         a);
    }
    if (npcs > kXcMid) {
      a.len_lo = kXcMid;
      a.len_hi = ~0ull;
      hipLaunchKernelGGL((k_xc_call<1024, kXcCap>), dim3((uint32_t)ncalls), dim3(1024), 0, ctx->stream, a);
    }
    SG_HIP(hipGetLastError());
    return SG_OK;
  };
  const TwoPath tp{all_general, sel != nullptr, ncalls, npcs, kXcCap, need_a, o_scal};
  uint64_t ng = 0;
  int rc = two_path_first(ctx, tp, first_pass, [&](uint64_t n) { return xc_general_bytes(n, ncalls); },
                          &ctx->exec_cover_general, &ng);
  if (rc) return rc;
  if (ng) {
    rc = xc_general(ctx, a, ng, need_a);
    if (rc) return rc;
  }
  rc = scan_counts(ctx, a.cnt, d_cov_off, ncalls, scan_a);
  if (rc) return rc;
  if (d_cov) {
    ScopedTimer tm(ctx, "exec_cover_emit");
    hipLaunchKernelGGL(k_xc_emit, dim3(div_up(ncalls, 4)), dim3(256), 0, ctx->stream, d_call_off, ncalls, npcs,
                       (const uint32_t*)a.tmp, (const uint64_t*)d_cov_off, d_cov, cov_cap);
  }
  SG_HIP(hipGetLastError());
  return SG_OK;
}

static int xc_limits(uint64_t ncalls, uint64_t npcs, int dedup) {
  if (npcs >= (1ull << 32) || ncalls >= (1ull << 31) || dedup < 0 || dedup > 1) {
    set_error("sg_exec_cover: %llu PCs, %llu calls, dedup %d (the limits are 2^32 - 1 and 2^31 - 1; dedup is 0 or 1)",
              (unsigned long long)npcs, (unsigned long long)ncalls, dedup);
    return SG_EINVAL;
  }
  return SG_OK;
}

}  // namespace sg

using namespace sg;

extern "C" {

int sg_exec_cover_dev(sg_ctx* ctx, const uint64_t* d_pcs, const uint64_t* d_call_off, uint64_t ncalls, uint64_t npcs,
                      int dedup, uint64_t* d_cov_off, uint32_t* d_cov, uint64_t cov_cap) {
  if (!ctx || !d_call_off || !d_cov_off || (npcs && !d_pcs) || (cov_cap && !d_cov)) return SG_EINVAL;
  int rc = xc_limits(ncalls, npcs, dedup);
  if (rc) return rc;
  std::lock_guard<std::mutex> g(ctx->mu);
  rc = ensure_device(ctx);
  if (rc) return rc;
  return exec_cover(ctx, d_pcs, d_call_off, ncalls, npcs, dedup, d_cov_off, d_cov, cov_cap);
}

int sg_exec_cover(sg_ctx* ctx, const uint64_t* pcs, const uint64_t* call_off, size_t ncalls, int dedup,
                  uint64_t* cov_off, uint32_t* cov, size_t cov_cap) {
  if (!ctx || !call_off || !cov_off || (cov_cap && !cov)) return SG_EINVAL;
  const uint64_t npcs = call_off[ncalls];
  if (!offsets_ok(call_off, ncalls) || (npcs && !pcs)) return SG_EINVAL;
  int rc = xc_limits(ncalls, npcs, dedup);
  if (rc) return rc;
  // npcs values always suffice: a smaller cap is staged as it is
  const uint64_t ccap = cov_cap < npcs ? cov_cap : npcs;
  WsPlan p;
  const size_t o_pcs = p.add(npcs * 8 + 8), o_co = p.add((ncalls + 1) * 8), o_cov_off = p.add((ncalls + 1) * 8),
               o_cov = p.add(ccap * 4 + 4);
  std::lock_guard<std::mutex> g(ctx->mu);
  rc = ensure_device(ctx);
  if (rc) return rc;
  rc = dstage_reserve(ctx, p);
  if (rc) return rc;
  uint64_t* dpcs = dstage_at<uint64_t>(ctx, o_pcs);
  uint64_t* dco = dstage_at<uint64_t>(ctx, o_co);
  uint64_t* dcov_off = dstage_at<uint64_t>(ctx, o_cov_off);
  uint32_t* dcov = dstage_at<uint32_t>(ctx, o_cov);
  if ((rc = upload(ctx, dpcs, pcs, npcs * 8))) return rc;
  if ((rc = upload(ctx, dco, call_off, (ncalls + 1) * 8))) return rc;
  rc = exec_cover(ctx, dpcs, dco, ncalls, npcs, dedup, dcov_off, ccap ? dcov : nullptr, ccap);
  if (rc) return rc;
  return csr_download(ctx, cov_off, dcov_off, ncalls, cov, dcov, 4, cov_cap);
}

}  // extern "C"
