// Executor-exact comparisons: the flag_collect_comps branch of
// handle_completion (executor/executor.h:379-387) over a batch of raw
// KCOV_TRACE_CMP buffers.  Per call: std::sort under operator< (:665-673),
// std::unique under operator== (:659-663), kcov_comparison_t::write (:621-657).
// pc takes no part in either operator and is never written, so the output is
// the call's distinct (type, arg1, arg2), ascending as unsigned 64-bit triples,
// then extended and laid out as write() does.
//
// Fast shape (k_ec_call): a workgroup per call.
//  - The call's records are streamed once against an LDS open-addressing set.
//    An entry is {tag, local record index + 1}, claimed with one 64-bit CAS; a
//    probe that meets an equal tag compares the whole key against the entry's
//    record in the (immutable, cached) input, so no entry is ever half written.
//  - A lane whose claim succeeded holds a new key in registers.  A wave's new
//    keys go, in lane order, to the call's workspace slots (below) at a place
//    taken with one LDS add per wave; after the stream they are read back, in
//    order, into LDS (structure of arrays, over the table, which is done),
//    padded with all-ones keys to a power of two and sorted by a bitonic
//    network.
//  - The sorted keys go back, raw, to the workspace: a triple per record slot
//    at the call's record offset (distinct <= records), with the call's
//    comparison and word counts.
//  Three instances, each launched over all calls (a workgroup whose call
//  belongs to another leaves at once): calls of at most kEcSmall records take
//  256 threads and 6 KiB of LDS, calls of at most kEcMid 512 threads and
//  48 KiB (three workgroups per CU), longer ones 1024 threads and 96 KiB:
//  kEcCap distinct records in a table of 2 kEcCap entries.  The first two hold
//  any call of theirs.  A call with more distinct records than kEcCap (or
//  whose probe walked the whole table) is flagged, not truncated, and takes the
// General path (ec_general), on the stages of sg_rank.hip: order-preserving
// rank compression with the radix sort, over the flagged calls' records only:
// distinct arg2 -> rank A; rank(arg1) << 32 | A -> rank B; rank(type) << 32 | B
// -> rank C; a sort of call << 32 | C, first occurrences; a survivor's triple
// is read back through the tables of distinct values.  It writes the same
// workspace triples.  exec_comps() leaves the choice of the calls, the one read
// of their count and the workspace's growth to two_path_first (sg_rank.h).
// scan_counts over the calls' counts gives comp_off and word_off; k_ec_emit, a
// wave per call, extends the operands (after sort and unique, as the
// reference) and writes triples and words at those offsets.  The words are the
// WRITER's layout (two operand words unless the size is 8, :646-656); the
// reader of this snapshot takes the opposite widths (ipc_linux.go:272-289) and
// sg_ipc_comps keeps reading those: the two are not reconciled.  The device
// consumer of the triples is sg_hint_seed.hip; its fused call takes the raw
// workspace keys (exec_comps with `raw`) and skips k_ec_emit.
// Every loop is bounded by a count known on entry (records of the call, table
// entries, sort size).
#include "sg_rank.h"

namespace sg {

constexpr uint32_t kEcSmall = 256;      // records of a call of the small shape
constexpr uint32_t kEcMid = 2048;       // ... and of the middle one
constexpr int kEcMidThreads = 512;
constexpr uint32_t kEcCap = SG_EXEC_COMPS_FAST_CAP;  // distinct records of a call of the large shape
constexpr uint64_t kEcPad = ~0ull;

struct EcArgs {
  const uint64_t* recs;      // {type, arg1, arg2, pc}
  const uint64_t* call_off;  // [ncalls+1]
  uint64_t ncalls, nrecs;
  uint64_t len_lo, len_hi;   // the launch's calls: len_lo < records <= len_hi
  uint64_t* tmp;             // [3 nrecs] a call's sorted distinct keys at its record offset
  uint32_t* cnt;             // [ncalls] zeroed: distinct records
  uint32_t* wcnt;            // [ncalls] zeroed: words
  uint8_t* flag;             // [ncalls] zeroed: 1 = the general path's
  uint64_t* gbase;           // [ncalls] a flagged call's place among the general path's records
  unsigned long long* scal;  // zeroed: {flagged calls, their records}
};

__device__ __forceinline__ uint64_t ec_hash(uint64_t t, uint64_t a1, uint64_t a2) {
  uint64_t h = a1 * 0x9E3779B97F4A7C15ull;
  h ^= h >> 32;
  h = (h + a2) * 0xC2B2AE3D27D4EB4Full;
  h ^= h >> 29;
  h = (h + t) * 0x165667B19E3779F9ull;
  h ^= h >> 32;
  return h;
}

__device__ __forceinline__ bool ec_less(uint64_t t, uint64_t a1, uint64_t a2, uint64_t u, uint64_t b1, uint64_t b2) {
  // executor.h:665-673
  if (t != u) return t < u;
  if (a1 != b1) return a1 < b1;
  return a2 < b2;
}

template <int kThreads, uint32_t kCap>
__global__ __launch_bounds__(kThreads) void k_ec_call(EcArgs a) {
  constexpr uint32_t kTab = 2 * kCap;
  static_assert((kCap & (kCap - 1)) == 0, "a power of two");
  __shared__ uint64_t lds[3 * kCap];  // the table (2 kCap entries), then the keys (3 arrays of kCap)
  __shared__ uint32_t s_ndist, s_ovf, s_big;
  const uint64_t c = blockIdx.x;
  const uint32_t tid = threadIdx.x, lane = tid & 63;
  uint64_t r0, r1;
  sgd::csr_range(a.call_off, c, a.nrecs, r0, r1);
  const uint64_t len = r1 - r0;
  if (len <= a.len_lo || len > a.len_hi) return;  // the other shape's call (or an empty one)
  const uint64_t* __restrict__ rec = a.recs + 4 * r0;
  unsigned long long* tab = (unsigned long long*)lds;
  for (uint32_t i = tid; i < kTab; i += kThreads) tab[i] = 0;
  if (tid == 0) {
    s_ndist = 0;
    s_ovf = 0;
    s_big = 0;
  }
  __syncthreads();
  // ---- the distinct records ----
  // A lane whose claim succeeded holds a new key: the wave's new keys go, in
  // lane order, to the call's workspace slots at a place taken with one LDS
  // add per wave (claims <= records streamed, so the place is in the call).
  uint64_t* dst = a.tmp + 3 * r0;
  bool over = false;
  for (uint64_t i0 = 0; i0 < len; i0 += kThreads) {
    const uint64_t i = i0 + tid;
    uint64_t t = 0, a1 = 0, a2 = 0;
    bool fresh = false;
    if (i < len) {
      t = rec[4 * i];
      a1 = rec[4 * i + 1];
      a2 = rec[4 * i + 2];
      const uint64_t h = ec_hash(t, a1, a2);
      const unsigned long long mine = (h << 32) | (uint32_t)(i + 1);  // tag = the hash's low half
      uint32_t s = (uint32_t)(h >> 32) & (kTab - 1);
      bool placed = false;
      for (uint32_t step = 0; step < kTab; step++) {
        const unsigned long long old = atomicCAS(&tab[s], 0ull, mine);
        if (old == 0) {
          fresh = placed = true;
          break;
        }
        if ((old >> 32) == (mine >> 32)) {
          const uint64_t j = (uint32_t)old - 1;  // < len: an earlier claim of this call
          if (rec[4 * j] == t && rec[4 * j + 1] == a1 && rec[4 * j + 2] == a2) {
            placed = true;
            break;
          }
        }
        s = (s + 1) & (kTab - 1);
      }
      if (!placed) atomicOr(&s_ovf, 1u);  // the table is full: the call is flagged, the record is not dropped
    }
    const uint64_t fm = __ballot(fresh);
    if (fm) {  // (wave-uniform)
      uint32_t base = 0;
      if (lane == 0) base = atomicAdd(&s_ndist, (uint32_t)__popcll(fm));
      base = __shfl(base, 0);
      if (fresh) {
        const uint64_t at = base + (uint32_t)__popcll(fm & ((1ull << lane) - 1));
        if (at < len) {
          dst[3 * at] = t;
          dst[3 * at + 1] = a1;
          dst[3 * at + 2] = a2;
        }
      }
    }
    if (kCap < kEcSmall || len > kCap) {  // (uniform) only such a call can pass the capacity
      __syncthreads();
      const bool o = s_ndist > kCap || s_ovf;
      __syncthreads();
      if (o) {
        over = true;
        break;
      }
    }
  }
  __syncthreads();  // the probes are done, the workspace keys visible to the workgroup
  if (over || s_ndist > kCap || s_ovf) {
    if (tid == 0) {
      a.flag[c] = 1;
      a.gbase[c] = atomicAdd(&a.scal[1], (unsigned long long)len);
      atomicAdd(&a.scal[0], 1ull);
    }
    return;
  }
  const uint32_t n = s_ndist;
  // ---- the keys into LDS, over the table ----
  uint64_t* k0 = lds;
  uint64_t* k1 = lds + kCap;
  uint64_t* k2 = lds + 2 * kCap;
  for (uint32_t i = tid; i < n; i += kThreads) {
    k0[i] = dst[3 * (uint64_t)i];
    k1[i] = dst[3 * (uint64_t)i + 1];
    k2[i] = dst[3 * (uint64_t)i + 2];
  }
  uint32_t P = 1;
  while (P < n) P <<= 1;  // <= kCap
  for (uint32_t i = n + tid; i < P; i += kThreads) {
    k0[i] = kEcPad;  // sorts last; equal to a real key at most in value
    k1[i] = kEcPad;
    k2[i] = kEcPad;
  }
  __syncthreads();
  // ---- bitonic sort of P keys ----
  for (uint32_t k = 2; k <= P; k <<= 1)
    for (uint32_t j = k >> 1; j > 0; j >>= 1) {
      for (uint32_t t = tid; t < P / 2; t += kThreads) {
        const uint32_t lo = ((t & ~(j - 1)) << 1) | (t & (j - 1)), hi = lo + j;
        const uint64_t x0 = k0[lo], x1 = k1[lo], x2 = k2[lo], y0 = k0[hi], y1 = k1[hi], y2 = k2[hi];
        const bool up = (lo & k) == 0;
        if (up ? ec_less(y0, y1, y2, x0, x1, x2) : ec_less(x0, x1, x2, y0, y1, y2)) {
          k0[lo] = y0;
          k1[lo] = y1;
          k2[lo] = y2;
          k0[hi] = x0;
          k1[hi] = x1;
          k2[hi] = x2;
        }
      }
      __syncthreads();
    }
  // ---- out: the raw keys, the counts ----
  uint32_t big = 0;
  for (uint32_t i = tid; i < n; i += kThreads) {
    const uint64_t t = k0[i];
    dst[3 * (uint64_t)i] = t;
    dst[3 * (uint64_t)i + 1] = k1[i];
    dst[3 * (uint64_t)i + 2] = k2[i];
    big += (t & 6) == 6;
  }
  big = __shfl(sgd::wave_incl_add(big), 63);
  if (lane == 0 && big) atomicAdd(&s_big, big);
  __syncthreads();
  if (tid == 0) {
    a.cnt[c] = n;
    a.wcnt[c] = 3 * n + 2 * s_big;  // executor.h:646-656: four operand words for size 8, two otherwise
  }
}

// ---- the general path's kernels (the shared stages: sg_rank.hip) ----------------
__global__ void k_ec_field(const uint64_t* __restrict__ recs, const uint32_t* __restrict__ gidx, uint64_t n,
                           uint32_t field, uint64_t* __restrict__ v, uint64_t* __restrict__ ka) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) v[i] = ka[i] = recs[4 * (uint64_t)gidx[i] + field];
}
struct EcTables {
  const uint64_t *ut, *u1, *u2, *ub, *uc;  // distinct types, arg1, arg2, rank(arg1) << 32 | A, rank(type) << 32 | B
};
__global__ void k_ec_gwrite(const uint64_t* __restrict__ keys, const uint32_t* __restrict__ flags,
                            const uint64_t* __restrict__ pos, uint64_t n, EcTables t,
                            const uint64_t* __restrict__ first, const uint64_t* __restrict__ call_off, uint64_t ncalls,
                            uint64_t nrecs, uint64_t* __restrict__ tmp, uint32_t* __restrict__ cnt,
                            uint32_t* __restrict__ wcnt) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n || !flags[i]) return;
  const uint64_t c = keys[i] >> 32;
  if (c >= ncalls) return;
  // every rank is below n: each table holds n entries
  const uint64_t kc = t.uc[min<uint64_t>((uint32_t)keys[i], n - 1)];
  const uint64_t kb = t.ub[min<uint64_t>((uint32_t)kc, n - 1)];
  const uint64_t typ = t.ut[min<uint64_t>(kc >> 32, n - 1)];
  const uint64_t a1 = t.u1[min<uint64_t>(kb >> 32, n - 1)];
  const uint64_t a2 = t.u2[min<uint64_t>((uint32_t)kb, n - 1)];
  uint64_t r0, r1;
  sgd::csr_range(call_off, c, nrecs, r0, r1);
  const uint64_t li = pos[i] - first[c];  // < the call's distinct records <= its records
  if (li >= r1 - r0) return;
  uint64_t* dst = tmp + 3 * (r0 + li);
  dst[0] = typ;
  dst[1] = a1;
  dst[2] = a2;
  atomicAdd(&cnt[c], 1u);
  atomicAdd(&wcnt[c], (typ & 6) == 6 ? 5u : 3u);
}

// a wave per call: the workspace triples, extended, to comps and words
__global__ __launch_bounds__(256) void k_ec_emit(const uint64_t* __restrict__ call_off, uint64_t ncalls, uint64_t nrecs,
                                                 const uint64_t* __restrict__ tmp,
                                                 const uint64_t* __restrict__ comp_off, uint64_t* __restrict__ comps,
                                                 uint64_t comps_cap, const uint64_t* __restrict__ word_off,
                                                 uint32_t* __restrict__ words, uint64_t words_cap) {
  const uint64_t c = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (c >= ncalls) return;
  const uint32_t lane = threadIdx.x & 63;
  const bool do_comps = comps && comp_off[ncalls] <= comps_cap;
  const bool do_words = words && word_off && word_off[ncalls] <= words_cap;
  if (!do_comps && !do_words) return;
  uint64_t r0, r1;
  sgd::csr_range(call_off, c, nrecs, r0, r1);
  const uint64_t o0 = comp_off[c], n = min(comp_off[c + 1] - o0, r1 - r0);
  const uint64_t* __restrict__ src = tmp + 3 * r0;
  uint64_t wrun = do_words ? word_off[c] : 0;
  const uint64_t wend = do_words ? word_off[c + 1] : 0;
  for (uint64_t base = 0; base < n; base += 64) {
    const uint64_t i = base + lane;
    const bool v = i < n;
    uint64_t typ = 0, a1 = 0, a2 = 0;
    if (v) {
      typ = src[3 * i];
      a1 = sgd::kcov_extend(typ, src[3 * i + 1]);
      a2 = sgd::kcov_extend(typ, src[3 * i + 2]);
      if (do_comps) {
        comps[3 * (o0 + i)] = typ;
        comps[3 * (o0 + i) + 1] = a1;
        comps[3 * (o0 + i) + 2] = a2;
      }
    }
    if (do_words) {  // (wave-uniform)
      const bool big = (typ & 6) == 6;
      const uint32_t wc = v ? (big ? 5u : 3u) : 0u;
      const uint32_t incl = sgd::wave_incl_add(wc);
      const uint64_t at = wrun + incl - wc;
      if (v && at + wc <= wend) {
        words[at] = (uint32_t)typ;
        if (big) {
          words[at + 1] = (uint32_t)a1;
          words[at + 2] = (uint32_t)(a1 >> 32);
          words[at + 3] = (uint32_t)a2;
          words[at + 4] = (uint32_t)(a2 >> 32);
        } else {
          words[at + 1] = (uint32_t)a1;
          words[at + 2] = (uint32_t)a2;
        }
      }
      wrun += __shfl(incl, 63);
    }
  }
}

// ec_general's workspace: four u32 and five u64 arrays of ng and a u64 per call of its own, then the shared stages'
static size_t ec_general_bytes(uint64_t ng, uint64_t ncalls) {
  return 4 * align256(ng * 4) + 5 * align256(ng * 8) + align256(ncalls * 8) + rank_ws_bytes(ng) + 4096;
}

// the flagged calls' ng records (places gbase) -> their workspace triples and counts
static int ec_general(sg_ctx* ctx, const EcArgs& a, uint64_t ng, size_t base) {
  ScopedTimer tm(ctx, "exec_comps_general");
  WsPlan p;
  p.total = base;
  const size_t o_gidx = p.add(ng * 4), o_gcall = p.add(ng * 4), o_rlo = p.add(ng * 4), o_rhi = p.add(ng * 4),
               o_ut = p.add(ng * 8), o_u1 = p.add(ng * 8), o_u2 = p.add(ng * 8), o_ub = p.add(ng * 8),
               o_uc = p.add(ng * 8), o_first = p.add(a.ncalls * 8);
  const RankWs g = rank_ws(ctx, p, ng);
  uint32_t* gidx = (uint32_t*)ws_at(ctx, o_gidx);
  uint32_t* gcall = (uint32_t*)ws_at(ctx, o_gcall);
  uint32_t* rlo = (uint32_t*)ws_at(ctx, o_rlo);
  uint32_t* rhi = (uint32_t*)ws_at(ctx, o_rhi);
  uint64_t* first = (uint64_t*)ws_at(ctx, o_first);
  uint64_t *ut = (uint64_t*)ws_at(ctx, o_ut), *u1 = (uint64_t*)ws_at(ctx, o_u1), *u2 = (uint64_t*)ws_at(ctx, o_u2),
           *ub = (uint64_t*)ws_at(ctx, o_ub), *uc = (uint64_t*)ws_at(ctx, o_uc);
  const dim3 grid(div_up(ng, 256)), b(256);
  int rc = rank_fill(ctx, a.call_off, a.ncalls, a.nrecs, a.flag, a.gbase, ng, gidx, gcall);
  if (rc) return rc;
  const uint64_t rk = bits_below(ng), packed = (rk << 32) | rk;
  // 1. distinct arg2 -> A
  hipLaunchKernelGGL(k_ec_field, grid, b, 0, ctx->stream, a.recs, (const uint32_t*)gidx, ng, 2u, g.v, g.ka);
  if ((rc = rank_values(ctx, g, ~0ull, u2, rlo))) return rc;
  // 2. rank(arg1) << 32 | A -> B
  hipLaunchKernelGGL(k_ec_field, grid, b, 0, ctx->stream, a.recs, (const uint32_t*)gidx, ng, 1u, g.v, g.ka);
  if ((rc = rank_values(ctx, g, ~0ull, u1, rhi))) return rc;
  if ((rc = rank_pack(ctx, g, rhi, rlo))) return rc;
  if ((rc = rank_values(ctx, g, packed, ub, rlo))) return rc;
  // 3. rank(type) << 32 | B -> C
  hipLaunchKernelGGL(k_ec_field, grid, b, 0, ctx->stream, a.recs, (const uint32_t*)gidx, ng, 0u, g.v, g.ka);
  if ((rc = rank_values(ctx, g, ~0ull, ut, rhi))) return rc;
  if ((rc = rank_pack(ctx, g, rhi, rlo))) return rc;
  if ((rc = rank_values(ctx, g, packed, uc, rlo))) return rc;
  // 4. sort call << 32 | C; 5. first occurrences; 6. the survivors' triples through the tables
  uint64_t* sorted = nullptr;
  if ((rc = rank_group_first(ctx, g, gcall, rlo, a.ncalls, first, &sorted))) return rc;
  EcTables t{ut, u1, u2, ub, uc};
  hipLaunchKernelGGL(k_ec_gwrite, grid, b, 0, ctx->stream, (const uint64_t*)sorted, (const uint32_t*)g.flags,
                     (const uint64_t*)g.pos, ng, t, (const uint64_t*)first, a.call_off, a.ncalls, a.nrecs, a.tmp, a.cnt,
                     a.wcnt);
  SG_HIP(hipGetLastError());
  return SG_OK;
}

// sg_exec_comps_dev's body; ctx lock held, the device ensured (sg_internal.h)
int exec_comps(sg_ctx* ctx, const uint64_t* d_recs, const uint64_t* d_call_off, uint64_t ncalls, uint64_t nrecs,
               uint64_t* d_comp_off, uint64_t* d_comps, uint64_t comps_cap, uint64_t* d_word_off, uint32_t* d_words,
               uint64_t words_cap, EcRaw* raw) {
  ctx->exec_comps_general = 0;
  if (raw) *raw = EcRaw{};
  if (ncalls == 0 || nrecs == 0) {
    SG_HIP(hipMemsetAsync(d_comp_off, 0, (ncalls + 1) * 8, ctx->stream));
    if (d_word_off) SG_HIP(hipMemsetAsync(d_word_off, 0, (ncalls + 1) * 8, ctx->stream));
    return SG_OK;
  }
  const bool all_general = ctx->opt[kOptExecCompsPath] == 0;
  WsPlan p;
  const size_t o_cnt = p.add(ncalls * 4), o_wcnt = p.add(ncalls * 4), o_flag = p.add(ncalls), o_scal = p.add(256);
  const size_t zeroed = p.total;
  const size_t o_gbase = p.add(ncalls * 8), o_tmp = p.add(nrecs * 24);
  const size_t scan_a = p.total;
  const size_t need_a = p.total + scan_ws_bytes(ncalls);
  EcArgs a{};
  a.recs = d_recs;
  a.call_off = d_call_off;
  a.ncalls = ncalls;
  a.nrecs = nrecs;
  auto first_pass = [&]() -> int {
    a.cnt = (uint32_t*)ws_at(ctx, o_cnt);
    a.wcnt = (uint32_t*)ws_at(ctx, o_wcnt);
    a.flag = (uint8_t*)ws_at(ctx, o_flag);
    a.scal = (unsigned long long*)ws_at(ctx, o_scal);
    a.gbase = (uint64_t*)ws_at(ctx, o_gbase);
    a.tmp = (uint64_t*)ws_at(ctx, o_tmp);
    SG_HIP(hipMemsetAsync(ws_at(ctx, 0), 0, zeroed, ctx->stream));
    if (all_general) return rank_flag_all(ctx, d_call_off, ncalls, nrecs, nullptr, a.flag, a.gbase, a.scal);
    ScopedTimer tm(ctx, "exec_comps_call");
    a.len_lo = 0;
    a.len_hi = kEcSmall;
    hipLaunchKernelGGL((k_ec_call<256, kEcSmall>), dim3((uint32_t)ncalls), dim3(256), 0, ctx->stream, a);
    if (nrecs > kEcSmall) {
      a.len_lo = kEcSmall;
      a.len_hi = kEcMid;
      hipLaunchKernelGGL((k_ec_call<kEcMidThreads, kEcMid>), dim3((uint32_t)ncalls), dim3(kEcMidThreads), 0, ctx->stream,
                         a);
    }
    if (nrecs > kEcMid) {
      a.len_lo = kEcMid;
      a.len_hi = ~0ull;
      hipLaunchKernelGGL((k_ec_call<1024, kEcCap>), dim3((uint32_t)ncalls), dim3(1024), 0, ctx->stream, a);
    }
    SG_HIP(hipGetLastError());
    return SG_OK;
  };
  const TwoPath tp{all_general, false, ncalls, nrecs, kEcCap, need_a, o_scal};
  uint64_t ng = 0;
  int rc = two_path_first(ctx, tp, first_pass, [&](uint64_t n) { return ec_general_bytes(n, ncalls); },
                          &ctx->exec_comps_general, &ng);
  if (rc) return rc;
  if (ng) {
    rc = ec_general(ctx, a, ng, need_a);
    if (rc) return rc;
  }
  rc = scan_counts(ctx, a.cnt, d_comp_off, ncalls, scan_a);
  if (rc) return rc;
  if (d_word_off) {
    rc = scan_counts(ctx, a.wcnt, d_word_off, ncalls, scan_a);
    if (rc) return rc;
  }
  if (raw) {  // the caller reads the workspace keys itself; the word counts and the scan's workspace are done with
    raw->tmp = a.tmp;
    raw->cnt = a.wcnt;
    raw->scan_off = scan_a;
    return SG_OK;
  }
  if (d_comps || (d_word_off && d_words)) {
    ScopedTimer tm(ctx, "exec_comps_emit");
    hipLaunchKernelGGL(k_ec_emit, dim3(div_up(ncalls, 4)), dim3(256), 0, ctx->stream, d_call_off, ncalls, nrecs,
                       (const uint64_t*)a.tmp, (const uint64_t*)d_comp_off, d_comps, comps_cap,
                       (const uint64_t*)d_word_off, d_words, words_cap);
  }
  SG_HIP(hipGetLastError());
  return SG_OK;
}

int ec_limits(uint64_t ncalls, uint64_t nrecs) {
  if (nrecs >= (1ull << 32) || ncalls >= (1ull << 31)) {
    set_error("sg_exec_comps: %llu records, %llu calls (the limits are 2^32 - 1 and 2^31 - 1)",
              (unsigned long long)nrecs, (unsigned long long)ncalls);
    return SG_EINVAL;
  }
  return SG_OK;
}

}  // namespace sg

using namespace sg;

extern "C" {

int sg_exec_comps_dev(sg_ctx* ctx, const uint64_t* d_recs, const uint64_t* d_call_off, uint64_t ncalls, uint64_t nrecs,
                      uint64_t* d_comp_off, uint64_t* d_comps, uint64_t comps_cap, uint64_t* d_word_off,
                      uint32_t* d_words, uint64_t words_cap) {
  if (!ctx || !d_call_off || !d_comp_off || (nrecs && !d_recs) || (comps_cap && !d_comps) ||
      (d_word_off && words_cap && !d_words))
    return SG_EINVAL;
  int rc = ec_limits(ncalls, nrecs);
  if (rc) return rc;
  std::lock_guard<std::mutex> g(ctx->mu);
  rc = ensure_device(ctx);
  if (rc) return rc;
  return exec_comps(ctx, d_recs, d_call_off, ncalls, nrecs, d_comp_off, d_comps, comps_cap, d_word_off, d_words,
                    words_cap);
}

int sg_exec_comps(sg_ctx* ctx, const uint64_t* recs, const uint64_t* call_off, size_t ncalls, uint64_t* comp_off,
                  uint64_t* comps, size_t comps_cap, uint64_t* word_off, uint32_t* words, size_t words_cap) {
  if (!ctx || !call_off || !comp_off || (comps_cap && !comps) || (word_off && words_cap && !words)) return SG_EINVAL;
  const uint64_t nrecs = call_off[ncalls];
  if (!offsets_ok(call_off, ncalls) || (nrecs && !recs)) return SG_EINVAL;
  int rc = ec_limits(ncalls, nrecs);
  if (rc) return rc;
  // nrecs triples and 5 nrecs words always suffice: a smaller cap is staged as it is
  const uint64_t ccap = comps_cap < nrecs ? comps_cap : nrecs;
  const uint64_t wcap = !word_off ? 0 : (words_cap < 5 * nrecs ? words_cap : 5 * nrecs);
  WsPlan p;
  const size_t o_recs = p.add(nrecs * 32 + 32), o_co = p.add((ncalls + 1) * 8), o_comp_off = p.add((ncalls + 1) * 8),
               o_word_off = p.add((ncalls + 1) * 8), o_comps = p.add(ccap * 24 + 24), o_words = p.add(wcap * 4 + 4);
  std::lock_guard<std::mutex> g(ctx->mu);
  rc = ensure_device(ctx);
  if (rc) return rc;
  rc = dstage_reserve(ctx, p);
  if (rc) return rc;
  uint64_t* drecs = dstage_at<uint64_t>(ctx, o_recs);
  uint64_t* dco = dstage_at<uint64_t>(ctx, o_co);
  uint64_t* dcomp_off = dstage_at<uint64_t>(ctx, o_comp_off);
  uint64_t* dword_off = dstage_at<uint64_t>(ctx, o_word_off);
  uint64_t* dcomps = dstage_at<uint64_t>(ctx, o_comps);
  uint32_t* dwords = dstage_at<uint32_t>(ctx, o_words);
  if ((rc = upload(ctx, drecs, recs, nrecs * 32))) return rc;
  if ((rc = upload(ctx, dco, call_off, (ncalls + 1) * 8))) return rc;
  rc = exec_comps(ctx, drecs, dco, ncalls, nrecs, dcomp_off, ccap ? dcomps : nullptr, ccap,
                  word_off ? dword_off : nullptr, wcap ? dwords : nullptr, wcap);
  if (rc) return rc;
  SG_HIP(hipMemcpyAsync(comp_off, dcomp_off, (ncalls + 1) * 8, hipMemcpyDeviceToHost, ctx->stream));
  if (word_off) SG_HIP(hipMemcpyAsync(word_off, dword_off, (ncalls + 1) * 8, hipMemcpyDeviceToHost, ctx->stream));
  SG_HIP(hipStreamSynchronize(ctx->stream));
  if (comp_off[ncalls] && comp_off[ncalls] <= comps_cap)
    SG_HIP(hipMemcpyAsync(comps, dcomps, comp_off[ncalls] * 24, hipMemcpyDeviceToHost, ctx->stream));
  if (word_off && word_off[ncalls] && word_off[ncalls] <= words_cap)
    SG_HIP(hipMemcpyAsync(words, dwords, word_off[ncalls] * 4, hipMemcpyDeviceToHost, ctx->stream));
  SG_HIP(hipStreamSynchronize(ctx->stream));
  return SG_OK;
}

}  // extern "C"
