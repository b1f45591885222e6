// sg_prefix.hip -- prefix_begin / prefix_end over the partitioned path (sg_part.h).
//
// Two-phase triage (the prefix protocol, syzkaller_amd/shard.py).  Begin runs
// the bucket stage of each record slice against base in emitting form: the
// batch's signal not in base is set in marks, and each such s is kept once,
// with its first record, as a pair in the slot's workspace.  Slice j is
// tested against base | marks, so a signal of an earlier slice is not
// re-emitted by a later one: the pairs are the first owners over the whole
// batch.  End: record r is queued iff it owns a pair whose s is in neither
// maxSignal nor the prefix (k_prefix_flags).  That is the sequential loop
// against M = maxsig | prefix for any M containing base: every s of the batch
// outside M is outside base, so its pair is kept, and its first owner is the
// loop's (a record is queued iff it is the first to hold some s outside M).
// That is the form option prefix_pairs 1 selects.  The default keeps the
// partitions instead: begin marks the buckets (k_bucket_mark, the base slice
// in LDS), end runs the bucket stage against maxsig | prefix.  On a fresh C3
// slice (1.76G entries, 361M pairs) the pairs' flag pass (3.9 ms: two random
// cache lines per pair) costs more than the mark pass (2 x 1.0 ms); the pair
// form's end shrinks with the batch's novelty, the kept partitions' does not.
#include "sg_part.h"

namespace sg {

// Marks: nwords |= every signal of the partition's buckets that is not in mwords
// (a workgroup per bucket: its maxSignal slice in LDS, its newSignal words
// written by it alone).  Entries are read as 16-B quads from the bucket start
// rounded down (the pass-2 buffer is padded), kMarkU quads per thread in
// flight; the first ones are issued before the slice is installed.  kFirst:
// nwords = those signals (every word written, empty buckets' too: no clear
// beforehand and no read of the old words).
constexpr int kMarkT = 256, kMarkU = 2;
// bcnt (nullable): per bucket, the signals this launch newly marks (summed by
// k_sum_counts into the batch's count of distinct signals not in mwords; one
// atomic per wave on a single counter serialised: 2 x 3.3 ms per C3 slice)
template <bool kFirst>
__global__ __launch_bounds__(kMarkT) void k_bucket_mark(const uint32_t* __restrict__ in, const uint4* __restrict__ bdesc,
                                                        const uint32_t* __restrict__ mwords,
                                                        uint32_t* __restrict__ nwords,
                                                        uint32_t* __restrict__ bcnt) {
  __shared__ uint32_t mslice[kBucketWords];
  __shared__ uint32_t nbits[kBucketWords];
  __shared__ uint32_t wcnt[kMarkT / 64];
  constexpr int kW = kBucketWords / kMarkT;  // slice words per thread
  typedef uint32_t mvec __attribute__((ext_vector_type(kW)));
  const uint32_t b = blockIdx.x, tid = threadIdx.x;
  const uint4 q = bdesc[b];
  if (q.x >= q.y) {
    if (kFirst) *reinterpret_cast<mvec*>(nwords + bucket_word(b, kW * tid)) = mvec{};
    if (bcnt && tid == 0) bcnt[b] = 0;
    return;
  }
  constexpr uint32_t kStep = kMarkT * 4 * kMarkU;
  auto load = [&](uint32_t base, v4u32 (&v)[kMarkU]) {
#pragma unroll
    for (int u = 0; u < kMarkU; u++) {
      const uint32_t p = base + (u * kMarkT + tid) * 4;
      v[u] = v4u32{0, 0, 0, 0};
      if (p < q.y) v[u] = __builtin_nontemporal_load(reinterpret_cast<const v4u32*>(in + p));
    }
  };
  uint32_t base = q.x & ~3u;
  v4u32 v[kMarkU];
  load(base, v);
  {
    const uint64_t w0 = bucket_word(b, kW * tid);
    reinterpret_cast<mvec*>(mslice)[tid] = *reinterpret_cast<const mvec*>(mwords + w0);
    reinterpret_cast<mvec*>(nbits)[tid] = mvec{};
  }
  __syncthreads();
  for (;;) {
    const uint32_t next = base + kStep;
    v4u32 y[kMarkU];
    if (next < q.y) load(next, y);
#pragma unroll
    for (int u = 0; u < kMarkU; u++) {
      const uint32_t p = base + (u * kMarkT + tid) * 4;
#pragma unroll
      for (int j = 0; j < 4; j++) {
        const uint32_t sl = v[u][j] >> 16;
        const bool live = p + j >= q.x && p + j < q.y;
        if (live && !((mslice[sl >> 5] >> (sl & 31)) & 1u)) atomicOr(&nbits[sl >> 5], 1u << (sl & 31));
      }
    }
    if (next >= q.y) break;
    base = next;
    for (int u = 0; u < kMarkU; u++) v[u] = y[u];
  }
  __syncthreads();
  uint32_t fresh = 0;  // this thread's newly marked signals
  if (kFirst) {
    const mvec nb = reinterpret_cast<const mvec*>(nbits)[tid];
    *reinterpret_cast<mvec*>(nwords + bucket_word(b, kW * tid)) = nb;
#pragma unroll
    for (int j = 0; j < kW; j++) fresh += __popc(nb[j]);
  } else {
    for (uint32_t i = tid; i < kBucketWords; i += kMarkT)
      if (nbits[i]) {
        uint32_t* w = nwords + bucket_word(b, i);
        const uint32_t old = *w;
        fresh += __popc(nbits[i] & ~old);
        *w = old | nbits[i];
      }
  }
  if (bcnt) {
    const uint32_t wsum = __builtin_amdgcn_readlane(sgd::wave_incl_add(fresh), 63);
    if ((tid & 63) == 0) wcnt[tid >> 6] = wsum;
    __syncthreads();
    if (tid == 0) {
      uint32_t t = 0;
#pragma unroll
      for (int i = 0; i < kMarkT / 64; i++) t += wcnt[i];
      bcnt[b] = t;
    }
  }
}

// *acc += the n counts (one workgroup)
__global__ __launch_bounds__(1024) void k_sum_counts(const uint32_t* __restrict__ c, uint32_t n,
                                                     unsigned long long* __restrict__ acc) {
  __shared__ unsigned long long ws[16];
  unsigned long long t = 0;
  for (uint32_t i = threadIdx.x; i < n; i += 1024) t += c[i];
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) t += __shfl_xor(t, o);
  if ((threadIdx.x & 63) == 0) ws[threadIdx.x >> 6] = t;
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned long long s = 0;
    for (int i = 0; i < 16; i++) s += ws[i];
    *acc += s;
  }
}

// The slot's workspace stands in for the context's during one call (the
// partition code addresses the workspace through ctx->ws): swapped in, and
// out again with whatever the call made of it.
struct SlotWs {
  sg_ctx* c;
  PrefixSlot& s;
  SlotWs(sg_ctx* c_, PrefixSlot& s_) : c(c_), s(s_) { c->ws.swap(s.ws); }
  ~SlotWs() { c->ws.swap(s.ws); }
};

// The slot's workspace grows to the size asked for rounded up to 64 MiB, not
// by doubling, since it is kept.
static size_t slot_cap(size_t bytes) { return (bytes + (64u << 20) - 1) & ~size_t((64u << 20) - 1); }

// flags of the kept pairs {s, record}: kFixU pairs per thread in flight (one
// pair per thread and step: 7.2 ms per C3 slice, eight: 3.9 ms).  Bound by
// the random cache-line accesses, two per pair (the bitmap word, the flag
// byte): 361M pairs of a fresh C3 slice at ~0.2 G lines/s/CU
constexpr int kFixT = 256, kFixU = 8;
__global__ __launch_bounds__(kFixT) void k_prefix_flags(const uint2* __restrict__ pairs,
                                                        const unsigned long long* __restrict__ npairs,
                                                        const uint32_t* __restrict__ mwords,
                                                        const uint32_t* __restrict__ owords, uint8_t* __restrict__ rec_new) {
  constexpr uint32_t kNone = 0xFFFFFFFFu;  // (records < 2^32 - 1)
  const uint64_t n = *npairs, stride = (uint64_t)gridDim.x * kFixT * kFixU;
  for (uint64_t base = (uint64_t)blockIdx.x * kFixT * kFixU + threadIdx.x; base < n; base += stride) {
    uint2 p[kFixU];
#pragma unroll
    for (int u = 0; u < kFixU; u++) {
      const uint64_t i = base + (uint64_t)u * kFixT;
      if (i < n) {
        const unsigned long long v = __builtin_nontemporal_load(reinterpret_cast<const unsigned long long*>(pairs) + i);
        p[u] = make_uint2((uint32_t)v, (uint32_t)(v >> 32));
      } else {
        p[u] = make_uint2(0u, kNone);
      }
    }
    uint32_t t[kFixU], w[kFixU];
#pragma unroll
    for (int u = 0; u < kFixU; u++) {
      t[u] = sgd::set_pos(p[u].x);
      w[u] = p[u].y != kNone ? mwords[t[u] >> 5] : ~0u;
    }
    if (owords) {
#pragma unroll
      for (int u = 0; u < kFixU; u++)
        if (p[u].y != kNone) w[u] |= owords[t[u] >> 5];
    }
#pragma unroll
    for (int u = 0; u < kFixU; u++)
      if (!((w[u] >> (t[u] & 31)) & 1u)) rec_new[p[u].y] = 1;
  }
}

// end's set updates: newsig |= marks & ~(maxsig | prefix), maxsig |= marks
__global__ void k_prefix_merge(const uint32_t* __restrict__ marks, uint32_t* __restrict__ mwords,
                               const uint32_t* __restrict__ owords, uint32_t* __restrict__ nwords) {
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t w = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; w < kSetWords / 4; w += stride) {
    const uint4 c = reinterpret_cast<const uint4*>(marks)[w];
    if (!(c.x | c.y | c.z | c.w)) continue;
    uint4 m = reinterpret_cast<uint4*>(mwords)[w];
    if (nwords) {
      uint4 o = owords ? reinterpret_cast<const uint4*>(owords)[w] : make_uint4(0, 0, 0, 0);
      uint4 nw = reinterpret_cast<uint4*>(nwords)[w];
      nw.x |= c.x & ~(m.x | o.x);
      nw.y |= c.y & ~(m.y | o.y);
      nw.z |= c.z & ~(m.z | o.z);
      nw.w |= c.w & ~(m.w | o.w);
      reinterpret_cast<uint4*>(nwords)[w] = nw;
    }
    m.x |= c.x;
    m.y |= c.y;
    m.z |= c.z;
    m.w |= c.w;
    reinterpret_cast<uint4*>(mwords)[w] = m;
  }
}

int prefix_begin(sg_ctx* ctx, uint32_t slot, const uint32_t* base_words, uint32_t* marks_words, const uint32_t* d_vals,
                 const uint64_t* d_off, uint64_t n, uint64_t nrec, int form, uint64_t* d_ncand) {
  if (slot >= kPrefixSlots) {
    set_error("prefix triage: slot %u out of range", slot);
    return SG_EINVAL;
  }
  if (nrec >= 0xFFFFFFFFull || n >= 0xFFFFFFFFull - 2 * kPT) {
    set_error("prefix triage: a batch holds < 2^32 signal entries and < 2^32 - 1 records");
    return SG_EINVAL;
  }
  PrefixSlot& S = ctx->prefix[slot];
  S.slices.clear();
  S.open = false;
  S.keep = form < 0 ? ctx->opt[kOptPrefixPairs] == 0 : form != 1;
  const bool mark = form != 2;  // form 2: the partitions alone (a plain triage split in two)
  if (d_ncand) SG_HIP(hipMemsetAsync(d_ncand, 0, 8, ctx->stream));
  S.marks = marks_words;
  S.n = n;
  std::vector<RecSlice> sl;
  int rc = nrec ? record_slices(ctx, d_off, nrec, sl) : SG_OK;
  if (rc) return rc;
  if (!S.keep) {
    // the pairs: a counter, then <= n pairs
    rc = S.ws.grow_drop(slot_cap(256 + n * 8), ctx->stream);
    if (rc) return rc;
    unsigned long long* np = (unsigned long long*)S.ws.p;
    uint2* pairs = (uint2*)(S.ws.p + 256);
    SG_HIP(hipMemsetAsync(np, 0, 8, ctx->stream));
    SG_HIP(hipMemsetAsync(marks_words, 0, kSetBytes, ctx->stream));  // (the later slices' filter)
    size_t need = 0;
    for (const RecSlice& x : sl)
      if (x.e1 > x.e0)
        need = std::max(need, align256(bucket_plan_bytes(x.e1 - x.e0, x.r1 - x.r0)) + align256((x.r1 - x.r0 + 1) * 8));
    if (need) {
      rc = ws_reserve(ctx, need);
      if (rc) return rc;
    }
    for (const RecSlice& x : sl) {
      if (x.e1 == x.e0) continue;
      const uint64_t ns = x.e1 - x.e0, nr = x.r1 - x.r0;
      BucketPlan bp(ns, nr);
      uint64_t* roff = (uint64_t*)ws_at(ctx, align256(bucket_plan_bytes(ns, nr)));
      rc = rebase_offsets(ctx, d_off + x.r0, nr + 1, x.e0, roff);
      if (!rc) rc = partition_one(ctx, d_vals + x.e0, roff, 0, true, bp);
      if (rc) return rc;
      const EmitArgs e{pairs, np, (uint32_t)x.r0, 1, nullptr};
      rc = buckets_one(ctx, bp, const_cast<uint32_t*>(base_words), marks_words, nullptr, &e, marks_words);
      if (rc) return rc;
    }
    // (each distinct signal not in base is one pair)
    if (d_ncand) SG_HIP(hipMemcpyAsync(d_ncand, np, 8, hipMemcpyDeviceToDevice, ctx->stream));
    S.nrec = nrec;
    S.open = true;
    return SG_OK;
  }
  size_t total = 0;
  for (const RecSlice& x : sl)
    if (x.e1 > x.e0) total += align256(bucket_plan_bytes(x.e1 - x.e0, x.r1 - x.r0)) + align256((x.r1 - x.r0 + 1) * 8);
  rc = S.ws.grow_drop(slot_cap(total ? total : 256), ctx->stream);
  if (rc) return rc;
  SlotWs guard(ctx, S);
  size_t base = 0;
  bool first = true;
  for (const RecSlice& x : sl) {
    PrefixSlice ps{x.r0, x.r1, x.e0, x.e1, base};
    if (x.e1 > x.e0) {
      const uint64_t ns = x.e1 - x.e0, nr = x.r1 - x.r0;
      BucketPlan bp(ns, nr);
      const size_t roff_at = base + align256(bucket_plan_bytes(ns, nr));
      uint64_t* roff = (uint64_t*)ws_at(ctx, roff_at);
      rc = rebase_offsets(ctx, d_off + x.r0, nr + 1, x.e0, roff);
      if (!rc) rc = partition_one(ctx, d_vals + x.e0, roff, base, true, bp);
      if (rc) return rc;
      if (mark) {
        ScopedTimer tm(ctx, "bucket_mark");
        const uint32_t* v2 = bp.at<uint32_t>(ctx, kV2);
        const uint4* bd = bp.at<uint4>(ctx, kBD);
        // (per-bucket counts in the partition's non-empty flags, which the
        // bucket stage does not read)
        uint32_t* bc = d_ncand ? bp.at<uint32_t>(ctx, kBN) : nullptr;
        auto km = first ? k_bucket_mark<true> : k_bucket_mark<false>;  // the batch's first slice writes every marks word
        hipLaunchKernelGGL(km, dim3(kNumBuckets), dim3(kMarkT), 0, ctx->stream, v2, bd, base_words, marks_words, bc);
        if (bc)
          hipLaunchKernelGGL(k_sum_counts, dim3(1), dim3(1024), 0, ctx->stream, (const uint32_t*)bc, kNumBuckets,
                             (unsigned long long*)d_ncand);
        first = false;
      }
      SG_HIP(hipGetLastError());
      base = roff_at + align256((nr + 1) * 8);
    }
    S.slices.push_back(ps);
  }
  if (first && mark) SG_HIP(hipMemsetAsync(marks_words, 0, kSetBytes, ctx->stream));  // no entries
  S.nrec = nrec;
  S.open = true;
  return SG_OK;
}

int prefix_end(sg_ctx* ctx, uint32_t slot, uint32_t* mwords, const uint32_t* owords, uint32_t* nwords,
               uint8_t* d_rec_new, bool update) {
  if (slot >= kPrefixSlots || !ctx->prefix[slot].open) {
    set_error("prefix triage: no batch begun in slot %u", slot);
    return SG_EINVAL;
  }
  PrefixSlot& S = ctx->prefix[slot];
  S.open = false;
  if (S.nrec) SG_HIP(hipMemsetAsync(d_rec_new, 0, S.nrec, ctx->stream));
  if (!S.keep) {
    if (S.n) {
      ScopedTimer tm(ctx, "prefix_flags");
      hipLaunchKernelGGL(k_prefix_flags, dim3((uint32_t)std::min<uint64_t>(div_up(S.n, kFixT * kFixU), 2048)),
                         dim3(kFixT), 0,
                         ctx->stream, (const uint2*)(S.ws.p + 256), (const unsigned long long*)S.ws.p, mwords,
                         owords, d_rec_new);
    }
    if (ctx->debug_part && S.n) {  // diagnostics (syncs): the kept pairs
      unsigned long long np = 0;
      SG_HIP(hipMemcpyAsync(&np, S.ws.p, 8, hipMemcpyDeviceToHost, ctx->stream));
      SG_HIP(hipStreamSynchronize(ctx->stream));
      fprintf(stderr, "sg prefix: %llu entries, %llu pairs\n", (unsigned long long)S.n, np);
    }
    if (update && S.n) {
      ScopedTimer tm(ctx, "prefix_merge");
      hipLaunchKernelGGL(k_prefix_merge, dim3(8192), dim3(256), 0, ctx->stream, S.marks, mwords, owords, nwords);
    }
    SG_HIP(hipGetLastError());
    return SG_OK;
  }
  SlotWs guard(ctx, S);
  for (const PrefixSlice& x : S.slices) {
    if (x.e1 == x.e0) continue;
    const uint64_t ns = x.e1 - x.e0, nr = x.r1 - x.r0;
    BucketPlan bp(ns, nr);
    bp.rebase(x.ws_base);
    const int rc = buckets_one(ctx, bp, mwords, nwords, d_rec_new + x.r0, nullptr, owords);
    if (rc) return rc;
  }
  return SG_OK;
}

}  // namespace sg
