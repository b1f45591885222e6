// sg_call_prios.hip -- call-to-call priorities and the ChoiceTable's running
// sums from the corpus' call ids (prog/prio.go:27-36, :133-229, called from
// syz-manager/manager.go:816-837 and html.go:196-224).
//
// The table (sg_prio_table) keeps the pair counts of calcDynamicPrio
// (prio.go:138-151) exact, as 64-bit integers, next to the static matrix and
// the enabled bytes.  count[i][j] = sum over programs of n_p(i) * n_p(j), i != j,
// neither of them mmap.  The reference's float32 cell is min(count, 2^24): the
// saturation is applied where the counts are read (k_prio_finish), never where
// they are accumulated.
//
// sg_prio_table_add*, on the context's stream:
//  1. k_prio_merge, a thread per program of at most kPrioShort calls: every
//     first occurrence of an id becomes an entry (id, n, its place in the
//     program, the program's length) at the id's own place of a buffer shaped
//     like call_ids; repeats, mmap, ids >= ncalls (counted: "prio_bad_ids")
//     and the places of longer programs stay kPrioNone.  Longer programs are
//     listed for step 3.
//  2. k_prio_band: workgroup (b, s) owns the rows [b * R, b * R + R) of the
//     matrix as u32 cells in LDS (R * ncalls <= kPrioBandCells: the CU's whole
//     160 KiB, dynamic LDS, one workgroup of 16 waves per CU) and streams
//     part s of the entries, a wave 64 places at a time.  For each of them
//     whose id falls in the band, the wave reads that program's entries (at
//     most 64: a lane each, one coalesced load) and adds n_i * n_j to
//     row[id_i][id_j] in LDS.  The band is then added to the 64-bit counts:
//     contiguous 64-bit atomic adds, zero cells skipped.  No global atomic per
//     pair.
//     Bound of an LDS cell: a program of len <= kPrioShort calls adds
//     n_i * n_j <= (len / 2)^2 <= len * kPrioShort / 4 to a cell, so a part of
//     at most kPrioPart = 2^26 places adds at most 2^26 * 16 = 2^30 < 2^32
//     before its one flush.
//  3. k_prio_long, a workgroup per listed program, of any length: the
//     program's histogram over the ids in LDS (u32: a call takes fewer than
//     2^32 ids), its nonzero ids compacted, and n_i * n_j (64-bit) added to the
//     counts for every ordered pair of them.
//
// k_prio_finish, a workgroup per row: saturate, normalizePrio (prio.go:158-192)
// with every operation rounded to float32 in the reference's order, the
// multiply by the static row (prio.go:30-34) and BuildChoiceTable's masked
// running sum (prio.go:203-229).  The diagonal of the counts is zero, so every
// row has nzero >= 1, min < max whenever max > 0, and no NaN arises.
//
// Floating point: Go on amd64 does not fuse a * b + c, hipcc's default does in
// device code.  Contraction is off for this whole unit.  The division is the
// correctly rounded one (hipcc's default); no reciprocal, no __fdividef.
#include "sg_internal.h"

#include <algorithm>
#include <cmath>

#pragma clang fp contract(off)

struct sg_prio_table {
  sg_ctx* ctx = nullptr;
  sg::DevBuf<char> mem;  // the one device block: static, enabled, counts
  uint32_t ncalls = 0, mmap_id = SG_NO_CALL;
  float* stat = nullptr;                 // [ncalls * ncalls]
  uint8_t* enabled = nullptr;            // [ncalls]
  unsigned long long* counts = nullptr;  // [ncalls * ncalls]
};

namespace sg {
namespace {

constexpr uint32_t kPrioNone = 0xFFFFFFFFu;
// an entry: id (13 bits), n (7), place in the program (6), length - 1 (6)
constexpr uint32_t kIdBits = 13, kNBits = 7, kPosBits = 6;
static_assert(SG_PRIO_MAX_CALLS == 1u << kIdBits, "an entry's id field");
static_assert(kPrioShort == 1u << kPosBits && kPrioShort < (1u << kNBits), "an entry's n and place fields");
constexpr uint64_t kPrioPart = 1ull << 26;  // places per workgroup of k_prio_band at the most
constexpr uint32_t kPT = 256;
constexpr uint32_t kBandT = 1024;  // k_prio_band: the one workgroup that fits a CU's LDS, 16 waves

__device__ __forceinline__ uint32_t ent_id(uint32_t e) { return e & ((1u << kIdBits) - 1); }
__device__ __forceinline__ uint32_t ent_n(uint32_t e) { return (e >> kIdBits) & ((1u << kNBits) - 1); }
__device__ __forceinline__ uint32_t ent_pos(uint32_t e) { return (e >> (kIdBits + kNBits)) & ((1u << kPosBits) - 1); }
__device__ __forceinline__ uint32_t ent_len(uint32_t e) { return (e >> (kIdBits + kNBits + kPosBits)) + 1; }

struct AddArgs {
  const uint32_t* ids;
  const uint64_t* off;
  uint64_t nprogs, nids;
  uint32_t ncalls, mmap_id;
  uint32_t* ent;                // [nids], kPrioNone before k_prio_merge
  uint64_t* longs;              // [long_cap] programs longer than kPrioShort
  uint64_t long_cap;
  unsigned long long* nlong;    // zero before k_prio_merge
  unsigned long long* bad;      // the context's "prio_bad_ids"
  unsigned long long* counts;
};

__global__ __launch_bounds__(kPT) void k_prio_merge(AddArgs a) {
  const uint64_t stride = (uint64_t)gridDim.x * kPT;
  for (uint64_t p = (uint64_t)blockIdx.x * kPT + threadIdx.x; p < a.nprogs; p += stride) {
    uint64_t a0, a1;
    sgd::csr_range(a.off, p, a.nids, a0, a1);  // program p's ids, clamped to the buffer
    const uint64_t len = a1 - a0;
    if (len == 0) continue;
    if (len > kPrioShort) {
      const unsigned long long i = atomicAdd(a.nlong, 1ull);
      if (i < a.long_cap) a.longs[i] = p;
      continue;
    }
    uint32_t bad = 0;
    for (uint32_t k = 0; k < (uint32_t)len; k++) {
      const uint32_t id = a.ids[a0 + k];
      if (id >= a.ncalls) {
        bad++;
        continue;
      }
      if (id == a.mmap_id) continue;
      uint32_t n = 0;
      bool first = true;
      for (uint32_t j = 0; j < (uint32_t)len; j++)
        if (a.ids[a0 + j] == id) {
          if (j < k) {
            first = false;
            break;
          }
          n++;
        }
      if (first)
        a.ent[a0 + k] = id | (n << kIdBits) | (k << (kIdBits + kNBits)) | (((uint32_t)len - 1) << (kIdBits + kNBits + kPosBits));
    }
    if (bad) atomicAdd(a.bad, (unsigned long long)bad);
  }
}

__global__ __launch_bounds__(kBandT) void k_prio_band(const uint32_t* __restrict__ ent, uint64_t nids, uint32_t ncalls,
                                                      uint32_t rows, uint64_t part, unsigned long long* counts) {
  extern __shared__ uint32_t band[];  // kPrioBandCells
  const uint32_t r0 = blockIdx.x * rows, r1 = min(r0 + rows, ncalls);
  const uint32_t cells = (r1 - r0) * ncalls;  // <= rows * ncalls <= kPrioBandCells
  for (uint32_t c = threadIdx.x; c < cells; c += kBandT) band[c] = 0;
  __syncthreads();
  const uint32_t lane = threadIdx.x & 63;
  const uint64_t k0 = (uint64_t)blockIdx.y * part, k1 = min(k0 + part, nids);
  // a wave takes 64 places at a time; for each of them whose id is in the band, the wave
  // reads that program's entries (at most kPrioShort == 64), a lane each, and adds
  for (uint64_t kb = k0 + (threadIdx.x - lane); kb < k1; kb += kBandT) {
    const uint64_t k = kb + lane;
    const uint32_t e = k < k1 ? ent[k] : kPrioNone;
    const uint32_t id = ent_id(e);
    unsigned long long m = __ballot(e != kPrioNone && id >= r0 && id < r1);
    while (m) {
      const int src = __ffsll((long long)m) - 1;
      m &= m - 1;
      const uint32_t es = __shfl(e, src);
      const uint64_t ks = kb + src;
      const uint32_t ida = ent_id(es);
      const uint64_t j = ks - min<uint64_t>(ent_pos(es), ks) + lane;
      if (lane < ent_len(es) && j < nids) {
        const uint32_t e2 = ent[j];
        const uint32_t id2 = ent_id(e2);
        if (e2 != kPrioNone && id2 != ida && id2 < ncalls) atomicAdd(&band[(ida - r0) * ncalls + id2], ent_n(es) * ent_n(e2));
      }
    }
  }
  __syncthreads();
  unsigned long long* dst = counts + (uint64_t)r0 * ncalls;
  for (uint32_t c = threadIdx.x; c < cells; c += kBandT) {
    const uint32_t v = band[c];
    if (v) atomicAdd(&dst[c], (unsigned long long)v);
  }
}

__global__ __launch_bounds__(kPT) void k_prio_long(AddArgs a) {
  __shared__ uint32_t hist[SG_PRIO_MAX_CALLS];
  __shared__ uint16_t lst[SG_PRIO_MAX_CALLS];
  __shared__ uint32_t nd;
  const uint64_t nl = min<uint64_t>(*a.nlong, a.long_cap);
  for (uint64_t li = blockIdx.x; li < nl; li += gridDim.x) {
    const uint64_t p = min(a.longs[li], a.nprogs - 1);
    uint64_t a0, a1;
    sgd::csr_range(a.off, p, a.nids, a0, a1);  // program p's ids, clamped to the buffer
    for (uint32_t i = threadIdx.x; i < a.ncalls; i += kPT) hist[i] = 0;
    if (threadIdx.x == 0) nd = 0;
    __syncthreads();
    uint32_t bad = 0;
    for (uint64_t k = a0 + threadIdx.x; k < a1; k += kPT) {
      const uint32_t id = a.ids[k];
      if (id >= a.ncalls)
        bad++;
      else if (id != a.mmap_id)
        atomicAdd(&hist[id], 1u);
    }
    if (bad) atomicAdd(a.bad, (unsigned long long)bad);
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < a.ncalls; i += kPT)
      if (hist[i]) lst[atomicAdd(&nd, 1u)] = (uint16_t)i;  // (nd <= ncalls <= SG_PRIO_MAX_CALLS)
    __syncthreads();
    const uint32_t d = nd;
    for (uint32_t x = 0; x < d; x++) {
      const uint32_t ia = lst[x];
      const unsigned long long na = hist[ia];
      unsigned long long* row = a.counts + (uint64_t)ia * a.ncalls;
      for (uint32_t y = threadIdx.x; y < d; y += kPT) {
        const uint32_t ib = lst[y];
        if (ib != ia) atomicAdd(&row[ib], na * hist[ib]);
      }
    }
    __syncthreads();
  }
}

struct FinArgs {
  const unsigned long long* counts;
  const float* stat;
  const uint8_t* enabled;
  uint32_t ncalls;
  float* dynamic;  // each nullable
  float* prios;
  int32_t* run;
};

__global__ __launch_bounds__(kPT) void k_prio_finish(FinArgs a) {
  __shared__ float row[SG_PRIO_MAX_CALLS];
  __shared__ float smax[kPT / 64], smin[kPT / 64];
  __shared__ uint32_t snz[kPT / 64], ssum[kPT / 64];
  const uint32_t i = blockIdx.x, nc = a.ncalls, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint64_t base = (uint64_t)i * nc;
  // the reference's float32 cells, and the row's max, min over nonzero cells, zero cells (prio.go:160-173)
  float mx = 0.0f, mn = 1e10f;
  uint32_t nz = 0;
  for (uint32_t j = threadIdx.x; j < nc; j += kPT) {
    const unsigned long long c = a.counts[base + j];
    const float p = (float)(uint32_t)min(c, 1ull << 24);  // exact
    row[j] = p;
    if (mx < p) mx = p;
    if (p != 0.0f && mn > p) mn = p;
    if (p == 0.0f) nz++;
  }
  for (int m = 32; m; m >>= 1) {
    mx = fmaxf(mx, __shfl_xor(mx, m));
    mn = fminf(mn, __shfl_xor(mn, m));
    nz += __shfl_xor(nz, m);
  }
  if (lane == 0) {
    smax[wave] = mx;
    smin[wave] = mn;
    snz[wave] = nz;
  }
  __syncthreads();
  mx = smax[0], mn = smin[0], nz = snz[0];
  for (uint32_t w = 1; w < kPT / 64; w++) {
    mx = fmaxf(mx, smax[w]);
    mn = fminf(mn, smin[w]);
    nz += snz[w];
  }
  if (nz != 0) mn = mn / (2.0f * (float)nz);  // :174-176
  const float range = mx - mn;
  for (uint32_t j = threadIdx.x; j < nc; j += kPT) {
    float p = row[j];
    if (mx == 0.0f) {
      p = 1.0f;  // :178-181
    } else {
      if (p == 0.0f) p = mn;
      p = (p - mn) / range;  // :185, one rounding per operation
      p = p * 0.9f;
      p = p + 0.1f;
      if (p > 1.0f) p = 1.0f;
    }
    if (a.dynamic) a.dynamic[base + j] = p;
    p = p * a.stat[base + j];  // prio.go:32
    if (a.prios) a.prios[base + j] = p;
    row[j] = p;
  }
  if (!a.run) return;
  // BuildChoiceTable (prio.go:214-227): 256 columns per step, the sum carried
  const bool on = a.enabled[i] != 0;
  uint32_t carry = 0;
  for (uint32_t j0 = 0; j0 < nc; j0 += kPT) {
    const uint32_t j = j0 + threadIdx.x;
    uint32_t v = 0;
    if (on && j < nc && a.enabled[j]) v = (uint32_t)(int)(row[j] * 1000.0f);
    v = sgd::wave_incl_add(v);
    __syncthreads();  // (the sums of the step before are read)
    if (lane == 63) ssum[wave] = v;
    __syncthreads();
    for (uint32_t w = 0; w < wave; w++) v += ssum[w];
    if (j < nc) a.run[base + j] = (int32_t)(carry + v);
    carry += ssum[0] + ssum[1] + ssum[2] + ssum[3];
  }
}
static_assert(kPT == 256, "k_prio_finish sums four waves");

// the adds of one corpus: every pointer device memory; ctx lock held, the device ensured
int prio_add(sg_prio_table* t, const uint32_t* d_ids, const uint64_t* d_off, uint64_t nprogs, uint64_t nids) {
  sg_ctx* ctx = t->ctx;
  if (nprogs == 0 || nids == 0) return SG_OK;
  WsPlan plan;
  const uint64_t long_cap = nids / (kPrioShort + 1) + 1;
  const size_t o_ent = plan.add(nids * 4), o_long = plan.add(long_cap * 8), o_nl = plan.add(8);
  int rc = ws_reserve(ctx, plan);
  if (rc) return rc;
  AddArgs a{d_ids, d_off, nprogs, nids, t->ncalls, t->mmap_id, (uint32_t*)ws_at(ctx, o_ent), (uint64_t*)ws_at(ctx, o_long),
            long_cap, (unsigned long long*)ws_at(ctx, o_nl), (unsigned long long*)&ctx->dev.p->prio_bad_ids, t->counts};
  SG_HIP(hipMemsetAsync(a.ent, 0xFF, nids * 4, ctx->stream));
  SG_HIP(hipMemsetAsync(a.nlong, 0, 8, ctx->stream));
  {
    ScopedTimer tm(ctx, "prio_merge");
    hipLaunchKernelGGL(k_prio_merge, dim3(std::min<uint64_t>(div_up(nprogs, kPT), 1u << 20)), dim3(kPT), 0, ctx->stream, a);
  }
  SG_HIP(hipGetLastError());
  // the bands, and the parts of the places, none of more than kPrioPart places (sg_plan.h)
  const BandPlan bp = band_plan(t->ncalls, nids, kPrioBandCells, kBandT, kPrioPart);
  // (more than 64 KiB of LDS has to be allowed per kernel and device)
  constexpr uint32_t kBandBytes = kPrioBandCells * 4;
  SG_HIP(hipFuncSetAttribute((const void*)k_prio_band, hipFuncAttributeMaxDynamicSharedMemorySize, kBandBytes));
  {
    ScopedTimer tm(ctx, "prio_band");
    hipLaunchKernelGGL(k_prio_band, dim3(bp.nbands, bp.gridy), dim3(kBandT), kBandBytes, ctx->stream, a.ent, nids,
                       t->ncalls, bp.rows, bp.part, t->counts);
  }
  SG_HIP(hipGetLastError());
  {
    ScopedTimer tm(ctx, "prio_long");
    hipLaunchKernelGGL(k_prio_long, dim3((uint32_t)std::min<uint64_t>(long_cap, 256)), dim3(kPT), 0, ctx->stream, a);
  }
  SG_HIP(hipGetLastError());
  return SG_OK;
}

int prio_finish(sg_prio_table* t, float* d_dynamic, float* d_prios, int32_t* d_run) {
  sg_ctx* ctx = t->ctx;
  if (!d_dynamic && !d_prios && !d_run) return SG_OK;
  ScopedTimer tm(ctx, "prio_finish");
  const FinArgs a{t->counts, t->stat, t->enabled, t->ncalls, d_dynamic, d_prios, d_run};
  hipLaunchKernelGGL(k_prio_finish, dim3(t->ncalls), dim3(kPT), 0, ctx->stream, a);
  SG_HIP(hipGetLastError());
  return SG_OK;
}

// the three outputs of a host form in the staging buffer, then in the caller's arrays
struct OutPlan {
  size_t o[3];
  size_t cells;
  OutPlan(WsPlan& p, const sg_prio_table* t, const void* dynamic, const void* prios, const void* run) {
    cells = (size_t)t->ncalls * t->ncalls;
    const void* h[3] = {dynamic, prios, run};
    for (int k = 0; k < 3; k++) o[k] = h[k] ? p.add(cells * 4) : 0;
  }
  template <typename T>
  T* dev(sg_ctx* ctx, int k, const void* h) const {
    return h ? dstage_at<T>(ctx, o[k]) : nullptr;
  }
};

// finish into the staging buffer and copy out; waits once
int prio_finish_host(sg_prio_table* t, const OutPlan& op, float* dynamic, float* prios, int32_t* run) {
  sg_ctx* ctx = t->ctx;
  float *dd = op.dev<float>(ctx, 0, dynamic), *dp = op.dev<float>(ctx, 1, prios);
  int32_t* dr = op.dev<int32_t>(ctx, 2, run);
  int rc = prio_finish(t, dd, dp, dr);
  if (rc) return rc;
  if (dynamic) SG_HIP(hipMemcpyAsync(dynamic, dd, op.cells * 4, hipMemcpyDeviceToHost, ctx->stream));
  if (prios) SG_HIP(hipMemcpyAsync(prios, dp, op.cells * 4, hipMemcpyDeviceToHost, ctx->stream));
  if (run) SG_HIP(hipMemcpyAsync(run, dr, op.cells * 4, hipMemcpyDeviceToHost, ctx->stream));
  SG_HIP(hipStreamSynchronize(ctx->stream));
  return SG_OK;
}

// a host corpus: NULL pointers, the offsets, the id count, every id
int progs_ok(const char* fn, const sg_prio_table* t, const uint32_t* call_ids, const uint64_t* prog_off, size_t nprogs) {
  if (!t || !prog_off) {
    set_error("%s: invalid argument", fn);
    return SG_EINVAL;
  }
  if (!offsets_ok(prog_off, nprogs)) {
    set_error("%s: offsets start at 0 and do not decrease", fn);
    return SG_EINVAL;
  }
  const uint64_t nids = prog_off[nprogs];
  if (nids >= (1ull << 32)) {
    set_error("%s: %llu call ids (the limit is 2^32 - 1)", fn, (unsigned long long)nids);
    return SG_EINVAL;
  }
  if (nids && !call_ids) {
    set_error("%s: invalid argument", fn);
    return SG_EINVAL;
  }
  for (uint64_t k = 0; k < nids; k++)
    if (call_ids[k] >= t->ncalls) {
      set_error("%s: call id %u at %llu of %u calls", fn, call_ids[k], (unsigned long long)k, t->ncalls);
      return SG_EINVAL;
    }
  return SG_OK;
}


}  // namespace
}  // namespace sg

using namespace sg;

extern "C" {

int sg_prio_table_create(sg_ctx* ctx, uint32_t ncalls, uint32_t mmap_id, const float* static_prios, const uint8_t* enabled,
                         sg_prio_table** out) {
  const char* fn = "sg_prio_table_create";
  if (!ctx || !static_prios || !out) {
    set_error("%s: invalid argument", fn);
    return SG_EINVAL;
  }
  *out = nullptr;
  if (ncalls == 0 || ncalls > SG_PRIO_MAX_CALLS) {
    set_error("%s: %u calls (1 to %u)", fn, ncalls, SG_PRIO_MAX_CALLS);
    return SG_EINVAL;
  }
  if (mmap_id != SG_NO_CALL && mmap_id >= ncalls) {
    set_error("%s: mmap id %u of %u calls", fn, mmap_id, ncalls);
    return SG_EINVAL;
  }
  const size_t cells = (size_t)ncalls * ncalls;
  for (size_t k = 0; k < cells; k++)
    if (!(static_prios[k] >= 0.0f && static_prios[k] <= 1.0f)) {  // (a NaN fails both)
      set_error("%s: static priority %g at [%zu][%zu] is not in [0, 1]", fn, (double)static_prios[k], k / ncalls,
                k % ncalls);
      return SG_EINVAL;
    }
  std::lock_guard<std::mutex> g(ctx->mu);
  int rc = ensure_device(ctx);
  if (rc) return rc;
  sg_prio_table* t = new sg_prio_table();
  t->ctx = ctx;
  t->ncalls = ncalls;
  t->mmap_id = mmap_id;
  WsPlan bp;
  const size_t o_cnt = bp.add(cells * 8), o_st = bp.add(cells * 4), o_en = bp.add(ncalls);
  rc = t->mem.grow_drop(bp.total, nullptr);
  if (rc) {
    delete t;
    return rc;
  }
  char* b = t->mem.p;
  t->counts = (unsigned long long*)(b + o_cnt);
  t->stat = (float*)(b + o_st);
  t->enabled = (uint8_t*)(b + o_en);
  auto fill = [&]() -> int {
    SG_HIP(hipMemsetAsync(t->counts, 0, cells * 8, ctx->stream));
    int rc = upload(ctx, t->stat, static_prios, cells * 4);
    if (rc) return rc;
    if (enabled) {
      if ((rc = upload(ctx, t->enabled, enabled, ncalls))) return rc;
    } else {
      SG_HIP(hipMemsetAsync(t->enabled, 1, ncalls, ctx->stream));
    }
    SG_HIP(hipStreamSynchronize(ctx->stream));  // (the host arrays are the caller's again)
    return SG_OK;
  };
  rc = fill();
  if (rc) {
    (void)hipStreamSynchronize(ctx->stream);
    delete t;
    return rc;
  }
  *out = t;
  return SG_OK;
}

void sg_prio_table_destroy(sg_prio_table* t) {
  if (!t) return;
  {
    std::lock_guard<std::mutex> g(t->ctx->mu);
    hipSetDevice(t->ctx->device);
    hipStreamSynchronize(t->ctx->stream);
  }
  delete t;
}

int sg_prio_table_clear(sg_prio_table* t) {
  if (!t) {
    set_error("sg_prio_table_clear: invalid argument");
    return SG_EINVAL;
  }
  sg_ctx* ctx = t->ctx;
  std::lock_guard<std::mutex> g(ctx->mu);
  int rc = ensure_device(ctx);
  if (rc) return rc;
  SG_HIP(hipMemsetAsync(t->counts, 0, (size_t)t->ncalls * t->ncalls * 8, ctx->stream));
  return SG_OK;
}

int sg_prio_table_add_dev(sg_prio_table* t, const uint32_t* d_call_ids, const uint64_t* d_prog_off, uint64_t nprogs,
                          uint64_t nids) {
  const char* fn = "sg_prio_table_add_dev";
  if (!t || !d_prog_off || (nids && !d_call_ids)) {
    set_error("%s: invalid argument", fn);
    return SG_EINVAL;
  }
  if (nids >= (1ull << 32)) {
    set_error("%s: %llu call ids (the limit is 2^32 - 1)", fn, (unsigned long long)nids);
    return SG_EINVAL;
  }
  sg_ctx* ctx = t->ctx;
  std::lock_guard<std::mutex> g(ctx->mu);
  int rc = ensure_device(ctx);
  if (rc) return rc;
  return prio_add(t, d_call_ids, d_prog_off, nprogs, nids);
}

int sg_prio_table_add(sg_prio_table* t, const uint32_t* call_ids, const uint64_t* prog_off, size_t nprogs) {
  int rc = progs_ok("sg_prio_table_add", t, call_ids, prog_off, nprogs);
  if (rc) return rc;
  const uint64_t nids = prog_off[nprogs];
  sg_ctx* ctx = t->ctx;
  std::lock_guard<std::mutex> g(ctx->mu);
  rc = ensure_device(ctx);
  if (rc) return rc;
  if (nids == 0) return SG_OK;
  WsPlan plan;
  const size_t o_ids = plan.add(nids * 4), o_off = plan.add((nprogs + 1) * 8);
  rc = dstage_reserve(ctx, plan);
  if (rc) return rc;
  uint32_t* dids = dstage_at<uint32_t>(ctx, o_ids);
  uint64_t* doff = dstage_at<uint64_t>(ctx, o_off);
  if ((rc = upload(ctx, dids, call_ids, nids * 4))) return rc;
  if ((rc = upload(ctx, doff, prog_off, (nprogs + 1) * 8))) return rc;
  rc = prio_add(t, dids, doff, nprogs, nids);
  if (rc) return rc;
  SG_HIP(hipStreamSynchronize(ctx->stream));  // (the host arrays are the caller's again)
  return SG_OK;
}

int sg_prio_table_counts(sg_prio_table* t, uint64_t* counts) {
  if (!t || !counts) {
    set_error("sg_prio_table_counts: invalid argument");
    return SG_EINVAL;
  }
  sg_ctx* ctx = t->ctx;
  std::lock_guard<std::mutex> g(ctx->mu);
  int rc = ensure_device(ctx);
  if (rc) return rc;
  SG_HIP(hipMemcpyAsync(counts, t->counts, (size_t)t->ncalls * t->ncalls * 8, hipMemcpyDeviceToHost, ctx->stream));
  SG_HIP(hipStreamSynchronize(ctx->stream));
  return SG_OK;
}

int sg_call_prios_dev(sg_prio_table* t, float* d_dynamic, float* d_prios, int32_t* d_run) {
  if (!t) {
    set_error("sg_call_prios_dev: invalid argument");
    return SG_EINVAL;
  }
  sg_ctx* ctx = t->ctx;
  std::lock_guard<std::mutex> g(ctx->mu);
  int rc = ensure_device(ctx);
  if (rc) return rc;
  return prio_finish(t, d_dynamic, d_prios, d_run);
}

int sg_call_prios(sg_prio_table* t, float* dynamic, float* prios, int32_t* run) {
  if (!t) {
    set_error("sg_call_prios: invalid argument");
    return SG_EINVAL;
  }
  sg_ctx* ctx = t->ctx;
  std::lock_guard<std::mutex> g(ctx->mu);
  int rc = ensure_device(ctx);
  if (rc) return rc;
  if (!dynamic && !prios && !run) return SG_OK;
  WsPlan plan;
  const OutPlan op(plan, t, dynamic, prios, run);
  rc = dstage_reserve(ctx, plan);
  if (rc) return rc;
  return prio_finish_host(t, op, dynamic, prios, run);
}

int sg_call_prios_from_progs(sg_prio_table* t, const uint32_t* call_ids, const uint64_t* prog_off, size_t nprogs,
                             float* dynamic, float* prios, int32_t* run) {
  int rc = progs_ok("sg_call_prios_from_progs", t, call_ids, prog_off, nprogs);
  if (rc) return rc;
  const uint64_t nids = prog_off[nprogs];
  sg_ctx* ctx = t->ctx;
  std::lock_guard<std::mutex> g(ctx->mu);
  rc = ensure_device(ctx);
  if (rc) return rc;
  WsPlan plan;
  const size_t o_ids = plan.add(nids * 4 + 4), o_off = plan.add((nprogs + 1) * 8);
  const OutPlan op(plan, t, dynamic, prios, run);
  rc = dstage_reserve(ctx, plan);
  if (rc) return rc;
  uint32_t* dids = dstage_at<uint32_t>(ctx, o_ids);
  uint64_t* doff = dstage_at<uint64_t>(ctx, o_off);
  SG_HIP(hipMemsetAsync(t->counts, 0, (size_t)t->ncalls * t->ncalls * 8, ctx->stream));
  if ((rc = upload(ctx, dids, call_ids, nids * 4))) return rc;
  if ((rc = upload(ctx, doff, prog_off, (nprogs + 1) * 8))) return rc;
  if ((rc = prio_add(t, dids, doff, nprogs, nids))) return rc;
  return prio_finish_host(t, op, dynamic, prios, run);
}

}  // extern "C"
