// sg_sigset.hip -- map[hash.Sig]bool on the device and hubSync's diff over it:
// the fuzzer's corpusHashes (syz-fuzzer/fuzzer.go:480-484), the manager's
// hubCorpus and its Add / Del (syz-manager/manager.go:1021-1025, :1053-1069),
// minimizeCorpus' sweep (:788-793), loadDB's check (syz-hub/state/state.go:91-101).
//
// A set is a dense store of 20-byte keys (five u32 words each, insertion
// order) and an open-addressing table of u32 indices with a power-of-two number
// of slots, at most half of them used.  Index i < count names store key i;
// count <= i < count + n names key i - count of the batch's scratch area,
// which an earlier launch (the SHA-1 kernels, or a copy) has written: every
// key a kernel of this file compares is complete and visible since a kernel
// boundary.  kEmpty is an index value, never a key value.
//
// No thread ever waits for another (the first-owner idiom of DESIGN 2):
//  * k_ss_insert, a thread per batch key, probes from the key's home slot
//    (its first four bytes, little-endian, masked).  Empty slot: atomicCAS
//    the own index in.  Occupied (or the CAS lost): compare the 20 bytes the
//    slot's index names with the own ones; equal: atomicMin the own index in
//    and stop; unequal: next slot.  A slot's key class never changes once
//    claimed, so a stale read of a slot is either "empty" (the CAS then
//    returns the truth) or an index of the class it will always hold.  Only
//    32-bit words are exchanged inside the launch.
//  * k_ss_flags (a later launch): is_new[k] iff the slot found for key k holds
//    k's own index.  An old key's index is below every batch index, so the
//    atomicMin leaves it in place.
//  * scan_counts over the flags, then k_ss_compact: owner k's key goes to
//    store[count + pos[k]] and its slot takes that final index.  The store
//    stays exactly the set, in insertion order.
//  * sg_sigset_remove (mgr.Corpus.Delete, syz-hub/state/state.go:181-183):
//    k_ss_remove_mark finds each batch key's store index and atomicMin's the
//    batch position into first[index]; a later launch flags the removed keys
//    (first[index] is their own position) and the survivors (first[] still
//    empty); the survivors are gathered into the second half's store and a
//    fresh table is built from it, as sg_hub_sync does: no tombstones.
// A set has two halves of {store, table}, each buffer owning its block and
// capacity (SigHalf, sg_internal.h; DevBuf, sg_buf.h).  The set is `cur`;
// hub_sync, remove and the hub corpus' purge build the new set in `next` and
// swap the halves once, so either half may be the one that grows next.
// Growth rebuilds a larger table from the store by the same insert kernel
// before the batch is inserted (the table's capacity is its slot count, a
// power of two, never rounded); the store grows from 1024 keys by doubling
// with a device copy of its keys (rec_reserve).
// Every index is checked against count + n before it is used as an address,
// and every probe loop is bounded by the number of slots.
#include "sg_internal.h"

#include <algorithm>
#include <cstddef>

// (struct sg_sigset: sg_internal.h; the hub corpus of sg_hub_state.hip keeps its keys in one)
static_assert(offsetof(sg_sigset, count) == 8, "tests/test_prog_hashes.py plants a count in a readable block");

namespace sg {
namespace {

constexpr uint32_t kEmpty = 0xFFFFFFFFu;
constexpr uint32_t kKeyDw = SG_SIG_BYTES / 4;
constexpr uint64_t kMaxKeys = 1ull << 31;
constexpr uint64_t kMinSlots = 64;
constexpr uint32_t kST = 256;

struct View {
  const uint32_t* store;
  uint32_t count;
  const uint64_t* count_dev;  // when set: the count, device-resident (hub_sync's fresh set)
  const uint32_t* scratch;
  uint32_t n;
  uint32_t* table;
  uint32_t mask;  // slots - 1
};

__device__ __forceinline__ uint32_t view_count(const View& v) {
  return v.count_dev ? (uint32_t)min<uint64_t>(*v.count_dev, 0x7FFFFFFFull) : v.count;
}

// the key index i names, or null for an index that names none
__device__ __forceinline__ const uint32_t* key_at(const View& v, uint32_t count, uint32_t i) {
  if (i < count) return v.store + (uint64_t)i * kKeyDw;
  if (i - count < v.n) return v.scratch + (uint64_t)(i - count) * kKeyDw;
  return nullptr;
}

__device__ __forceinline__ bool key_eq(const uint32_t* a, const uint32_t k[kKeyDw]) {
  bool eq = true;
#pragma unroll
  for (uint32_t w = 0; w < kKeyDw; w++) eq = eq && a[w] == k[w];
  return eq;
}

__device__ __forceinline__ void key_load(const uint32_t* p, uint32_t k[kKeyDw]) {
#pragma unroll
  for (uint32_t w = 0; w < kKeyDw; w++) k[w] = p[w];
}

// the slot that holds k's class, or kEmpty; reads only
__device__ __forceinline__ uint32_t find_slot(const View& v, uint32_t count, const uint32_t k[kKeyDw]) {
  uint32_t s = k[0] & v.mask;
  for (uint32_t probe = 0; probe <= v.mask; probe++, s = (s + 1) & v.mask) {
    const uint32_t cur = v.table[s];
    if (cur == kEmpty) return kEmpty;
    const uint32_t* kp = key_at(v, count, cur);
    if (kp && key_eq(kp, k)) return s;
  }
  return kEmpty;
}

// indices [i0, i0 + m) into the table
__global__ __launch_bounds__(kST) void k_ss_insert(View v, uint32_t i0, uint32_t m) {
  const uint64_t t = (uint64_t)blockIdx.x * kST + threadIdx.x;
  if (t >= m) return;
  const uint32_t idx = i0 + (uint32_t)t;
  const uint32_t* own = key_at(v, v.count, idx);
  if (!own) return;
  uint32_t k[kKeyDw];
  key_load(own, k);
  uint32_t s = k[0] & v.mask;
  for (uint32_t probe = 0; probe <= v.mask; probe++, s = (s + 1) & v.mask) {
    uint32_t cur = __hip_atomic_load(&v.table[s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (cur == kEmpty) {
      cur = atomicCAS(&v.table[s], kEmpty, idx);
      if (cur == kEmpty) return;  // claimed
    }
    const uint32_t* kp = key_at(v, v.count, cur);
    if (kp && key_eq(kp, k)) {
      atomicMin(&v.table[s], idx);
      return;
    }
  }
}

// batch key t: its slot, and whether it owns it
__global__ __launch_bounds__(kST) void k_ss_flags(View v, uint32_t* __restrict__ flag, uint32_t* __restrict__ slot,
                                                   uint8_t* __restrict__ is_new) {
  const uint64_t t = (uint64_t)blockIdx.x * kST + threadIdx.x;
  if (t >= v.n) return;
  uint32_t k[kKeyDw];
  key_load(v.scratch + t * kKeyDw, k);
  const uint32_t s = find_slot(v, v.count, k);
  const uint32_t f = s != kEmpty && v.table[s] == v.count + (uint32_t)t;
  flag[t] = f;
  slot[t] = s;
  if (is_new) is_new[t] = (uint8_t)f;
}

// owners onto the store's tail, their slots to the final indices
__global__ __launch_bounds__(kST) void k_ss_compact(View v, const uint32_t* __restrict__ flag,
                                                     const uint32_t* __restrict__ slot, const uint64_t* __restrict__ pos,
                                                     uint32_t* __restrict__ store, uint64_t store_cap) {
  const uint64_t t = (uint64_t)blockIdx.x * kST + threadIdx.x;
  if (t >= v.n || !flag[t]) return;
  const uint64_t dst = (uint64_t)v.count + pos[t];
  const uint32_t s = slot[t];
  if (dst >= store_cap || s > v.mask) return;
#pragma unroll
  for (uint32_t w = 0; w < kKeyDw; w++) store[dst * kKeyDw + w] = v.scratch[t * kKeyDw + w];
  v.table[s] = (uint32_t)dst;
}

// out[t] = 1 iff key t of `keys` is in the set v (want == 1) or is not (want == 0); with `only`, keys whose
// only[t] is zero give 0
__global__ __launch_bounds__(kST) void k_ss_lookup(View v, const uint32_t* __restrict__ keys, uint64_t n,
                                                    const uint32_t* __restrict__ only, uint32_t want,
                                                    uint8_t* __restrict__ out8, uint32_t* __restrict__ out32) {
  const uint64_t t = (uint64_t)blockIdx.x * kST + threadIdx.x;
  if (t >= n) return;
  uint32_t r = 0;
  if (!only || only[t]) {
    uint32_t k[kKeyDw];
    key_load(keys + t * kKeyDw, k);
    const uint32_t found = find_slot(v, view_count(v), k) != kEmpty;
    r = found == want;
  }
  if (out8) out8[t] = (uint8_t)r;
  if (out32) out32[t] = r;
}

// keys with flag set, in order, to out[pos[t]]
__global__ __launch_bounds__(kST) void k_ss_gather(const uint32_t* __restrict__ keys, uint64_t n,
                                                    const uint32_t* __restrict__ flag, const uint64_t* __restrict__ pos,
                                                    uint32_t* __restrict__ out, uint64_t cap) {
  const uint64_t t = (uint64_t)blockIdx.x * kST + threadIdx.x;
  if (t >= n || !flag[t] || pos[t] >= cap) return;
#pragma unroll
  for (uint32_t w = 0; w < kKeyDw; w++) out[pos[t] * kKeyDw + w] = keys[t * kKeyDw + w];
}

// acc[t] |= key t of `keys` is in the set v (one launch per set of the hub corpus' purge)
__global__ __launch_bounds__(kST) void k_ss_lookup_or(View v, const uint32_t* __restrict__ keys, uint64_t n,
                                                       uint32_t* __restrict__ acc) {
  const uint64_t t = (uint64_t)blockIdx.x * kST + threadIdx.x;
  if (t >= n || acc[t]) return;
  uint32_t k[kKeyDw];
  key_load(keys + t * kKeyDw, k);
  if (find_slot(v, view_count(v), k) != kEmpty) acc[t] = 1;
}

// remove, first launch: batch key t names store index hit[t] (kEmpty: not in the set); first[i] becomes the
// least t that names i.  first[] starts all kEmpty, so afterwards first[i] == kEmpty marks a survivor.
__global__ __launch_bounds__(kST) void k_ss_remove_mark(View v, const uint32_t* __restrict__ keys, uint64_t n,
                                                         uint32_t* __restrict__ hit, uint32_t* __restrict__ first) {
  const uint64_t t = (uint64_t)blockIdx.x * kST + threadIdx.x;
  if (t >= n) return;
  uint32_t k[kKeyDw];
  key_load(keys + t * kKeyDw, k);
  const uint32_t s = find_slot(v, v.count, k);
  uint32_t i = s == kEmpty ? kEmpty : v.table[s];
  if (i >= v.count) i = kEmpty;
  hit[t] = i;
  if (i != kEmpty) atomicMin(&first[i], (uint32_t)t);
}

// remove, second launch: removed[t] and, for the store, keep[i]
__global__ __launch_bounds__(kST) void k_ss_remove_flags(const uint32_t* __restrict__ hit, uint64_t n,
                                                          const uint32_t* __restrict__ first, uint64_t count,
                                                          uint8_t* __restrict__ removed, uint32_t* __restrict__ keep) {
  const uint64_t t = (uint64_t)blockIdx.x * kST + threadIdx.x;
  if (t < n) removed[t] = hit[t] < count && first[hit[t]] == (uint32_t)t;
  if (t < count) keep[t] = first[t] == kEmpty;
}

uint64_t slots_for(uint64_t keys) {
  uint64_t s = kMinSlots;
  while (s < 2 * keys) s *= 2;
  return s;
}

int launch_insert(sg_ctx* ctx, const View& v, uint32_t i0, uint32_t m) {
  if (!m) return SG_OK;
  ScopedTimer tm(ctx, "sigset_insert");
  hipLaunchKernelGGL(k_ss_insert, dim3(div_up(m, kST)), dim3(kST), 0, ctx->stream, v, i0, m);
  SG_HIP(hipGetLastError());
  return SG_OK;
}

// the set of h's first `count` keys, for a batch of n scratch keys at `scratch`
View view_of(const SigHalf& h, uint64_t count, const uint32_t* scratch = nullptr, uint64_t n = 0) {
  return View{h.keys(), (uint32_t)count, nullptr, scratch, (uint32_t)n, h.table.p, h.mask()};
}

// a table of at least `slots` slots (exactly `slots` when it has to grow), all empty
int table_fresh(sg_ctx* ctx, DevBuf<uint32_t>& table, uint64_t slots) {
  const int rc = table.grow_drop(slots, ctx->stream);
  if (rc) return rc;
  SG_HIP(hipMemsetAsync(table.p, 0xFF, table.cap * 4, ctx->stream));
  return SG_OK;
}

// a half for a fresh set of up to `keys` keys: room in the store (nothing kept), an empty table
int half_fresh(sg_ctx* ctx, SigHalf& h, uint64_t keys) {
  const int rc = rec_reserve(ctx, h.store, std::max<uint64_t>(keys, 1), 0);
  return rc ? rc : table_fresh(ctx, h.table, slots_for(keys));
}

// the table sized for count + n keys: a larger one is rebuilt from the store
int grow_for(sg_sigset* s, uint64_t n) {
  sg_ctx* ctx = s->ctx;
  SigHalf& h = s->cur;
  int rc = rec_reserve(ctx, h.store, s->count + n, s->count);
  if (rc) return rc;
  const uint64_t need = slots_for(s->count + n);
  if (need <= h.table.cap) return SG_OK;
  DevBuf<uint32_t> nt;  // (freed here unless it is swapped in)
  if ((rc = table_fresh(ctx, nt, need))) return rc;
  const View v{h.keys(), (uint32_t)s->count, nullptr, nullptr, 0, nt.p, (uint32_t)(nt.cap - 1)};
  rc = launch_insert(ctx, v, 0, (uint32_t)s->count);
  const hipError_t e = hipStreamSynchronize(ctx->stream);
  if (rc || e != hipSuccess) return rc ? rc : hip_fail(e, "grow_for");
  h.table.swap(nt);
  return nt.release();
}

// workspace of an add of n scratch keys: flags, slots, positions, the scan
struct AddPlan {
  size_t o_flag, o_slot, o_pos, o_scan, total;
  AddPlan(size_t base, uint64_t n) {
    o_flag = base;
    o_slot = o_flag + align256(n * 4);
    o_pos = o_slot + align256(n * 4);
    o_scan = o_pos + align256((n + 1) * 8);
    total = o_scan + scan_ws_bytes(n);
  }
};

// insert, flags, scan, compact of n scratch keys (device) into the half h holding `count`; is_new nullable.
// The new count is count + pos[n] (device, at ws o_pos + 8 * n).
int add_scratch(sg_ctx* ctx, const SigHalf& h, uint64_t count, const uint32_t* d_keys, uint64_t n, const AddPlan& ap,
                uint8_t* d_is_new) {
  const View v = view_of(h, count, d_keys, n);
  uint32_t* flag = (uint32_t*)ws_at(ctx, ap.o_flag);
  uint32_t* slot = (uint32_t*)ws_at(ctx, ap.o_slot);
  uint64_t* pos = (uint64_t*)ws_at(ctx, ap.o_pos);
  int rc = launch_insert(ctx, v, (uint32_t)count, (uint32_t)n);
  if (rc) return rc;
  if (n) {
    ScopedTimer tm(ctx, "sigset_flags");
    hipLaunchKernelGGL(k_ss_flags, dim3(div_up(n, kST)), dim3(kST), 0, ctx->stream, v, flag, slot, d_is_new);
  }
  SG_HIP(hipGetLastError());
  if ((rc = scan_counts(ctx, flag, pos, n, ap.o_scan))) return rc;
  if (n) {
    ScopedTimer tm(ctx, "sigset_compact");
    hipLaunchKernelGGL(k_ss_compact, dim3(div_up(n, kST)), dim3(kST), 0, ctx->stream, v, (const uint32_t*)flag,
                       (const uint32_t*)slot, (const uint64_t*)pos, h.keys(), (uint64_t)h.store.cap);
  }
  SG_HIP(hipGetLastError());
  return SG_OK;
}

int sigs_ok(const char* fn, const sg_sigset* s, const uint8_t* sigs, size_t n, const uint8_t* out) {
  if (!s || (n && (!sigs || !out))) {
    set_error("%s: invalid argument", fn);
    return SG_EINVAL;
  }
  if ((uint64_t)n >= kMaxKeys) {
    set_error("%s: %llu identities (the limit is 2^31 - 1)", fn, (unsigned long long)n);
    return SG_EINVAL;
  }
  return SG_OK;
}

int room_ok(const char* fn, const sg_sigset* s, uint64_t n) {
  if (s->count + n >= kMaxKeys) {
    set_error("%s: the set would reach 2^31 identities", fn);
    return SG_EINVAL;
  }
  return SG_OK;
}

// sg_sigset_add_new / _add_progs after the checks; keys: host identities, or null to hash the programs
int add_common(sg_sigset* s, const uint8_t* keys, const uint8_t* bytes, const uint64_t* off, size_t n, uint8_t* sigs,
               uint8_t* is_new) {
  sg_ctx* ctx = s->ctx;
  std::lock_guard<std::mutex> g(ctx->mu);
  int rc = ensure_device(ctx);
  if (rc) return rc;
  if (n == 0) return SG_OK;
  const uint64_t nbytes = keys ? 0 : off[n];
  WsPlan plan;
  const size_t o_keys = plan.add(n * SG_SIG_BYTES), o_new = plan.add(n), o_bytes = plan.add(nbytes + 4),
               o_off = plan.add((n + 1) * 8);
  if ((rc = dstage_reserve(ctx, plan))) return rc;
  const size_t hash_ws = keys ? 0 : align256(prog_hashes_ws(n));
  const AddPlan ap(hash_ws, n);
  if ((rc = ws_reserve(ctx, ap.total))) return rc;
  if ((rc = grow_for(s, n))) return rc;
  uint32_t* dkeys = dstage_at<uint32_t>(ctx, o_keys);
  uint8_t* dnew = dstage_at<uint8_t>(ctx, o_new);
  if (keys) {
    if ((rc = upload(ctx, dkeys, keys, n * SG_SIG_BYTES))) return rc;
  } else {
    uint8_t* dbytes = dstage_at<uint8_t>(ctx, o_bytes);
    uint64_t* doff = dstage_at<uint64_t>(ctx, o_off);
    if ((rc = upload(ctx, dbytes, bytes, nbytes))) return rc;
    if ((rc = upload(ctx, doff, off, (n + 1) * 8))) return rc;
    if ((rc = prog_hashes(ctx, dbytes, doff, n, nbytes, (uint8_t*)dkeys, 0))) return rc;
    if (sigs) SG_HIP(hipMemcpyAsync(sigs, dkeys, n * SG_SIG_BYTES, hipMemcpyDeviceToHost, ctx->stream));
  }
  if ((rc = add_scratch(ctx, s->cur, s->count, dkeys, n, ap, dnew))) return rc;
  uint64_t added = 0;
  SG_HIP(hipMemcpyAsync(is_new, dnew, n, hipMemcpyDeviceToHost, ctx->stream));
  SG_HIP(hipMemcpyAsync(&added, (uint64_t*)ws_at(ctx, ap.o_pos) + n, 8, hipMemcpyDeviceToHost, ctx->stream));
  SG_HIP(hipStreamSynchronize(ctx->stream));
  s->count += std::min<uint64_t>(added, n);
  return SG_OK;
}

}  // namespace

// ---- what sg_hub_state.hip takes from this file (sg_internal.h) ----
int sigset_new(sg_ctx* ctx, uint64_t hint, sg_sigset** out) {
  sg_sigset* s = new sg_sigset();
  s->ctx = ctx;
  const int rc = grow_for(s, std::max<uint64_t>(hint, 1));
  if (rc) {
    delete s;
    return rc;
  }
  *out = s;
  return SG_OK;
}

void sigset_delete(sg_sigset* s) { delete s; }

size_t sigset_add_ws(uint64_t n) { return AddPlan(0, n).total; }

int sigset_add_dev(sg_sigset* s, const uint32_t* d_keys, uint64_t n, uint8_t* d_is_new, size_t ws_base, size_t* o_pos) {
  sg_ctx* ctx = s->ctx;
  const AddPlan ap(ws_base, n);
  *o_pos = ap.o_pos;
  int rc = room_ok("sigset_add_dev", s, n);
  if (rc) return rc;
  if ((rc = grow_for(s, n))) return rc;
  if ((rc = add_scratch(ctx, s->cur, s->count, d_keys, n, ap, d_is_new))) return rc;
  uint64_t added = 0;
  SG_HIP(hipMemcpyAsync(&added, (uint64_t*)ws_at(ctx, ap.o_pos) + n, 8, hipMemcpyDeviceToHost, ctx->stream));
  SG_HIP(hipStreamSynchronize(ctx->stream));
  s->count += std::min<uint64_t>(added, n);
  return SG_OK;
}

int sigset_lookup_dev(sg_sigset* s, const uint32_t* d_keys, uint64_t n, uint32_t want, uint32_t* out32) {
  if (!n) return SG_OK;
  sg_ctx* ctx = s->ctx;
  const View v = view_of(s->cur, s->count);
  ScopedTimer tm(ctx, "sigset_lookup");
  hipLaunchKernelGGL(k_ss_lookup, dim3(div_up(n, kST)), dim3(kST), 0, ctx->stream, v, d_keys, n, (const uint32_t*)nullptr,
                     want, (uint8_t*)nullptr, out32);
  SG_HIP(hipGetLastError());
  return SG_OK;
}

int sigset_lookup_or_dev(sg_sigset* s, const uint32_t* d_keys, uint64_t n, uint32_t* acc) {
  if (!n) return SG_OK;
  sg_ctx* ctx = s->ctx;
  const View v = view_of(s->cur, s->count);
  ScopedTimer tm(ctx, "sigset_lookup");
  hipLaunchKernelGGL(k_ss_lookup_or, dim3(div_up(n, kST)), dim3(kST), 0, ctx->stream, v, d_keys, n, acc);
  SG_HIP(hipGetLastError());
  return SG_OK;
}

int sigset_gather_dev(sg_ctx* ctx, const uint32_t* d_keys, uint64_t n, const uint32_t* d_flag, const uint64_t* d_pos,
                      uint32_t* d_out, uint64_t cap) {
  if (!n) return SG_OK;
  ScopedTimer tm(ctx, "sigset_gather");
  hipLaunchKernelGGL(k_ss_gather, dim3(div_up(n, kST)), dim3(kST), 0, ctx->stream, d_keys, n, d_flag, d_pos, d_out, cap);
  SG_HIP(hipGetLastError());
  return SG_OK;
}

int sigset_rebuild_dev(sg_sigset* s, const uint32_t* d_keep, const uint64_t* d_pos, uint64_t newcount) {
  sg_ctx* ctx = s->ctx;
  const uint64_t c = s->count;
  if (newcount > c) newcount = c;
  int rc = half_fresh(ctx, s->next, newcount);
  if (rc) return rc;
  if ((rc = sigset_gather_dev(ctx, s->cur.keys(), c, d_keep, d_pos, s->next.keys(), newcount))) return rc;
  if ((rc = launch_insert(ctx, view_of(s->next, newcount), 0, (uint32_t)newcount))) return rc;
  SG_HIP(hipStreamSynchronize(ctx->stream));
  s->cur.swap(s->next);
  s->count = newcount;
  return SG_OK;
}

}  // namespace sg

using namespace sg;

extern "C" {

int sg_sigset_create(sg_ctx* ctx, uint64_t capacity_hint, sg_sigset** out) {
  const char* fn = "sg_sigset_create";
  if (!ctx || !out) {
    set_error("%s: invalid argument", fn);
    return SG_EINVAL;
  }
  *out = nullptr;
  if (capacity_hint >= kMaxKeys) {
    set_error("%s: a hint of %llu identities (the limit is 2^31 - 1)", fn, (unsigned long long)capacity_hint);
    return SG_EINVAL;
  }
  std::lock_guard<std::mutex> g(ctx->mu);
  const int rc = ensure_device(ctx);
  return rc ? rc : sigset_new(ctx, capacity_hint, out);
}

void sg_sigset_destroy(sg_sigset* s) {
  if (!s) return;
  {
    std::lock_guard<std::mutex> g(s->ctx->mu);
    hipSetDevice(s->ctx->device);
    hipStreamSynchronize(s->ctx->stream);
  }
  delete s;
}

int sg_sigset_clear(sg_sigset* s) {
  if (!s) {
    set_error("sg_sigset_clear: invalid argument");
    return SG_EINVAL;
  }
  sg_ctx* ctx = s->ctx;
  std::lock_guard<std::mutex> g(ctx->mu);
  int rc = ensure_device(ctx);
  if (rc) return rc;
  SG_HIP(hipMemsetAsync(s->cur.table.p, 0xFF, s->cur.table.cap * 4, ctx->stream));
  s->count = 0;
  return SG_OK;
}

int sg_sigset_count(sg_sigset* s, uint64_t* out) {
  if (!s || !out) {
    set_error("sg_sigset_count: invalid argument");
    return SG_EINVAL;
  }
  std::lock_guard<std::mutex> g(s->ctx->mu);
  *out = s->count;
  return SG_OK;
}

int sg_sigset_export(sg_sigset* s, uint8_t* sigs, size_t cap, size_t* n) {
  if (!s || !n || (cap && !sigs)) {
    set_error("sg_sigset_export: invalid argument");
    return SG_EINVAL;
  }
  sg_ctx* ctx = s->ctx;
  std::lock_guard<std::mutex> g(ctx->mu);
  int rc = ensure_device(ctx);
  if (rc) return rc;
  *n = s->count;
  if (s->count && s->count <= cap) {
    SG_HIP(hipMemcpyAsync(sigs, s->cur.keys(), s->count * SG_SIG_BYTES, hipMemcpyDeviceToHost, ctx->stream));
    SG_HIP(hipStreamSynchronize(ctx->stream));
  }
  return SG_OK;
}

int sg_sigset_contains(sg_sigset* s, const uint8_t* sigs, size_t n, uint8_t* present) {
  int rc = sigs_ok("sg_sigset_contains", s, sigs, n, present);
  if (rc) return rc;
  sg_ctx* ctx = s->ctx;
  std::lock_guard<std::mutex> g(ctx->mu);
  rc = ensure_device(ctx);
  if (rc) return rc;
  if (n == 0) return SG_OK;
  WsPlan plan;
  const size_t o_keys = plan.add(n * SG_SIG_BYTES), o_out = plan.add(n);
  if ((rc = dstage_reserve(ctx, plan))) return rc;
  uint32_t* dkeys = dstage_at<uint32_t>(ctx, o_keys);
  uint8_t* dout = dstage_at<uint8_t>(ctx, o_out);
  if ((rc = upload(ctx, dkeys, sigs, n * SG_SIG_BYTES))) return rc;
  const View v = view_of(s->cur, s->count);
  {
    ScopedTimer tm(ctx, "sigset_lookup");
    hipLaunchKernelGGL(k_ss_lookup, dim3(div_up(n, kST)), dim3(kST), 0, ctx->stream, v, (const uint32_t*)dkeys, (uint64_t)n,
                       (const uint32_t*)nullptr, 1u, dout, (uint32_t*)nullptr);
  }
  SG_HIP(hipGetLastError());
  SG_HIP(hipMemcpyAsync(present, dout, n, hipMemcpyDeviceToHost, ctx->stream));
  SG_HIP(hipStreamSynchronize(ctx->stream));
  return SG_OK;
}

int sg_sigset_add_new(sg_sigset* s, const uint8_t* sigs, size_t n, uint8_t* is_new) {
  const char* fn = "sg_sigset_add_new";
  int rc = sigs_ok(fn, s, sigs, n, is_new);
  if (rc) return rc;
  if ((rc = room_ok(fn, s, n))) return rc;
  return add_common(s, sigs, nullptr, nullptr, n, nullptr, is_new);
}

int sg_sigset_add_progs(sg_sigset* s, const uint8_t* bytes, const uint64_t* off, size_t nprogs, uint8_t* sigs,
                        uint8_t* is_new) {
  const char* fn = "sg_sigset_add_progs";
  if (!s || (nprogs && !is_new)) {
    set_error("%s: invalid argument", fn);
    return SG_EINVAL;
  }
  int rc = prog_texts_ok(fn, bytes, off, nprogs);
  if (rc) return rc;
  if ((uint64_t)nprogs >= kMaxKeys) {
    set_error("%s: %llu programs (the limit is 2^31 - 1)", fn, (unsigned long long)nprogs);
    return SG_EINVAL;
  }
  if ((rc = room_ok(fn, s, nprogs))) return rc;
  return add_common(s, nullptr, bytes, off, nprogs, sigs, is_new);
}

int sg_hub_sync(sg_sigset* hub, const uint8_t* bytes, const uint64_t* off, size_t nprogs, uint8_t* sigs, uint8_t* add,
                uint8_t* del_sigs, size_t del_cap, size_t* ndel) {
  const char* fn = "sg_hub_sync";
  if (!hub || !ndel || (nprogs && !add) || (del_cap && !del_sigs)) {
    set_error("%s: invalid argument", fn);
    return SG_EINVAL;
  }
  int rc = prog_texts_ok(fn, bytes, off, nprogs);
  if (rc) return rc;
  if ((uint64_t)nprogs >= kMaxKeys) {
    set_error("%s: %llu programs (the limit is 2^31 - 1)", fn, (unsigned long long)nprogs);
    return SG_EINVAL;
  }
  if ((uint64_t)del_cap < hub->count) {  // (read before the lock: a set is one caller's at a time, as the map is under mgr.mu)
    set_error("%s: del_cap %llu below the set's %llu identities", fn, (unsigned long long)del_cap,
              (unsigned long long)hub->count);
    return SG_EINVAL;
  }
  sg_ctx* ctx = hub->ctx;
  std::lock_guard<std::mutex> g(ctx->mu);
  rc = ensure_device(ctx);
  if (rc) return rc;
  const uint64_t n = nprogs, c = hub->count, nbytes = off[nprogs];
  // staging: the corpus, its identities, add, the deleted identities; workspace: the hashes', the add's, the del's
  WsPlan plan;
  const size_t o_keys = plan.add(n * SG_SIG_BYTES + 4), o_add = plan.add(n + 1), o_bytes = plan.add(nbytes + 4),
               o_off = plan.add((n + 1) * 8), o_del = plan.add(c * SG_SIG_BYTES + 4);
  if ((rc = dstage_reserve(ctx, plan))) return rc;
  const AddPlan ap(align256(prog_hashes_ws(n)), n);
  const size_t o_dflag = ap.total, o_dpos = o_dflag + align256(c * 4 + 4), o_dscan = o_dpos + align256((c + 1) * 8);
  if ((rc = ws_reserve(ctx, o_dscan + scan_ws_bytes(c)))) return rc;
  if ((rc = half_fresh(ctx, hub->next, n))) return rc;
  uint32_t* dkeys = dstage_at<uint32_t>(ctx, o_keys);
  uint8_t* dadd = dstage_at<uint8_t>(ctx, o_add);
  uint32_t* ddel = dstage_at<uint32_t>(ctx, o_del);
  if (n) {
    uint8_t* dbytes = dstage_at<uint8_t>(ctx, o_bytes);
    uint64_t* doff = dstage_at<uint64_t>(ctx, o_off);
    if ((rc = upload(ctx, dbytes, bytes, nbytes))) return rc;
    if ((rc = upload(ctx, doff, off, (n + 1) * 8))) return rc;
    if ((rc = prog_hashes(ctx, dbytes, doff, n, nbytes, (uint8_t*)dkeys, 0))) return rc;
    if (sigs) SG_HIP(hipMemcpyAsync(sigs, dkeys, n * SG_SIG_BYTES, hipMemcpyDeviceToHost, ctx->stream));
  }
  // the fresh set: the corpus' identities in first-occurrence order
  if ((rc = add_scratch(ctx, hub->next, 0, dkeys, n, ap, nullptr))) return rc;
  const uint32_t* flag = (const uint32_t*)ws_at(ctx, ap.o_flag);
  const uint64_t* count2 = (const uint64_t*)ws_at(ctx, ap.o_pos) + n;
  const View vold = view_of(hub->cur, c);
  View vnew = view_of(hub->next, 0);
  vnew.count_dev = count2;
  uint32_t* dflag = (uint32_t*)ws_at(ctx, o_dflag);
  uint64_t* dpos = (uint64_t*)ws_at(ctx, o_dpos);
  {
    ScopedTimer tm(ctx, "hub_sync_diff");
    // Add: the owners the old set does not hold
    if (n)
      hipLaunchKernelGGL(k_ss_lookup, dim3(div_up(n, kST)), dim3(kST), 0, ctx->stream, vold, (const uint32_t*)dkeys, n, flag,
                         0u, dadd, (uint32_t*)nullptr);
    // Del: the old identities the fresh set does not hold
    if (c)
      hipLaunchKernelGGL(k_ss_lookup, dim3(div_up(c, kST)), dim3(kST), 0, ctx->stream, vnew,
                         (const uint32_t*)hub->cur.keys(), c, (const uint32_t*)nullptr, 0u, (uint8_t*)nullptr, dflag);
  }
  SG_HIP(hipGetLastError());
  if ((rc = scan_counts(ctx, dflag, dpos, c, o_dscan))) return rc;
  if (c) {
    ScopedTimer tm(ctx, "hub_sync_gather");
    hipLaunchKernelGGL(k_ss_gather, dim3(div_up(c, kST)), dim3(kST), 0, ctx->stream, (const uint32_t*)hub->cur.keys(), c,
                       (const uint32_t*)dflag, (const uint64_t*)dpos, ddel, c);
  }
  SG_HIP(hipGetLastError());
  uint64_t got[2] = {0, 0};  // the fresh set's count, the deleted identities
  if (n) SG_HIP(hipMemcpyAsync(add, dadd, n, hipMemcpyDeviceToHost, ctx->stream));
  SG_HIP(hipMemcpyAsync(&got[0], count2, 8, hipMemcpyDeviceToHost, ctx->stream));
  SG_HIP(hipMemcpyAsync(&got[1], dpos + c, 8, hipMemcpyDeviceToHost, ctx->stream));
  SG_HIP(hipStreamSynchronize(ctx->stream));
  const uint64_t nd = std::min(got[1], c);
  if (nd) {
    SG_HIP(hipMemcpyAsync(del_sigs, ddel, nd * SG_SIG_BYTES, hipMemcpyDeviceToHost, ctx->stream));
    SG_HIP(hipStreamSynchronize(ctx->stream));
  }
  *ndel = nd;
  hub->cur.swap(hub->next);
  hub->count = std::min(got[0], n);
  return SG_OK;
}

int sg_sigset_remove(sg_sigset* s, const uint8_t* sigs, size_t n, uint8_t* removed) {
  int rc = sigs_ok("sg_sigset_remove", s, sigs, n, removed);
  if (rc) return rc;
  sg_ctx* ctx = s->ctx;
  std::lock_guard<std::mutex> g(ctx->mu);
  rc = ensure_device(ctx);
  if (rc) return rc;
  if (n == 0) return SG_OK;
  const uint64_t c = s->count;
  WsPlan plan;
  const size_t o_keys = plan.add(n * SG_SIG_BYTES), o_rem = plan.add(n);
  if ((rc = dstage_reserve(ctx, plan))) return rc;
  WsPlan wp;
  const size_t o_hit = wp.add(n * 4), o_first = wp.add(c * 4 + 4), o_keep = wp.add(c * 4 + 4), o_pos = wp.add((c + 1) * 8),
               o_scan = wp.add(scan_ws_bytes(c));
  if ((rc = ws_reserve(ctx, wp))) return rc;
  uint32_t* dkeys = dstage_at<uint32_t>(ctx, o_keys);
  uint8_t* drem = dstage_at<uint8_t>(ctx, o_rem);
  uint32_t* hit = (uint32_t*)ws_at(ctx, o_hit);
  uint32_t* first = (uint32_t*)ws_at(ctx, o_first);
  uint32_t* keep = (uint32_t*)ws_at(ctx, o_keep);
  uint64_t* pos = (uint64_t*)ws_at(ctx, o_pos);
  if ((rc = upload(ctx, dkeys, sigs, n * SG_SIG_BYTES))) return rc;
  SG_HIP(hipMemsetAsync(first, 0xFF, c * 4 + 4, ctx->stream));
  const View v = view_of(s->cur, c);
  {
    ScopedTimer tm(ctx, "sigset_remove");
    hipLaunchKernelGGL(k_ss_remove_mark, dim3(div_up(n, kST)), dim3(kST), 0, ctx->stream, v, (const uint32_t*)dkeys,
                       (uint64_t)n, hit, first);
    hipLaunchKernelGGL(k_ss_remove_flags, dim3(div_up(std::max<uint64_t>(n, c), kST)), dim3(kST), 0, ctx->stream,
                       (const uint32_t*)hit, (uint64_t)n, (const uint32_t*)first, c, drem, keep);
  }
  SG_HIP(hipGetLastError());
  if ((rc = scan_counts(ctx, keep, pos, c, o_scan))) return rc;
  uint64_t left = 0;
  SG_HIP(hipMemcpyAsync(removed, drem, n, hipMemcpyDeviceToHost, ctx->stream));
  SG_HIP(hipMemcpyAsync(&left, pos + c, 8, hipMemcpyDeviceToHost, ctx->stream));
  SG_HIP(hipStreamSynchronize(ctx->stream));
  if (left >= c) return SG_OK;  // nothing was in the set
  return sigset_rebuild_dev(s, keep, pos, left);
}

}  // extern "C"
