// sg_ctx.hip -- the context of libsyzsig.so: errors, the grow-only buffers'
// reserves, uploads and downloads, the first-owner keys, kernel timing, and the
// lifecycle, marker, option and counter entry points.
#include "sg_internal.h"

#include <cstring>
#include <memory>

namespace sg {

static thread_local std::string g_err;

void set_error(const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  g_err = buf;
}

int hip_fail(hipError_t e, const char* what) {
  set_error("HIP error %d (%s) in %s", (int)e, hipGetErrorString(e), what);
  if (e == hipErrorOutOfMemory) return SG_ENOMEM;
  if (e == hipErrorNoDevice || e == hipErrorInvalidDevice || e == hipErrorNoBinaryForGpu) return SG_ENODEV;
  return SG_EHIP;
}

int ensure_device(sg_ctx* ctx) {
  hipError_t e = hipSetDevice(ctx->device);
  if (e != hipSuccess) return hip_fail(e, "hipSetDevice");
  // hipGetLastError after our launches must see only our errors.  The one
  // known stale code left on this thread by another library (torch's
  // "invalid device ordinal" after spawning multiprocess workers) is dropped
  // silently; any other pending error belongs to the caller's own HIP work,
  // so it is reported on stderr before it is cleared, not hidden.
  const hipError_t stale = hipPeekAtLastError();
  if (stale != hipSuccess) {
    if (stale != hipErrorInvalidDevice)
      fprintf(stderr, "libsyzsig: clearing a pending HIP error of the calling thread: %d (%s)\n", (int)stale,
              hipGetErrorString(stale));
    (void)hipGetLastError();
  }
  return SG_OK;
}

int ws_reserve(sg_ctx* ctx, size_t bytes) {
  return ctx->ws.grow_drop(grow_cap(ctx->ws.cap, bytes, 64u << 20), ctx->stream);
}

// (the staging buffers also wait for the host pipeline's DMAs on copy_stream)
int pin_reserve(sg_ctx* ctx, size_t bytes) {
  return ctx->pin.grow_drop(grow_cap(ctx->pin.cap, bytes, 16u << 20), ctx->stream, ctx->copy_stream);
}

int dstage_reserve(sg_ctx* ctx, size_t bytes) {
  return ctx->dstage.grow_drop(grow_cap(ctx->dstage.cap, bytes, 16u << 20), ctx->stream, ctx->copy_stream);
}

int slice_off_reserve(sg_ctx* ctx, size_t n) { return ctx->slice_off.grow_drop(n, ctx->stream); }

static int plan_ok(const WsPlan& plan) {
  if (!plan.overflow) return SG_OK;
  set_error("a buffer plan of more than %d regions", WsPlan::kMaxRegions);
  return SG_EINVAL;
}
int ws_reserve(sg_ctx* ctx, const WsPlan& plan) { return plan_ok(plan) ? SG_EINVAL : ws_reserve(ctx, plan.total); }
int dstage_reserve(sg_ctx* ctx, const WsPlan& plan) {
  return plan_ok(plan) ? SG_EINVAL : dstage_reserve(ctx, plan.total);
}

int upload(sg_ctx* ctx, void* d_dst, const void* h_src, size_t bytes) {
  if (bytes) SG_HIP(hipMemcpyAsync(d_dst, h_src, bytes, hipMemcpyHostToDevice, ctx->stream));
  return SG_OK;
}

int csr_download(sg_ctx* ctx, uint64_t* h_off, const uint64_t* d_off, uint64_t n, void* h_vals, const void* d_vals,
                 size_t elem, uint64_t cap) {
  SG_HIP(hipMemcpyAsync(h_off, d_off, (n + 1) * 8, hipMemcpyDeviceToHost, ctx->stream));
  SG_HIP(hipStreamSynchronize(ctx->stream));
  if (h_off[n] && h_off[n] <= cap)
    SG_HIP(hipMemcpyAsync(h_vals, d_vals, h_off[n] * elem, hipMemcpyDeviceToHost, ctx->stream));
  SG_HIP(hipStreamSynchronize(ctx->stream));
  return SG_OK;
}

int owner_keys(sg_ctx* ctx, uint64_t nkeys, uint32_t* key_lo) {
  if (nkeys > ctx->owner_key_space) {
    set_error("batch of %llu keys exceeds the first-owner key space (%llu)", (unsigned long long)nkeys,
              (unsigned long long)ctx->owner_key_space);
    return SG_EINVAL;
  }
  if (!ctx->owner.p) {  // (adopted once its fill is queued)
    DevBuf<uint32_t> nb;
    const int rc = nb.grow_drop(kOwnerEntries, nullptr);
    if (rc) return rc;
    SG_HIP(hipMemsetAsync(nb.p, 0xFF, kOwnerEntries * sizeof(uint32_t), ctx->stream));
    ctx->owner.swap(nb);
    ctx->owner_floor = ctx->owner_key_space;
  }
  if (ctx->owner_floor < nkeys) {
    // Key space exhausted (after ~4G keys): start a fresh generation.
    SG_HIP(hipMemsetAsync(ctx->owner.p, 0xFF, kOwnerEntries * sizeof(uint32_t), ctx->stream));
    ctx->owner_floor = ctx->owner_key_space;
    ctx->owner_resets++;
  }
  ctx->owner_floor -= nkeys;
  *key_lo = (uint32_t)ctx->owner_floor;
  return SG_OK;
}

// ---- kernel timing ---------------------------------------------------------
void timer_begin(sg_ctx* ctx, const char* name, int* slot) {
  KernelTimer& t = ctx->timer;
  *slot = -1;
  if (!t.enabled) return;
  auto it = t.ids.find(name);
  int id;
  if (it == t.ids.end()) {
    id = (int)t.names.size();
    t.ids[name] = id;
    t.names.push_back(name);
    t.ms.push_back(0);
    t.count.push_back(0);
  } else {
    id = it->second;
  }
  while (t.pool.size() < 2) {
    t.events.emplace_back();
    if (t.events.back().create(hipEventDefault)) return;
    t.pool.push_back(t.events.back());
  }
  const hipEvent_t a = t.pool.back();
  t.pool.pop_back();
  const hipEvent_t b = t.pool.back();
  t.pool.pop_back();
  hipEventRecord(a, ctx->stream);
  t.pending.push_back({id, a, b});
  *slot = (int)t.pending.size() - 1;
}

void timer_end(sg_ctx* ctx, int slot) {
  if (slot < 0) return;
  hipEventRecord(ctx->timer.pending[slot].b, ctx->stream);
}

static void timer_collect(sg_ctx* ctx) {
  KernelTimer& t = ctx->timer;
  for (auto& r : t.pending) {
    hipEventSynchronize(r.b);
    float ms = 0;
    hipEventElapsedTime(&ms, r.a, r.b);
    t.ms[r.id] += ms;
    t.count[r.id] += 1;
    t.pool.push_back(r.a);
    t.pool.push_back(r.b);
  }
  t.pending.clear();
}

}  // namespace sg

using namespace sg;

// ---- C-ABI -------------------------------------------------------------------
extern "C" {

const char* sg_version(void) { return "syzsig 0.1 gfx950"; }
const char* sg_last_error(void) { return g_err.c_str(); }

int sg_ctx_create(int device, sg_ctx** out) {
  if (!out) {
    set_error("sg_ctx_create: out is NULL");
    return SG_EINVAL;
  }
  *out = nullptr;
  int ndev = 0;
  hipError_t e = hipGetDeviceCount(&ndev);
  if (e != hipSuccess || ndev == 0) {
    set_error("no HIP device available (libsyzsig has no CPU path)");
    return SG_ENODEV;
  }
  if (device < 0 || device >= ndev) {
    set_error("device %d out of range (%d devices)", device, ndev);
    return SG_EINVAL;
  }
  hipDeviceProp_t prop;
  SG_HIP(hipGetDeviceProperties(&prop, device));
  if (strncmp(prop.gcnArchName, "gfx950", 6) != 0) {
    set_error("device %d is %s; libsyzsig is built for gfx950 (MI355X) only", device, prop.gcnArchName);
    return SG_ENODEV;
  }
  std::unique_ptr<sg_ctx> c(new sg_ctx());  // (a failure below returns through its delete)
  c->device = device;
  c->max_launch_recs = kMaxLaunchRecords;
  // the diagnostics switches of the GPU scripts, read once here (every other
  // option is set by sg_ctx_set_option; nothing reads the environment later)
  c->debug_part = getenv("SG_DEBUG_PART") != nullptr;
  {
    static const struct { const char* name; int opt; int64_t lo, hi; } kSeed[] = {
        {"SG_BUCKET_BLOCKS", kOptBucketBlocks, INT64_MIN, INT64_MAX}, {"SG_FLAG_SKIP", kOptFlagSkip, -1, 1},
        {"SG_FLAG_SKIP_U16", -1, -1, 1}};  // (opt -1: flag_skip_u16, which is no row of sg_opts.h)
    for (const auto& s : kSeed)
      if (const char* e = getenv(s.name)) {
        const int64_t v = std::min(std::max<int64_t>(strtoll(e, nullptr, 10), s.lo), s.hi);
        if (s.opt >= 0)
          c->opt[s.opt] = v;
        else
          c->fs_u16_opt = (int)v;
      }
  }
  if (const char* e = getenv("SG_PREFIX_PAIRS")) c->opt[kOptPrefixPairs] = strtoll(e, nullptr, 10) != 0;
  c->cpu_quota = host_cpu_quota();
  int rc = ensure_device(c.get());
  if (!rc) rc = c->own_stream.create(hipStreamDefault);  // blocking: ordered with the null stream
  if (!rc) rc = c->dev.grow_drop(1, nullptr);
  if (rc) return rc;
  SG_HIP(hipMemset(c->dev.p, 0, sizeof(CtxDev)));
  c->stream = c->own_stream;
  *out = c.release();
  return SG_OK;
}

void sg_ctx_destroy(sg_ctx* ctx) {
  if (!ctx) return;
  hipSetDevice(ctx->device);
  hipStreamSynchronize(ctx->stream);
  if (ctx->copy_stream.h) hipStreamSynchronize(ctx->copy_stream);  // (before the buffers its DMAs use go)
  delete ctx;  // (every member frees itself, the streams last: sg_internal.h)
}

int sg_ctx_sync(sg_ctx* ctx) {
  if (!ctx) return SG_EINVAL;
  SG_HIP(hipStreamSynchronize(ctx->stream));
  return SG_OK;
}

int sg_ctx_set_stream(sg_ctx* ctx, void* hip_stream) {
  if (!ctx) return SG_EINVAL;
  ctx->stream = (hipStream_t)hip_stream;  // NULL: the device's legacy default stream
  return SG_OK;
}

int sg_ctx_reset_stream(sg_ctx* ctx) {
  if (!ctx) return SG_EINVAL;
  ctx->stream = ctx->own_stream;
  return SG_OK;
}

void* sg_ctx_stream(sg_ctx* ctx) { return ctx ? (void*)ctx->stream : nullptr; }

int sg_ctx_timing(sg_ctx* ctx, int enable) {
  if (!ctx) return SG_EINVAL;
  std::lock_guard<std::mutex> g(ctx->mu);
  timer_collect(ctx);
  KernelTimer& t = ctx->timer;
  for (auto& v : t.ms) v = 0;
  for (auto& v : t.count) v = 0;
  t.enabled = enable != 0;
  return SG_OK;
}

int sg_ctx_kernel_time(sg_ctx* ctx, const char* name, double* ms, uint64_t* launches) {
  if (!ctx || !name) return SG_EINVAL;
  std::lock_guard<std::mutex> g(ctx->mu);
  timer_collect(ctx);
  KernelTimer& t = ctx->timer;
  auto it = t.ids.find(name);
  if (ms) *ms = it == t.ids.end() ? 0 : t.ms[it->second];
  if (launches) *launches = it == t.ids.end() ? 0 : t.count[it->second];
  return SG_OK;
}

}  // extern "C"

namespace sg {
// one-thread kernels that only mark a point of the stream in kernel traces
__global__ void k_mark_begin(uint32_t* sink, uint32_t tag) {
  if (tag == 0xFFFFFFFFu) *sink = tag;  // never taken: keeps the launch from being elided
}
__global__ void k_mark_end(uint32_t* sink, uint32_t tag) {
  if (tag == 0xFFFFFFFFu) *sink = tag;
}
}  // namespace sg

extern "C" {

int sg_ctx_marker(sg_ctx* ctx, int end, uint32_t tag) {
  if (!ctx || tag == 0xFFFFFFFFu) return SG_EINVAL;
  std::lock_guard<std::mutex> g(ctx->mu);
  int rc = ensure_device(ctx);
  if (rc) return rc;
  if (end)
    hipLaunchKernelGGL(k_mark_end, dim3(1), dim3(1), 0, ctx->stream, (uint32_t*)&ctx->dev.p->scalar, tag);
  else
    hipLaunchKernelGGL(k_mark_begin, dim3(1), dim3(1), 0, ctx->stream, (uint32_t*)&ctx->dev.p->scalar, tag);
  SG_HIP(hipGetLastError());
  return SG_OK;
}

int sg_ctx_set_option(sg_ctx* ctx, const char* key, int64_t value) {
  if (!ctx || !key) return SG_EINVAL;
  std::lock_guard<std::mutex> g(ctx->mu);
  if (!strcmp(key, "max_launch_records")) {  // records per partitioned launch (lowered for slicing tests)
    if (value < 0 || (uint64_t)value > kMaxLaunchRecords) {
      set_error("sg_ctx_set_option: max_launch_records in 1..%llu (0: the default)",
                (unsigned long long)kMaxLaunchRecords);
      return SG_EINVAL;
    }
    ctx->max_launch_recs = value ? (uint64_t)value : kMaxLaunchRecords;
    return SG_OK;
  }
  if (!strcmp(key, "owner_key_space")) {  // Minimize's key space (lowered to reach the generation reset)
    if (ctx->owner.p) {
      set_error("sg_ctx_set_option: owner_key_space is set before the first-owner table exists");
      return SG_EINVAL;
    }
    if (value < 0 || (uint64_t)value > 0xFFFFFFFFull) {
      set_error("sg_ctx_set_option: owner_key_space in 1..2^32-1 (0: the default)");
      return SG_EINVAL;
    }
    ctx->owner_key_space = value ? (uint64_t)value : 0xFFFFFFFFull;
    return SG_OK;
  }
  if (!strcmp(key, "debug_part")) {
    ctx->debug_part = value != 0;
    return SG_OK;
  }
  if (!strcmp(key, "flag_skip_u16")) {  // the split launch's late pass 2 (sg_ctx::fs_u16_opt)
    if (value < -1 || value > 1) {
      set_error("sg_ctx_set_option: flag_skip_u16 in -1..1");
      return SG_EINVAL;
    }
    ctx->fs_u16_opt = (int)value;
    return SG_OK;
  }
  for (int i = 0; i < kOptCount; i++) {  // the range-checked ones (sg_opts.h)
    const SgOptRow& o = kSgOpts[i];
    if (strcmp(key, o.name)) continue;
    if (value < o.lo || value > o.hi) {
      set_error("sg_ctx_set_option: %s in %lld..%lld", key, (long long)o.lo, (long long)o.hi);
      return SG_EINVAL;
    }
    ctx->opt[i] = value;
    return SG_OK;
  }
  set_error("sg_ctx_set_option: unknown option '%s'", key);
  return SG_EINVAL;
}

int sg_ctx_get_option(sg_ctx* ctx, const char* key, int64_t* out) {
  if (!ctx || !key || !out) return SG_EINVAL;
  std::lock_guard<std::mutex> g(ctx->mu);
  if (!strcmp(key, "max_launch_records")) {
    *out = (int64_t)ctx->max_launch_recs;
    return SG_OK;
  }
  if (!strcmp(key, "owner_key_space")) {
    *out = (int64_t)ctx->owner_key_space;
    return SG_OK;
  }
  if (!strcmp(key, "debug_part")) {
    *out = ctx->debug_part;
    return SG_OK;
  }
  if (!strcmp(key, "flag_skip_u16")) {
    *out = ctx->fs_u16_opt;
    return SG_OK;
  }
  for (int i = 0; i < kOptCount; i++)
    if (!strcmp(key, kSgOpts[i].name)) {
      *out = ctx->opt[i];
      return SG_OK;
    }
  set_error("sg_ctx_get_option: unknown option '%s'", key);
  return SG_EINVAL;
}

}  // extern "C"

// ---- counters: one row each (sg_ctx_counter) ----------------------------------
namespace {
typedef uint64_t Quad[4];
enum CtrKind { kHost, kHost4, kDev32, kDev64, kConst, kCalc };
enum CtrCalc : uint64_t { kOwnerFloor, kM0Queued, kM0Logh, kCpuQuota, kFsFullBlocks, kFsAllFlagged, kFsU16, kWsBytes };
#define SG_DEV(field) offsetof(CtxDev, field)
struct Counter {
  const char* name;
  CtrKind kind;
  uint64_t arg;  // kHost4: the element, kDev32 / kDev64: the offset in CtxDev, kConst: the value, kCalc: which
  uint64_t sg_ctx::*host = nullptr;  // kHost: a host field, read under the lock without touching the stream
  Quad sg_ctx::*host4 = nullptr;     // kHost4: likewise, one of four
};
// (a device word, kDev32 / kDev64: the stream is waited for, then the field copied)
const Counter kCounters[] = {
    {"owner_resets", kHost, 0, &sg_ctx::owner_resets},
    {"owner_floor", kCalc, kOwnerFloor},  // the key space while there is no table
    {"owner_key_space", kHost, 0, &sg_ctx::owner_key_space},
    {"max_launch_records", kHost, 0, &sg_ctx::max_launch_recs},
    {"host_copy_bytes", kHost, 0, &sg_ctx::host_copy_bytes},  // the host ingest's last call (sg_host.hip)
    {"host_copy_ns", kHost, 0, &sg_ctx::host_copy_ns},
    {"host_wait_ns", kHost, 0, &sg_ctx::host_wait_ns},
    {"host_copy_threads", kHost, 0, &sg_ctx::host_threads},
    {"m0_filter_used", kHost, 0, &sg_ctx::m0f_used},          // record slices the M0 filter finished (sg_m0filter.hip)
    {"m0_filter_fallback", kHost, 0, &sg_ctx::m0f_fallback},  // ... and those whose survivors overflowed
    {"m0_filter_survivors", kHost, 0, &sg_ctx::m0f_survivors},  // survivors of the last filtered slice
    {"m0_filter_queued_milli", kCalc, kM0Queued},  // queued fraction x1000 of the last partitioned slice (~0: unknown)
    {"m0_filter_halves_log", kCalc, kM0Logh},      // the index's parts per slice (log2) the auto regime uses now
    {"flag_skip_used", kHost, 0, &sg_ctx::fs_used},     // bucket launches run in two phases (sg_bucket.hip)
    {"flag_skip_full_blocks", kCalc, kFsFullBlocks},    // fully queued record blocks the last of them found
    {"flag_skip_all_flagged", kCalc, kFsAllFlagged},    // ... and those whose second phase ran map-free (k_bucket_sets)
    {"hints_candidates", kHost, 0, &sg_ctx::hints_cands},  // the last sg_hints_replacers* call's matches (sg_hints.hip)
    {"exec_comps_general", kHost, 0, &sg_ctx::exec_comps_general},  // the last sg_exec_comps* call's general-path calls
    {"exec_cover_general", kHost, 0, &sg_ctx::exec_cover_general},  // the last sg_exec_cover* call's general-path calls
    {"merge_pairs_generic", kHost4, 0, nullptr, &sg_ctx::merge_pairs},  // the last merge_dev call's pairs per path
    {"merge_pairs_diff_small", kHost4, 1, nullptr, &sg_ctx::merge_pairs},
    {"merge_pairs_gap", kHost4, 2, nullptr, &sg_ctx::merge_pairs},
    {"merge_pairs_tile", kHost4, 3, nullptr, &sg_ctx::merge_pairs},
    {"canon_wave_lists", kHost4, 0, nullptr, &sg_ctx::canon_stats},  // the last canonicalize_dev call's per path
    {"canon_block_lists", kHost4, 1, nullptr, &sg_ctx::canon_stats},
    {"canon_big_segments", kHost4, 2, nullptr, &sg_ctx::canon_stats},
    {"canon_merge_passes", kHost4, 3, nullptr, &sg_ctx::canon_stats},  // ... and its rank-merge launches
    {"owned_big_records", kDev32, SG_DEV(owned_big)},  // an ordered-output call's records left to the big kernel
    // the last sg_triage_runs_from_kcov* call's candidates folded by foreach for a cover that is not
    // non-decreasing, and per route of the cover fold (sg_triage_runs.hip)
    {"triage_runs_wide", kDev32, SG_DEV(tr_wide)},
    {"triage_runs_copied", kDev32, SG_DEV(tr_route[kTrCopied])},
    {"triage_runs_sorted", kDev32, SG_DEV(tr_route[kTrSorted])},
    {"triage_runs_ranked", kDev32, SG_DEV(tr_route[kTrRanked])},
    {"triage_runs_foreach", kDev32, SG_DEV(tr_route[kTrForeach])},
    {"prio_bad_ids", kDev64, SG_DEV(prio_bad_ids)},  // ids >= ncalls sg_prio_table_add_dev skipped
    {"sha1_long_progs", kDev64, SG_DEV(sha1_long_progs)},  // programs that took the long SHA-1 path (sg_prog_hash.hip)
    {"sha1_long_len", kConst, kSha1Long},  // bytes of the longest program on the short SHA-1 path (SG_SHA1_LONG)
    {"inflate_long_streams", kDev64, SG_DEV(inflate_long_streams)},  // wave-per-stream path (sg_inflate.hip)
    {"inflate_long_len", kConst, kInflateLong},  // longest compressed stream on the lane path (SG_INFLATE_LONG)
    {"deflate_long_streams", kDev64, SG_DEV(deflate_long_streams)},  // wave-per-stream path (sg_deflate.hip)
    {"deflate_long_len", kConst, kDeflateLong},  // longest input on the lane path (SG_DEFLATE_LONG)
    {"deflate_stored_streams", kDev64, SG_DEV(deflate_forms[0])},  // the last deflate count's streams per form
    {"deflate_fixed_streams", kDev64, SG_DEV(deflate_forms[1])},
    {"deflate_dynamic_streams", kDev64, SG_DEV(deflate_forms[2])},
    {"prio_band_cells", kConst, kPrioBandCells},  // u32 cells of a row band of the pair count
    {"prio_short_len", kConst, kPrioShort},       // calls of a program on the pair count's band path
    {"triage_runs_sort_cap", kConst, kTrSort},    // values a cover fold may hold on the LDS-sort route
    {"tinput_chunk", kConst, kTinChunk},          // values of new_k per LDS chunk of Intersection (sg_tinput.h)
    {"exec_comps_fast_cap", kConst, SG_EXEC_COMPS_FAST_CAP},  // distinct records a call may hold on the fast shape
    {"exec_cover_fast_cap", kConst, SG_EXEC_COVER_FAST_CAP},  // distinct PCs a call may hold on the fast shape
    {"cover_pages_tile", kConst, kPagesTile},  // bytes of the bodies per workgroup of sg_cover_pages' copy
    {"cpu_quota_milli", kCalc, kCpuQuota},
    {"workspace_bytes", kCalc, kWsBytes},  // the workspace buffer's capacity (ws_reserve)
};

int counter_calc(sg_ctx* ctx, uint64_t which, uint64_t* out) {
  if ((which == kFsFullBlocks || which == kFsAllFlagged || which == kFsU16) && ctx->fs_pending) {  // (the last split launch's words may still be on their way)
    SG_HIP(hipEventSynchronize(ctx->fs_ev));
    ctx->fs_pending = false;
    ctx->fs_full_blocks = ctx->pinned.p->fs_full_blocks;
    ctx->fs_all_flagged = ctx->pinned.p->fs_all_flagged;
    ctx->fs_u16 = ctx->pinned.p->fs_u16;
  }
  switch (which) {
    case kOwnerFloor: *out = ctx->owner.p ? ctx->owner_floor : ctx->owner_key_space; break;
    case kM0Queued: *out = ctx->m0f_queued < 0 ? ~0ull : (uint64_t)(ctx->m0f_queued * 1000.0 + 0.5); break;
    case kM0Logh: *out = (uint64_t)ctx->m0f_logh; break;
    case kCpuQuota: *out = (uint64_t)(ctx->cpu_quota * 1000.0 + 0.5); break;
    case kFsFullBlocks: *out = ctx->fs_full_blocks; break;
    case kFsAllFlagged: *out = ctx->fs_all_flagged; break;
    case kFsU16: *out = ctx->fs_u16; break;
    case kWsBytes: *out = ctx->ws.cap; break;
  }
  return SG_OK;
}
}  // namespace

extern "C" int sg_ctx_counter(sg_ctx* ctx, const char* name, uint64_t* out) {
  if (!ctx || !name || !out) return SG_EINVAL;
  std::lock_guard<std::mutex> g(ctx->mu);
  // split launches whose window-2 pass 2 ran in 2-byte entries: read with the two flag_skip words above
  if (!strcmp(name, "flag_skip_u16")) return counter_calc(ctx, kFsU16, out);
  for (const Counter& c : kCounters) {
    if (strcmp(name, c.name)) continue;
    if (c.kind == kCalc) return counter_calc(ctx, c.arg, out);
    uint64_t v = c.kind == kConst ? c.arg : 0;
    if (c.kind == kHost) v = ctx->*c.host;
    if (c.kind == kHost4) v = (ctx->*c.host4)[c.arg];
    if (c.kind == kDev32 || c.kind == kDev64) {  // (little-endian: four bytes land in v's low half)
      SG_HIP(hipStreamSynchronize(ctx->stream));
      SG_HIP(hipMemcpy(&v, (const char*)ctx->dev.p + c.arg, c.kind == kDev64 ? 8 : 4, hipMemcpyDeviceToHost));
    }
    *out = v;
    return SG_OK;
  }
  set_error("sg_ctx_counter: unknown counter '%s'", name);
  return SG_EINVAL;
}
