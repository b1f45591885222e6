// sg_internal.h -- shared host/device plumbing of libsyzsig.so (not installed).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <deque>
#include <map>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/syzsig.h"
#include "sg_buf.h"
#include "sg_opts.h"
#include "sg_plan.h"

namespace sg {

// 2^32-bit direct-indexed signal bitmap: 2^27 words = 512 MiB.
constexpr uint64_t kSetWords = 1ull << 27;
constexpr uint64_t kSetBytes = kSetWords * 4;
// First-owner table: one u32 key per possible signal value = 16 GiB.
constexpr uint64_t kOwnerEntries = 1ull << 32;
constexpr uint32_t kOwnerInf = 0xFFFFFFFFu;
// Records per launch of the partitioned triage (256 groups of 2^16 records);
// larger batches run as consecutive record slices (sg_part_triage.hip).
constexpr uint64_t kMaxLaunchRecords = 1ull << 24;

// Element tiles of the streaming kernels: 256 threads, one uint4 (4 values)
// per lane per step, 4 steps per wave -> 4096 values per workgroup tile;
// a "chunk" is one wave-instruction's 256 values and carries a 4 x u64
// ballot mask (bit l of word k <-> value 4l+k of the chunk).
constexpr int kBlock = 256;
constexpr int kChunk = 256;
constexpr int kTile = 4096;
constexpr int kChunksPerTile = kTile / kChunk;  // 16
constexpr int kWin = 1024;                      // record-offset window kept in LDS per tile

void set_error(const char* fmt, ...);

struct KernelTimer {
  bool enabled = false;
  struct Rec {
    int id;
    hipEvent_t a, b;
  };
  std::vector<Rec> pending;
  std::vector<hipEvent_t> pool;
  std::deque<Event> events;  // the owner of every event of pending and pool
  std::map<std::string, int> ids;
  std::vector<std::string> names;
  std::vector<double> ms;
  std::vector<uint64_t> count;
};

}  // namespace sg

// one record slice of a two-phase (prefix) triage: records [r0, r1),
// entries [e0, e1), its partition at workspace offset ws_base
struct PrefixSlice {
  uint64_t r0, r1, e0, e1;
  size_t ws_base;
};

// One kept batch of the two-phase triage: its record slices and their
// partitions (or, with option prefix_pairs, its first-owner pairs), in a workspace of
// its own (two slots, so one batch's exchange can run while the next one is
// partitioned)
struct PrefixSlot {
  std::vector<PrefixSlice> slices;
  uint64_t nrec = 0;
  uint64_t n = 0;              // signal entries of the batch (bounds the pairs)
  uint32_t* marks = nullptr;   // begin's marks (end's set updates)
  bool keep = false;           // partitions kept instead of pairs
  bool open = false;
  sg::DevBuf<char> ws;  // swapped with the context's during the slot's calls (sg_prefix.hip SlotWs)
};
constexpr uint32_t kPrefixSlots = 2;

namespace sg {
// The cover fold's routes (sg_triage_runs.hip), counted in CtxDev::tr_route
enum : uint32_t { kTrCopied = 0, kTrSorted = 1, kTrRanked = 2, kTrForeach = 3, kTrRoutes = 4 };
// The context's device words: one allocation, zeroed at creation (sg_ctx::dev).
// A launch site takes &ctx->dev.p->field; the counters among them are read by
// sg_ctx_counter alone, after a stream sync (its table says what each counts).
struct CtxDev {
  uint64_t scalar;          // call-scoped: sg_set_new's, sg_set_count_missing_dev's, has_difference's, a marker's
  uint32_t m0f_queued;      // queued records of the last counted partitioned slice (sg_m0filter.hip)
  uint32_t fs_full_blocks;  // full record blocks of the last split bucket launch (sg_bucket.hip)
  uint32_t fs_all_flagged;  // ... and the split launches whose second phase ran map-free (cumulative; copied with it)
  uint32_t fs_u16;          // ... and those whose window-2 pass 2 wrote 2-byte entries (cumulative; same copy)
  uint32_t owned_big;       // "owned_big_records": zeroed by an ordered-output call, added to by each slice's launch
  uint32_t tr_wide;         // "triage_runs_wide", and the cover fold's routes after it (zeroed together)
  uint32_t tr_route[kTrRoutes];
  uint64_t prio_bad_ids, sha1_long_progs, inflate_long_streams;  // (cumulative over the context's life)
  uint64_t deflate_long_streams;  // likewise (sg_deflate.hip)
  uint64_t deflate_forms[3];      // the last deflate_count's streams per form: stored, fixed, dynamic
};
static_assert(offsetof(CtxDev, scalar) % 8 == 0 && offsetof(CtxDev, prio_bad_ids) % 8 == 0 &&
                  offsetof(CtxDev, sha1_long_progs) % 8 == 0 && offsetof(CtxDev, inflate_long_streams) % 8 == 0 &&
                  offsetof(CtxDev, deflate_long_streams) % 8 == 0 && offsetof(CtxDev, deflate_forms) % 8 == 0,
              "64-bit device words are 8-byte aligned");
static_assert(offsetof(CtxDev, tr_route) == offsetof(CtxDev, tr_wide) + 4, "wide and the routes are zeroed together");
// ... and the pinned words two of them are copied to, read without a host wait once the event has passed
struct CtxPinned {
  uint32_t m0f_queued;      // behind sg_ctx::m0f_ev
  uint32_t fs_full_blocks;  // behind sg_ctx::fs_ev
  uint32_t fs_all_flagged;  // likewise (one copy)
  uint32_t fs_u16;          // likewise
};
}  // namespace sg

// Nothing here is a raw owning handle: sg_ctx_destroy waits for stream and copy_stream and deletes the
// context.  The members go in reverse order of declaration, so the two streams stand first: every event is
// destroyed before the stream it was recorded on, and every buffer before either stream.
struct sg_ctx {
  int device = 0;
  sg::Stream own_stream;
  hipStream_t stream = nullptr;  // own_stream, or the caller's (sg_ctx_set_stream)
  // the host ingest pipeline (sg_host.hip): its copy stream and the events
  // between the two staging slots' DMA and triage
  sg::Stream copy_stream;
  sg::Event pipe_ev[4];
  int64_t opt[kOptCount];
  sg_ctx() { for (int i = 0; i < kOptCount; i++) opt[i] = kSgOpts[i].def; }
  sg::DevBuf<sg::CtxDev> dev;
  // the M0 filter's buffers (lazy, sg_m0filter.hip) and its regime state: the
  // last record slice's outcome (1 filtered, 0 partitioned), the queued
  // records of the last partitioned slice (counted on the device, read back
  // through pinned once m0f_ev has passed: no host wait) and its record
  // count; slices it filtered and fell back on (counters)
  sg::DevBuf<char> m0f;
  sg::Buf<sg::CtxPinned, true> pinned;  // (lazy, with m0f_ev: m0f_host_alloc)
  sg::Event m0f_ev;
  int m0f_last = -1;             // -1 nothing yet
  bool m0f_pending = false;
  uint64_t m0f_nrec = 0;
  double m0f_queued = -1;        // queued fraction of the last partitioned slice (-1 unknown)
  uint64_t m0f_used = 0, m0f_fallback = 0, m0f_survivors = 0;
  uint32_t m0f_backoff = 0, m0f_skip = 0;  // auto: slices not to try after fallbacks (doubling, <= 64)
  // the split bucket stage (flag_skip): launches split, and the summary bits
  // of the last one (counted on the device, read through pinned once fs_ev
  // has passed), with the launches so far whose second phase ran map-free
  // (every record flagged by the first; the device's running count, same copy)
  uint64_t fs_used = 0, fs_full_blocks = 0, fs_all_flagged = 0, fs_u16 = 0;
  // option flag_skip_u16: a split launch's pass 2 over the second window after the summary, in 2-byte entries when
  // every record is flagged (-1 whenever the launch splits, 0 never, 1 with the split forced; sg_part_triage.hip)
  int fs_u16_opt = -1;
  sg::Event fs_ev;
  bool fs_pending = false;
  int m0f_logh = 0;  // auto: the index in 2^m0f_logh parts per slice (raised when a slice's index overflows)
  // host CPUs this process may use (cgroup cpu.max quota, else the affinity
  // mask), read at creation: sizes the host ingest's copy threads
  double cpu_quota = 0;
  // the host ingest's last call (sg_host.hip): bytes copied pageable -> pinned,
  // the wall time of those copies and of its waits for the staging slots'
  // DMA, and the copy threads used
  uint64_t host_copy_bytes = 0, host_copy_ns = 0, host_wait_ns = 0, host_threads = 0;
  // the last sg_hints_replacers* call's (slot, pair) matches, before deduplication (sg_hints.hip)
  uint64_t hints_cands = 0;
  // the calls the last sg_exec_comps* call sent down the general path (sg_exec_comps.hip)
  uint64_t exec_comps_general = 0;
  // ... and the last sg_exec_cover* call (sg_exec_cover.hip)
  uint64_t exec_cover_general = 0;
  // the last merge_dev call's pairs per path (generic, k_diff_small, and
  // k_merge_small's gap / tile forms) and the last canonicalize_dev call's
  // segments per path (a wave each, a workgroup each, the big path) with its
  // rank-merge passes (sg_merge.hip): host arithmetic over the lengths
  uint64_t merge_pairs[4] = {0, 0, 0, 0};
  uint64_t canon_stats[4] = {0, 0, 0, 0};
  // grow-only device workspace and pinned host staging (capacities in bytes;
  // grown by ws_reserve / pin_reserve, contents dropped)
  sg::DevBuf<char> ws;
  sg::PinBuf pin;
  // grow-only device staging for the host entry points' inputs / outputs (dstage_reserve)
  sg::DevBuf<char> dstage;
  // sg_inflate_batch's outputs on their way to the host (grow-only from 16 MiB; sg_inflate.hip), and those of
  // sg_deflate_batch, sg_db_serialize and sg_db_compact (sg_deflate.hip, sg_db.hip)
  sg::DevBuf<uint8_t> inflate_out;
  // first-owner table and its decreasing key floor; the key space is 2^32 - 1
  // (option owner_key_space lowers it, so tests reach the generation reset)
  sg::DevBuf<uint32_t> owner;  // (lazy: owner_keys)
  uint64_t owner_floor = 0;
  uint64_t owner_key_space = 0xFFFFFFFFull;
  uint64_t owner_resets = 0;
  // partitioned triage: records per launch (option max_launch_records lowers
  // it, for tests of the record slicing) and diagnostics (option debug_part)
  uint64_t max_launch_recs = 0;
  // two-phase triage state (prefix_begin / prefix_end, sg_prefix.hip)
  PrefixSlot prefix[kPrefixSlots];
  bool debug_part = false;
  // rebased record offsets of record slices (grow-only, to the exact size: slice_off_reserve)
  sg::DevBuf<uint64_t> slice_off;
  // a batch's record-slice cuts, found on the device (sg_part_triage.hip k_slice_cuts)
  sg::DevBuf<uint64_t> slice_cuts;
  // cached Zipf generator tables (alias method + rank->pc permutation; sg_exec.hip gen_tables)
  sg::DevBuf<uint32_t> gen_prob, gen_alias, gen_perm;
  uint64_t gen_seed = 0;
  double gen_s = 0;
  uint32_t gen_nranks = 0;
  sg::KernelTimer timer;
  std::mutex mu;
};

struct sg_set {
  sg_ctx* ctx = nullptr;
  uint32_t* words = nullptr;  // the bitmap: mem's block, or the caller's (sg_set_wrap_dev)
  sg::DevBuf<uint32_t> mem;   // empty in a wrapper
};

// map[hash.Sig]bool on the device (sg_sigset.hip)
struct SigKey {
  uint32_t w[SG_SIG_BYTES / 4];
};
// One {store, table} pair of a set.  The store's capacity is in keys; the
// table's is its slot count, always the power of two that was asked for (the
// probes mask with it).
struct SigHalf {
  sg::DevBuf<SigKey> store;
  sg::DevBuf<uint32_t> table;
  uint32_t* keys() const { return (uint32_t*)store.p; }
  uint32_t mask() const { return (uint32_t)(table.cap - 1); }
  void swap(SigHalf& o) {
    store.swap(o.store);
    table.swap(o.table);
  }
};
struct sg_sigset {
  sg_ctx* ctx = nullptr;
  uint64_t count = 0;  // identities held (kept on the host: every call that changes it waits)
  SigHalf cur;
  // hub_sync, remove and the hub corpus' purge build the new set here, then swap the halves
  SigHalf next;
};

namespace sg {

// ---- host helpers (sg_ctx.hip) ----
// (hip_fail and SG_HIP: sg_buf.h)
int ensure_device(sg_ctx* ctx);
// Grow-only buffers, each by grow_cap (sg_plan.h) from its floor: 64 MiB of
// workspace, 16 MiB of pinned and of device staging.  Growing drops the
// contents and waits for ctx->stream first (the staging buffers: for
// ctx->copy_stream too).  The plan forms (WsPlan) reserve plan.total and
// refuse a plan with more regions than it records.
int ws_reserve(sg_ctx* ctx, size_t bytes);
int ws_reserve(sg_ctx* ctx, const WsPlan& plan);
inline void* ws_at(sg_ctx* ctx, size_t off) { return ctx->ws.p + off; }
int pin_reserve(sg_ctx* ctx, size_t bytes);
// The host forms' staging: plan the regions, reserve once, then bind each
// pointer from the offset WsPlan::add returned (the buffer may move in the
// reserve, never after it).
int dstage_reserve(sg_ctx* ctx, size_t bytes);
int dstage_reserve(sg_ctx* ctx, const WsPlan& plan);
template <typename T>
inline T* dstage_at(sg_ctx* ctx, size_t off) {
  return (T*)(ctx->dstage.p + off);
}
// Room for `need` elements in a buffer that runs parallel to a set's keys (the
// key store itself, the hub corpus' records): 1024 elements, then doubling,
// the first `keep` kept (copied on ctx->stream, waited for).
constexpr size_t kRecFloor = 1024;
template <typename T>
int rec_reserve(sg_ctx* ctx, DevBuf<T>& b, size_t need, size_t keep) {
  return b.grow_keep(grow_cap(b.cap, need, kRecFloor), keep, ctx->stream);
}
// ctx->slice_off of exactly `n` offsets when it holds fewer (waits for ctx->stream).
int slice_off_reserve(sg_ctx* ctx, size_t n);
// Host -> device on ctx->stream; nothing for zero bytes.
int upload(sg_ctx* ctx, void* d_dst, const void* h_src, size_t bytes);
// CSR download on ctx->stream: the n + 1 offsets, a wait, then the off[n] *
// elem payload bytes when there are any and off[n] <= cap, and a second wait.
int csr_download(sg_ctx* ctx, uint64_t* h_off, const uint64_t* d_off, uint64_t n, void* h_vals, const void* d_vals,
                 size_t elem, uint64_t cap);
// Reserve `nkeys` first-owner keys: returns key_lo such that keys
// key_lo .. key_lo+nkeys-1 are below every key already stored in the table.
int owner_keys(sg_ctx* ctx, uint64_t nkeys, uint32_t* key_lo);

// Kernel timing around launches on ctx->stream.
void timer_begin(sg_ctx* ctx, const char* name, int* slot);
void timer_end(sg_ctx* ctx, int slot);
struct ScopedTimer {
  sg_ctx* c;
  int slot = -1;
  ScopedTimer(sg_ctx* ctx, const char* name) : c(ctx) { timer_begin(ctx, name, &slot); }
  ~ScopedTimer() { timer_end(c, slot); }
};

inline uint32_t div_up(uint64_t a, uint64_t b) { return (uint32_t)((a + b - 1) / b); }

// Device exclusive scan of u32 counts into u64 offsets, out[n] = total
// (sg_scan.hip).  Uses the workspace tail beyond `ws_used`.
int scan_counts(sg_ctx* ctx, const uint32_t* d_in, uint64_t* d_out, uint64_t n, size_t ws_used);
size_t scan_ws_bytes(uint64_t n);

// Members of a set, ascending, into device memory (sg_set.hip; ctx lock held).
int set_export_dev(sg_set* set, uint32_t* d_out, uint64_t cap, uint64_t* total);
// SignalAdd of device-resident values (sg_set.hip; ctx lock held, stream-ordered).
int set_add_dev_locked(sg_set* set, const uint32_t* d_vals, uint64_t n);

// A batch in host memory through pinned double-buffered staging, record
// slice by record slice, each slice's copies overlapping the previous one's
// partitioned triage (sg_host.hip); takes the ctx lock.
double host_cpu_quota();
int host_copy_threads(const sg_ctx* ctx);
int host_pipeline(sg_ctx* ctx, uint32_t* mwords, uint32_t* nwords, const uint32_t* vals, const uint64_t* rec_off,
                  uint64_t nrec, uint8_t* rec_new, bool trace);
// Partitioned flags-only triage (sg_part_triage.hip); ctx lock held.  trace:
// d_vals are raw per-call PC traces, triaged by their edge signal.
int bucket_triage(sg_ctx* ctx, uint32_t* mwords, uint32_t* nwords, const uint32_t* d_vals, const uint64_t* d_off,
                  uint64_t n, uint64_t nrec, uint8_t* d_rec_new, bool trace = false);
// Candidate emission of the partitioned path (sharded triage, sg_shard.hip;
// the prefix protocol's pair form): each distinct s not in the snapshot, once
// per launch, as {s, rec_base + first record}, counted per owning shard when
// shard_cnt is given.
struct EmitArgs {
  uint2* pairs;
  unsigned long long* npairs;
  uint32_t rec_base;
  uint32_t nshards;
  unsigned long long* shard_cnt;
  bool update;  // also update the sets (their new bits = the emitted signals); no record flags
  unsigned long long* gcur;  // update form: pairs group-major, group g's at goff[g << 16] + gcur[g]++
  const uint64_t* goff;      //   (goff: the launch's record offsets)
};
// Workgroups of `kernel` resident on the whole device at once (cached per device).
uint32_t persistent_grid(sg_ctx* ctx, const void* kernel, int threads);
// d_out[i] = d_off[i] - base, i < n (a record slice's offsets rebased).
int rebase_offsets(sg_ctx* ctx, const uint64_t* d_off, uint64_t n, uint64_t base, uint64_t* d_out);
// Workspace bytes of one partitioned launch over n entries / nrec records.
size_t bucket_plan_bytes(uint64_t n, uint64_t nrec);
// A batch's record slices (<= max_launch_recs records, <= lim entries unless
// one record alone holds more), as {r0, r1, e0, e1} quadruples: cuts found on
// the device, one wait (sg_part_triage.hip k_slice_cuts).
int record_slice_cuts(sg_ctx* ctx, const uint64_t* d_off, uint64_t nrec, uint64_t lim, std::vector<uint64_t>& cuts);
// Two-phase triage (sg_prefix.hip): begin ORs into marks_words the batch's
// signal not in base_words and keeps the batch's partitions (or each such
// signal's first record) in the slot; end flags the records against
// mwords | owords and, with `update`, updates mwords / nwords.
// form: 0 kept partitions, 1 first-owner pairs, -1 from option prefix_pairs; d_ncand
// (nullable, device): the batch's distinct signals not in base_words.
int prefix_begin(sg_ctx* ctx, uint32_t slot, const uint32_t* base_words, uint32_t* marks_words, const uint32_t* d_vals,
                 const uint64_t* d_off, uint64_t n, uint64_t nrec, int form = -1, uint64_t* d_ncand = nullptr);
int prefix_end(sg_ctx* ctx, uint32_t slot, uint32_t* mwords, const uint32_t* owords, uint32_t* nwords, uint8_t* d_rec_new,
               bool update);
// One emitting launch (nrec <= kMaxLaunchRecords, n < 2^32 - 2^15), scratch
// at ws_base (reserved by the caller).
int bucket_emit(sg_ctx* ctx, const uint32_t* mwords, const uint32_t* d_vals, const uint64_t* d_off, uint64_t n,
                uint64_t nrec, const EmitArgs& emit, size_t ws_base);
// The ordered outputs' bucket stage (one launch, limits as bucket_emit):
// mwords / nwords (nullable) gain the batch's new signals, and each new
// signal is written once as {s, its first record} (records launch-relative),
// group-major: the pairs of record group g (records g << 16 ..) at
// pairs[d_off[g << 16] + i], i < gcur[g] (device, zeroed by the caller; a
// group's new signals never outnumber its entries); no record flags.
int bucket_emit_update(sg_ctx* ctx, uint32_t* mwords, uint32_t* nwords, const uint32_t* d_vals, const uint64_t* d_off,
                       uint64_t n, uint64_t nrec, uint2* pairs, unsigned long long* gcur, size_t ws_base);
constexpr uint32_t kRecGroupBits = 16;  // records per group of the partitioned path: 2^16
// Workspace bytes beyond two key buffers of radix_sort_u64 (sg_sort.hip).
size_t radix_sort_ws(uint64_t n);
int radix_sort_u64(sg_ctx* ctx, uint64_t* a, uint64_t* b, uint64_t n, size_t ws_used, uint64_t** sorted,
                   uint64_t vary = 0);
// One stable radix pass over keys in runs of a gapped buffer (run order kept
// within a digit), written contiguously into dst (sg_sort.hip; syncs).
int radix_pass_runs(sg_ctx* ctx, const uint64_t* src, const std::vector<uint64_t>& run_start,
                    const std::vector<uint64_t>& run_cnt, uint32_t shift, uint64_t* dst, size_t ws_used);
size_t radix_pass_runs_ws(uint64_t n, uint64_t nruns);

// sg_exec_comps_dev's body (sg_exec_comps.hip; ctx lock held, the device
// ensured).  With `raw` it stops before k_ec_emit: d_comp_off is filled, no
// triples and no words are written, and raw tells where the workspace holds
// the calls' sorted distinct keys, raw (call c's at tmp + 3 * call_off[c],
// comp_off[c + 1] - comp_off[c] of them), until the next ws_reserve.  tmp is
// null when the batch has no calls or no records (nothing was reserved).
struct EcRaw {
  const uint64_t* tmp = nullptr;
  uint32_t* cnt = nullptr;  // [ncalls] scratch of the same reservation, free for the caller
  size_t scan_off = 0;      // scan_counts' workspace for ncalls counts, likewise
};
int exec_comps(sg_ctx* ctx, const uint64_t* d_recs, const uint64_t* d_call_off, uint64_t ncalls, uint64_t nrecs,
               uint64_t* d_comp_off, uint64_t* d_comps, uint64_t comps_cap, uint64_t* d_word_off, uint32_t* d_words,
               uint64_t words_cap, EcRaw* raw = nullptr);
int ec_limits(uint64_t ncalls, uint64_t nrecs);
// sg_exec_signal_dev's body, and with d_rec_new sg_exec_signal_queued_dev's
// (sg_exec.hip; ctx lock held, the device ensured).  Plans the workspace from 0.
int exec_signal_body(sg_ctx* ctx, const uint32_t* d_pcs, const uint64_t* d_call_off, const uint64_t* d_prog_off,
                     uint64_t nprog, uint64_t ncalls, uint64_t npcs, const uint8_t* d_rec_new, uint32_t* d_sig_vals,
                     uint64_t* d_sig_off);
// sg_exec_cover_dev's body (sg_exec_cover.hip; ctx lock held, the device
// ensured).  With sel ([ncalls], nullable) only the calls with sel[c] != 0 run;
// the others get empty lists.  Plans the workspace from 0.
int exec_cover(sg_ctx* ctx, const uint64_t* d_pcs, const uint64_t* d_call_off, uint64_t ncalls, uint64_t npcs, int dedup,
               uint64_t* d_cov_off, uint32_t* d_cov, uint64_t cov_cap, const uint8_t* sel = nullptr);
// read by sg_ctx_counter as "prio_band_cells" and "prio_short_len"
constexpr uint32_t kPrioBandCells = 40960;  // u32 cells of a row band: the CU's 160 KiB of LDS
constexpr uint32_t kPrioShort = 64;         // calls of a program on the band path; longer ones take k_prio_long
// read by sg_ctx_counter as "sha1_long_len" (SG_SHA1_LONG)
constexpr uint32_t kSha1Long = SG_SHA1_LONG;
// read by sg_ctx_counter as "cover_pages_tile": bytes of the bodies a workgroup of k_pg_copy writes (sg_cover_pages.hip)
constexpr uint32_t kPagesTile = 4096;
// read by sg_ctx_counter as "triage_runs_sort_cap" and "tinput_chunk"
constexpr uint32_t kTrSort = 8192;    // values the cover fold sorts in LDS (64 KiB of keys)
constexpr uint32_t kTinChunk = 8192;  // values of a per LDS chunk of tin_intersect (32 KiB)
// Canonicalize of device segments in place: off (host, nseg + 1), out_len
// (host) the canonical lengths; and the batched merge of device-resident
// lists, pair k da[a_beg[k] .. + a_len[k]) op db[b_beg[k] .. + b_len[k]) into
// dout[out_beg[k] ..), the pair descriptors and out_len host arrays
// (sg_merge.hip; ctx lock held; both wait for their lengths).
int canonicalize_dev(sg_ctx* ctx, uint32_t* d_vals, const uint64_t* off, uint64_t nseg, uint64_t* out_len);
int merge_dev(sg_ctx* ctx, int op, const uint32_t* da, const uint32_t* db, uint32_t* dout, const uint64_t* a_beg,
              const uint64_t* a_len, const uint64_t* b_beg, const uint64_t* b_len, const uint64_t* out_beg,
              size_t npair, uint64_t* out_len);
// The join and the sorts behind sg_hints_replacers* (sg_hints.hip; ctx lock
// held).  Plans the context workspace from offset 0 and may move it.  With
// reps_in_ws the replacers go to a workspace buffer of min(cap, candidates)
// slots (*ws_reps), for a host form to copy out.
int hints_replacers(sg_ctx* ctx, const uint64_t* d_pair_off, const uint64_t* d_pairs, uint64_t nrec,
                    const uint64_t* d_val_off, const uint64_t* d_vals, uint64_t nvals, uint64_t* d_rep_off,
                    uint64_t* d_reps, uint64_t cap, bool reps_in_ws, uint64_t** ws_reps);

// sg_prog_hashes_dev's body (sg_prog_hash.hip; ctx lock held, the device
// ensured): d_sigs[20 * p ..) = SHA-1 of program p, every range clamped to
// nbytes.  Uses prog_hashes_ws(nprogs) bytes of the workspace from ws_used on,
// reserved by the caller.  nprogs < 2^32.
size_t prog_hashes_ws(uint64_t nprogs);
int prog_hashes(sg_ctx* ctx, const uint8_t* d_bytes, const uint64_t* d_off, uint64_t nprogs, uint64_t nbytes,
                uint8_t* d_sigs, size_t ws_used);
// what the host forms over program texts reject (fn names the caller)
int prog_texts_ok(const char* fn, const uint8_t* bytes, const uint64_t* off, size_t nprogs);

// What sg_hub_state.hip takes from sg_sigset.hip (ctx lock held, the device
// ensured; keys are device memory, five u32 words each).
constexpr uint64_t kSigsetMaxKeys = 1ull << 31;
int sigset_new(sg_ctx* ctx, uint64_t hint, sg_sigset** out);
void sigset_delete(sg_sigset* s);
// sg_sigset_add_new of n device keys: d_is_new ([n], nullable) as is_new; waits,
// and s->count is the new count on return.  Leaves in the workspace, until its
// next use, flag ([n] u32: key k entered the store) at ws_base and pos ([n + 1],
// the flags' scan: key k went to store index old count + pos[k]) at *o_pos.
// Uses sigset_add_ws(n) bytes from ws_base on, reserved by the caller.
size_t sigset_add_ws(uint64_t n);
int sigset_add_dev(sg_sigset* s, const uint32_t* d_keys, uint64_t n, uint8_t* d_is_new, size_t ws_base, size_t* o_pos);
// out32[k] = 1 iff d_keys[k] is in s (want 1) or is not (want 0)
int sigset_lookup_dev(sg_sigset* s, const uint32_t* d_keys, uint64_t n, uint32_t want, uint32_t* out32);
// acc[k] |= d_keys[k] is in s
int sigset_lookup_or_dev(sg_sigset* s, const uint32_t* d_keys, uint64_t n, uint32_t* acc);
// The set without the keys whose keep[i] is zero, the rest in their order:
// pos is keep's scan ([count + 1]) and newcount its total, read back by the
// caller.  A fresh store and table, swapped in (no tombstones); waits.
int sigset_rebuild_dev(sg_sigset* s, const uint32_t* d_keep, const uint64_t* d_pos, uint64_t newcount);
// out[pos[t]] = keys[t] for the t < n with flag[t] != 0 and pos[t] < cap
int sigset_gather_dev(sg_ctx* ctx, const uint32_t* d_keys, uint64_t n, const uint32_t* d_flag, const uint64_t* d_pos,
                      uint32_t* d_out, uint64_t cap);

// prog.CallSet over a batch (sg_call_set.hip; ctx lock held, the device ensured).
// call_sets_count: d_status [nprogs] and d_line_off [nprogs + 1] (its last
// entry the batch's call lines), from call_sets_ws(nprogs, nbytes) bytes of the
// workspace at ws_used, reserved by the caller; offsets_checked: the host has
// seen that they do not decrease (prog_texts_ok).  call_sets_emit, with that
// workspace untouched since: the lines' spans and ids when the total is <= cap
// (compared on the device).  tab may be null (every id SG_NAME_UNKNOWN).
size_t call_sets_ws(uint64_t nprogs, uint64_t nbytes);
int call_sets_limits(const char* fn, uint64_t nprogs, uint64_t nbytes);
int call_sets_count(sg_ctx* ctx, const uint8_t* d_bytes, const uint64_t* d_off, uint64_t nprogs, uint64_t nbytes,
                    uint8_t* d_status, uint64_t* d_line_off, size_t ws_used, bool offsets_checked);
int call_sets_emit(sg_ctx* ctx, sg_nametab* tab, const uint8_t* d_bytes, const uint64_t* d_off, uint64_t nprogs,
                   uint64_t nbytes, const uint8_t* d_status, const uint64_t* d_line_off, uint64_t* d_name_pos,
                   uint32_t* d_name_len, uint32_t* d_name_id, uint64_t cap, size_t ws_used);
sg_ctx* nametab_ctx(const sg_nametab* tab);
uint64_t nametab_names(const sg_nametab* tab);

// Raw DEFLATE over a batch of streams (sg_inflate.hip; ctx lock held, the
// device ensured).  Stream p is d_in[d_beg[p], d_end[p]), clamped to nbytes: a
// CSR passes off and off + 1, a database file the starts and ends of its
// framed values.  inflate_count: status, consumed and output length of every
// stream, from inflate_ws(n) bytes of the workspace at ws_used, reserved by
// the caller; *d_sorted is where that workspace holds the sorted keys.
// inflate_offsets: scan_counts of the lengths (which the caller may have
// edited: a zero length is a stream nobody wants) in the same workspace.
// inflate_write, with the workspace untouched since the count: the outputs of
// the OK streams with a span, when d_out_off[n] <= cap (compared on the
// device).  n < 2^32.
// "inflate_long_len" reads SG_INFLATE_LONG.
constexpr uint32_t kInflateLong = SG_INFLATE_LONG;
constexpr uint64_t kInflateMaxOut = 1ull << 33;
size_t inflate_ws(uint64_t n);
int inflate_count(sg_ctx* ctx, const uint8_t* d_in, const uint64_t* d_beg, const uint64_t* d_end, uint64_t n,
                  uint64_t nbytes, uint8_t* d_status, uint64_t* d_consumed, uint32_t* d_olen, size_t ws_used,
                  const uint64_t** d_sorted);
int inflate_offsets(sg_ctx* ctx, const uint32_t* d_olen, uint64_t* d_out_off, uint64_t n, size_t ws_used);
int inflate_write(sg_ctx* ctx, const uint8_t* d_in, const uint64_t* d_beg, const uint64_t* d_end, uint64_t n,
                  uint64_t nbytes, const uint64_t* d_sorted, const uint8_t* d_status, const uint64_t* d_out_off,
                  uint8_t* d_out, uint64_t cap);

// Raw DEFLATE the other way (sg_deflate.hip; ctx lock held, the device
// ensured), in the same shape.  deflate_count: the exact length and the form
// (0 stored, 1 fixed, 2 dynamic) of every stream's encoding, from
// deflate_ws(n) bytes of the workspace at ws_used; it also sets the context's
// form counts and adds to "deflate_long_streams".  deflate_offsets: scan_counts
// of the lengths (which the caller may have edited: a zero length is a stream
// nobody wants).  deflate_write, with the workspace untouched since the count:
// stream p into d_out[d_out_off[p] + shift[p], d_out_off[p + 1] + shift[p])
// (d_shift null: no shift), clamped to cap, when d_out_off[n] + extra <= cap
// (compared on the device).  n < 2^32; a stream's input is cut at
// kDeflateMaxIn bytes, so that its length fits 32 bits (the host forms reject
// longer ones: deflate_texts_ok).
// "deflate_long_len" reads SG_DEFLATE_LONG.
constexpr uint32_t kDeflateLong = SG_DEFLATE_LONG;
constexpr uint64_t kDeflateMaxIn = (1ull << 32) - (1ull << 20);
size_t deflate_ws(uint64_t n);
int deflate_count(sg_ctx* ctx, const uint8_t* d_in, const uint64_t* d_beg, const uint64_t* d_end, uint64_t n,
                  uint64_t nbytes, uint32_t* d_olen, uint8_t* d_form, size_t ws_used, const uint64_t** d_sorted);
int deflate_offsets(sg_ctx* ctx, const uint32_t* d_olen, uint64_t* d_out_off, uint64_t n, size_t ws_used);
int deflate_write(sg_ctx* ctx, const uint8_t* d_in, const uint64_t* d_beg, const uint64_t* d_end, uint64_t n,
                  uint64_t nbytes, const uint64_t* d_sorted, const uint64_t* d_out_off, const uint64_t* d_shift,
                  uint64_t extra, uint8_t* d_out, uint64_t cap);
int deflate_texts_ok(const char* fn, const uint8_t* in, const uint64_t* in_off, size_t n);

}  // namespace sg

// ---- device helpers -------------------------------------------------------
namespace sgd {

// Layout of a set's 2^32-bit bitmap: signal s = bytes (b3 b2 b1 b0) is bit
// set_pos(s) = (b2 b1 b3 b0).  The low 5 bits are s's own, so this is a fixed
// permutation of 32-bit words; 8 consecutive words (256 signals, one b0 range)
// stay together.  It makes the 2^16 signals of one (b2, b1) -- the partitioned
// triage's bucket (sg_bucket.hip) -- one contiguous 8 KiB slice: the raw top
// byte of an edge signal is the top byte of hash(prev PC) and would pile the
// edges of the hottest PCs into a few buckets.  Export walks the words in s
// order (sg_set.hip), so members still come out ascending.
__host__ __device__ __forceinline__ uint32_t set_pos(uint32_t s) {
  return ((s & 0x00FFFF00u) << 8) | ((s >> 16) & 0xFF00u) | (s & 0xFFu);
}
__host__ __device__ __forceinline__ uint32_t set_sig(uint32_t p) {  // inverse of set_pos
  return ((p & 0xFF00u) << 16) | ((p >> 8) & 0x00FFFF00u) | (p & 0xFFu);
}
// word of the bitmap holding s-order word ws (= s >> 5)
__host__ __device__ __forceinline__ uint32_t set_word(uint32_t ws) {
  return (((ws >> 3) & 0xFFFFu) << 11) | ((ws >> 19) << 3) | (ws & 7u);
}
// The executor's edge hash (executor/executor.h:497-505): an edge's signal
// is pc ^ hash(previous pc of the call), 0 before the call's first pc
// (executor.h:392-396).
__host__ __device__ __forceinline__ uint32_t exec_hash(uint32_t a) {
  a = (a ^ 61) ^ (a >> 16);
  a = a + (a << 3);
  a = a ^ (a >> 4);
  a = a * 0x27d4eb2du;
  a = a ^ (a >> 15);
  return a;
}

__device__ __forceinline__ bool test_bit(const uint32_t* words, uint32_t s) {
  return (words[set_pos(s) >> 5] >> (s & 31)) & 1u;
}
__device__ __forceinline__ void set_bit(uint32_t* words, uint32_t s) {
  atomicOr(&words[set_pos(s) >> 5], 1u << (s & 31));
}

// List i of a CSR over `total` members, clamped to them: r0 <= r1 <= total
// whatever off holds.  A device form's offsets are checked by nobody, and this
// is what keeps it inside its buffers.
__device__ __forceinline__ void csr_range(const uint64_t* off, uint64_t i, uint64_t total, uint64_t& r0,
                                          uint64_t& r1) {
  r0 = min(off[i], total);
  r1 = min(max(off[i + 1], r0), total);
}

// kcov_comparison_t::write's extension of an operand (executor/executor.h:632-645)
__device__ __forceinline__ uint64_t kcov_extend(uint64_t typ, uint64_t x) {
  switch (typ & 6) {
    case 0:
      return (uint64_t)(int64_t)(int8_t)x;
    case 2:
      return (uint64_t)(int64_t)(int16_t)x;
    case 4:
      return (uint64_t)(int64_t)(int32_t)x;
  }
  return x;
}

// The first j in [0, n] with a[j] >= v (lb64) or a[j] > v (ub64), a ascending.
// The interval halves on every iteration whatever the array holds, sorted or
// not, so either loop ends within 64 steps without a counter of its own.
__device__ __forceinline__ uint64_t lb64(const uint64_t* a, uint64_t n, uint64_t v) {
  uint64_t lo = 0, hi = n;
  while (lo < hi) {
    uint64_t mid = (lo + hi) >> 1;
    if (a[mid] < v)
      lo = mid + 1;
    else
      hi = mid;
  }
  return lo;
}
__device__ __forceinline__ uint64_t ub64(const uint64_t* a, uint64_t n, uint64_t v) {
  uint64_t lo = 0, hi = n;
  while (lo < hi) {
    uint64_t mid = (lo + hi) >> 1;
    if (a[mid] <= v)
      lo = mid + 1;
    else
      hi = mid;
  }
  return lo;
}

// largest r in [lo, hi] with off[r] <= i (off non-decreasing), searched in
// `off` (global or LDS pointer): among equal offsets the last one, and lo
// itself when i is below off[lo] (off[lo] is never read).
template <typename P>
__device__ __forceinline__ uint64_t seg_search(P off, uint64_t lo, uint64_t hi, uint64_t i) {
  while (lo < hi) {
    uint64_t mid = lo + (hi - lo + 1) / 2;
    if (off[mid] <= i)
      lo = mid;
    else
      hi = mid - 1;
  }
  return lo;
}

// Inclusive wave64 scans through DPP: row shifts within the 16-lane rows,
// then the row broadcasts of lanes 15 and 31 (no LDS-crossbar shuffles; the
// per-tile scans of the partition and merge kernels run on one wave while
// the others wait at a barrier).  Both need the full wave: a lane that has
// exited hands its neighbours 0 (add) or -1 (max) instead of its partial
// result, so every caller keeps all 64 lanes to the call, idle ones with 0 / -1.
__device__ __forceinline__ uint32_t wave_incl_add(uint32_t x) {
  x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x111, 0xF, 0xF, false);  // row_shr:1
  x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x112, 0xF, 0xF, false);  // row_shr:2
  x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x114, 0xF, 0xF, false);  // row_shr:4
  x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x118, 0xF, 0xF, false);  // row_shr:8
  x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x142, 0xA, 0xF, false);  // row_bcast:15
  x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x143, 0xC, 0xF, false);  // row_bcast:31
  return x;
}

// the same for max over values >= -1 (-1: nothing yet)
__device__ __forceinline__ int wave_incl_max(int x) {
  x = max(x, __builtin_amdgcn_update_dpp(-1, x, 0x111, 0xF, 0xF, false));
  x = max(x, __builtin_amdgcn_update_dpp(-1, x, 0x112, 0xF, 0xF, false));
  x = max(x, __builtin_amdgcn_update_dpp(-1, x, 0x114, 0xF, 0xF, false));
  x = max(x, __builtin_amdgcn_update_dpp(-1, x, 0x118, 0xF, 0xF, false));
  x = max(x, __builtin_amdgcn_update_dpp(-1, x, 0x142, 0xA, 0xF, false));
  x = max(x, __builtin_amdgcn_update_dpp(-1, x, 0x143, 0xC, 0xF, false));
  return x;
}

}  // namespace sgd
