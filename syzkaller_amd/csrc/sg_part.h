// sg_part.h -- the contract between the stages of the partitioned new-signal
// triage (internal to sg_partition / sg_bucket / sg_m0filter / sg_part_triage
// / sg_prefix .hip; the rest of the library sees sg_internal.h): geometry,
// entry layouts, the workspace plan and the stages' entry points.
//
// The partitioned triage is the fast path of
// sg_triage_batch when the caller does not ask for the ordered diff lists).
//
// Reference: syz-fuzzer/fuzzer.go:645-693.  Its observable results are which
// call records get queued for triage (fuzzer.go:678-690) and the updated
// maxSignal / newSignal (fuzzer.go:673-674); the diff slice (fuzzer.go:669)
// is a transient that only feeds those SignalAdd calls.
//
// Same first-owner rule as sg_triage.hip: a record is new iff it is the
// first, in sequential order, to contain some signal s not in maxSignal.
// Owners are minima over record indices, so the order of entries inside a
// partition never matters; what has to travel with each entry is its record.
// Every stream here is 4 bytes per signal entry:
//
//   tiles   the batch is cut into pass-1 tiles of <= kPT entries that span
//           <= kRecCap records (cuts at every kPT-th entry and at every
//           kRecCap-th record offset), so an entry's record is
//           trec[tile] + an 8-bit in-tile index;
//   groups  records in runs of 2^16 (group g = records [g << 16, +2^16));
//           every group boundary is a kRecCap-th record offset, hence a
//           tile cut, so a group is a run of whole tiles [gt[g], gt[g+1]);
//   pass 1  partition by the top byte of s (256 slices of 2^24 signals):
//           entry = s << 8 | rec_in_tile, runs laid out [slice][tile];
//   pass 2  per (slice, group), cut into chunks of <= kPT entries;
//           partition by bits 16..23 of s: entry = (s & 0xFFFF) << 16 |
//           record_in_group, runs laid out [byte][chunk];
//   bucket  one workgroup per 2^16-signal bucket (d, f): its 8 KiB maxSignal
//           slice in LDS is the new-signal test; a candidate (s not in
//           maxSignal) at bucket position i has record (group(i) << 16) |
//           (entry & 0xFFFF), group(i) from the bucket's group boundaries,
//           and goes into an LDS hash map s -> min(record).  The
//           bucket's new bits go back to maxSignal / newSignal from their
//           only writer.  Buckets whose distinct candidates overflow the map
//           are redone by a direct-table kernel.
// Each partition pass = a byte histogram per tile (LDS counters) + a device
// exclusive scan + a scatter (tile in registers, LDS counting-rank, staged
// by digit, written in digit runs).  No global atomics on the data path, no
// random HBM access, no 16 GiB owner table.
//   M0 filter (low-novelty batches, sg_m0filter.hip): between pass 1 and
//           pass 2, each slice's run tested against a packed index of the
//           slice's maxSignal in LDS; only the survivors go on, to a small
//           exact tail, and pass 2 and the bucket stage do not run.
#pragma once

#include <algorithm>

#include "sg_internal.h"

namespace sg {

#ifndef SG_PT
#define SG_PT 16384
#endif
#ifndef SG_PTHREADS
#define SG_PTHREADS 1024
#endif
constexpr int kPT = SG_PT;                   // entries per partition tile / chunk
constexpr int kPThreads = SG_PTHREADS;       // 16 waves
// Partition key.  The passes and buckets work on t = set_pos(s), the
// position of s in a set's bitmap (sg_internal.h): bytes (b2 b1 b3 b0) of
// s = (b3 b2 b1 b0).  Pass 1 partitions by b2, pass 2 by b1, and a bucket
// holds the 2^16 signals of one (b2, b1): bitmap words [b << 11, +2048), its
// LDS slice bit for t is t & 0xFFFF.
// Entry layouts.  Pass 1: t << 8 | record-in-tile (kRecCap records per tile
// at most).  Pass 2: (t & 0xFFFF) << 16 | record-in-group.
constexpr uint32_t kRecCap = 256;              // records per pass-1 tile
constexpr uint32_t kGroupBits = 16;
constexpr uint32_t kGroupRecs = 1u << kGroupBits;  // records per group
constexpr uint32_t kMaxGroups = 256;           // groups per launch (larger batches run in record slices)
static_assert(kGroupRecs % kRecCap == 0, "group boundaries must be tile cuts");
constexpr uint32_t kNumBuckets = 1u << 16;   // (top byte, second byte) of s
constexpr uint32_t kBucketWords = 2048;      // 2^16 signals
static_assert(kMaxLaunchRecords == (uint64_t)kMaxGroups * kGroupRecs, "records per partitioned launch");

__host__ __device__ __forceinline__ uint32_t part_key(uint32_t s) { return sgd::set_pos(s); }
__host__ __device__ __forceinline__ uint32_t part_sig(uint32_t t) { return sgd::set_sig(t); }
__host__ __device__ __forceinline__ uint32_t p1_digit(uint32_t s) { return (s >> 16) & 0xFFu; }  // part_key(s) >> 24
// maxSignal word holding bucket b's LDS slice word j
__host__ __device__ __forceinline__ uint64_t bucket_word(uint32_t b, uint32_t j) {
  return ((uint64_t)b << 11) | j;
}

typedef uint32_t v4u32 __attribute__((ext_vector_type(4)));
// a wave-uniform value: kept in a scalar register
__device__ __forceinline__ uint32_t uni(uint32_t v) { return __builtin_amdgcn_readfirstlane(v); }

// last t in [lo, hi) with row[t] <= x (row non-decreasing, row[lo] <= x)
__device__ __forceinline__ uint32_t last_le(const uint32_t* row, uint32_t lo, uint32_t hi, uint32_t x) {
  while (hi - lo > 1) {
    const uint32_t mid = (lo + hi) >> 1;
    if (row[mid] <= x)
      lo = mid;
    else
      hi = mid;
  }
  return lo;
}

// Record-flag summary of a split launch: one bit per block of kFsRecs
// consecutive records of the launch, set iff every existing record of the block
// was flagged when k_flag_summary ran between the two bucket launches.
// Nothing clears a flag within a call, so a store to such a record would
// rewrite a 1: the second launch (kSkip) and the direct-table kernel leave it
// out.  At the launch maximum of 2^24 records the summary is 512 B.
// When every block's bit is set (the count of set bits equals the launch's
// blocks), no flag store is left at all and the second launch's work is the
// set update alone: k_bucket_sets takes it, without the owner map.
constexpr uint32_t kFsBits = 12, kFsRecs = 1u << kFsBits;
constexpr uint32_t kFsWords = (uint32_t)(kMaxLaunchRecords >> kFsBits) / 32;
static_assert(kFsWords * 32ull * kFsRecs == kMaxLaunchRecords, "summary covers a launch's records");

// Entries per launch above which a batch is cut into record slices: about one
// C2 batch.  Twice that makes the (b2, b1) buckets twice as large, and a
// tenth of them overflow the LDS candidate map into the slow spill kernel.
constexpr uint64_t kSliceEntries = 1ull << 30;

// The record slices of a batch: <= max_launch_recs records and <=
// kSliceEntries entries each (unless one record alone holds more).
struct RecSlice {
  uint64_t r0, r1, e0, e1;
};

// Workspace of one partitioned launch over n entries / nrec records: the
// regions in the order they are laid out (sg_partition.hip gives their sizes).
enum Region : int {
  kTS, kTR, kGT,       // pass-1 tiles: starts (T + 1), first records; each record group's first tile (NG + 1)
  kH1, kO1, kV1, kB1,  // pass 1: histogram [slice][tile], its scan (the run starts), entries, their top bytes
  kNC, kCB,            // chunks per slice-group, their scan ([ng] = the number of pass-2 chunks)
  kCS, kCG, kCF,       // chunk starts, chunk slice-groups, each slice's first chunk (257)
  kCD, kDT,            // per pass-2 block: chunk descriptor, tile range
  kBD, kGB,            // buckets: descriptors {lo, hi, c0, nch}, group boundaries [bucket][group]
  kH2, kO2, kV2,       // pass 2: histogram [byte][chunk], its scan, entries
  kSP, kTK,            // spilled buckets (count, list); four ticket words (a split launch's phases: 0, 1 and, map-free, 2, 3), the late pass 2's bounds (kLate*) + record-flag summary
  kBN, kBP,            // bucket non-empty flags, their scan ([kNumBuckets] = the list's length)
  kLB, kLQ,            // the non-empty buckets in bucket order, and their descriptors
  kSC, kKM,            // scan32's block sums; trace batches' kept-entry words
  kRegions
};
static_assert(kRegions <= sizeof(WsPlan::off) / sizeof(size_t), "the plan's regions fit WsPlan");

// A split launch whose pass 2 runs late (option flag_skip_u16; the flags
// path of bucket_triage_one alone).  The first window of the bucket list is
// its first *nlist >> k entries, as in every split launch; pass 2 works per
// (slice, group) chunk, so the partition's boundary is rounded up to the
// slice: with D the slice after the window's last bucket (0: the window is
// empty), the chunks of slices < D are scattered before the first bucket
// launch, in 4-byte entries, those of slices >= D after the flag summary --
// in 2-byte entries, the 16-bit signal alone, when every record is flagged
// (k_p2_scatter16, k_bucket_sets<true>), else in 4-byte entries
// (k_p2_scatter, k_bucket<.., kSkip>).  A 2-byte entry stands at byte
// 2 * position of the pass-2 buffer, so the bucket descriptors serve both
// widths.  The rest of slice D - 1 past the first window is in 4-byte entries
// either way (k_bucket_sets<false> over it).  With every bucket non-empty (a
// C2 batch) D = 256 >> k and that rest is empty.
// The two device words that say where the boundary lies, after the four
// tickets of kTK: the list position of slice D's first bucket, and the number
// of chunks of the slices < D (k_late_bounds, sg_bucket.hip).
enum : uint32_t { kLateList = 4, kLateChunks = 5, kTkWords = 8 };
struct P2Late {
  int win;                 // 1: the chunks of slices < D, 2: the others
  bool u16;                // win 2: the 2-byte form
  const uint32_t* bounds;  // the launch's kTK words
  const uint32_t* fs_cnt;  // win 2: the summary's full blocks against the launch's: all-flagged iff equal
  uint32_t fs_nblk;
  uint32_t* fs_u16;        // "flag_skip_u16"
};

// A BucketPlan's pass-2 output (kV2) holds 4-byte entries, (t & 0xFFFF) << 16
// | record-in-group, for every caller that keeps or reuses a partition: the
// two-phase protocol and the pipelined loop (sg_prefix.hip), the ordered
// outputs, the emitting bucket forms, the M0-filter regime's fallback and the
// trace entry's front stage run partition_pass2 whole, before any flag exists.
// Only a late pass 2 (P2Late) leaves 2-byte entries there, and only in a
// window that k_bucket_sets<true> then reads: nothing else sees them, and an
// all-flagged window cannot spill, so k_bucket_direct reads 4-byte entries.
struct BucketPlan {
  uint64_t n, nrec, nA, nB, T, NG, ng, gmax;
  WsPlan p;         // offsets from the plan's start, indexed by Region
  size_t base = 0;  // the plan's start in the workspace
  BucketPlan(uint64_t n_, uint64_t nrec_);
  void rebase(size_t b) { base += b; }
  template <typename E>
  E* at(sg_ctx* ctx, Region r) const { return (E*)ws_at(ctx, base + p.off[r]); }
};

// ---- the stages' entry points (ctx lock held) ----
// sg_partition.hip.  One launch's partition in the workspace from ws_base
// (reserved by the caller when `reserved`); bp.n > 0, bp.nrec > 0.  pass1
// validates, reserves and rebases bp, then the tiles and pass 1 (plane: with
// the pass-2 digit plane).  pass2, with bp as pass 1 left it: the chunks,
// pass 2, the bucket tables and the list of non-empty buckets (plane false:
// first the digit plane that pass 1 left out).  partition_one: both.
int partition_pass1(sg_ctx* ctx, const uint32_t* d_vals, const uint64_t* d_off, size_t ws_base, bool reserved,
                    BucketPlan& bp, bool trace, bool plane);
int partition_pass2(sg_ctx* ctx, const BucketPlan& bp, bool plane = true);
// pass 2 in its parts, for a late pass 2: the chunk tables, byte histogram and
// scan; the bucket tables and list (they need the scan alone); the chunk
// descriptors again, the blocks of each window contiguous; one window's scatter
int partition_pass2_tables(sg_ctx* ctx, const BucketPlan& bp, bool plane);
int partition_pass2_buckets(sg_ctx* ctx, const BucketPlan& bp);
int partition_pass2_windows(sg_ctx* ctx, const BucketPlan& bp, const uint32_t* bounds);
int partition_pass2_scatter(sg_ctx* ctx, const BucketPlan& bp, const P2Late* late);
int partition_one(sg_ctx* ctx, const uint32_t* d_vals, const uint64_t* d_off, size_t ws_base, bool reserved,
                  BucketPlan& bp, bool trace = false);
// sg_bucket.hip
// split: -1 by the regime, else buckets_split's answer for this launch; 2 = pass 2 stopped after
// partition_pass2_buckets, and the scatters run here, around the first bucket launch
int buckets_one(sg_ctx* ctx, const BucketPlan& bp, uint32_t* mwords, uint32_t* nwords, uint8_t* d_rec_new,
                const EmitArgs* emit, const uint32_t* owords = nullptr, int split = -1);
// the flags path's bucket stage for this launch: 0 one launch, 1 split, 2 split with a late pass 2
int buckets_split(sg_ctx* ctx, const BucketPlan& bp, const uint8_t* d_rec_new, bool late_ok);
// sg_m0filter.hip: the filter over pass 1's output, and its regime
int m0_filter(sg_ctx* ctx, const BucketPlan& bp, uint32_t* mwords, uint32_t* nwords, uint8_t* d_rec_new, bool* done);
bool m0f_try(sg_ctx* ctx);
void m0f_poll(sg_ctx* ctx);
int m0f_note_partitioned(sg_ctx* ctx, const uint8_t* d_rec_new, uint64_t nrec);
int m0f_host_alloc(sg_ctx* ctx);
// sg_part_triage.hip
int record_slices(sg_ctx* ctx, const uint64_t* d_off, uint64_t nrec, std::vector<RecSlice>& out,
                  uint64_t lim = kSliceEntries);
int bucket_triage_one(sg_ctx* ctx, uint32_t* mwords, uint32_t* nwords, const uint32_t* d_vals, const uint64_t* d_off,
                      uint64_t n, uint64_t nrec, uint8_t* d_rec_new, const EmitArgs* emit = nullptr, size_t ws_base = 0,
                      bool trace = false);

}  // namespace sg
