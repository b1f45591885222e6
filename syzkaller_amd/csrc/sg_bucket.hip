// sg_bucket.hip -- the bucket stage of the partitioned triage (sg_part.h):
// one workgroup per 2^16-signal bucket of the partition's output, in its
// flagging, pair-emitting and update-emitting forms, and the direct-table
// kernel for the buckets that overflow the candidate map.
#include "sg_part.h"

namespace sg {

#ifndef SG_BTHREADS
#define SG_BTHREADS 512
#endif
constexpr int kBThreads = SG_BTHREADS;     // bucket-kernel workgroup
constexpr int kBWaves = kBThreads == 512 ? 6 : 8;  // waves per SIMD it is built for
constexpr int kBU = 4;                       // entries per thread per round in the bucket kernel
constexpr uint32_t kHash = 8192;             // candidate map slots per bucket (32 bits each, see map_insert)
constexpr uint32_t kMaxProbe = 31;           // linear-probe cap before a bucket spills
constexpr uint32_t kEmpty = 0xFFFFFFFFu;

// ---------------------------------------------------------------- bucket ---
struct BucketArgs {
  const uint32_t* in;      // pass-2 output
  const uint4* bdesc;      // per-bucket {lo, hi, c0, nch}
  const uint32_t* gbnd;    // [bucket][group]: first bucket position of each group's entries
  uint32_t NG;             // groups
  uint32_t* mwords;        // maxSignal
  const uint32_t* owords;  // nullable: the test is against mwords | owords (words that gain bits get both)
  uint32_t* nwords;        // newSignal (nullable)
  uint8_t* rec_new;        // per record: owns some new signal
  uint32_t* spill;         // buckets left for the direct-table kernel
  uint32_t* nspill;
  uint32_t* ticket;        // persistent bucket kernel: list entries handed out past 2 x grid
  const uint32_t* blist_b; // non-empty buckets, in bucket order ...
  const uint4* blist_q;    // ... and their descriptors
  const uint32_t* nlist;   // device: their number
  // the list window of a split launch (flag_skip): with A = *nlist >> win_shift,
  // win 1 takes entries [0, A), win 2 [A, *nlist), 0 all of them
  // with a late pass 2 (P2Late, sg_part.h) and B = bounds[kLateList] >= A: win 3 takes [A, B), the 4-byte rest of
  // the boundary slice, win 4 [B, *nlist), the slices scattered after the summary
  uint32_t win, win_shift;
  const uint32_t* bounds;  // the launch's kTK words (win 3, 4)
  const uint32_t* fsum;    // nullable: bit per kFsRecs records of the launch, set: every flag of the block is set already
  // the second phase of a split launch: all-flagged iff *fs_cnt (the summary's full blocks) == fs_nblk (the
  // launch's blocks); then k_bucket_sets takes window 2 and counts itself in *fs_all, else k_bucket<.., kSkip>
  const uint32_t* fs_cnt;
  uint32_t fs_nblk;
  uint32_t* fs_all;
  uint64_t* dbg;          // diagnostics (k_bucket<true>): per block {start, end, buckets, rounds, 4 phase cycle sums}
  // candidate emission (sharded triage, sg_shard.hip; the prefix protocol's
  // begin): instead of flagging records and updating maxSignal, every
  // distinct candidate s of the batch is written once, with its first
  // record, as {s, rec_base + record}, and set in nwords when that is given
  uint2* pairs;
  unsigned long long* npairs;
  uint32_t rec_base;
  uint32_t nshards;         // pairs are counted per owning shard (shard_of) ...
  unsigned long long* shard_cnt;  // ... when this is given
  uint32_t update;          // emitting form that also updates mwords / nwords (the ordered outputs) ...
  unsigned long long* gcur; // ... with the pairs group-major: pairs of group g's records appended at
  const uint64_t* goff;     //     goff[g << 16] + gcur[g] (goff: the launch's record offsets; a group's
};                          //     pairs never outnumber its entries)

// Owning shard of a signal in the hash-sharded multi-GPU triage: the murmur3
// finaliser of s, scaled to [0, nshards).
__device__ __forceinline__ uint32_t shard_of(uint32_t s, uint32_t nshards) {
  s ^= s >> 16;
  s *= 0x85EBCA6Bu;
  s ^= s >> 13;
  s *= 0xC2B2AE35u;
  s ^= s >> 16;
  return (uint32_t)(((uint64_t)s * nshards) >> 32);
}

constexpr uint32_t kMaxShards = 64;

// Block-aggregated append of up to kPer pairs per lane (valid where rec !=
// kEmpty): one global atomic per call and block (a per-wave atomic on the one
// pair counter was the emitting launch's bottleneck); each pair is also
// counted in the block's LDS shard counters.  Called by every thread.
template <int kPer>
__device__ __forceinline__ void emit_pairs(const BucketArgs& a, const uint32_t (&sig)[kPer], const uint32_t (&rec)[kPer],
                                           uint32_t* shcnt) {
  constexpr uint32_t kNone = 0xFFFFFFFFu;
  __shared__ uint32_t ewc[16];  // per-wave totals, then offsets (<= 1024 threads)
  __shared__ unsigned long long ebase;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, nw = blockDim.x >> 6;
  uint32_t c = 0;
#pragma unroll
  for (int k = 0; k < kPer; k++) c += rec[k] != kNone ? 1u : 0u;
  uint32_t incl = c;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const uint32_t y = __shfl_up(incl, o);
    if (lane >= o) incl += y;
  }
  if (lane == 63) ewc[w] = incl;
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t acc = 0;
    for (int i = 0; i < nw; i++) {
      const uint32_t v = ewc[i];
      ewc[i] = acc;
      acc += v;
    }
    ebase = acc ? atomicAdd(a.npairs, (unsigned long long)acc) : 0ull;
  }
  __syncthreads();
  uint64_t pos = ebase + ewc[w] + incl - c;
#pragma unroll
  for (int k = 0; k < kPer; k++)
    if (rec[k] != kNone) {
      a.pairs[pos++] = make_uint2(sig[k], a.rec_base + rec[k]);
      if (a.shard_cnt) atomicAdd(&shcnt[shard_of(sig[k], a.nshards)], 1u);
    }
  __syncthreads();  // ewc / ebase are rewritten by the next call
}

// Group-major append (the ordered outputs): up to kPer pairs per thread
// (valid where rec != kEmpty), counted per record group in LDS, one global
// cursor atomic per group and call, then placed.  Order within a group is
// free: the pairs are sorted by record afterwards.  lcnt (LDS, kMaxGroups
// words) is zero on entry and on exit.  Called by every thread.
template <int kPer>
__device__ __forceinline__ void emit_grouped(const BucketArgs& a, const uint32_t (&sig)[kPer], const uint32_t (&rec)[kPer],
                                             uint32_t* lcnt, unsigned long long* lbase) {
  constexpr uint32_t kNone = 0xFFFFFFFFu;
#pragma unroll
  for (int k = 0; k < kPer; k++)
    if (rec[k] != kNone) atomicAdd(&lcnt[rec[k] >> kGroupBits], 1u);
  __syncthreads();
  for (uint32_t g = threadIdx.x; g < a.NG; g += blockDim.x) {
    const uint32_t c = lcnt[g];
    lbase[g] = c ? a.goff[(uint64_t)g << kGroupBits] + atomicAdd(&a.gcur[g], (unsigned long long)c) : 0ull;
    lcnt[g] = 0;
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < kPer; k++)
    if (rec[k] != kNone) {
      const uint32_t g = rec[k] >> kGroupBits;
      a.pairs[lbase[g] + atomicAdd(&lcnt[g], 1u)] = make_uint2(sig[k], rec[k]);
    }
  __syncthreads();
  for (uint32_t g = threadIdx.x; g < a.NG; g += blockDim.x) lcnt[g] = 0;
  __syncthreads();
}

__device__ __forceinline__ void flush_shard_counts(const BucketArgs& a, const uint32_t* shcnt) {
  if (a.shard_cnt)
    for (uint32_t i = threadIdx.x; i < a.nshards; i += blockDim.x)
      if (shcnt[i]) atomicAdd(&a.shard_cnt[i], (unsigned long long)shcnt[i]);
}

// group of bucket position p >= gb[0]: last g < NG with gb[g] <= p
__device__ __forceinline__ uint32_t group_of(const uint32_t* gb, uint32_t NG, uint32_t p) {
  uint32_t lo = 0, hi = NG;
  while (hi - lo > 1) {
    const uint32_t mid = (lo + hi) >> 1;
    if (gb[mid] <= p)
      lo = mid;
    else
      hi = mid;
  }
  return lo;
}

// Record of the candidate entry x at a bucket position of group g.  Records
// are what the first-owner rule takes the minimum of (fuzzer.go:665 order).
__device__ __forceinline__ uint32_t entry_record(uint32_t g, uint32_t x) { return (g << kGroupBits) | (x & 0xFFFFu); }

// Persistent: each workgroup takes buckets one after another (the first one
// by its index, then by ticket) and runs through them as one stream of
// rounds of kBU entries per thread.  Per round and thread: the LDS
// new-signal test of its kBU entries, then each candidate's record (group by
// a search over the bucket's group boundaries in LDS) inserted into the map.
// Rounds have no barrier: the waves of a workgroup meet only at bucket ends.
// While a round is processed the thread's next one is in flight -- the same
// bucket's next round, or the next bucket's first round together with its
// maxSignal slice and group boundaries.  The ticket after that is fetched a
// bucket ahead, so no dependent load is exposed.
constexpr uint32_t kGroupWords = (kMaxGroups + kBThreads - 1) / kBThreads;  // group boundaries per thread
constexpr int kWPT = kBucketWords / kBThreads;  // LDS slice words per thread
typedef uint32_t wvec __attribute__((ext_vector_type(kWPT)));
struct BucketPre {  // a bucket's first loads, held in registers
  uint32_t msw[kBucketWords / kBThreads];
  uint32_t nsw[kBucketWords / kBThreads];  // newSignal words (only this block writes them)
  uint32_t gw[kGroupWords];                // group boundaries
};

// Rounds start 4-aligned (the bucket start rounded down): thread t holds
// entries base + kBU t .. + kBU - 1 as 16-B loads (immediate offsets, one
// address); entry i is live iff lo <= i < hi.  The pass-2 buffer is padded,
// so the quad reads past hi stay in bounds.
__device__ __forceinline__ uint32_t round_pos(uint32_t base, int u) { return base + threadIdx.x * kBU + u; }

__device__ __forceinline__ void bucket_round_load(const BucketArgs& a, uint32_t base, uint32_t hi,
                                                  uint32_t (&x)[kBU]) {
  const uint4* p = reinterpret_cast<const uint4*>(a.in + base) + threadIdx.x * (kBU / 4);
#pragma unroll
  for (int j = 0; j < kBU / 4; j++) {
    // non-temporal: the streamed entries would otherwise push the record-flag
    // lines out of L2 (measured: 1.9 -> 1.27 GB of writes per launch)
    uint4 v = make_uint4(0, 0, 0, 0);
    if (round_pos(base, 4 * j) < hi) {
      const v4u32 t = __builtin_nontemporal_load(reinterpret_cast<const v4u32*>(p + j));
      v = make_uint4(t[0], t[1], t[2], t[3]);
    }
    x[4 * j] = v.x;
    x[4 * j + 1] = v.y;
    x[4 * j + 2] = v.z;
    x[4 * j + 3] = v.w;
  }
}

__device__ __forceinline__ void bucket_pre_load(const BucketArgs& a, uint32_t b, BucketPre& P) {
  // LDS slice words kWPT tid .. + kWPT - 1
  const uint64_t w0 = bucket_word(b, kWPT * threadIdx.x);
  wvec m = *reinterpret_cast<const wvec*>(a.mwords + w0);
  if (a.owords) m |= *reinterpret_cast<const wvec*>(a.owords + w0);
  wvec nw = {};
  if (a.nwords) nw = *reinterpret_cast<const wvec*>(a.nwords + w0);
#pragma unroll
  for (int j = 0; j < kWPT; j++) {
    P.msw[j] = m[j];
    P.nsw[j] = nw[j];
  }
  const uint32_t* gr = a.gbnd + (uint64_t)b * a.NG;
#pragma unroll
  for (int j = 0; j < (int)kGroupWords; j++) {
    const uint32_t i = j * kBThreads + threadIdx.x;
    P.gw[j] = i < a.NG ? gr[i] : 0u;
  }
}

// the list window [l0, l0 + nl) of the launch (BucketArgs::win)
__device__ __forceinline__ void list_window(const BucketArgs& a, uint32_t& l0, uint32_t& nl) {
  nl = *a.nlist;
  l0 = 0;
  if (!a.win) return;
  const uint32_t na = nl >> a.win_shift;
  if (a.win <= 2) {
    l0 = a.win == 2 ? na : 0;
    nl = a.win == 2 ? nl - na : na;
  } else {
    const uint32_t nb = a.bounds[kLateList];
    l0 = a.win == 3 ? na : nb;
    nl = a.win == 3 ? nb - na : nl - nb;
  }
}

// The bounds of a late pass 2 (sg_part.h): D = the slice after the last bucket
// of the list's first window (0: the window is empty); the list position of
// slice D's first bucket (lpos: the non-empty flags' scan, lpos[kNumBuckets]
// = the list's length) and the first chunk of slice D.
__global__ void k_late_bounds(const uint32_t* __restrict__ lpos, const uint32_t* __restrict__ blist_b,
                              const uint32_t* __restrict__ cfirst, uint32_t shift, uint32_t* __restrict__ tk) {
  const uint32_t na = lpos[kNumBuckets] >> shift;
  const uint32_t D = na ? (blist_b[na - 1] >> 8) + 1 : 0u;
  tk[kLateList] = lpos[D << 8];
  tk[kLateChunks] = cfirst[D];
}

// thread 0: bucket and descriptor of entry t of the list window [l0, l0 + nl)
// (kNumBuckets: past the end)
__device__ __forceinline__ uint32_t list_bucket(const BucketArgs& a, uint32_t t, uint32_t l0, uint32_t nl, uint4* q) {
  if (t >= nl) return kNumBuckets;
  *q = a.blist_q[l0 + t];
  return a.blist_b[l0 + t];
}

// the record-flag summary of a split launch (sg_part.h): is rec's block full
__device__ __forceinline__ bool fs_full(const uint32_t* fs, uint32_t rec) {
  return (fs[rec >> (kFsBits + 5)] >> ((rec >> kFsBits) & 31u)) & 1u;
}

// A wave per block: lane l tests the 16 flags from 1024 j + 16 l, j < 4.
// sum is zero on entry; *nfull counts the bits set.
__global__ __launch_bounds__(256) void k_flag_summary(const uint8_t* __restrict__ rec_new, uint32_t nrec,
                                                      uint32_t* __restrict__ sum, uint32_t* __restrict__ nfull) {
  const uint32_t blk = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (blk >= (nrec + kFsRecs - 1) >> kFsBits) return;  // (per wave)
  bool full = true;
#pragma unroll
  for (int j = 0; j < 4; j++) {
    const uint32_t i = blk * kFsRecs + j * 1024 + lane * 16;
    if (i + 16 <= nrec && ((uintptr_t)(rec_new + i) & 15) == 0) {
      const uint4 v = *reinterpret_cast<const uint4*>(rec_new + i);
      for (uint32_t w : {v.x, v.y, v.z, v.w}) full &= ((w - 0x01010101u) & ~w & 0x80808080u) == 0;  // no zero byte
    } else {
      for (uint32_t k = i; k < i + 16 && k < nrec; k++) full &= rec_new[k] != 0;
    }
  }
  if (__all(full) && lane == 0) {
    atomicOr(&sum[blk >> 5], 1u << (blk & 31));
    atomicAdd(nfull, 1u);
  }
}

// block-uniform values read from LDS: keep them in scalar registers
__device__ __forceinline__ uint4 uni(uint4 v) { return make_uint4(uni(v.x), uni(v.y), uni(v.z), uni(v.w)); }

// The candidate map: kHash = 8192 slots of 32 bits, linear probing.  The
// bucket's 16-bit signal sl goes through a bijection y = sl * kMapMul (mod
// 2^16): home slot = y >> 3, tag = y & 7.  A slot holds
//   tag << 29 | displacement << 24 | record        (record < 2^24 = kMaxGroups << 16)
// so the slot index and its top byte give back sl, and one 32-bit atomicMin
// lowers the record of an equal key.  Displacements stay <= kMaxProbe - 1 =
// 30, so no entry equals kEmpty (displacement field 31).
constexpr uint32_t kMapMul = 0x6F4Bu;  // odd: invertible mod 2^16
constexpr uint32_t inv16(uint32_t c) {
  uint32_t x = c;  // Newton: each step doubles the correct low bits (c * c == 1 mod 8 for odd c)
  for (int i = 0; i < 4; i++) x = (x * (2u - c * x)) & 0xFFFFu;
  return x;
}
constexpr uint32_t kMapInv = inv16(kMapMul);
static_assert(((kMapMul * kMapInv) & 0xFFFFu) == 1u, "kMapInv");
static_assert(kHash == 8192 && kMaxProbe <= 31, "13-bit slots, 5-bit displacements");
static_assert((uint64_t)kMaxGroups << kGroupBits <= (1u << 24), "records fit 24 bits");
constexpr uint32_t kRecMask = 0xFFFFFFu;

__device__ __forceinline__ uint32_t map_signal(uint32_t slot, uint32_t v) {  // sl of an occupied slot
  const uint32_t home = (slot - ((v >> 24) & 31u)) & (kHash - 1);
  return (((home << 3) | (v >> 29)) * kMapInv) & 0xFFFFu;
}

// A first insert is one CAS; a repeat of a signal lowers the record with a
// 32-bit min (equal key bits above the record).
__device__ __forceinline__ bool map_insert(uint32_t* ht, uint32_t sl, uint32_t rec, uint32_t disp0 = 0) {
  const uint32_t y = (sl * kMapMul) & 0xFFFFu;
  const uint32_t home = y >> 3, tag = y & 7u;
  for (uint32_t disp = disp0; disp < kMaxProbe; disp++) {
    const uint32_t mine = (tag << 29) | (disp << 24) | rec;
    uint32_t* slot = &ht[(home + disp) & (kHash - 1)];
    const uint32_t old = atomicCAS(slot, kEmpty, mine);
    if (old == kEmpty) return true;
    if ((old >> 24) == (mine >> 24)) {
      if ((old & kRecMask) > rec) atomicMin(slot, mine);
      return true;
    }
  }
  return false;  // map (nearly) full: the bucket spills
}

// A ticket: a plain atomicAdd, its result read at the next install.  (An
// inline-asm atomic waited for only there measured the same, 2.32-2.34 ms,
// and leaves the compiler unaware that its result register is pending: r05
// removed it.)
__device__ __forceinline__ uint32_t take_ticket(uint32_t* p) { return atomicAdd(p, 1u); }

// kEmit: 0 flags and set updates, 1 candidate pairs (counted per owning
// shard), 2 the ordered outputs' new-signal pairs, group-major, with the set
// updates.  kSkip (kEmit 0, the second launch of a split one): the flush
// leaves out the flag stores of record blocks whose summary bit is set.
template <bool kDbg, int kEmit, bool kSkip = false>
__global__ __launch_bounds__(kBThreads) __attribute__((amdgpu_waves_per_eu(kBWaves))) void k_bucket(BucketArgs a) {
  static_assert(!kSkip || kEmit == 0, "the summary guards flag stores");
  if (kSkip && *a.fs_cnt == a.fs_nblk) return;  // all-flagged: k_bucket_sets has this window
  __shared__ uint32_t fsum[kSkip ? kFsWords : 1];
  __shared__ uint32_t mslice[kBucketWords];
  __shared__ uint32_t nbits[kBucketWords];
  __shared__ uint32_t ht[kHash];
  __shared__ alignas(16) uint32_t gb[kMaxGroups];  // the bucket's group boundaries (kEmpty past NG)
  __shared__ uint32_t sh_fail;         // some insert found the map full: the bucket spills
  __shared__ uint32_t sh_b[2];
  __shared__ uint4 sh_q[2];
  __shared__ uint32_t shcnt[kEmit == 1 ? kMaxShards : 1];  // emitted pairs per owning shard
  __shared__ uint32_t lcnt[kEmit == 2 ? kMaxGroups : 1];    // group-major emission: pairs per record group ...
  __shared__ unsigned long long lbase[kEmit == 2 ? kMaxGroups : 1];  // ... and where they go
  const int tid = threadIdx.x;
  if (kEmit == 1)
    for (uint32_t i = tid; i < kMaxShards; i += kBThreads) shcnt[i] = 0;
  if (kEmit == 2)
    for (uint32_t i = tid; i < kMaxGroups; i += kBThreads) lcnt[i] = 0;
  const uint32_t NG = a.NG;
  constexpr uint32_t kRound = kBThreads * kBU;
  // diagnostics (kDbg): block span, buckets, rounds, cycles per phase as wave 0 sees them
  const uint64_t t_start = kDbg ? wall_clock64() : 0;
  uint64_t n_buckets = 0, n_rounds = 0;
  uint64_t ph[7] = {0, 0, 0, 0, 0, 0, 0};  // install, rounds, -, flush | rounds: test, inserts, -
  uint64_t tk = kDbg ? clock64() : 0;
  for (uint32_t i = tid; i < kHash; i += kBThreads) ht[i] = kEmpty;
  for (uint32_t i = tid; i < kBucketWords; i += kBThreads) nbits[i] = 0;
  if (tid == 0) sh_fail = 0;
  if (kSkip)
    for (uint32_t i = tid; i < kFsWords; i += kBThreads) fsum[i] = a.fsum[i];
  // list entries: blockIdx and gridDim + blockIdx first, then tickets from
  // 2 x gridDim.  Thread 0 takes each ticket a bucket before it resolves it and
  // resolves it a bucket before it is needed, so neither wait is exposed.
  uint32_t nl, l0;
  list_window(a, l0, nl);  // a split launch's window of the list
  // (tickets are taken at every install, also past the list's end: waiting
  // for the list entry before taking the next would be another round trip)
  uint32_t pend_t = 0;  // thread 0: ticket taken, not yet resolved
  if (tid == 0) {
    uint4 q0 = make_uint4(0, 0, 0, 0), q1 = make_uint4(0, 0, 0, 0);
    sh_b[0] = list_bucket(a, blockIdx.x, l0, nl, &q0);
    sh_q[0] = q0;
    sh_b[1] = list_bucket(a, gridDim.x + blockIdx.x, l0, nl, &q1);
    sh_q[1] = q1;
    pend_t = take_ticket(a.ticket);
  }
  __syncthreads();
  uint32_t b = uni(sh_b[0]), b1 = uni(sh_b[1]);
  uint4 q = uni(sh_q[0]), q1 = uni(sh_q[1]);
  if (b >= kNumBuckets) {
    if (kDbg && tid == 0) {
      for (int j = 0; j < 8; j++) a.dbg[8 * blockIdx.x + j] = 0;
      a.dbg[8 * blockIdx.x] = t_start;
      a.dbg[8 * blockIdx.x + 1] = wall_clock64();
    }
    return;
  }
  uint32_t x[kBU], y[kBU];
  BucketPre P;
  bucket_round_load(a, q.x & ~3u, q.y, x);
  bucket_pre_load(a, b, P);
  while (b < kNumBuckets) {
    const uint32_t lo = q.x, hi = q.y;
    // the previous bucket is done with the LDS.  (A barrier that waits for
    // LDS operations only, s_waitcnt lgkmcnt(0) + s_barrier, measured equal:
    // gfx950's __syncthreads does not wait for global loads and stores either.)
    __syncthreads();
    {
      wvec mv;
#pragma unroll
      for (int j = 0; j < kWPT; j++) mv[j] = P.msw[j];
      reinterpret_cast<wvec*>(mslice)[tid] = mv;
    }
    uint32_t ns[kWPT];  // newSignal words kWPT tid .. + kWPT - 1
#pragma unroll
    for (int j = 0; j < kWPT; j++) ns[j] = P.nsw[j];
#pragma unroll
    for (int j = 0; j < (int)kGroupWords; j++) {
      const uint32_t i = j * kBThreads + tid;
      if (i < kMaxGroups) gb[i] = i < NG ? P.gw[j] : kEmpty;
    }
    // thread 0: resolve the pending ticket (published after the rounds) and take the next one
    uint32_t pend_b = kNumBuckets;
    uint4 pend_q = make_uint4(0, 0, 0, 0);
    if (tid == 0) {
      // (pend_t was taken a bucket ago; the install waited for older loads already)
      pend_b = list_bucket(a, 2 * gridDim.x + pend_t, l0, nl, &pend_q);
      pend_t = take_ticket(a.ticket);
      sh_fail = 0;  // (every wave read the previous bucket's before the barrier above)
    }
    __syncthreads();
    const uint32_t gbl = NG <= 64 ? gb[threadIdx.x & 63] : kEmpty;  // boundary of group lane (kEmpty past NG)
    if (kDbg) {
      const uint64_t t = clock64();
      ph[0] += t - tk;
      tk = t;
    }
    n_buckets++;
    // Rounds: no barrier inside -- the waves run through the bucket on their
    // own, meeting only in the map's atomics.
    for (uint32_t base = lo & ~3u;;) {
      n_rounds++;
      // the next round in flight: this bucket's, or the next bucket's first
      // (one load call: separate calls per case load into different
      // registers and their join would wait for them)
      const uint32_t next = base + kRound;
      const bool last = next >= hi;
      if (!last || b1 < kNumBuckets) bucket_round_load(a, last ? q1.x & ~3u : next, last ? q1.y : hi, y);
      if (last && b1 < kNumBuckets) bucket_pre_load(a, b1, P);
      // this thread's kBU consecutive entries: the new-signal test (fuzzer.go:666),
      // all LDS reads issued before the first use
      const uint32_t p0 = round_pos(base, 0);
      // (the spill flag read with the slice words: one LDS wait for both)
      const uint32_t failed = __hip_atomic_load(&sh_fail, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
      uint32_t mw[kBU];
#pragma unroll
      for (int u = 0; u < kBU; u++) mw[u] = mslice[x[u] >> 21];
      uint32_t cm = 0;
#pragma unroll
      for (int u = 0; u < kBU; u++) {
        const uint32_t i = p0 + u;
        const uint32_t miss = ((~mw[u]) >> ((x[u] >> 16) & 31)) & 1u;
        cm |= (miss & (i >= lo ? 1u : 0u) & (i < hi ? 1u : 0u)) << u;
      }
      if (kDbg) {
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        const uint64_t t = clock64();
        ph[4] += t - tk;
        tk = t;
      }
      // (a relaxed atomic read: a volatile one would wait for every load in flight)
      // each entry's group (its record is group << 16 | the entry's low half;
      // entries are in group order).  Up to 64 groups the bucket's
      // boundaries sit one per lane (gbl): the groups before the wave's
      // first position are counted with a ballot, and the (rare) boundaries
      // inside the wave's kBU * 64 positions are stepped over uniformly.
      uint32_t gu[kBU];
      if (NG <= 64) {
        const uint32_t pw = base + (threadIdx.x & ~63u) * kBU;
        // group of p = (boundaries <= p) - 1; positions before the first
        // boundary are outside the bucket (never candidates): clamped to 0
        const uint32_t nle = (uint32_t)__popcll(__ballot(gbl <= pw));
#pragma unroll
        for (int u = 0; u < kBU; u++) gu[u] = nle;
        for (uint64_t c = __ballot(gbl > pw && gbl < pw + 64 * kBU); c; c &= c - 1) {
          const uint32_t bk = __builtin_amdgcn_readlane(gbl, __ffsll((unsigned long long)c) - 1);
#pragma unroll
          for (int u = 0; u < kBU; u++) gu[u] += p0 + u >= bk ? 1u : 0u;
        }
#pragma unroll
        for (int u = 0; u < kBU; u++) gu[u] = gu[u] ? gu[u] - 1 : 0u;
      }
      if (cm && failed == 0) {
        if (NG > 64) {  // the groups by search, stepped forward
          uint32_t g = group_of(gb, NG, p0 + __builtin_ctz(cm));
          uint32_t nb = g + 1 < NG ? gb[g + 1] : kEmpty;  // next boundary
#pragma unroll
          for (int u = 0; u < kBU; u++) {
            if ((cm >> u) & 1u)
              while (nb <= p0 + u) {
                g++;
                nb = g + 1 < NG ? gb[g + 1] : kEmpty;
              }
            gu[u] = g;
          }
        }
        // first probes of the thread's candidates in flight together, four
        // at a time (straight-line, predicated): most land on an empty slot
        // or on their own key; the rest take the probing loop below
        uint32_t slow = 0;
#pragma unroll
        for (int h = 0; h < kBU; h += 4) {
          uint32_t mine[4], old[4];
#pragma unroll
          for (int j = 0; j < 4; j++) {
            const int u = h + j;
            mine[j] = kEmpty;
            old[j] = kEmpty;
            if ((cm >> u) & 1u) {
              const uint32_t y = ((x[u] >> 16) * kMapMul) & 0xFFFFu;
              mine[j] = ((y & 7u) << 29) | entry_record(gu[u], x[u]);
              old[j] = atomicCAS(&ht[y >> 3], kEmpty, mine[j]);
            }
          }
#pragma unroll
          for (int j = 0; j < 4; j++) {
            const int u = h + j;
            if ((cm >> u) & 1u) {
              const uint32_t sl = x[u] >> 16;
              if (old[j] == kEmpty) continue;  // inserted (its new bit is set at the flush)
              if ((old[j] >> 24) == (mine[j] >> 24)) {
                if ((old[j] & kRecMask) > (mine[j] & kRecMask))
                  atomicMin(&ht[((sl * kMapMul) & 0xFFFFu) >> 3], mine[j]);
              } else {
                slow |= 1u << u;
              }
            }
          }
        }
        while (slow) {  // collisions: probe on from displacement 1
          const int u = __builtin_ctz(slow);
          slow &= slow - 1;
          uint32_t xu = x[0], gk = gu[0];
#pragma unroll
          for (int k = 1; k < kBU; k++) {
            xu = k == u ? x[k] : xu;
            gk = k == u ? gu[k] : gk;
          }
          if (!map_insert(ht, xu >> 16, entry_record(gk, xu), 1)) {
            // the others stop inserting (the bucket is redone)
            __hip_atomic_store(&sh_fail, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            break;
          }
        }
      }
      if (kDbg) {
        const uint64_t t = clock64();
        ph[5] += t - tk;
        tk = t;
      }
      if (last) break;
      base = next;
#pragma unroll
      for (int u = 0; u < kBU; u++) x[u] = y[u];
    }
    if (tid == 0) {  // the bucket after next
      sh_b[0] = pend_b;
      sh_q[0] = pend_q;
    }
    if (kDbg) {
      const uint64_t t = clock64();
      ph[1] += t - tk;
      tk = t;
    }
    // (a failing insert stored sh_fail before the barrier: a plain barrier and
    // one LDS read cost less than __syncthreads_or, 2.57 -> 2.43 ms per launch)
    __syncthreads();
    const bool spill = __hip_atomic_load(&sh_fail, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) != 0;
    if (kDbg) {  // the wait for the block's slowest wave
      const uint64_t t = clock64();
      ph[2] += t - tk;
      tk = t;
    }
    if (spill) {  // map full: redo with the direct table (no global writes yet)
      if (tid == 0) a.spill[atomicAdd(a.nspill, 1u)] = b;
      for (uint32_t i = tid; i < kHash; i += kBThreads) ht[i] = kEmpty;
      for (uint32_t i = tid; i < kBucketWords; i += kBThreads) nbits[i] = 0;
    } else if (kEmit == 2) {
      // the ordered outputs: every new signal with its first record,
      // group-major (the slots read twice: counted per group, then placed;
      // order inside a group is free, the pairs are sorted by record later)
      constexpr int kOwn = kHash / kBThreads;
#pragma unroll
      for (int k = 0; k < kOwn; k++) {
        const uint32_t v = ht[k * kBThreads + tid];
        if (v != kEmpty) {
          atomicAdd(&lcnt[(v & kRecMask) >> kGroupBits], 1u);
          const uint32_t sl = map_signal(k * kBThreads + tid, v);
          atomicOr(&nbits[sl >> 5], 1u << (sl & 31));
        }
      }
      __syncthreads();
      for (uint32_t g = tid; g < a.NG; g += kBThreads) {
        const uint32_t c = lcnt[g];
        lbase[g] = c ? a.goff[(uint64_t)g << kGroupBits] + atomicAdd(&a.gcur[g], (unsigned long long)c) : 0ull;
        lcnt[g] = 0;
      }
      __syncthreads();
#pragma unroll
      for (int k = 0; k < kOwn; k++) {
        const uint32_t i = k * kBThreads + tid;
        const uint32_t v = ht[i];
        if (v != kEmpty) {
          const uint32_t r = v & kRecMask, g = r >> kGroupBits;
          a.pairs[lbase[g] + atomicAdd(&lcnt[g], 1u)] = make_uint2(part_sig((b << 16) | map_signal(i, v)), r);
          ht[i] = kEmpty;
        }
      }
      const wvec nb = reinterpret_cast<const wvec*>(nbits)[tid];
      const wvec mw = reinterpret_cast<const wvec*>(mslice)[tid];
      const uint64_t w0 = bucket_word(b, kWPT * tid);
#pragma unroll
      for (int j = 0; j < kWPT; j++)
        if (nb[j]) {
          a.mwords[w0 + j] = mw[j] | nb[j];
          if (a.nwords) a.nwords[w0 + j] = ns[j] | nb[j];
        }
      reinterpret_cast<wvec*>(nbits)[tid] = wvec{};
      __syncthreads();  // (every placement read its lcnt before the reset)
      for (uint32_t g = tid; g < a.NG; g += kBThreads) lcnt[g] = 0;
    } else if (kEmit == 1) {
      // every distinct candidate of the bucket with its first record: the
      // thread's occupied slots counted, one block scan and one global
      // atomic for the bucket's run of pairs, then the slots re-read and
      // written (two barriers per bucket; with the pairs held in registers
      // between two scans, six)
      constexpr int kOwn = kHash / kBThreads;  // slots per thread
      __shared__ uint32_t ewc[kBThreads / 64];
      __shared__ unsigned long long ebase;
      const int lane = tid & 63, w = tid >> 6;
      uint32_t c = 0;
#pragma unroll
      for (int k = 0; k < kOwn; k++) c += ht[k * kBThreads + tid] != kEmpty ? 1u : 0u;
      const uint32_t incl = sgd::wave_incl_add(c);
      if (lane == 63) ewc[w] = incl;
      __syncthreads();
      if (tid == 0) {
        uint32_t acc = 0;
#pragma unroll
        for (int i = 0; i < kBThreads / 64; i++) {
          const uint32_t v = ewc[i];
          ewc[i] = acc;
          acc += v;
        }
        ebase = acc ? atomicAdd(a.npairs, (unsigned long long)acc) : 0ull;
      }
      __syncthreads();
      uint64_t pos = ebase + ewc[w] + incl - c;
      if (c) {
#pragma unroll
        for (int k = 0; k < kOwn; k++) {
          const uint32_t i = k * kBThreads + tid;
          const uint32_t v = ht[i];
          if (v != kEmpty) {
            const uint32_t sl = map_signal(i, v);
            const uint32_t sg = part_sig((b << 16) | sl);
            a.pairs[pos++] = make_uint2(sg, a.rec_base + (v & kRecMask));
            if (a.shard_cnt) atomicAdd(&shcnt[shard_of(sg, a.nshards)], 1u);
            if (a.nwords || a.update) atomicOr(&nbits[sl >> 5], 1u << (sl & 31));
            ht[i] = kEmpty;
          }
        }
      }
      __syncthreads();  // nbits complete; ewc / ebase free for the next bucket
      if (a.update) {  // the candidates are the new signals: words kWPT tid .., this block their only writer
        const wvec nb = reinterpret_cast<const wvec*>(nbits)[tid];
        const wvec mw = reinterpret_cast<const wvec*>(mslice)[tid];
        const uint64_t w0 = bucket_word(b, kWPT * tid);
#pragma unroll
        for (int j = 0; j < kWPT; j++)
          if (nb[j]) {
            a.mwords[w0 + j] = mw[j] | nb[j];
            if (a.nwords) a.nwords[w0 + j] = ns[j] | nb[j];
          }
      } else if (a.nwords) {  // the candidates' bits: words kWPT tid .., written by this block alone
        const wvec nb = reinterpret_cast<const wvec*>(nbits)[tid];
        uint32_t* ng = a.nwords + bucket_word(b, kWPT * tid);
#pragma unroll
        for (int j = 0; j < kWPT; j++)
          if (nb[j]) ng[j] = ns[j] | nb[j];
      }
      reinterpret_cast<wvec*>(nbits)[tid] = wvec{};
    } else {
      // a record is queued iff it owns some signal (fuzzer.go:678-690): its
      // flag is set (a record owns signals in many buckets; all set 1)
      constexpr int kOwn = kHash / kBThreads;  // slots per thread
      // the new-signal bits come from the map here, one pass over the slots
      // with the flag stores (an LDS OR per first insert in the rounds cost
      // more: 2.46 -> 2.34 ms per C2 launch), then the word write-back
      {
#pragma unroll
        for (int k = 0; k < kOwn; k++) {
          const uint32_t i = k * kBThreads + tid;
          const uint32_t v = ht[i];
          ht[i] = kEmpty;
          if (v != kEmpty) {
            const uint32_t sl = map_signal(i, v);
            atomicOr(&nbits[sl >> 5], 1u << (sl & 31));
            if (!kSkip || !fs_full(fsum, v & kRecMask)) a.rec_new[v & kRecMask] = 1;
          }
        }
        __syncthreads();
      }
      {
        // words kWPT tid ..: this block is their only writer
        const uint64_t w0 = bucket_word(b, kWPT * tid);
        uint32_t* mg = a.mwords + w0;
        uint32_t* ng = a.nwords ? a.nwords + w0 : nullptr;
        const wvec nb = reinterpret_cast<const wvec*>(nbits)[tid];
        uint32_t any = 0;
#pragma unroll
        for (int j = 0; j < kWPT; j++) any |= nb[j];
        if (any) {
          const wvec mw = reinterpret_cast<const wvec*>(mslice)[tid];
#pragma unroll
          for (int j = 0; j < kWPT; j++)
            if (nb[j]) {
              mg[j] = mw[j] | nb[j];
              if (ng) ng[j] = ns[j] | nb[j];
            }
          reinterpret_cast<wvec*>(nbits)[tid] = wvec{};
        }
      }
    }
    if (kDbg) {
      const uint64_t t = clock64();
      ph[3] += t - tk;
      tk = t;
    }
    __syncthreads();  // sh_b[0] / sh_q[0] are written
    if (kDbg) {
      const uint64_t t = clock64();
      ph[6] += t - tk;
      tk = t;
    }
    b = b1;
    q = q1;
    b1 = uni(sh_b[0]);
    q1 = uni(sh_q[0]);
#pragma unroll
    for (int u = 0; u < kBU; u++) x[u] = y[u];
  }
  if (kEmit == 1) {
    __syncthreads();
    flush_shard_counts(a, shcnt);
  }
  if (kDbg && tid == 0) {
    a.dbg[8 * blockIdx.x] = t_start;
    a.dbg[8 * blockIdx.x + 1] = wall_clock64();
    a.dbg[8 * blockIdx.x + 2] = n_buckets;
    a.dbg[8 * blockIdx.x + 3] = n_rounds;
    for (int j = 0; j < 4; j++) a.dbg[8 * blockIdx.x + 4 + j] = ph[j];
    a.dbg[8 * gridDim.x + 3 * blockIdx.x] = ph[4];
    a.dbg[8 * gridDim.x + 3 * blockIdx.x + 1] = ph[5];
    a.dbg[8 * gridDim.x + 3 * blockIdx.x + 2] = ph[6];
  }
}

// ------------------------------------------------------------ sets only ---
// The second phase of a split launch whose records are all flagged already
// (sg_part.h): no flag store of the window can change anything, so what is
// left of a bucket is its set update, the bits of its entries that are not in
// mwords | owords.  That needs no owner: no map, no records, no group
// boundaries, and the bucket cannot spill.  Same list, window, tickets and
// entry loads as k_bucket; per bucket the slice and a zeroed new-bits slice in
// LDS, a test and an LDS OR per candidate entry, and the write-back of the
// words that gained bits from their only writer.  Two barriers per bucket:
// after its rounds, and after the write-back that also installs the next
// bucket's slice (a thread owns the same kWPT words of both).
// (The slice read decides the OR.  ORing every live entry and masking at the
// write-back needs no slice in LDS but three times the LDS atomics: measured
// slower, 1.58 against 1.37 ms per C2 bucket stage in alternated runs of one
// job)
// k16: the window's entries are the 2-byte ones of a late pass 2 (sg_part.h),
// the 16-bit signal at byte 2 * position: a 16-B load holds 8 of them, rounds
// start 8-aligned, and nothing is shifted away.
constexpr int kSQ = 2;                           // 16-B loads per thread and round, each contiguous over the workgroup
struct SetsPre {  // a bucket's first loads, held in registers
  uint32_t msw[kWPT];
  uint32_t nsw[kWPT];
};

// entries of a 16-B load, of one of a round's kSQ loads over the workgroup, and of a round
template <bool k16> constexpr uint32_t kSE = k16 ? 8 : 4;
template <bool k16> constexpr uint32_t kSQuad = kBThreads * kSE<k16>;
template <bool k16> constexpr uint32_t kSRound = kSQuad<k16> * kSQ;

template <bool k16>
__device__ __forceinline__ uint32_t sets_pos(uint32_t base, int j) {
  return base + j * kSQuad<k16> + threadIdx.x * kSE<k16>;
}

// (base aligned to a load; a load is issued when its first entry is below hi:
// the padded pass-2 buffer covers the rest of it, as in bucket_round_load)
template <bool k16>
__device__ __forceinline__ void sets_round_load(const BucketArgs& a, uint32_t base, uint32_t hi, v4u32 (&x)[kSQ]) {
#pragma unroll
  for (int j = 0; j < kSQ; j++) {
    x[j] = v4u32{0, 0, 0, 0};
    const uint32_t p = sets_pos<k16>(base, j);
    if (p < hi)
      x[j] = __builtin_nontemporal_load(
          reinterpret_cast<const v4u32*>(reinterpret_cast<const char*>(a.in) + (uint64_t)p * (k16 ? 2 : 4)));
  }
}

// entry u of a load: its slice word and bit
template <bool k16>
__device__ __forceinline__ uint32_t sets_sig(const v4u32& x, int u) {
  return k16 ? (x[u >> 1] >> (16 * (u & 1))) & 0xFFFFu : x[u] >> 16;
}

__device__ __forceinline__ void sets_pre_load(const BucketArgs& a, uint32_t b, SetsPre& P) {
  const uint64_t w0 = bucket_word(b, kWPT * threadIdx.x);
  wvec m = *reinterpret_cast<const wvec*>(a.mwords + w0);
  if (a.owords) m |= *reinterpret_cast<const wvec*>(a.owords + w0);
  wvec nw = {};
  if (a.nwords) nw = *reinterpret_cast<const wvec*>(a.nwords + w0);
#pragma unroll
  for (int j = 0; j < kWPT; j++) {
    P.msw[j] = m[j];
    P.nsw[j] = nw[j];
  }
}

template <bool k16>
__global__ __launch_bounds__(kBThreads) __attribute__((amdgpu_waves_per_eu(8))) void k_bucket_sets(BucketArgs a) {
  if (*a.fs_cnt != a.fs_nblk) return;  // some record is not flagged yet: k_bucket<.., kSkip> has this window
  __shared__ alignas(16) uint32_t mslice[kBucketWords];
  __shared__ alignas(16) uint32_t nbits[kBucketWords];
  __shared__ uint32_t sh_b[2];
  __shared__ uint4 sh_q[2];
  constexpr uint32_t kE = kSE<k16>;
  const int tid = threadIdx.x;
  uint32_t nl, l0;
  list_window(a, l0, nl);
  // list entries and tickets as in k_bucket
  uint32_t pend_t = 0;
  if (tid == 0) {
    uint4 q0 = make_uint4(0, 0, 0, 0), q1 = make_uint4(0, 0, 0, 0);
    sh_b[0] = list_bucket(a, blockIdx.x, l0, nl, &q0);
    sh_q[0] = q0;
    sh_b[1] = list_bucket(a, gridDim.x + blockIdx.x, l0, nl, &q1);
    sh_q[1] = q1;
    pend_t = take_ticket(a.ticket);
    if (blockIdx.x == 0 && a.fs_all) atomicAdd(a.fs_all, 1u);  // "flag_skip_all_flagged" (once per split launch)
  }
  __syncthreads();
  uint32_t b = uni(sh_b[0]), b1 = uni(sh_b[1]);
  uint4 q = uni(sh_q[0]), q1 = uni(sh_q[1]);
  if (b >= kNumBuckets) return;
  v4u32 x[kSQ], y[kSQ];
  SetsPre P;
  sets_round_load<k16>(a, q.x & ~(kE - 1), q.y, x);
  sets_pre_load(a, b, P);
  // the bucket's words kWPT tid .. + kWPT - 1: mwords | owords into the slice (read back at the bucket's end),
  // newSignal's held in registers
  wvec ns;
  {
    wvec mv;
#pragma unroll
    for (int j = 0; j < kWPT; j++) {
      mv[j] = P.msw[j];
      ns[j] = P.nsw[j];
    }
    reinterpret_cast<wvec*>(mslice)[tid] = mv;
    reinterpret_cast<wvec*>(nbits)[tid] = wvec{};
  }
  __syncthreads();
  while (b < kNumBuckets) {
    const uint32_t lo = q.x, hi = q.y;
    // thread 0: resolve the pending ticket (published after the rounds) and take the next one
    uint32_t pend_b = kNumBuckets;
    uint4 pend_q = make_uint4(0, 0, 0, 0);
    if (tid == 0) {
      pend_b = list_bucket(a, 2 * gridDim.x + pend_t, l0, nl, &pend_q);
      pend_t = take_ticket(a.ticket);
    }
    for (uint32_t base = lo & ~(kE - 1);;) {
      // the next round in flight: this bucket's, or the next bucket's first with its words
      const uint32_t next = base + kSRound<k16>;
      const bool last = next >= hi;
      if (!last || b1 < kNumBuckets) sets_round_load<k16>(a, last ? q1.x & ~(kE - 1) : next, last ? q1.y : hi, y);
      if (last && b1 < kNumBuckets) sets_pre_load(a, b1, P);
#pragma unroll
      for (int j = 0; j < kSQ; j++)  // four entries at a time: their LDS reads issued before the first use
#pragma unroll
        for (int h = 0; h < (int)kE; h += 4) {
          uint32_t mw[4];
#pragma unroll
          for (int u = 0; u < 4; u++) mw[u] = mslice[sets_sig<k16>(x[j], h + u) >> 5];
#pragma unroll
          for (int u = 0; u < 4; u++) {
            const uint32_t i = sets_pos<k16>(base, j) + h + u, v = sets_sig<k16>(x[j], h + u);
            const uint32_t bit = 1u << (v & 31);
            if (i >= lo && i < hi && !(mw[u] & bit)) atomicOr(&nbits[v >> 5], bit);
          }
        }
      // (after the last round too: then the next bucket's first round, if there is one)
#pragma unroll
      for (int j = 0; j < kSQ; j++) x[j] = y[j];
      if (last) break;
      base = next;
    }
    if (tid == 0) {  // the bucket after next
      sh_b[0] = pend_b;
      sh_q[0] = pend_q;
    }
    __syncthreads();  // every OR of the bucket is done
    {
      // words kWPT tid ..: this block is their only writer
      const uint64_t w0 = bucket_word(b, kWPT * tid);
      const wvec nb = reinterpret_cast<const wvec*>(nbits)[tid];
      const wvec cm = reinterpret_cast<const wvec*>(mslice)[tid];
      uint32_t any = 0;
#pragma unroll
      for (int j = 0; j < kWPT; j++) {
        any |= nb[j];
        if (nb[j]) {
          a.mwords[w0 + j] = cm[j] | nb[j];
          if (a.nwords) a.nwords[w0 + j] = ns[j] | nb[j];
        }
      }
      if (any) reinterpret_cast<wvec*>(nbits)[tid] = wvec{};
      if (b1 < kNumBuckets) {  // the next bucket's words (P was loaded in the last round)
        wvec mv;
#pragma unroll
        for (int j = 0; j < kWPT; j++) {
          mv[j] = P.msw[j];
          ns[j] = P.nsw[j];
        }
        reinterpret_cast<wvec*>(mslice)[tid] = mv;
      }
    }
    b = b1;
    q = q1;
    b1 = uni(sh_b[0]);
    q1 = uni(sh_q[0]);
    __syncthreads();  // the slices stand; sh_b[0] / sh_q[0] are read
  }
}

// Buckets with too many distinct candidates: a direct first-owner table over
// one eighth of the bucket (8192 signals, 32 KiB of LDS) per job; the
// (bucket, eighth) jobs are independent (each owns its eighth's 256 bitmap
// words), so a few huge spilled buckets spread over many workgroups.
constexpr int kDThreads = 1024;
template <bool kEmit>
__global__ __launch_bounds__(kDThreads) void k_bucket_direct(BucketArgs a) {
  constexpr uint32_t kQ = 8192, kNQ = 65536 / kQ, kQW = kQ / 32;
  __shared__ uint32_t owner[kQ];
  __shared__ uint32_t mpart[kQW];
  __shared__ uint32_t nbits[kQW];
  __shared__ uint32_t gb[kMaxGroups];
  __shared__ uint32_t shcnt[kEmit ? kMaxShards : 1];
  __shared__ uint32_t lcnt[kEmit ? kMaxGroups : 1];
  __shared__ unsigned long long lbase[kEmit ? kMaxGroups : 1];
  __shared__ uint32_t fsum[kEmit ? 1 : kFsWords];  // after a split launch: its summary (else zero)
  const int tid = threadIdx.x;
  const uint32_t nsp = *a.nspill, NG = a.NG;
  if (!kEmit)  // (the job loop's first barrier orders it)
    for (uint32_t i = tid; i < kFsWords; i += kDThreads) fsum[i] = a.fsum ? a.fsum[i] : 0u;
  if (kEmit) {
    for (uint32_t i = tid; i < kMaxShards; i += kDThreads) shcnt[i] = 0;
    for (uint32_t i = tid; i < kMaxGroups; i += kDThreads) lcnt[i] = 0;
    __syncthreads();
  }
  for (uint32_t job = blockIdx.x; job < nsp * kNQ; job += gridDim.x) {
    const uint32_t b = a.spill[job / kNQ], qq = job % kNQ;
    const uint4 q = a.bdesc[b];
    for (uint32_t i = tid; i < kQW; i += kDThreads) {
      const uint64_t w = bucket_word(b, qq * kQW + i);
      mpart[i] = a.mwords[w] | (a.owords ? a.owords[w] : 0u);
      nbits[i] = 0;
    }
    for (uint32_t i = tid; i < NG; i += kDThreads) gb[i] = a.gbnd[(uint64_t)b * NG + i];
    for (uint32_t i = tid; i < kQ; i += kDThreads) owner[i] = kEmpty;
    __syncthreads();
    for (uint32_t i = q.x + tid; i < q.y; i += kDThreads) {
      const uint32_t x = a.in[i];
      const uint32_t sl = x >> 16, sq = sl % kQ;
      if (sl / kQ != qq || ((mpart[sq >> 5] >> (sq & 31)) & 1u)) continue;
      atomicMin(&owner[sq], entry_record(group_of(gb, NG, i), x));
      atomicOr(&nbits[sq >> 5], 1u << (sq & 31));
    }
    __syncthreads();
    if (kEmit) {
      constexpr int kPer = kQ / kDThreads;
      uint32_t sig[kPer], rec[kPer];
#pragma unroll
      for (int k = 0; k < kPer; k++) {
        const uint32_t i = k * kDThreads + tid;
        sig[k] = part_sig((b << 16) | (qq * kQ + i));
        rec[k] = owner[i];
      }
      if (a.gcur)
        emit_grouped(a, sig, rec, lcnt, lbase);
      else
        emit_pairs(a, sig, rec, shcnt);
      for (uint32_t i = tid; i < kQW; i += kDThreads) {
        const uint32_t nb = nbits[i];
        if (!nb) continue;
        const uint64_t w = bucket_word(b, qq * kQW + i);
        if (a.update) a.mwords[w] = mpart[i] | nb;
        if (a.nwords) a.nwords[w] |= nb;
      }
    } else {
      for (uint32_t i = tid; i < kQ; i += kDThreads)
        if (owner[i] != kEmpty && !fs_full(fsum, owner[i])) a.rec_new[owner[i]] = 1;
      for (uint32_t i = tid; i < kQW; i += kDThreads) {
        const uint32_t nb = nbits[i];
        if (nb) {
          const uint64_t w = bucket_word(b, qq * kQW + i);
          a.mwords[w] = mpart[i] | nb;
          if (a.nwords) a.nwords[w] |= nb;
        }
      }
    }
    __syncthreads();
  }
  if (kEmit) flush_shard_counts(a, shcnt);
}

// Grid of a persistent kernel: every block resident at once (CUs x blocks
// per CU from the occupancy query), cached per kernel.
uint32_t persistent_grid(sg_ctx* ctx, const void* kernel, int threads) {
  static std::mutex mu;
  static std::map<std::pair<int, const void*>, uint32_t> cache;
  std::lock_guard<std::mutex> lock(mu);
  const auto key = std::make_pair(ctx->device, kernel);
  auto it = cache.find(key);
  if (it != cache.end()) return it->second;
  int per_cu = 0, cus = 0;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, threads, 0) != hipSuccess || per_cu < 1)
    per_cu = 1;
  if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, ctx->device) != hipSuccess || cus < 1)
    cus = 256;
  const uint32_t grid = (uint32_t)(per_cu * cus);
  cache[key] = grid;
  return grid;
}

// The split bucket stage's regime: option flag_skip 1 always, 0 never.  The
// split pays when the first launch leaves nearly every record flagged, that
// is in a batch that queues nearly all of its records (a fresh corpus: every
// record owns ~200 new signals spread over all buckets); in a low-novelty
// batch it only adds a launch (measured +0.05 ms on the steady batch).  A
// block's stores are skipped only when all of its kFsRecs records are queued:
// with a queued fraction q that is q^4096 of the blocks (0.29 at 0.9997, 0.66
// at 0.9999), and the measured gain of 0.17 ms with every block full covers
// the added launch from about 0.3 of them.  auto therefore splits when the
// last counted partitioned slice of the context queued at least kFsQueued of
// its records (the count that the M0 filter's regime reads): a fresh corpus.
// Before the first count is read -- a context's first slice, or its count
// still in flight -- it does not; while a later count is in flight the last
// one read stands.
constexpr double kFsQueued = 0.9997;
static bool fs_split(sg_ctx* ctx) {
  const int64_t o = ctx->opt[kOptFlagSkip];
  if (o >= 0) return o != 0;
  m0f_poll(ctx);
  return ctx->m0f_queued >= kFsQueued;
}

// The flags path's bucket stage for this launch: 0 one launch, 1 split, 2
// split with a late pass 2 (P2Late, sg_part.h; late_ok: the caller can run
// pass 2 in parts).  Option flag_skip_u16: -1 late whenever the launch splits,
// 0 never, 1 late with the split forced.
int buckets_split(sg_ctx* ctx, const BucketPlan& bp, const uint8_t* d_rec_new, bool late_ok) {
  if (ctx->debug_part || !d_rec_new || bp.nrec > kMaxLaunchRecords) return 0;
  const int u = late_ok ? ctx->fs_u16_opt : 0;
  if (u > 0) return 2;
  return fs_split(ctx) ? (u ? 2 : 1) : 0;
}

// The bucket stage: the bucket kernels over the partition's buckets (bp as
// partition_pass1 rebased it): flags and set updates, or (emit) the candidate pairs.
int buckets_one(sg_ctx* ctx, const BucketPlan& bp, uint32_t* mwords, uint32_t* nwords, uint8_t* d_rec_new,
                const EmitArgs* emit, const uint32_t* owords, int split_mode) {
  const uint64_t nrec = bp.nrec;
  const uint32_t* gcount = bp.at<uint32_t>(ctx, kCB) + bp.ng;  // device: number of pass-2 chunks
  uint4* bdesc = bp.at<uint4>(ctx, kBD);
  uint32_t* nspill = bp.at<uint32_t>(ctx, kSP);
  const bool dbg = ctx->debug_part;
  BucketArgs ba{};
  ba.in = bp.at<uint32_t>(ctx, kV2);
  ba.bdesc = bdesc;
  ba.gbnd = bp.at<uint32_t>(ctx, kGB);
  ba.NG = (uint32_t)bp.NG;
  ba.mwords = mwords;
  ba.owords = owords;
  ba.nwords = nwords;
  ba.rec_new = d_rec_new;
  ba.nspill = nspill;
  ba.spill = nspill + 1;
  ba.ticket = bp.at<uint32_t>(ctx, kTK);
  if (emit) {
    ba.pairs = emit->pairs;
    ba.npairs = emit->npairs;
    ba.rec_base = emit->rec_base;
    ba.nshards = emit->nshards;
    ba.shard_cnt = emit->shard_cnt;
    ba.update = emit->update ? 1u : 0u;
    ba.gcur = emit->gcur;
    ba.goff = emit->goff;
  }
  uint32_t bgrid = persistent_grid(ctx, (const void*)k_bucket<false, 0>, kBThreads);
  // diagnostics: option bucket_blocks caps the persistent grid (leaves CUs
  // to kernels on other streams)
  const int64_t cap_blocks = ctx->opt[kOptBucketBlocks];
  if (cap_blocks > 0 && (uint64_t)cap_blocks < bgrid) bgrid = (uint32_t)cap_blocks;
  DevBuf<uint64_t> ddbg;
  if (dbg) {
    const int rc = ddbg.grow_drop((size_t)bgrid * 11, nullptr);
    if (rc) return rc;
    ba.dbg = ddbg.p;
  }
  // The flags path in two launches (option flag_skip): the first 1 / 2^k of
  // the bucket list with every flag stored, the record-flag summary, then the
  // rest of the list without the stores that the summary shows to rewrite a 1.
  if (split_mode < 0) split_mode = emit ? 0 : buckets_split(ctx, bp, d_rec_new, false);
  const bool split = split_mode != 0, late = split_mode == 2;
  uint32_t* fsum = ba.ticket + kTkWords;
  uint32_t* fcnt = &ctx->dev.p->fs_full_blocks;
  if (split) {
    int rc = ctx->fs_ev.create(hipEventDisableTiming);
    if (!rc) rc = m0f_host_alloc(ctx);
    if (rc) return rc;
    SG_HIP(hipMemsetAsync(fcnt, 0, 4, ctx->stream));
  }
  SG_HIP(hipMemsetAsync(ba.ticket, 0, split ? (kTkWords + kFsWords) * 4 : 4, ctx->stream));
  SG_HIP(hipMemsetAsync(nspill, 0, 4, ctx->stream));
  ba.blist_b = bp.at<uint32_t>(ctx, kLB);
  ba.blist_q = bp.at<uint4>(ctx, kLQ);
  ba.nlist = bp.at<uint32_t>(ctx, kBP) + kNumBuckets;
  {
    ScopedTimer tm(ctx, "bucket_triage");
    if (split) {
      ba.win = 1;
      ba.win_shift = (uint32_t)ctx->opt[kOptFlagSkipSplit];
      ba.bounds = ba.ticket;
    }
    P2Late pl{1, false, ba.ticket, fcnt, (uint32_t)div_up(nrec, kFsRecs), &ctx->dev.p->fs_u16};
    if (late) {
      // the first window's slices scattered now, in 4-byte entries (the other chunks after the summary)
      hipLaunchKernelGGL(k_late_bounds, dim3(1), dim3(1), 0, ctx->stream, (const uint32_t*)bp.at<uint32_t>(ctx, kBP),
                         ba.blist_b, (const uint32_t*)bp.at<uint32_t>(ctx, kCF), ba.win_shift, ba.ticket);
      int rc = partition_pass2_windows(ctx, bp, ba.ticket);
      if (!rc) rc = partition_pass2_scatter(ctx, bp, &pl);
      if (rc) return rc;
    }
    auto kb = emit  ? (emit->gcur ? k_bucket<false, 2> : k_bucket<false, 1>)
              : dbg ? k_bucket<true, 0>
                    : k_bucket<false, 0>;
    hipLaunchKernelGGL(kb, dim3(bgrid), dim3(kBThreads), 0, ctx->stream, ba);
    if (late) {
      // The 2-byte entries of an all-flagged launch land at byte 2 * position, over the 4-byte entries of other
      // buckets: whatever still reads those runs first.  The first window's spilled buckets now (their flags
      // also reach the summary), leaving an empty spill list to the second phase ...
      hipLaunchKernelGGL(k_bucket_direct<false>, dim3(512), dim3(kDThreads), 0, ctx->stream, ba);
      SG_HIP(hipMemsetAsync(nspill, 0, 4, ctx->stream));
    }
    if (split) {
      hipLaunchKernelGGL(k_flag_summary, dim3(div_up(div_up(nrec, kFsRecs), 4)), dim3(256), 0, ctx->stream,
                         (const uint8_t*)d_rec_new, (uint32_t)nrec, fsum, fcnt);
      ba.win = 2;
      ba.ticket++;
      ba.fsum = fsum;  // (the direct-table kernel below honours it too)
      // Both forms of the second phase over the window; each reads the
      // summary's count first and returns unless the launch is its case (the
      // decision stays on the device: the call is stream-ordered).  Every
      // record flagged: the map-free k_bucket_sets, with a ticket of its own.
      ba.fs_cnt = fcnt;
      ba.fs_nblk = (uint32_t)div_up(nrec, kFsRecs);
      ba.fs_all = &ctx->dev.p->fs_all_flagged;
      BucketArgs bs = ba;
      bs.ticket = ba.ticket + 1;
      uint32_t sgrid = persistent_grid(ctx, (const void*)k_bucket_sets<false>, kBThreads);
      if (cap_blocks > 0 && (uint64_t)cap_blocks < sgrid) sgrid = (uint32_t)cap_blocks;
      if (late) {
        // ... and, all-flagged, the rest of the boundary slice, 4-byte entries of the first scatter (empty when
        // every bucket is non-empty).  Then the second window's slices in both forms of the scatter.
        bs.win = 3;
        hipLaunchKernelGGL(k_bucket_sets<false>, dim3(sgrid), dim3(kBThreads), 0, ctx->stream, bs);
        pl.win = 2;
        int rc = partition_pass2_scatter(ctx, bp, &pl);
        pl.u16 = true;
        if (!rc) rc = partition_pass2_scatter(ctx, bp, &pl);
        if (rc) return rc;
      }
      hipLaunchKernelGGL((k_bucket<false, 0, true>), dim3(bgrid), dim3(kBThreads), 0, ctx->stream, ba);
      if (late) {  // all-flagged: the late slices, 2-byte entries, with a ticket of their own
        bs.win = 4;
        bs.ticket = ba.ticket + 2;
        bs.fs_all = nullptr;  // (the launch is counted once, by the window-3 launch)
        uint32_t ugrid = persistent_grid(ctx, (const void*)k_bucket_sets<true>, kBThreads);
        if (cap_blocks > 0 && (uint64_t)cap_blocks < ugrid) ugrid = (uint32_t)cap_blocks;
        hipLaunchKernelGGL(k_bucket_sets<true>, dim3(ugrid), dim3(kBThreads), 0, ctx->stream, bs);
      } else {
        hipLaunchKernelGGL(k_bucket_sets<false>, dim3(sgrid), dim3(kBThreads), 0, ctx->stream, bs);
      }
    }
  }
  if (split) {
    // (three words: the last launch's full blocks, and the context's all-flagged and 2-byte launches so far)
    static_assert(offsetof(CtxDev, fs_all_flagged) == offsetof(CtxDev, fs_full_blocks) + 4 &&
                      offsetof(CtxDev, fs_u16) == offsetof(CtxDev, fs_full_blocks) + 8 &&
                      offsetof(CtxPinned, fs_all_flagged) == offsetof(CtxPinned, fs_full_blocks) + 4 &&
                      offsetof(CtxPinned, fs_u16) == offsetof(CtxPinned, fs_full_blocks) + 8,
                  "the three words travel in one copy");
    SG_HIP(hipMemcpyAsync(&ctx->pinned.p->fs_full_blocks, fcnt, 12, hipMemcpyDeviceToHost, ctx->stream));
    SG_HIP(hipEventRecord(ctx->fs_ev, ctx->stream));
    ctx->fs_pending = true;
    ctx->fs_used++;
  }
  {
    ScopedTimer tm(ctx, "bucket_spill");
    auto kd = emit ? k_bucket_direct<true> : k_bucket_direct<false>;
    hipLaunchKernelGGL(kd, dim3(512), dim3(kDThreads), 0, ctx->stream, ba);
  }
  SG_HIP(hipGetLastError());
  if (dbg) {  // diagnostics: chunk and spill counts (syncs)
    uint32_t g = 0, sp = 0;
    SG_HIP(hipMemcpyAsync(&g, gcount, 4, hipMemcpyDeviceToHost, ctx->stream));
    SG_HIP(hipMemcpyAsync(&sp, nspill, 4, hipMemcpyDeviceToHost, ctx->stream));
    SG_HIP(hipStreamSynchronize(ctx->stream));
    fprintf(stderr, "sg part: n=%llu nrec=%llu tiles=%llu chunks=%u (bound %llu) spilled_buckets=%u\n",
            (unsigned long long)bp.n, (unsigned long long)nrec, (unsigned long long)bp.T, g,
            (unsigned long long)bp.gmax, sp);
    std::vector<uint4> bd(kNumBuckets);
    std::vector<uint64_t> hd((size_t)bgrid * 11);
    SG_HIP(hipMemcpy(bd.data(), bdesc, bd.size() * 16, hipMemcpyDeviceToHost));
    SG_HIP(hipMemcpy(hd.data(), ddbg.p, hd.size() * 8, hipMemcpyDeviceToHost));
    double qa = 0, qb = 0, qc = 0;
    for (uint32_t i = 0; i < bgrid; i++) {
      qa += hd[8 * bgrid + 3 * i];
      qb += hd[8 * bgrid + 3 * i + 1];
      qc += hd[8 * bgrid + 3 * i + 2];
    }
    std::vector<uint32_t> sz(kNumBuckets);
    uint64_t rounds = 0;
    for (uint32_t b = 0; b < kNumBuckets; b++) {
      sz[b] = bd[b].y - bd[b].x;
      rounds += (sz[b] + 8191) / 8192;
    }
    std::sort(sz.begin(), sz.end());
    uint64_t t0 = ~0ull, t1 = 0;
    std::vector<double> dur;
    uint64_t maxr = 0;
    double phs[4] = {0, 0, 0, 0}, nbk = 0, nrd = 0;
    for (uint32_t i = 0; i < bgrid; i++) {
      t0 = std::min(t0, hd[8 * i]);
      t1 = std::max(t1, hd[8 * i + 1]);
      dur.push_back((hd[8 * i + 1] - hd[8 * i]) / 100.0);  // 100 MHz clock -> us
      maxr = std::max(maxr, hd[8 * i + 3]);
      nbk += hd[8 * i + 2];
      nrd += hd[8 * i + 3];
      for (int j = 0; j < 4; j++) phs[j] += hd[8 * i + 4 + j];
    }
    fprintf(stderr, "sg bucket per bucket (cycles, wave 0): install %.0f | rounds: test %.0f insert %.0f tail %.0f | "
            "end barrier %.0f flush %.0f final barrier %.0f | rounds/bucket %.2f\n", phs[0] / nbk, qa / nbk, qb / nbk,
            phs[1] / nbk, phs[2] / nbk, phs[3] / nbk, qc / nbk, nrd / nbk);
    std::sort(dur.begin(), dur.end());
    fprintf(stderr,
            "sg bucket: sizes max=%u p99=%u median=%u rounds=%llu | blocks=%u span=%.1fus dur min=%.1f med=%.1f "
            "max=%.1f us, max rounds/block=%llu\n",
            sz.back(), sz[kNumBuckets * 99 / 100], sz[kNumBuckets / 2], (unsigned long long)rounds, bgrid,
            (t1 - t0) / 100.0, dur.front(), dur[dur.size() / 2], dur.back(), (unsigned long long)maxr);
  }
  return SG_OK;
}

}  // namespace sg
