// sg_m0filter.hip -- the M0 filter of the partitioned triage (sg_part.h): on
// low-novelty batches it replaces pass 2 and the bucket stage; and its regime.
#include "sg_part.h"

namespace sg {

// The fuzzer's steady state (r06): nearly every entry of a batch is already
// in maxSignal (fuzzer.go:666 ends most records at the SignalNew test; the
// bench's steady batch: 139K candidates among 880M entries), yet pass 2 and
// the bucket stage move every entry.  A random probe of any exact table of
// maxSignal costs each CU ~10 cycles wherever the table lives (L2, Infinity
// Cache or HBM; scripts/micro/m0_filter.hip: 55-91 G probes/s), so the test
// has to be in LDS -- and pass 1 already groups the entries by slice (b2: 2^24
// signals).  A slice's part of maxSignal is ~50K signals (12.8M / 256): too
// many for its 2 MiB of bitmap, few enough for a packed index in LDS:
//   k_m0_index  per slice, one 16-B header per 2^11-signal filter bucket
//               (8192: 128 KiB): up to 8 of the bucket's set positions as
//               16-bit fields (ascending, 0x8000 in the unused ones), or,
//               past 8, the first 7 and in field 7 0x8000 | the block of the
//               next 8 in a small per-slice pool (kFOvBlocks 8-value blocks);
//               the rest (past 15, or past 7 when the pool is full) in the
//               slice's spill list (kFSpill positions; past it, signals are
//               not proven, only re-checked by the tail); one read of the
//               slice's bitmap;
//   k_m0_filter per slice part, the slice's index in LDS (159 KiB); every
//               pass-1 entry reads its bucket's header and the first block of
//               its overflow list (the pool's dummy block 0 for a bucket
//               without one) -- two ds_read_b128, the second one's address
//               from the first -- and compares its position with the 16
//               fields by packed 16-bit xor / min; an entry not found is
//               looked up in the spill list (held in registers, 8 per lane,
//               a wave-wide compare per such entry) and, not there either,
//               survives, as (position, slice);
//   tail        if the survivors fit (kFSurvCap): each survivor still outside
//               maxSignal (the exact bitmap test) gets its record (its pass-1
//               tile by a search over the slice's run starts) and takes
//               min(record) per signal in a hash table; then every distinct
//               signal sets its first owner's flag and its bits in maxSignal
//               and newSignal -- the bucket stage's results (fuzzer.go:669-690)
//               over the candidates.
// When the survivors overflow, pass 2 and the bucket stage run on the same
// pass-1 output.  Option m0_filter -1 (auto, m0f_try) tries the filter after a
// slice it filtered and after a partitioned slice that queued under a quarter
// of its records.
constexpr uint32_t kFRemBits = 11;                      // positions per filter bucket: 2^11
constexpr uint32_t kFBuckets = 1u << (24 - kFRemBits);  // 8192 per slice
constexpr uint32_t kFOvBlocks = 1984;                   // overflow pool per slice: 8-value u16 blocks (31 KiB);
                                                        // block 0 the dummy
constexpr uint32_t kFPad = 0x8000u;                     // an unused field (no position; >= it: a block link)
constexpr uint32_t kFSpill = 512;                       // spill list per index part (8 registers per lane)
constexpr uint32_t kFHMax = 4;                          // index parts per slice, at most (option m0_filter_halves)
constexpr uint32_t kFIdx = 256 * kFHMax;                // index parts in all
constexpr uint32_t kFSurvCap = 1u << 20;                // survivors per launch
constexpr uint32_t kFTableBits = 21;                    // the tail's table: 2^21 u64 slots
constexpr int kFThreads = 1024;
#ifndef SG_FPARTS
#define SG_FPARTS 8
#endif
#ifndef SG_FU
#define SG_FU 4  // 16-B entry loads per thread per step
#endif
#ifndef SG_FEH
#define SG_FEH 4  // entries whose LDS reads are in flight together
#endif
constexpr uint32_t kFParts = SG_FPARTS;                 // filter workgroups per slice
constexpr uint32_t kFWgCap = 4 * kFSurvCap / (256 * kFParts);  // survivors per filter workgroup (its own region:
                                                              // 4x the mean share at the cap, 32 MiB in all)
constexpr unsigned long long kFEmpty = ~0ull;

struct M0F {
  uint4* tab;                 // [index part][bucket] headers (part = slice << log H | half)
  uint16_t* ovals;            // [index part][8 kFOvBlocks] overflow pool
  uint32_t* cursor;           // [index part] overflow blocks placed (may pass the pool)
  uint32_t* nspill;           // [index part] spilled positions (may pass kFSpill)
  uint32_t* spill;            // [index part][kFSpill] positions in the slice
  uint32_t* nsurv;            // [0] survivors in the regions that held theirs, [1] != 0: some region overflowed,
                              // [2] != 0: some index part overflowed (values past its pool and spill list)
  uint2* surv;                // (position, slice), kFWgCap per filter workgroup
  uint32_t* wgcnt;            // [filter workgroup] survivors in its region
  unsigned long long* table;  // signal << 32 | min record; kFEmpty between launches
};
static size_t m0f_bytes() {
  return (uint64_t)kFIdx * kFBuckets * 16 + (uint64_t)kFIdx * kFOvBlocks * 16 + kFIdx * 4 + 256 + kFIdx * 4 +
         (uint64_t)kFIdx * kFSpill * 4 + 256ull * kFParts * kFWgCap * 8 +
         256ull * kFParts * 4 + (8ull << kFTableBits);
}
static M0F m0f_bind(char* b) {
  M0F f;
  f.tab = (uint4*)b;
  b += (uint64_t)kFIdx * kFBuckets * 16;
  f.ovals = (uint16_t*)b;
  b += (uint64_t)kFIdx * kFOvBlocks * 16;
  f.cursor = (uint32_t*)b;
  f.nsurv = f.cursor + kFIdx;
  f.nspill = f.cursor + kFIdx + 64;
  b += kFIdx * 4 + 256 + kFIdx * 4;
  f.spill = (uint32_t*)b;
  b += (uint64_t)kFIdx * kFSpill * 4;
  f.surv = (uint2*)b;
  b += 256ull * kFParts * kFWgCap * 8;
  f.wgcnt = (uint32_t*)b;
  b += 256ull * kFParts * 4;
  f.table = (unsigned long long*)b;
  return f;
}

// grid (kFBuckets / 256, 256): thread t of block (e, d) indexes filter
// bucket 256 e + t of slice d, its 64 bitmap words (256 B) read as 16 quads;
// it walks their set bits in order into its header's fields and its overflow
// list, whose blocks one cursor add per wave places.  (A wave per 64 buckets,
// lane l holding word l of each, measured 0.40-0.45 ms per steady step: 128
// wave scans per 64 buckets; this form 0.24 ms.)
// kLogH: the slice's index in 2^kLogH parts (halves h of its positions, each
// with its own 8192 buckets of 2^(11 - kLogH) positions, pool and spill list:
// past ~14M signals of maxSignal one part no longer holds a slice); grid
// (kFBuckets / 256, 256 << kLogH), blockIdx.y = slice << kLogH | h.
template <int kLogH>
__global__ __launch_bounds__(256) void k_m0_index(const uint32_t* __restrict__ mwords, uint4* __restrict__ tab,
                                                   uint16_t* __restrict__ ovals, uint32_t* __restrict__ cursor,
                                                   uint32_t* __restrict__ nspill, uint32_t* __restrict__ spill,
                                                   uint32_t* __restrict__ flags) {
  constexpr int kQ = 16 >> kLogH;                // bitmap quads per bucket
  constexpr uint32_t kRB = kFRemBits - kLogH;    // position bits in a bucket
  const uint32_t dh = blockIdx.y, lane = threadIdx.x & 63;
  const uint32_t d = dh >> kLogH, h = dh & ((1u << kLogH) - 1);
  const uint32_t j = blockIdx.x * 256 + threadIdx.x;
  const uint4* src = reinterpret_cast<const uint4*>(mwords + ((uint64_t)d << 19) + ((uint64_t)h << (19 - kLogH)) +
                                                    (uint64_t)j * (4 * kQ));
  uint4 q[kQ];
#pragma unroll
  for (int i = 0; i < kQ; i++) q[i] = src[i];
  uint32_t n = 0;
#pragma unroll
  for (int i = 0; i < kQ; i++) n += __popc(q[i].x) + __popc(q[i].y) + __popc(q[i].z) + __popc(q[i].w);
  // the overflow block of a bucket past 8 values
  const uint32_t ob = n > 8 ? 1u : 0u;
  const uint32_t oi = sgd::wave_incl_add(ob);
  const uint32_t otot = (uint32_t)__builtin_amdgcn_readlane((int)oi, 63);
  uint32_t obase = 0;
  if (lane == 0 && otot) obase = atomicAdd(&cursor[dh], otot);
  obase = (uint32_t)__builtin_amdgcn_readfirstlane((int)obase);
  const uint32_t ost = 1 + obase + oi - ob;  // first block (block 0: none, the filter's dummy)
  const bool ok = ob && ost + ob <= kFOvBlocks;  // (else the rest is spilled)
  uint16_t* out = ovals + ((uint64_t)dh * kFOvBlocks + ost) * 8;
  const uint32_t kin = n > 8 ? 7u : 8u;  // values in the header
  // the spill list's slots for the rest (past 15 values, or past 7 with the
  // pool full), one add per wave (past the index's capacity, an add per
  // spilled value -- ~10^4-10^5 per slice on one counter -- took 3.7-14 ms at
  // an 18-41M maxSignal)
  const uint32_t kst = ok ? 15u : 7u, nsw = n > 8 && n > kst ? n - kst : 0u;
  const uint32_t si = sgd::wave_incl_add(nsw);
  const uint32_t stot = (uint32_t)__builtin_amdgcn_readlane((int)si, 63);
  uint32_t sbase = 0;
  if (lane == 0 && stot) sbase = atomicAdd(&nspill[dh], stot);
  sbase = (uint32_t)__builtin_amdgcn_readfirstlane((int)sbase) + si - nsw;
  if (nsw && sbase + nsw > kFSpill) flags[2] = 1u;  // (values past the part's capacity: a larger H would hold them)
  uint64_t lo = 0, hi = 0;               // fields 0..3, 4..7
  uint32_t k = 0;
#pragma unroll
  for (int i = 0; i < kQ; i++) {
    const uint32_t wq[4] = {q[i].x, q[i].y, q[i].z, q[i].w};
#pragma unroll
    for (int c = 0; c < 4; c++) {
      uint32_t m = wq[c];
      while (m) {
        const uint32_t v = (uint32_t)(32 * (4 * i + c)) + (uint32_t)__builtin_ctz(m);  // ascending in k
        m &= m - 1;
        if (k < kin) {
          if (k < 4)
            lo |= (uint64_t)v << (16 * k);
          else
            hi |= (uint64_t)v << (16 * (k - 4));
        } else if (ok && k < 15) {
          out[k - 7] = (uint16_t)v;
        } else {  // (rare: past 15 values, or the pool full)
          const uint32_t at = sbase + k - kst;
          if (at < kFSpill) spill[(uint64_t)dh * kFSpill + at] = (h << (24 - kLogH)) | (j << kRB) | v;
        }
        k++;
      }
    }
  }
  for (uint32_t f = min(n, kin); f < 8; f++) {  // unused fields, and field 7 past 8 values
    const uint64_t v = f == 7 && n > 8 && ok ? kFPad | ost : kFPad;
    if (f < 4)
      lo |= v << (16 * f);
    else
      hi |= v << (16 * (f - 4));
  }
  if (ok)
    for (uint32_t t = n - 7; t < 8; t++) out[t] = (uint16_t)kFPad;  // the block's padding
  tab[(uint64_t)dh * kFBuckets + j] = make_uint4((uint32_t)lo, (uint32_t)(lo >> 32), (uint32_t)hi, (uint32_t)(hi >> 32));
}

typedef unsigned short m0f_u16x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ uint32_t m0f_min16(uint32_t a, uint32_t b) {  // v_pk_min_u16
  return __builtin_bit_cast(uint32_t, __builtin_elementwise_min(__builtin_bit_cast(m0f_u16x2, a),
                                                               __builtin_bit_cast(m0f_u16x2, b)));
}

// grid (kFParts, 256): part x of slice d's pass-1 run.  Per thread and step
// 4 SG_FU entries, the next two steps' loads in flight while one is tested.
// A survivor is written as (position, slice).
template <int kLogH>
__global__ __launch_bounds__(kFThreads) void k_m0_filter(const uint32_t* __restrict__ v1,
                                                          const uint32_t* __restrict__ goff1, uint32_t T,
                                                          const uint4* __restrict__ tab,
                                                          const uint16_t* __restrict__ ovals,
                                                          const uint32_t* __restrict__ cursor,
                                                          const uint32_t* __restrict__ nspill,
                                                          const uint32_t* __restrict__ spill,
                                                          uint2* __restrict__ surv, uint32_t* __restrict__ nsurv,
                                                          uint32_t* __restrict__ wgcnt) {
  constexpr uint32_t logh = kLogH;  // (a constant: as a kernel argument its shifts cost 0.1 ms per launch)
  // the overflow pool, then the headers (one array: both bases fit the
  // ds_read offset field)
  __shared__ v4u32 lds[kFOvBlocks + kFBuckets];
  // the workgroup's survivors so far, in its own region of surv (an LDS
  // cursor: a returning global atomic per survivor wave makes the compiler
  // wait for every load in flight, the next step's entries included; one
  // counter read by every wave each step measured 12 ms per C2 step)
  __shared__ uint32_t wsurv;
  // grid (parts, 256, 2^logh): part x of slice d's run against index part hp
  // (the positions p with p >> (24 - logh) == hp; the other entries pass as
  // found -- each entry is tested by exactly one index part)
  const uint32_t d = blockIdx.y, hp = blockIdx.z, dh = (d << logh) | hp, tid = threadIdx.x, lane = tid & 63;
  const uint32_t R0 = goff1[(uint64_t)d * T], R1 = goff1[(uint64_t)(d + 1) * T];
  const uint64_t len = R1 - R0;
  const uint32_t a = R0 + (uint32_t)(len * blockIdx.x / gridDim.x), b = R0 + (uint32_t)(len * (blockIdx.x + 1) / gridDim.x);
  const uint32_t wg = dh * gridDim.x + blockIdx.x;
  if (a >= b) {
    if (tid == 0) wgcnt[wg] = 0;
    return;
  }
  const uint32_t rb = kFRemBits - logh;  // position bits in a bucket
  constexpr uint32_t topm = logh ? ~0u << (32 - logh) : 0u;  // (the part's bits of an entry)
  const uint32_t toph = logh ? hp << ((32 - logh) & 31) : 0u;
  const uint32_t nob = min(cursor[dh] + 1, kFOvBlocks);
  uint2* wsv = surv + (uint64_t)wg * kFWgCap;
  if (tid == 0) wsurv = 0;
  const v4u32* hsrc = reinterpret_cast<const v4u32*>(tab + (uint64_t)dh * kFBuckets);
  {
    v4u32 t[kFBuckets / kFThreads];  // (all in flight, then stored)
#pragma unroll
    for (uint32_t u = 0; u < kFBuckets / kFThreads; u++) t[u] = hsrc[tid + u * kFThreads];
#pragma unroll
    for (uint32_t u = 0; u < kFBuckets / kFThreads; u++) lds[kFOvBlocks + tid + u * kFThreads] = t[u];
  }
  const v4u32* osrc = reinterpret_cast<const v4u32*>(ovals + (uint64_t)dh * kFOvBlocks * 8);
  for (uint32_t i = 1 + tid; i < nob; i += kFThreads) lds[i] = osrc[i];
  if (tid == 0) lds[0] = v4u32{kFPad * 0x10001u, kFPad * 0x10001u, kFPad * 0x10001u, kFPad * 0x10001u};  // dummy
  // the spill list, entry 64 i + lane in sp[i] (~0u: none)
  const uint32_t nsp = min(nspill[dh], kFSpill);
  uint32_t sp[kFSpill / 64];
#pragma unroll
  for (int i = 0; i < (int)(kFSpill / 64); i++)
    sp[i] = 64 * i + lane < nsp ? spill[(uint64_t)dh * kFSpill + 64 * i + lane] : ~0u;
  __syncthreads();
  // 4 SG_FU entries per thread per step, two more steps in flight (one
  // 16-wave workgroup per CU holds the LDS index, so the stream's depth is
  // per thread)
  constexpr int U = SG_FU;
  constexpr int E = 4 * U;
  constexpr int EH = SG_FEH;
  const uint32_t qa = a & ~3u;
  constexpr uint32_t kStep = 4 * kFThreads * U;
  // (unpredicated loads, clamped to the run's last quad: a load under a
  // branch makes the compiler wait for every load in flight at the join, the
  // next steps' included -- the step then paid a whole memory latency)
  const uint32_t qlast = (b - 1) & ~3u;
  auto load = [&](uint32_t q0, uint32_t(&en)[E]) {
#pragma unroll
    for (int u = 0; u < U; u++) {
      const uint32_t q = min(q0 + 4 * kFThreads * u, qlast);
      const v4u32 t = __builtin_nontemporal_load(reinterpret_cast<const v4u32*>(v1 + q));
      en[4 * u] = t[0];
      en[4 * u + 1] = t[1];
      en[4 * u + 2] = t[2];
      en[4 * u + 3] = t[3];
    }
  };
  // Three entry buffers in rotation (a register copy from a buffer whose
  // loads are in flight would wait for them): step i tests one while the
  // next two steps' loads land in the others.
  uint32_t bA[E], bB[E], bC[E];
  auto step = [&](uint32_t q0, const uint32_t(&e)[E]) {
    if (__builtin_amdgcn_readfirstlane(__hip_atomic_load(&wsurv, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP)) >
        kFWgCap)
      return;  // (overflowing: the partition goes on)
    // the entries inside [a, b): all of them unless the wave's step crosses
    // an end of the part (a uniform test)
    const uint32_t qw = (uint32_t)__builtin_amdgcn_readfirstlane((int)q0);  // lane 0's
    uint32_t vm = (1u << E) - 1;
    const bool full = qw >= a && qw + 4 * 63 + 3 + 4 * kFThreads * (U - 1) < b;
    if (!full) {
      vm = 0;
#pragma unroll
      for (int k = 0; k < E; k++)
        vm |= (q0 + 4 * kFThreads * (k >> 2) + (k & 3) - a < b - a ? 1u : 0u) << k;
    }
    // Branch-free per entry: the header and its overflow list's first block
    // (else the dummy block 0) are read for every entry; a position past the
    // first block (a bucket past 15 values) is not proven here and survives
    // -- the tail re-checks every survivor against the bitmap.
    uint32_t hm = 0;  // bit k: entry k found
    uint32_t sk = 0;  // the last entry not found (the only survivor of most lanes that have one)
#pragma unroll
    for (int k0 = 0; k0 < E; k0 += EH) {
      v4u32 h[EH];
#pragma unroll
      for (int k = 0; k < EH; k++) h[k] = lds[kFOvBlocks + ((e[k0 + k] >> (8 + rb)) & (kFBuckets - 1))];
      v4u32 o[EH];
#pragma unroll
      for (int k = 0; k < EH; k++)
        o[k] = lds[__builtin_elementwise_sub_sat(h[k][3] >> 16, kFPad)];
#pragma unroll
      for (int kk = 0; kk < EH; kk++) {
        const uint32_t rep = ((e[k0 + kk] >> 8) & ((1u << rb) - 1)) * 0x10001u;
        const uint32_t m = m0f_min16(m0f_min16(m0f_min16(h[kk][0] ^ rep, h[kk][1] ^ rep),
                                               m0f_min16(h[kk][2] ^ rep, h[kk][3] ^ rep)),
                                     m0f_min16(m0f_min16(o[kk][0] ^ rep, o[kk][1] ^ rep),
                                               m0f_min16(o[kk][2] ^ rep, o[kk][3] ^ rep)));
        const bool hit = min(m & 0xFFFFu, m >> 16) == 0 || (logh && (e[k0 + kk] & topm) != toph);
        hm |= (hit ? 1u : 0u) << (k0 + kk);
        sk = hit ? sk : e[k0 + kk];
      }
    }
    uint32_t svm = vm & ~hm;  // bit k: entry k survives
    const uint64_t anysv = __ballot(svm != 0);
    if (anysv && full && !__ballot(svm & (svm - 1))) {
      // (rare in the steady state) at most one survivor per lane, entry sk:
      // its position against the spill list (all lanes comparing their part
      // of it, one survivor lane after the other), then one slot per survivor
      bool sv = svm != 0;
      if (nsp) {
        const uint32_t key = (sk >> 8) & 0xFFFFFFu;
        for (uint64_t bal = anysv; bal; bal &= bal - 1) {
          const int l = __builtin_ctzll(bal);
          const uint32_t kl = (uint32_t)__builtin_amdgcn_readlane((int)key, l);
          bool f = false;
#pragma unroll
          for (int i = 0; i < (int)(kFSpill / 64); i++) f |= sp[i] == kl;
          if (__ballot(f) && lane == (uint32_t)l) sv = false;
        }
      }
      const uint64_t bal = __ballot(sv);
      if (bal) {
        const int first = __builtin_ctzll(bal);
        uint32_t at = 0;
        if (lane == (uint32_t)first) at = atomicAdd(&wsurv, (uint32_t)__popcll(bal));
        at = (uint32_t)__shfl((int)at, first) + (uint32_t)__popcll(bal & ((1ull << lane) - 1));
        const uint32_t k = (uint32_t)__builtin_ctz(svm | 0x80000000u);
        if (sv && at < kFWgCap) wsv[at] = make_uint2(q0 + 4 * kFThreads * (k >> 2) + (k & 3), d);
      }
    } else if (anysv) {  // several survivors in a lane, or a step across an end of the part
      if (nsp) {
        // each entry not found so far: its position against the spill list,
        // all lanes comparing their part of it
#pragma unroll
        for (int k = 0; k < E; k++) {
          uint64_t bal = __ballot((svm >> k) & 1u);
          while (bal) {
            const int l = __builtin_ctzll(bal);
            bal &= bal - 1;
            const uint32_t key = (uint32_t)__builtin_amdgcn_readlane((int)(e[k] >> 8), l) & 0xFFFFFFu;
            bool f = false;
#pragma unroll
            for (int i = 0; i < (int)(kFSpill / 64); i++) f |= sp[i] == key;
            if (__ballot(f) && lane == (uint32_t)l) svm &= ~(1u << k);
          }
        }
      }
#pragma unroll
      for (int k = 0; k < E; k++) {
        const bool sv = (svm >> k) & 1u;
        const uint64_t bal = __ballot(sv);
        if (!bal) continue;
        const uint32_t p = q0 + 4 * kFThreads * (k >> 2) + (k & 3);
        const int first = __builtin_ctzll(bal);
        uint32_t at = 0;
        if (lane == (uint32_t)first) at = atomicAdd(&wsurv, (uint32_t)__popcll(bal));
        at = (uint32_t)__shfl((int)at, first) + (uint32_t)__popcll(bal & ((1ull << lane) - 1));
        if (sv && at < kFWgCap) wsv[at] = make_uint2(p, d);
      }
    }
  };
  // A wave-uniform loop with one exit, three steps per iteration (lane 0's
  // position qw; every lane runs every step, the positions past b masked by
  // vm, up to two steps past the end).  vmcnt counts in issue order, and the
  // compiler's waits are merged over every path into the loop head: a
  // per-lane exit (a divergent loop), an exit between steps, or the
  // scheduler issuing bA's prologue loads last each made the first step wait
  // for every load in flight.
  uint32_t q0 = qa + 4 * tid;
  uint32_t qw = (uint32_t)__builtin_amdgcn_readfirstlane((int)q0);
  load(q0, bA);
  __builtin_amdgcn_sched_barrier(0);
  load(q0 + kStep, bB);
  __builtin_amdgcn_sched_barrier(0);
  load(q0 + 2 * kStep, bC);
  __builtin_amdgcn_sched_barrier(0);
  while (qw < b) {
    step(q0, bA);
    load(q0 + 3 * kStep, bA);  // (each buffer reloaded right after its step)
    q0 += kStep;
    step(q0, bB);
    load(q0 + 3 * kStep, bB);
    q0 += kStep;
    step(q0, bC);
    load(q0 + 3 * kStep, bC);
    q0 += kStep;
    qw += 3 * kStep;
  }
  __syncthreads();
  if (tid == 0) {
    const uint32_t c = wsurv;
    wgcnt[wg] = c;
    // the total, and a flag past a region (the host then partitions).  (Once
    // the total for an overflowed region was kFSurvCap + 1: 4096 of them
    // wrapped the 32-bit sum to a small count, the tail took the survivors
    // for fitting, and its table filled -- a hang at 16 workgroups per slice.)
    if (c > kFWgCap)
      atomicOr(nsurv + 1, 1u);
    else
      atomicAdd(nsurv, c);
  }
}

__device__ __forceinline__ uint32_t m0f_hash(uint32_t s) {
  s ^= s >> 16;
  s *= 0x7FEB352Du;
  s ^= s >> 15;
  return s;
}

// the survivors still outside maxSignal (a value past an index cap is only
// re-checked here): each one's record (its pass-1 tile by a search over the
// slice's run starts), then min(record) per signal
__global__ void k_m0_tail_insert(const uint2* __restrict__ surv, const uint32_t* __restrict__ wgcnt,
                                 const uint32_t* __restrict__ v1,
                                 const uint32_t* __restrict__ goff1, uint32_t T, const uint32_t* __restrict__ trec,
                                 const uint32_t* __restrict__ mwords, unsigned long long* __restrict__ table) {
  // grid (4, filter workgroups): the survivors of region y, strided
  const uint32_t nw = min(wgcnt[blockIdx.y], kFWgCap);
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < nw; i += gridDim.x * blockDim.x) {
  const uint2 q = surv[(uint64_t)blockIdx.y * kFWgCap + i];  // (position, slice)
  const uint32_t e = v1[q.x], t = (q.y << 24) | (e >> 8);
  if ((mwords[t >> 5] >> (t & 31)) & 1u) continue;
  const uint32_t s = part_sig(t);
  const uint32_t rec = trec[last_le(goff1 + (uint64_t)q.y * T, 0, T, q.x)] + (e & 0xFFu);
  const unsigned long long key = ((unsigned long long)s << 32) | rec;
  constexpr uint32_t mask = (1u << kFTableBits) - 1;
  // (bounded: at most kFSurvCap keys in 2^21 slots, so a free or equal slot
  // always comes first; the bound only keeps a broken invariant from hanging)
  for (uint32_t h = m0f_hash(s) & mask, probe = 0; probe <= mask; h = (h + 1) & mask, probe++) {
    const unsigned long long old = atomicCAS(&table[h], kFEmpty, key);
    if (old == kFEmpty) break;
    if ((uint32_t)(old >> 32) == s) {
      if (old > key) atomicMin(&table[h], key);
      break;
    }
  }
  }
}

// every distinct new signal: its first owner queued, its bits set (and the
// slot emptied for the next launch)
__global__ void k_m0_tail_flush(unsigned long long* __restrict__ table, uint32_t* __restrict__ mwords,
                                uint32_t* __restrict__ nwords, uint8_t* __restrict__ rec_new) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  const unsigned long long v = table[i];
  if (v == kFEmpty) return;
  table[i] = kFEmpty;
  rec_new[(uint32_t)v] = 1;
  const uint32_t t = part_key((uint32_t)(v >> 32)), bit = 1u << (t & 31);
  atomicOr(&mwords[t >> 5], bit);
  if (nwords) atomicOr(&nwords[t >> 5], bit);
}

// the pinned words the regimes read without a host wait (CtxPinned), with
// m0f_ev; the block is adopted last
int m0f_host_alloc(sg_ctx* ctx) {
  if (ctx->pinned.p) return SG_OK;
  Buf<CtxPinned, true> nb;
  int rc = nb.grow_drop(1, nullptr);
  if (!rc) rc = ctx->m0f_ev.create(hipEventDisableTiming);
  if (!rc) ctx->pinned.swap(nb);
  return rc;
}

// the queued fraction of the last counted partitioned slice, once its copy has landed
void m0f_poll(sg_ctx* ctx) {
  if (ctx->m0f_pending && hipEventQuery(ctx->m0f_ev) == hipSuccess) {
    ctx->m0f_pending = false;
    ctx->m0f_queued = (double)ctx->pinned.p->m0f_queued / (double)(ctx->m0f_nrec ? ctx->m0f_nrec : 1);
  }
}

// The M0 filter on pass 1's output (bp as partition_pass1 left it): *done when
// its tail has produced the flags and set updates; otherwise the survivors
// overflowed and the caller goes on with pass 2 and the bucket stage (nothing
// written yet).
int m0_filter(sg_ctx* ctx, const BucketPlan& bp, uint32_t* mwords, uint32_t* nwords, uint8_t* d_rec_new, bool* done) {
  const uint32_t* v1 = bp.at<uint32_t>(ctx, kV1);
  const uint32_t* goff1 = bp.at<uint32_t>(ctx, kO1);
  *done = false;
  if (!ctx->m0f.p) {  // (adopted once its table is empty)
    DevBuf<char> nb;
    const int rc = nb.grow_drop(m0f_bytes(), nullptr);
    if (rc) return rc;
    SG_HIP(hipMemsetAsync(m0f_bind(nb.p).table, 0xFF, 8ull << kFTableBits, ctx->stream));
    ctx->m0f.swap(nb);
  }
  const M0F f = m0f_bind(ctx->m0f.p);
  const uint32_t T = (uint32_t)bp.T;
  SG_HIP(hipMemsetAsync(f.cursor, 0, kFIdx * 4 + 256 + kFIdx * 4, ctx->stream));  // cursors, survivor and spill counts
  // the index in 2^logh parts per slice (auto: 1, or 2 after a part
  // overflowed and the survivors with it; 4 only forced; the filter's
  // workgroups stay 2048: kFParts >> logh per slice and part, each part's pass
  // reading the whole slice run)
  const int logh = ctx->opt[kOptM0Halves] >= 0 ? (int)ctx->opt[kOptM0Halves] : ctx->m0f_logh;
  {
    ScopedTimer tm(ctx, "m0_index");
    auto ki = logh == 0 ? k_m0_index<0> : logh == 1 ? k_m0_index<1> : k_m0_index<2>;
    hipLaunchKernelGGL(ki, dim3(kFBuckets / 256, 256u << logh), dim3(256), 0, ctx->stream, (const uint32_t*)mwords,
                       f.tab, f.ovals, f.cursor, f.nspill, f.spill, f.nsurv);
  }
  {
    ScopedTimer tm(ctx, "m0_filter");
    auto kf = logh == 0 ? k_m0_filter<0> : logh == 1 ? k_m0_filter<1> : k_m0_filter<2>;
    hipLaunchKernelGGL(kf, dim3(kFParts >> logh, 256, 1u << logh), dim3(kFThreads), 0, ctx->stream, v1, goff1, T,
                       (const uint4*)f.tab, (const uint16_t*)f.ovals, (const uint32_t*)f.cursor,
                       (const uint32_t*)f.nspill, (const uint32_t*)f.spill, f.surv, f.nsurv, f.wgcnt);
  }
  SG_HIP(hipGetLastError());
  // (the host ingest's pinned staging may be in a DMA now: a pageable read)
  uint32_t nsv[3] = {0, 0, 0};
  SG_HIP(hipMemcpyAsync(nsv, f.nsurv, 12, hipMemcpyDeviceToHost, ctx->stream));
  SG_HIP(hipStreamSynchronize(ctx->stream));
  const uint32_t ns = nsv[0];
  ctx->m0f_survivors = nsv[1] ? kFSurvCap + 1 : ns;
  if (nsv[1] || ns > kFSurvCap) {
    ctx->m0f_fallback++;
    ctx->m0f_last = 0;
    // auto: a fallback on a slice that was expected to filter (a maxSignal
    // past the index's capacity, or a novelty burst) -- the next 1, 2, 4 ..
    // 64 slices are not tried
    if (ctx->opt[kOptM0Halves] < 0 && nsv[2] && ctx->m0f_logh < 1) {
      // an index part overflowed: two parts, tried again at once (each part's
      // pass streams the whole run: at 18M signals two parts filter in 1.6 ms
      // against 2.8 ms of pass 2 and buckets; four, at 41M, took 3.9 ms --
      // past two parts auto backs off to the partition instead)
      ctx->m0f_logh++;
    } else if (ctx->opt[kOptM0Filter] < 0) {
      ctx->m0f_backoff = ctx->m0f_backoff ? std::min<uint32_t>(2 * ctx->m0f_backoff, 64) : 1;
      ctx->m0f_skip = ctx->m0f_backoff;
    }
    return SG_OK;
  }
  if (ns) {
    ScopedTimer tm(ctx, "m0_tail");
    hipLaunchKernelGGL(k_m0_tail_insert, dim3(4, 256 * kFParts), dim3(256), 0, ctx->stream,
                       (const uint2*)f.surv, (const uint32_t*)f.wgcnt, v1, goff1, T,
                       (const uint32_t*)bp.at<uint32_t>(ctx, kTR), (const uint32_t*)mwords, f.table);
    hipLaunchKernelGGL(k_m0_tail_flush, dim3((1u << kFTableBits) / 256), dim3(256), 0, ctx->stream, f.table, mwords,
                       nwords, d_rec_new);
  }
  SG_HIP(hipGetLastError());
  ctx->m0f_used++;
  ctx->m0f_last = 1;
  ctx->m0f_backoff = ctx->m0f_skip = 0;
  *done = true;
  return SG_OK;
}

// queued records of a partitioned slice: one add per block
__global__ void k_count_flags(const uint8_t* __restrict__ f, uint64_t n, uint32_t* __restrict__ out) {
  uint32_t c = 0;
  for (uint64_t i = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) * 4; i < n; i += (uint64_t)gridDim.x * blockDim.x * 4)
    for (int k = 0; k < 4; k++) c += i + k < n && f[i + k] ? 1u : 0u;
  c = sgd::wave_incl_add(c);
  if ((threadIdx.x & 63) == 63 && c) atomicAdd(out, c);
}

// After a partitioned slice (auto regime): its queued records counted on the
// device and copied to pinned memory behind an event, read by a later m0f_try.
int m0f_note_partitioned(sg_ctx* ctx, const uint8_t* d_rec_new, uint64_t nrec) {
  ctx->m0f_last = 0;
  // (read by the auto regimes of the M0 filter and of the split bucket stage)
  if ((ctx->opt[kOptM0Filter] >= 0 && ctx->opt[kOptFlagSkip] >= 0) || ctx->m0f_pending) return SG_OK;
  int rc = m0f_host_alloc(ctx);
  if (rc) return rc;
  uint32_t* dcnt = &ctx->dev.p->m0f_queued;
  SG_HIP(hipMemsetAsync(dcnt, 0, 4, ctx->stream));
  hipLaunchKernelGGL(k_count_flags, dim3(std::min<uint64_t>(256, div_up(nrec, 1024))), dim3(256), 0, ctx->stream,
                     d_rec_new, nrec, dcnt);
  SG_HIP(hipMemcpyAsync(&ctx->pinned.p->m0f_queued, dcnt, 4, hipMemcpyDeviceToHost, ctx->stream));
  SG_HIP(hipEventRecord(ctx->m0f_ev, ctx->stream));
  ctx->m0f_pending = true;
  ctx->m0f_nrec = nrec;
  return SG_OK;
}

// The M0 filter's regime: option m0_filter 1 always tries it, 0 never.  auto
// (the fuzzer's loop, batch after batch) tries it after a slice it filtered,
// and after a partitioned slice whose queued fraction was below kFTryQueued
// (in the steady state 9 % of the records are queued, in a fresh batch all:
// fresh batches then never pay for it); on the context's first slice it is
// tried.  A queued count still in flight keeps the previous choice.  After a
// fallback it backs off (m0f_skip): a low-novelty batch whose maxSignal is
// past the index's capacity would otherwise fall back on every slice.
constexpr double kFTryQueued = 0.25;
bool m0f_try(sg_ctx* ctx) {
  const int64_t o = ctx->opt[kOptM0Filter];
  if (o >= 0) return o != 0;
  m0f_poll(ctx);
  if (ctx->m0f_skip) {  // (backing off after fallbacks)
    ctx->m0f_skip--;
    return false;
  }
  if (ctx->m0f_last < 0) return true;
  if (ctx->m0f_last == 1) return true;
  return ctx->m0f_queued >= 0 && ctx->m0f_queued < kFTryQueued;
}

}  // namespace sg
