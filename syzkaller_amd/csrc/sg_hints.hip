// Comparison hints: the comparison half of the executor output reader
// (pkg/ipc/ipc_linux.go:257-304) and shrinkExpand (prog/hints.go:150-177) over
// a batch.  A call's CompMap is kept as the reader's AddComp sequence, a list
// of {key, value} pairs; the hint stage is a join of the argument values'
// shrunk / sign-extended forms against the pairs' keys.
//
// Ingest (sg_ipc_comps*):
//  - k_comps_walk: a wave per program.  The record headers stay a chain; a
//    comparison region is scanned 256 words at a time: every word is a
//    transition function of a 6-state automaton (0 a type word is due, 1..4
//    operand words left, 5 a bad type, absorbing), the functions compose, and
//    a wave scan of the compositions gives every word its state.  Writes per
//    record the region's start, its comparison count and its pair count, per
//    program the status (sg_ipc_parse's, path for path);
//  - scan of the pair counts -> pair_off;
//  - k_comps_emit: a wave per record repeats the region scan and writes the
//    pairs in the reader's order.
// Join (sg_hints_replacers*):
//  - k_hints_join: a workgroup per record; tiles of 512 value slots, their at
//    most 7 mutants each in an LDS open-addressing table (8192 entries, load
//    <= 1/2), the record's pairs streamed against it (records of at most 64
//    slots: one tile in a 1024-entry table); counted in one pass, appended in
//    a second;
//  - radix sorts (the distinct-values stage is sg_rank.hip's): the candidates'
//    replacers -> the distinct replacers U; then the keys (slot << 32 | rank in
//    U) -> first occurrences -> rep_off, reps.
// Every loop is bounded by a count known on entry (region words, table
// capacity, pair count) or halves its interval (sgd::lb64).
#include "sg_rank.h"

namespace sg {

enum : int32_t {  // include/syzsig.h SG_IPC_*, as sg_ipc.hip
  kOk = 0,
  kNoNcmd = 1,
  kShortHeader = 2,
  kBadIndex = 3,
  kBadCallNum = 4,
  kDouble = 5,
  kSignalSize = 6,
  kCoverSize = 7,
  kCompsShort = 8,
  kCompsType = 9,
};

// ---- the comparison automaton ----------------------------------------------
// A transition function is its six results, 3 bits each: bits 3s..3s+2 = f(s).
constexpr uint32_t kFnTail = (0u << 3) | (1u << 6) | (2u << 9) | (3u << 12) | (5u << 15);  // s -> s - 1, 5 -> 5
constexpr uint32_t kFnId = 0u | (1u << 3) | (2u << 6) | (3u << 9) | (4u << 12) | (5u << 15);
constexpr int kCmpWords = 4;                   // consecutive words per lane
constexpr uint32_t kCmpChunk = 64 * kCmpWords;  // words per wave step

__device__ __forceinline__ uint32_t cmp_fn(uint32_t w) {
  // ipc_linux.go:266 (typ > 7), :272 (two operand words when (typ & 6) == 6, four otherwise)
  return (w > 7u ? 5u : ((w & 6u) == 6u ? 2u : 4u)) | kFnTail;
}
__device__ __forceinline__ uint32_t cmp_apply(uint32_t f, uint32_t s) { return (f >> (3 * s)) & 7u; }
// first f, then g
__device__ __forceinline__ uint32_t cmp_compose(uint32_t f, uint32_t g) {
  uint32_t h = 0;
#pragma unroll
  for (int s = 0; s < 6; s++) h |= cmp_apply(g, cmp_apply(f, s)) << (3 * s);
  return h;
}

// One wave step over words [base, base + 256) of a region that ends at `end`:
// lane l holds words base + 4l .. base + 4l + 3.
struct CmpChunk {
  uint32_t w[kCmpWords];
  uint32_t valid;  // bit k: word k lies before `end`
  uint32_t tmask;  // bit k: word k is a type word
  uint32_t dmask;  // bit k: word k is the last operand word of a comparison
  uint32_t tbase;  // type words of the region before this lane's words
};

// state / ntypes: the automaton's state and the type words seen before `base`
// (wave-uniform), advanced past the chunk.  All 64 lanes call it.
__device__ __forceinline__ void cmp_scan_chunk(const uint32_t* __restrict__ out, uint64_t base, uint64_t end,
                                               uint32_t lane, uint32_t& state, uint32_t& ntypes, CmpChunk& c) {
  const uint64_t p0 = base + (uint64_t)lane * kCmpWords;
  uint32_t f = kFnId;
  c.valid = 0;
#pragma unroll
  for (int k = 0; k < kCmpWords; k++) {
    const bool v = p0 + k < end;
    c.w[k] = v ? out[p0 + k] : 0u;
    if (v) {
      c.valid |= 1u << k;
      f = cmp_compose(f, cmp_fn(c.w[k]));
    }
  }
  // inclusive scan of the compositions, lane order
  uint32_t incl = f;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const uint32_t t = __shfl_up(incl, d);
    if ((int)lane >= d) incl = cmp_compose(t, incl);
  }
  const uint32_t prev = __shfl_up(incl, 1);
  uint32_t s = cmp_apply(lane ? prev : kFnId, state);
  c.tmask = 0;
  c.dmask = 0;
#pragma unroll
  for (int k = 0; k < kCmpWords; k++)
    if (c.valid & (1u << k)) {
      if (s == 0) c.tmask |= 1u << k;
      const uint32_t sn = cmp_apply(cmp_fn(c.w[k]), s);
      if (s != 0 && sn == 0) c.dmask |= 1u << k;
      s = sn;
    }
  const uint32_t nt = (uint32_t)__popc(c.tmask);
  const uint32_t tincl = sgd::wave_incl_add(nt);
  c.tbase = ntypes + tincl - nt;
  ntypes += __shfl(tincl, 63);
  state = cmp_apply(__shfl(incl, 63), state);
}

// The reader's AddComp calls of the comparison whose type word `typ` is at
// word p (ipc_linux.go:272-302): 0, 1 or 2 pairs; its operands, when all its
// words lie before `end`.
__device__ __forceinline__ uint32_t cmp_pairs(const uint32_t* __restrict__ out, uint64_t p, uint64_t end, uint32_t typ,
                                              uint64_t& op1, uint64_t& op2) {
  const uint32_t k = (typ & 6u) == 6u ? 2u : 4u;
  if (end - p <= k) return 0;  // cut: the program fails, its pairs are dropped
  if (k == 2) {
    op1 = out[p + 1];
    op2 = out[p + 2];
  } else {
    op1 = (uint64_t)out[p + 1] | ((uint64_t)out[p + 2] << 32);
    op2 = (uint64_t)out[p + 3] | ((uint64_t)out[p + 4] << 32);
  }
  if (op1 == op2) return 0;       // :290-293
  return (typ & 1u) ? 1u : 2u;    // :294-302: (op2, op1), and (op1, op2) unless one operand was const
}

struct CompsArgs {
  const uint32_t* out;
  const uint64_t* out_off;   // [nprog+1]
  const uint64_t* call_off;  // [nprog+1]
  const uint32_t* call_nums; // [nrec] or null
  uint64_t nprog;
  int32_t* status;    // [nprog]
  uint8_t* seen;      // [nrec] workspace, zeroed: Signal != nil
  uint64_t* cmp_src;  // [nrec] zeroed: word position of the record's comparisons
  uint64_t* cmp_end;  // [nrec] zeroed: end of its program's region
  uint32_t* cmp_n;    // [nrec] zeroed: its comparison count
  uint32_t* pair_cnt; // [nrec] zeroed
};

// a wave per program; the header walk is k_ipc_walk's (sg_ipc.hip), check for check
__global__ __launch_bounds__(256) void k_comps_walk(CompsArgs a) {
  const uint64_t p = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (p >= a.nprog) return;
  const uint32_t lane = threadIdx.x & 63;
  const uint64_t r0 = a.call_off[p], r1 = a.call_off[p + 1], ncalls = r1 - r0;
  uint64_t pos = a.out_off[p];
  const uint64_t end = a.out_off[p + 1];
  const uint32_t* __restrict__ w = a.out;
  int32_t st = kOk;
  if (pos >= end) {
    if (lane == 0) a.status[p] = kNoNcmd;
    return;
  }
  const uint32_t ncmd = w[pos++];
  for (uint32_t i = 0; i < ncmd && st == kOk; i++) {
    if (end - pos < 7) {
      st = kShortHeader;
      break;
    }
    const uint32_t hv = lane < 7 ? w[pos + lane] : 0u;
    const uint32_t idx = __shfl(hv, 0), num = __shfl(hv, 1), nsig = __shfl(hv, 4), ncov = __shfl(hv, 5),
                   ncomps = __shfl(hv, 6);
    pos += 7;
    if (idx >= ncalls) {
      st = kBadIndex;
      break;
    }
    const uint64_t r = r0 + idx;
    // lane 0 alone reads and writes the record's workspace
    uint32_t chk = 0;
    if (lane == 0) chk = (a.call_nums && a.call_nums[r] != num ? 1u : 0u) | (a.seen[r] ? 2u : 0u);
    chk = __shfl(chk, 0);
    if (chk & 1u) {
      st = kBadCallNum;
      break;
    }
    if (chk & 2u) {
      st = kDouble;
      break;
    }
    if (nsig > end - pos) {
      st = kSignalSize;
      break;
    }
    if (lane == 0) a.seen[r] = 1;
    pos += nsig;
    if (ncov > end - pos) {
      st = kCoverSize;
      break;
    }
    pos += ncov;
    if (ncomps == 0) continue;
    // the comparison region: from pos until the ncomps-th comparison is
    // complete, a bad type is met, or the program's region ends
    const uint64_t src = pos;
    uint32_t state = 0, ntypes = 0, npairs = 0;
    bool closed = false;
    for (uint64_t base = src; base < end; base += kCmpChunk) {
      CmpChunk c;
      cmp_scan_chunk(w, base, end, lane, state, ntypes, c);
      // this lane's first event in the reader's order: a bad type at one of
      // the ncomps comparisons, or the last operand word of the ncomps-th
      uint32_t ev = 0, seen_t = c.tbase;
#pragma unroll
      for (int k = 0; k < kCmpWords; k++) {
        if (ev) break;
        if (c.tmask & (1u << k)) {
          if (seen_t < ncomps) {
            if (c.w[k] > 7u) {
              ev = 8u | 4u | k;  // bad type
            } else {
              uint64_t o1, o2;
              npairs += cmp_pairs(w, base + (uint64_t)lane * kCmpWords + k, end, c.w[k], o1, o2);
            }
          }
          seen_t++;
        } else if ((c.dmask & (1u << k)) && seen_t == ncomps) {
          ev = 8u | k;  // complete
        }
      }
      const uint64_t evl = __ballot(ev != 0);
      if (evl) {
        const int first = __ffsll((unsigned long long)evl) - 1;
        const uint32_t e = __shfl(ev, first);
        if (e & 4u)
          st = kCompsType;
        else
          pos = base + (uint64_t)first * kCmpWords + (e & 3u) + 1;
        closed = true;
        break;
      }
    }
    if (!closed) st = kCompsShort;
    if (st != kOk) break;
    // pairs of the lanes' type words: those past the closing word belong to
    // no comparison (seen_t >= ncomps) and were not counted
    const uint32_t tot = __shfl(sgd::wave_incl_add(npairs), 63);
    if (lane == 0) {
      a.cmp_src[r] = src;
      a.cmp_end[r] = end;
      a.cmp_n[r] = ncomps;
      a.pair_cnt[r] = tot;
    }
  }
  if (lane == 0) {
    a.status[p] = st;
    // a program whose output failed to parse contributes no comparisons
    // (the rule sg_ipc_parse applies to signal and cover)
    if (st != kOk)
      for (uint64_t r = r0; r < r1; r++) a.pair_cnt[r] = 0;
  }
}

// a wave per record: its pairs, in the reader's order, at pairs[pair_off[r] ..]
__global__ __launch_bounds__(256) void k_comps_emit(const uint32_t* __restrict__ out, const uint64_t* __restrict__ cmp_src,
                                                    const uint64_t* __restrict__ cmp_end,
                                                    const uint32_t* __restrict__ cmp_n,
                                                    const uint64_t* __restrict__ pair_off, uint64_t nrec, uint64_t cap,
                                                    uint64_t* __restrict__ pairs) {
  const uint64_t r = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= nrec) return;
  if (pair_off[nrec] > cap) return;
  const uint64_t o0 = pair_off[r], o1 = pair_off[r + 1];
  if (o0 == o1) return;
  const uint32_t lane = threadIdx.x & 63;
  const uint64_t src = cmp_src[r], end = cmp_end[r];
  const uint32_t ncomps = cmp_n[r];
  uint32_t state = 0, ntypes = 0;
  uint64_t run = o0;
  for (uint64_t base = src; base < end && ntypes < ncomps; base += kCmpChunk) {
    CmpChunk c;
    cmp_scan_chunk(out, base, end, lane, state, ntypes, c);
    uint64_t a1[2] = {0, 0}, a2[2] = {0, 0};  // a lane's 4 words hold at most 2 type words (a comparison is >= 3 words)
    uint32_t np[2] = {0, 0}, seen_t = c.tbase;
    int j = 0;
#pragma unroll
    for (int k = 0; k < kCmpWords; k++)
      if (c.tmask & (1u << k)) {
        if (seen_t < ncomps && c.w[k] <= 7u && j < 2) {
          uint64_t x1 = 0, x2 = 0;
          const uint32_t n = cmp_pairs(out, base + (uint64_t)lane * kCmpWords + k, end, c.w[k], x1, x2);
          if (j == 0) {
            np[0] = n;
            a1[0] = x1;
            a2[0] = x2;
          } else {
            np[1] = n;
            a1[1] = x1;
            a2[1] = x2;
          }
          j++;
        }
        seen_t++;
      }
    const uint32_t mine = np[0] + np[1];
    const uint32_t incl = sgd::wave_incl_add(mine);
    uint64_t at = run + incl - mine;
#pragma unroll
    for (int q = 0; q < 2; q++) {
      if (np[q] >= 1 && at < o1) {
        pairs[2 * at] = a2[q];  // AddComp(op2, op1)
        pairs[2 * at + 1] = a1[q];
      }
      if (np[q] == 2 && at + 1 < o1) {
        pairs[2 * at + 2] = a1[q];  // AddComp(op1, op2)
        pairs[2 * at + 3] = a2[q];
      }
      at += np[q];
    }
    run += __shfl(incl, 63);
  }
}

// ---- shrinkExpand ----------------------------------------------------------
// prog/rand.go:59-67 specialInts: 0, 1, and 2^k - 1, 2^k, 2^k + 1 for some k.
// In registers: a match tests one lane's value inside a divergent probe loop,
// where a table walk would be 33 dependent loads per match.
constexpr uint64_t kSpecialPow = (1ull << 5) | (1ull << 6) | (1ull << 7) | (1ull << 8) | (1ull << 9) | (1ull << 10) |
                                 (1ull << 11) | (1ull << 12) | (1ull << 15) | (1ull << 16) | (1ull << 31) |
                                 (1ull << 32);  // k with 2^k and 2^k - 1 special: 31, 32, ..., 4095, 4096, 2^15, 2^16, 2^31, 2^32
constexpr uint64_t kSpecialPlus = (1ull << 7) | (1ull << 8) | (1ull << 10) | (1ull << 15) | (1ull << 16) |
                                  (1ull << 31) | (1ull << 32);  // k with 2^k + 1 special: 129, 257, 1025, ...

__host__ __device__ __forceinline__ bool is_special(uint64_t x) {
  if (x <= 1) return true;
  if (x > 0x100000001ull) return false;
  // 2 <= x: at most one of x, x + 1 is a power of two; x - 1 and x + 1 both only for x = 3 (not special either way)
  if ((x & (x - 1)) == 0) return (kSpecialPow >> __builtin_ctzll(x)) & 1;
  if (((x + 1) & x) == 0) return (kSpecialPow >> __builtin_ctzll(x + 1)) & 1;
  if (((x - 1) & (x - 2)) == 0) return (kSpecialPlus >> __builtin_ctzll(x - 1)) & 1;
  return false;
}

// Two shapes of the join workgroup: records of up to kHjSmall value slots (a
// fuzzer's calls: a few arguments) take 256 threads and a 1024-entry table,
// 12.5 KiB of LDS, so eight workgroups share a CU; larger records take 1024
// threads and tiles of 512 slots in an 8192-entry table (100 KiB, one per CU).
// Both are launched over all records and a workgroup whose record belongs to
// the other shape leaves at once.  A table has 16 entries per slot of its
// tile: at most 7 are taken, so its load stays below 1/2.
constexpr uint32_t kHjSmall = 64;
constexpr uint32_t kHjTile = 512;   // value slots per tile of the large shape
// The count pass's scalars: {a record's count passed 32 bits, pair_off[nrec]},
// then the AND and the OR of the replacers, each in kHjStripes words (record r
// in stripe r % kHjStripes: 32 Ki workgroups on one address would queue up).
constexpr uint32_t kHjStripes = 64;
constexpr uint32_t kHjScal = 2 + 2 * kHjStripes;
constexpr uint32_t kHjEmpty = 0xFFFFFFFFu;

__device__ __forceinline__ uint32_t hj_hash(uint64_t k, uint32_t lg) {
  return (uint32_t)((k * 0x9E3779B97F4A7C15ull) >> (64 - lg));
}
// bits of a mutant of size code sc (8 << sc bits; 3: the whole value)
__device__ __forceinline__ uint64_t hj_mask(uint32_t sc) { return sc >= 3 ? ~0ull : (1ull << (8u << sc)) - 1; }

struct JoinArgs {
  const uint64_t* pair_off;  // [nrec+1]
  const uint64_t* pairs;     // {key, value}
  const uint64_t* val_off;   // [nrec+1]
  const uint64_t* vals;
  uint64_t nrec;
  uint64_t nv_lo, nv_hi;      // the launch's records: nv_lo < value slots <= nv_hi
  uint32_t* cnt;              // [nrec] (zeroed) count form: the record's candidates (low 32 bits)
  unsigned long long* scal;   // count form: kHjScal words, see below
  const uint64_t* cand_off;   // [nrec+1] emit form
  uint32_t* cslot;            // emit form: a candidate's global slot
  uint64_t* crep;             //            and its replacer
};

// A workgroup per record.  EMIT false: counts the record's candidates; true:
// appends them at cand_off[r] (their order within the record is irrelevant).
template <bool EMIT, int kHjThreads, uint32_t kTileSlots>
__global__ __launch_bounds__(kHjThreads) void k_hints_join(JoinArgs a) {
  constexpr uint32_t kHjCap = 16 * kTileSlots;
  static_assert(kTileSlots <= (uint32_t)kHjThreads && kTileSlots <= 0x10000u, "a thread per slot; 16-bit local slots");
  __shared__ uint64_t tkey[kHjCap];
  __shared__ uint32_t tmeta[kHjCap];  // local slot | size code << 16
  __shared__ uint64_t sval[kTileSlots];
  __shared__ unsigned long long red[3];
  __shared__ uint32_t cursor;
  const uint64_t r = blockIdx.x;
  const uint32_t tid = threadIdx.x;
  const uint64_t p0 = a.pair_off[r], p1 = a.pair_off[r + 1], v0 = a.val_off[r], v1 = a.val_off[r + 1];
  if (!EMIT && r == 0 && tid == 0 && a.nv_lo == 0) atomicExch(&a.scal[1], (unsigned long long)a.pair_off[a.nrec]);
  if (v1 - v0 <= a.nv_lo || v1 - v0 > a.nv_hi) return;  // the other shape's record (or no values)
  if (tid == 0) {
    red[0] = 0;
    red[1] = ~0ull;
    red[2] = 0;
    cursor = 0;
  }
  const uint64_t cbase = EMIT ? a.cand_off[r] : 0, cend = EMIT ? a.cand_off[r + 1] : 0;
  uint64_t mine = 0, m_and = ~0ull, m_or = 0;
  if (p1 > p0 && (!EMIT || cend > cbase))
    for (uint64_t t0 = v0; t0 < v1; t0 += kTileSlots) {
      const uint32_t ns = (uint32_t)min<uint64_t>(kTileSlots, v1 - t0);
      // capacity: the power of two >= 16 ns (>= 2 * 7 ns), at least 64
      uint32_t lg = 6;
      while ((1u << lg) < 16u * ns) lg++;  // <= log2 kHjCap
      const uint32_t cap = 1u << lg, hm = cap - 1;
      __syncthreads();  // the previous tile's probes are done
      for (uint32_t i = tid; i < cap; i += kHjThreads) tmeta[i] = kHjEmpty;
      if (tid < ns) sval[tid] = a.vals[t0 + tid];
      __syncthreads();
      if (tid < ns) {
        // hints.go:155-161: the mutants in increasing size; of equal values the
        // last assignment (the largest size) stays
        const uint64_t v = sval[tid];
        uint64_t m[7];
        uint32_t sc[7];
        bool live[7];
#pragma unroll
        for (int s = 0; s < 3; s++) {
          const uint64_t mk = hj_mask(s);
          m[2 * s] = v & mk;
          sc[2 * s] = s;
          live[2 * s] = true;
          m[2 * s + 1] = v | ~mk;
          sc[2 * s + 1] = s;
          live[2 * s + 1] = (v >> ((8u << s) - 1)) & 1u;
        }
        m[6] = v;
        sc[6] = 3;
        live[6] = true;
#pragma unroll
        for (int i = 0; i < 7; i++) {
          bool keep = live[i];
#pragma unroll
          for (int j = i + 1; j < 7; j++) keep = keep && !(live[j] && m[j] == m[i]);
          if (keep) {
            uint32_t h = hj_hash(m[i], lg);
            for (uint32_t step = 0; step < cap; step++) {
              if (atomicCAS(&tmeta[h], kHjEmpty, tid | (sc[i] << 16)) == kHjEmpty) {
                tkey[h] = m[i];
                break;
              }
              h = (h + 1) & hm;
            }
          }
        }
      }
      __syncthreads();
      for (uint64_t q = p0 + tid; q < p1; q += kHjThreads) {
        const uint64_t key = a.pairs[2 * q], nv = a.pairs[2 * q + 1];
        uint32_t h = hj_hash(key, lg);
        for (uint32_t step = 0; step < cap; step++) {
          const uint32_t meta = tmeta[h];
          if (meta == kHjEmpty) break;
          if (tkey[h] == key) {
            const uint64_t mask = hj_mask(meta >> 16);
            const uint64_t hi = nv & ~mask;  // hints.go:166
            if ((hi == 0 || hi == ~mask) && !is_special(nv & mask)) {
              const uint32_t ls = meta & 0xFFFFu;
              const uint64_t rep = (sval[ls] & ~mask) | (nv & mask);  // :170
              if (EMIT) {
                const uint64_t at = cbase + atomicAdd(&cursor, 1u);
                if (at < cend) {
                  a.cslot[at] = (uint32_t)(t0 + ls);
                  a.crep[at] = rep;
                }
              } else {
                mine++;
                m_and &= rep;
                m_or |= rep;
              }
            }
          }
          h = (h + 1) & hm;
        }
      }
    }
  if (EMIT) return;
  for (int d = 32; d; d >>= 1) {
    mine += __shfl_xor(mine, d);
    m_and &= __shfl_xor(m_and, d);
    m_or |= __shfl_xor(m_or, d);
  }
  __syncthreads();  // red[] is set
  if ((tid & 63) == 0 && mine) {
    atomicAdd(&red[0], (unsigned long long)mine);
    atomicAnd(&red[1], (unsigned long long)m_and);
    atomicOr(&red[2], (unsigned long long)m_or);
  }
  __syncthreads();
  if (tid == 0) {
    a.cnt[r] = (uint32_t)red[0];
    if (red[0]) {
      if (red[0] >> 32) atomicOr(&a.scal[0], 1ull);
      atomicAnd(&a.scal[2 + r % kHjStripes], red[1]);
      atomicOr(&a.scal[2 + kHjStripes + r % kHjStripes], red[2]);
    }
  }
}

// keys[i] = slot << 32 | rank of candidate i's replacer among the nu distinct ones: the rank and the
// pack in one kernel (sg_rank.hip's rank, then its pack, would be a launch and an array more)
__global__ void k_hj_rank(const uint32_t* __restrict__ cslot, const uint64_t* __restrict__ crep, uint64_t n,
                          const uint64_t* __restrict__ u, const uint64_t* __restrict__ nu_at,
                          uint64_t* __restrict__ keys) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  // the first j with u[j] >= crep[i]: the replacer is there
  keys[i] = ((uint64_t)cslot[i] << 32) | (uint32_t)sgd::lb64(u, *nu_at, crep[i]);
}
__global__ void k_hj_slot_count(const uint64_t* __restrict__ keys, const uint32_t* __restrict__ flags, uint64_t n,
                                uint32_t* __restrict__ scnt) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n && flags[i]) atomicAdd(&scnt[keys[i] >> 32], 1u);
}
__global__ void k_hj_write(const uint64_t* __restrict__ keys, const uint32_t* __restrict__ flags,
                           const uint64_t* __restrict__ pos, uint64_t n, const uint64_t* __restrict__ u,
                           const uint64_t* __restrict__ total_at, uint64_t cap, uint64_t* __restrict__ reps) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n || *total_at > cap) return;
  if (flags[i]) reps[pos[i]] = u[(uint32_t)keys[i]];
}

// both shapes of the join over all records
template <bool EMIT>
static void join_launch(sg_ctx* ctx, JoinArgs a) {
  a.nv_lo = 0;
  a.nv_hi = kHjSmall;
  hipLaunchKernelGGL((k_hints_join<EMIT, 256, kHjSmall>), dim3((uint32_t)a.nrec), dim3(256), 0, ctx->stream, a);
  a.nv_lo = kHjSmall;
  a.nv_hi = ~0ull;
  hipLaunchKernelGGL((k_hints_join<EMIT, 1024, kHjTile>), dim3((uint32_t)a.nrec), dim3(1024), 0, ctx->stream, a);
}

// The join and the sorts behind sg_hints_replacers* and sg_hints_from_kcov*
// (sg_internal.h); ctx lock held.  With reps_in_ws the replacers go to a
// workspace buffer of min(cap, candidates) slots (*ws_reps), for the host form
// to copy out.
int hints_replacers(sg_ctx* ctx, const uint64_t* d_pair_off, const uint64_t* d_pairs, uint64_t nrec,
                    const uint64_t* d_val_off, const uint64_t* d_vals, uint64_t nvals, uint64_t* d_rep_off,
                    uint64_t* d_reps, uint64_t cap, bool reps_in_ws, uint64_t** ws_reps) {
  if (ws_reps) *ws_reps = nullptr;
  ctx->hints_cands = 0;
  if (nvals >= (1ull << 32)) {
    set_error("sg_hints_replacers: %llu value slots (the limit is 2^32 - 1)", (unsigned long long)nvals);
    return SG_EINVAL;
  }
  if (nrec == 0 || nvals == 0) {
    SG_HIP(hipMemsetAsync(d_rep_off, 0, (nvals + 1) * 8, ctx->stream));
    return SG_OK;
  }
  WsPlan p;
  const size_t o_cnt = p.add(nrec * 4), o_coff = p.add((nrec + 1) * 8), o_scal = p.add(kHjScal * 8);
  const size_t scan_a = p.total;
  const size_t need_a = p.total + scan_ws_bytes(nrec);
  int rc = ws_reserve(ctx, need_a);
  if (rc) return rc;
  JoinArgs a{};
  a.pair_off = d_pair_off;
  a.pairs = d_pairs;
  a.val_off = d_val_off;
  a.vals = d_vals;
  a.nrec = nrec;
  unsigned long long got[kHjScal], init[kHjScal], total = 0;
  for (uint32_t i = 0; i < kHjScal; i++) init[i] = i >= 2 && i < 2 + kHjStripes ? ~0ull : 0ull;
  auto count = [&]() -> int {
    a.cnt = (uint32_t*)ws_at(ctx, o_cnt);
    a.scal = (unsigned long long*)ws_at(ctx, o_scal);
    SG_HIP(hipMemcpyAsync(a.scal, init, sizeof(init), hipMemcpyHostToDevice, ctx->stream));
    SG_HIP(hipMemsetAsync(a.cnt, 0, nrec * 4, ctx->stream));
    {
      ScopedTimer tm(ctx, "hints_join");
      join_launch<false>(ctx, a);
    }
    SG_HIP(hipGetLastError());
    return scan_counts(ctx, a.cnt, (uint64_t*)ws_at(ctx, o_coff), nrec, scan_a);
  };
  if (nrec >= (1ull << 31)) return SG_EINVAL;
  rc = count();
  if (rc) return rc;
  // the one device-to-host read (about 1 KiB, one wait): the candidate count
  // sizes the workspace, the replacers' varying bits choose the sort's passes
  SG_HIP(hipMemcpyAsync(got, a.scal, sizeof(got), hipMemcpyDeviceToHost, ctx->stream));
  SG_HIP(hipMemcpyAsync(&total, (const uint64_t*)ws_at(ctx, o_coff) + nrec, 8, hipMemcpyDeviceToHost, ctx->stream));
  SG_HIP(hipStreamSynchronize(ctx->stream));
  if (got[0] || total >= (1ull << 32) || got[1] >= (1ull << 32)) {
    set_error("sg_hints_replacers: %llu pairs, %s%llu matches (the limit of each is 2^32 - 1)", got[1],
              got[0] ? "more than " : "", total);
    return SG_EINVAL;
  }
  const uint64_t nc = total;
  ctx->hints_cands = nc;
  unsigned long long r_and = ~0ull, r_or = 0;
  for (uint32_t i = 0; i < kHjStripes; i++) {
    r_and &= got[2 + i];
    r_or |= got[2 + kHjStripes + i];
  }
  if (nc == 0) {
    SG_HIP(hipMemsetAsync(d_rep_off, 0, (nvals + 1) * 8, ctx->stream));
    return SG_OK;
  }
  const uint64_t wcap = reps_in_ws ? (cap < nc ? cap : nc) : 0;
  const size_t o_cslot = p.add(nc * 4), o_crep = p.add(nc * 8), o_ka = p.add(nc * 8), o_kb = p.add(nc * 8),
               o_flags = p.add(nc * 4), o_pos = p.add((nc + 1) * 8), o_u = p.add(nc * 8), o_scnt = p.add(nvals * 4),
               o_reps = p.add(wcap * 8);
  const size_t tail = p.total;
  const size_t scan_n = nc > nvals ? nc : nvals;
  rc = ws_reserve_redo(ctx, tail + radix_sort_ws(nc) + scan_ws_bytes(scan_n) + need_a, count);  // (the counts, again)
  if (rc) return rc;
  a.cand_off = (const uint64_t*)ws_at(ctx, o_coff);
  a.cslot = (uint32_t*)ws_at(ctx, o_cslot);
  a.crep = (uint64_t*)ws_at(ctx, o_crep);
  {
    ScopedTimer tm(ctx, "hints_join");
    join_launch<true>(ctx, a);
  }
  SG_HIP(hipGetLastError());
  uint64_t* ka = (uint64_t*)ws_at(ctx, o_ka);
  uint64_t* kb = (uint64_t*)ws_at(ctx, o_kb);
  uint32_t* flags = (uint32_t*)ws_at(ctx, o_flags);
  uint64_t* pos = (uint64_t*)ws_at(ctx, o_pos);
  uint64_t* u = (uint64_t*)ws_at(ctx, o_u);
  uint32_t* scnt = (uint32_t*)ws_at(ctx, o_scnt);
  uint64_t* reps = reps_in_ws ? (uint64_t*)ws_at(ctx, o_reps) : d_reps;
  const uint64_t rcap = reps_in_ws ? wcap : cap;
  const dim3 g(div_up(nc, 256)), b(256);
  {
    ScopedTimer tm(ctx, "hints_sort");
    // 1. the distinct replacers, ascending
    SG_HIP(hipMemcpyAsync(ka, a.crep, nc * 8, hipMemcpyDeviceToDevice, ctx->stream));
    uint64_t* sorted = nullptr;
    const uint64_t vary = r_and ^ r_or;  // the bits that differ between replacers
    rc = radix_sort_u64(ctx, ka, kb, nc, tail, &sorted, vary ? vary : 1);
    if (rc) return rc;
    if ((rc = rank_runs(ctx, sorted, nc, flags, pos, u, tail))) return rc;
    // 2. each candidate's rank; 3. sort (slot, rank)
    hipLaunchKernelGGL(k_hj_rank, g, b, 0, ctx->stream, (const uint32_t*)a.cslot, (const uint64_t*)a.crep, nc,
                       (const uint64_t*)u, (const uint64_t*)(pos + nc), ka);
    SG_HIP(hipGetLastError());
    const uint64_t kvary = (bits_below(nvals) << 32) | bits_below(nc);
    rc = radix_sort_u64(ctx, ka, kb, nc, tail, &sorted, kvary ? kvary : 1);
    if (rc) return rc;
    // 4. first occurrences -> rep_off; 5. reps = U[rank]
    if ((rc = rank_runs(ctx, sorted, nc, flags, pos, nullptr, tail))) return rc;
    SG_HIP(hipMemsetAsync(scnt, 0, nvals * 4, ctx->stream));
    hipLaunchKernelGGL(k_hj_slot_count, g, b, 0, ctx->stream, (const uint64_t*)sorted, (const uint32_t*)flags, nc, scnt);
    rc = scan_counts(ctx, scnt, d_rep_off, nvals, tail);
    if (rc) return rc;
    if (reps)
      hipLaunchKernelGGL(k_hj_write, g, b, 0, ctx->stream, (const uint64_t*)sorted, (const uint32_t*)flags,
                         (const uint64_t*)pos, nc, (const uint64_t*)u, (const uint64_t*)(d_rep_off + nvals), rcap, reps);
    SG_HIP(hipGetLastError());
  }
  if (ws_reps) *ws_reps = reps_in_ws ? reps : nullptr;
  return SG_OK;
}

}  // namespace sg

using namespace sg;

extern "C" {

int sg_ipc_comps_dev(sg_ctx* ctx, const uint32_t* d_out, const uint64_t* d_out_off, const uint64_t* d_call_off,
                     const uint32_t* d_call_nums, uint64_t nprog, uint64_t nrec, int32_t* d_status,
                     uint64_t* d_pair_off, uint64_t* d_pairs, uint64_t cap) {
  if (!ctx || !d_out_off || !d_call_off || !d_pair_off || (nprog && !d_status) || (cap && !d_pairs)) return SG_EINVAL;
  std::lock_guard<std::mutex> g(ctx->mu);
  int rc = ensure_device(ctx);
  if (rc) return rc;
  if (nrec == 0) SG_HIP(hipMemsetAsync(d_pair_off, 0, 8, ctx->stream));
  WsPlan p;
  const size_t o_src = p.add(nrec * 8), o_end = p.add(nrec * 8), o_n = p.add(nrec * 4), o_cnt = p.add(nrec * 4),
               o_seen = p.add(nrec);
  const size_t scan_off = p.total;
  rc = ws_reserve(ctx, p.total + scan_ws_bytes(nrec ? nrec : 1));
  if (rc) return rc;
  CompsArgs a{};
  a.out = d_out;
  a.out_off = d_out_off;
  a.call_off = d_call_off;
  a.call_nums = d_call_nums;
  a.nprog = nprog;
  a.status = d_status;
  a.cmp_src = (uint64_t*)ws_at(ctx, o_src);
  a.cmp_end = (uint64_t*)ws_at(ctx, o_end);
  a.cmp_n = (uint32_t*)ws_at(ctx, o_n);
  a.pair_cnt = (uint32_t*)ws_at(ctx, o_cnt);
  a.seen = (uint8_t*)ws_at(ctx, o_seen);
  if (nrec) SG_HIP(hipMemsetAsync(ws_at(ctx, 0), 0, scan_off, ctx->stream));
  if (nprog) {
    ScopedTimer tm(ctx, "comps_walk");
    hipLaunchKernelGGL(k_comps_walk, dim3(div_up(nprog, 4)), dim3(256), 0, ctx->stream, a);
  }
  SG_HIP(hipGetLastError());
  if (nrec == 0) return SG_OK;
  rc = scan_counts(ctx, a.pair_cnt, d_pair_off, nrec, scan_off);
  if (rc) return rc;
  if (d_pairs) {
    ScopedTimer tm(ctx, "comps_emit");
    hipLaunchKernelGGL(k_comps_emit, dim3(div_up(nrec, 4)), dim3(256), 0, ctx->stream, d_out,
                       (const uint64_t*)a.cmp_src, (const uint64_t*)a.cmp_end, (const uint32_t*)a.cmp_n,
                       (const uint64_t*)d_pair_off, nrec, cap, d_pairs);
  }
  SG_HIP(hipGetLastError());
  return SG_OK;
}

int sg_ipc_comps(sg_ctx* ctx, const uint32_t* out, const uint64_t* out_off, const uint64_t* call_off,
                 const uint32_t* call_nums, size_t nprog, int32_t* status, uint64_t* pair_off, uint64_t* pairs,
                 size_t cap) {
  if (!ctx || !out_off || !call_off || !pair_off || (cap && !pairs)) return SG_EINVAL;
  const uint64_t nwords = out_off[nprog], nrec = call_off[nprog];
  if (out_off[0] != 0 || call_off[0] != 0 || (nwords && !out) || (nprog && !status)) return SG_EINVAL;
  for (size_t q = 0; q < nprog; q++)
    if (out_off[q + 1] < out_off[q] || call_off[q + 1] < call_off[q] || out_off[q + 1] - out_off[q] > (1ull << 32))
      return SG_EINVAL;
  // a comparison is at least 3 words and yields at most 2 pairs
  const uint64_t bound = 2 * ((nwords + 2) / 3);
  WsPlan p;
  const size_t o_w = p.add(nwords * 4 + 4), o_oo = p.add((nprog + 1) * 8), o_co = p.add((nprog + 1) * 8),
               o_po = p.add((nrec + 1) * 8), o_num = p.add(nrec * 4 + 4), o_st = p.add(nprog * 4 + 4),
               o_pairs = p.add(bound * 16 + 16);
  uint32_t *dw, *dnum;
  uint64_t *doo, *dco, *dpo, *dpairs;
  int32_t* dst;
  {
    std::lock_guard<std::mutex> g(ctx->mu);
    int rc = ensure_device(ctx);
    if (rc) return rc;
    rc = dstage_reserve(ctx, p);
    if (rc) return rc;
    dw = dstage_at<uint32_t>(ctx, o_w);
    doo = dstage_at<uint64_t>(ctx, o_oo);
    dco = dstage_at<uint64_t>(ctx, o_co);
    dpo = dstage_at<uint64_t>(ctx, o_po);
    dnum = dstage_at<uint32_t>(ctx, o_num);
    dst = dstage_at<int32_t>(ctx, o_st);
    dpairs = dstage_at<uint64_t>(ctx, o_pairs);
  }
  int rc;
  if ((rc = upload(ctx, dw, out, nwords * 4))) return rc;
  if ((rc = upload(ctx, doo, out_off, (nprog + 1) * 8))) return rc;
  if ((rc = upload(ctx, dco, call_off, (nprog + 1) * 8))) return rc;
  if (call_nums && (rc = upload(ctx, dnum, call_nums, nrec * 4))) return rc;
  rc = sg_ipc_comps_dev(ctx, dw, doo, dco, call_nums ? dnum : nullptr, nprog, nrec, dst, dpo, dpairs, bound);
  if (rc) return rc;
  if (nprog) SG_HIP(hipMemcpyAsync(status, dst, nprog * 4, hipMemcpyDeviceToHost, ctx->stream));
  return csr_download(ctx, pair_off, dpo, nrec, pairs, dpairs, 16, cap);
}

int sg_hints_replacers_dev(sg_ctx* ctx, const uint64_t* d_pair_off, const uint64_t* d_pairs, uint64_t nrec,
                           const uint64_t* d_val_off, const uint64_t* d_vals, uint64_t nvals, uint64_t* d_rep_off,
                           uint64_t* d_reps, uint64_t cap) {
  if (!ctx || !d_pair_off || !d_val_off || !d_rep_off || (cap && !d_reps) || (nvals && !d_vals)) return SG_EINVAL;
  std::lock_guard<std::mutex> g(ctx->mu);
  int rc = ensure_device(ctx);
  if (rc) return rc;
  return hints_replacers(ctx, d_pair_off, d_pairs, nrec, d_val_off, d_vals, nvals, d_rep_off, d_reps, cap, false,
                         nullptr);
}

int sg_hints_replacers(sg_ctx* ctx, const uint64_t* pair_off, const uint64_t* pairs, size_t nrec,
                       const uint64_t* val_off, const uint64_t* vals, uint64_t* rep_off, uint64_t* reps, size_t cap) {
  if (!ctx || !pair_off || !val_off || !rep_off || (cap && !reps)) return SG_EINVAL;
  const uint64_t npairs = pair_off[nrec], nvals = val_off[nrec];
  if (!offsets_ok(pair_off, nrec) || !offsets_ok(val_off, nrec) || (npairs && !pairs) || (nvals && !vals))
    return SG_EINVAL;
  if (npairs >= (1ull << 32) || nvals >= (1ull << 32)) {
    set_error("sg_hints_replacers: %llu pairs, %llu value slots (the limit of each is 2^32 - 1)",
              (unsigned long long)npairs, (unsigned long long)nvals);
    return SG_EINVAL;
  }
  WsPlan p;
  const size_t o_po = p.add((nrec + 1) * 8), o_vo = p.add((nrec + 1) * 8), o_p = p.add(npairs * 16 + 16),
               o_v = p.add(nvals * 8 + 8), o_ro = p.add((nvals + 1) * 8);
  std::lock_guard<std::mutex> g(ctx->mu);
  int rc = ensure_device(ctx);
  if (rc) return rc;
  rc = dstage_reserve(ctx, p);
  if (rc) return rc;
  uint64_t* dpo = dstage_at<uint64_t>(ctx, o_po);
  uint64_t* dvo = dstage_at<uint64_t>(ctx, o_vo);
  uint64_t* dp = dstage_at<uint64_t>(ctx, o_p);
  uint64_t* dv = dstage_at<uint64_t>(ctx, o_v);
  uint64_t* dro = dstage_at<uint64_t>(ctx, o_ro);
  if ((rc = upload(ctx, dpo, pair_off, (nrec + 1) * 8))) return rc;
  if ((rc = upload(ctx, dvo, val_off, (nrec + 1) * 8))) return rc;
  if ((rc = upload(ctx, dp, pairs, npairs * 16))) return rc;
  if ((rc = upload(ctx, dv, vals, nvals * 8))) return rc;
  uint64_t* dreps = nullptr;  // (set whenever a replacer was written)
  rc = hints_replacers(ctx, dpo, dp, nrec, dvo, dv, nvals, dro, nullptr, cap, true, &dreps);
  if (rc) return rc;
  return csr_download(ctx, rep_off, dro, nvals, reps, dreps, 8, cap);
}

}  // extern "C"
