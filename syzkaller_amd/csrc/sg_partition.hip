// sg_partition.hip -- the two-pass partition of the partitioned triage
// (sg_part.h): pass-1 tiles, the group and chunk tables, the byte histograms,
// both scatters, the bucket tables and the list of non-empty buckets.
#include "sg_part.h"

namespace sg {

constexpr int kPWaves = kPThreads / 64;      // waves of a partition workgroup
constexpr int kPerWave = kPT / kPWaves;      // 1024 entries per wave, in order
constexpr int kSteps = kPerWave / 64;        // 16 entries per lane

// Blocks sharing an XCD (bid % 8 under round-robin dispatch) get a contiguous
// run of tiles, so partial lines at the seams of neighbouring tiles' digit
// runs merge in one L2.  A bijection on [0, g) for any g (speed only).
__device__ __forceinline__ uint32_t xcd_tile(uint32_t bid, uint32_t g) {
  const uint32_t x = bid & 7, q = g >> 3, r = g & 7;
  return (x < r ? x * (q + 1) : r * (q + 1) + (x - r) * q) + (bid >> 3);
}

// ------------------------------------------------------------- tile cuts ---
// Pass-1 tiles: sorted merge of A = {i * kPT : i < nA} and B = {rec_off[(j +
// 1) * kRecCap] : j < nB} (both non-decreasing; ties put A first).
// start[rank] = cut position (start[nA + nB] = n), aux[rank] = record holding
// the entry at the cut.  Coinciding cuts give empty tiles.
struct Cuts {
  uint64_t nA, step, nB, n;
  const uint64_t* rec_off;
  uint64_t nrec;
  uint32_t* start;
  uint32_t* aux;
  __device__ __forceinline__ uint64_t B(uint64_t j) const { return rec_off[(j + 1) * kRecCap]; }
  // #{j : B[j] < x}
  __device__ __forceinline__ uint64_t countB(uint64_t x) const {
    uint64_t lo = 0, hi = nB;
    while (lo < hi) {
      const uint64_t mid = (lo + hi) >> 1;
      if (B(mid) < x)
        lo = mid + 1;
      else
        hi = mid;
    }
    return lo;
  }
};

__global__ void k_cuts(Cuts c) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const uint64_t total = c.nA + c.nB;
  if (i > total) return;
  if (i == total) {
    c.start[total] = (uint32_t)c.n;
    return;
  }
  uint64_t x, rank;
  if (i < c.nA) {
    x = i * c.step;
    rank = i + c.countB(x);
  } else {
    const uint64_t j = i - c.nA;
    x = c.B(j);
    const uint64_t a = x / c.step + 1;
    rank = j + (a < c.nA ? a : c.nA);
  }
  c.start[rank] = (uint32_t)x;
  // record holding entry x (largest r with rec_off[r] <= x)
  const uint64_t xe = x < c.n ? x : (c.n ? c.n - 1 : 0);
  c.aux[rank] = (uint32_t)sgd::seg_search(c.rec_off, 0, c.nrec - 1, xe);
}

// Group g's first tile: the rank of the record cut at rec_off[g << 16] (cut
// j = g * kGroupRecs / kRecCap - 1 of B; see k_cuts); gt[NG] = T.
__global__ void k_group_tiles(const uint64_t* __restrict__ rec_off, uint64_t nA, uint32_t NG, uint32_t T,
                              uint32_t* __restrict__ gt) {
  const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g > NG) return;
  if (g == 0 || g == NG) {
    gt[g] = g ? T : 0u;
    return;
  }
  const uint64_t a = rec_off[(uint64_t)g * kGroupRecs] / kPT + 1;
  gt[g] = (uint32_t)((uint64_t)g * (kGroupRecs / kRecCap) - 1 + (a < nA ? a : nA));
}

// Pass-2 slice-groups: j = (slice j / NG, group j % NG) covers
// [gstart(j), gstart(j + 1)) of the pass-1 output (gt[NG] = T makes gstart(ng)
// the end); it is cut into ceil(size / kPT) chunks (none when empty).
__device__ __forceinline__ uint32_t group_start(const uint32_t* goff1, uint32_t T, uint32_t NG, const uint32_t* gt,
                                                uint64_t j) {
  return goff1[(j / NG) * T + gt[j % NG]];
}

__global__ void k_group_chunks(const uint32_t* __restrict__ goff1, uint32_t T, uint32_t NG,
                               const uint32_t* __restrict__ gt, uint64_t ng, uint32_t* __restrict__ nch) {
  const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= ng) return;
  const uint32_t sz = group_start(goff1, T, NG, gt, j + 1) - group_start(goff1, T, NG, gt, j);
  nch[j] = (sz + kPT - 1) / kPT;
}

// cbase = exclusive scan of nch (cbase[ng] = number of chunks G).  Writes the
// chunk list (start, slice-group) for c < G, start = n for G <= c <= gmax (the
// launch grids use gmax, an upper bound known on the host; n = the pass-1
// total, goff1[256 T], which is below the input count when a trace batch
// drops zero edges), and cfirst[d] = first chunk of slice d (cfirst[256] = G).
__global__ void k_chunk_list(const uint32_t* __restrict__ goff1, uint32_t T, uint32_t NG,
                             const uint32_t* __restrict__ gt, uint64_t ng,
                             const uint32_t* __restrict__ cbase, uint64_t gmax, uint32_t* __restrict__ cstart,
                             uint32_t* __restrict__ cgov, uint32_t* __restrict__ cfirst) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const uint32_t G = cbase[ng], n = goff1[256ull * T];
  if (i < ng) {
    const uint32_t g0 = group_start(goff1, T, NG, gt, i), g1 = group_start(goff1, T, NG, gt, i + 1);
    uint32_t c = cbase[i];
    for (uint32_t e = g0; e < g1; e += kPT, c++) {
      cstart[c] = e;
      cgov[c] = (uint32_t)i;
    }
  }
  if (i >= G && i <= gmax) {
    cstart[i] = n;
    cgov[i] = (uint32_t)(ng - 1);
  }
  if (i <= 256) cfirst[i] = i < 256 ? cbase[i * NG] : G;
}


// Per pass-2 block (the grid is the host bound gmax): desc = {start, end,
// slice-group, chunk} of chunk xcd_tile(bid, G) for bid < G, empty past G;
// dtile = the pass-1 tiles [first, last + 1) whose runs the chunk holds.
// Lets the pass-2 kernels start their data loads after one load.
// With `bounds` (a late pass 2, sg_part.h): blocks [0, G1) take the chunks
// [0, G1) of the first window's slices and blocks [G1, G) the others, each
// window's chunks spread over the XCDs as the whole list is without it.
__global__ void k_chunk_desc(const uint32_t* __restrict__ cstart, const uint32_t* __restrict__ cgov,
                             const uint32_t* __restrict__ gcount, uint64_t gmax, const uint32_t* __restrict__ goff1,
                             uint32_t T, uint32_t NG, const uint32_t* __restrict__ gt,
                             const uint32_t* __restrict__ bounds, uint4* __restrict__ desc,
                             uint2* __restrict__ dtile) {
  const uint64_t bid = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (bid >= gmax) return;
  const uint32_t G = *gcount;
  if (bid < G) {
    const uint32_t G1 = bounds ? min(bounds[kLateChunks], G) : 0u;
    const uint32_t c = bid < G1 ? xcd_tile((uint32_t)bid, G1) : G1 + xcd_tile((uint32_t)bid - G1, G - G1);
    const uint32_t s0 = cstart[c], s1 = cstart[c + 1], j = cgov[c];
    const uint32_t* row = goff1 + (uint64_t)(j / NG) * T;
    const uint32_t lo = gt[j % NG], hi = gt[j % NG + 1];
    desc[bid] = make_uint4(s0, s1, j, c);
    dtile[bid] = make_uint2(last_le(row, lo, hi, s0), last_le(row, lo, hi, s1 - 1) + 1);
  } else {
    desc[bid] = make_uint4(0, 0, 0, 0);
    dtile[bid] = make_uint2(0, 0);
  }
}

// --------------------------------------------------------- byte histogram ---
// hist[(v >> 24) * ncols + col] = count over one job's entries [s0, s1).
// Pass 1: job = tile t = xcd_tile(bid, T), [start[t], start[t+1]), T columns.
// Pass 2: job = the block's chunk descriptor, *ncols_dev columns; blocks
// without a chunk exit.  16-B aligned input (always, for pass 2) goes through
// k_hist_rep; k_p1_hist covers an unaligned caller buffer.
constexpr int kHistQ = kPT / 4 / kPThreads;  // uint4 loads per lane

__global__ __launch_bounds__(kPThreads) void k_p1_hist(const uint32_t* __restrict__ v,
                                                       const uint32_t* __restrict__ start, uint32_t* __restrict__ hist) {
  __shared__ uint32_t cnt[256];
  const uint32_t ncols = gridDim.x, t = xcd_tile(blockIdx.x, ncols), s0 = start[t], s1 = start[t + 1];
  const int tid = threadIdx.x;
  if (tid < 256) cnt[tid] = 0;
  uint32_t x[kPT / kPThreads];
#pragma unroll
  for (int k = 0; k < kPT / kPThreads; k++) {
    const uint32_t e = s0 + k * kPThreads + tid;
    x[k] = e < s1 ? v[e] : 0u;
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < kPT / kPThreads; k++)
    if (s0 + k * kPThreads + tid < s1) atomicAdd(&cnt[p1_digit(x[k])], 1u);
  __syncthreads();
  if (tid < 256) hist[(uint64_t)tid * ncols + t] = cnt[tid];
}

// Aligned-input histogram jobs: [s0, s1) of the input, output column col.
struct HistJob {
  uint32_t s0, s1, col;
};

struct HistRegs {
  uint4 x[kHistQ + 1];
  uint32_t y;
};

// threads 0-2 take the entries before quad q0, threads 3-5 those after quad q1
__device__ __forceinline__ uint32_t hist_edge(const HistJob& h, int tid) {
  const uint32_t q0 = (h.s0 + 3) >> 2, q1 = h.s1 >> 2;
  if (tid < 3) return h.s0 + tid < q0 * 4 && h.s0 + tid < h.s1 ? h.s0 + tid : 0xFFFFFFFFu;
  if (tid < 6) {
    const uint32_t e = q1 * 4 + (tid - 3);
    return e < h.s1 && e >= h.s0 && q1 >= q0 ? e : 0xFFFFFFFFu;
  }
  return 0xFFFFFFFFu;
}

// Unconditional buffer loads: the descriptor spans exactly the job's whole
// quads (resp. its entries), and the range check returns 0 past the end.
__device__ __forceinline__ void hist_load(const uint32_t* __restrict__ v, const HistJob& h, int tid, HistRegs& r) {
  const uint32_t s0 = uni(h.s0), s1 = uni(h.s1);
  const uint32_t q0 = (s0 + 3) >> 2, q1 = s1 >> 2;
  const uint32_t qbytes = q1 > q0 ? (q1 - q0) * 16u : 0u;
  const __amdgpu_buffer_rsrc_t rq =
      __builtin_amdgcn_make_buffer_rsrc((void*)(v + (uint64_t)q0 * 4), 0, (int)qbytes, 0x00020000);
#pragma unroll
  for (int k = 0; k <= kHistQ; k++) {
    const v4u32 t = __builtin_amdgcn_raw_buffer_load_b128(rq, (uint32_t)(k * kPThreads + tid) * 16u, 0, 0);
    r.x[k] = make_uint4(t[0], t[1], t[2], t[3]);
  }
  const __amdgpu_buffer_rsrc_t re =
      __builtin_amdgcn_make_buffer_rsrc((void*)(v + s0), 0, (int)((s1 - s0) * 4u), 0x00020000);
  const uint32_t e = hist_edge(h, tid);
  r.y = __builtin_amdgcn_raw_buffer_load_b32(re, (e - s0) * 4u, 0, 0);
}

// Bank-replicated counting: 32 copies of the 256 counters, copy = lane & 31,
// laid out so that counter (d, copy) sits in LDS bank copy: the 32 lanes of
// a half-wave always hit 32 distinct banks (a shared 256-counter table sees
// ~3.5-way conflicts per half-wave on random digits).  The copies are summed
// per digit at the end, each lane starting at a different copy.
// digit of an input value: pass 1 reads signals (p1_digit), pass 2 pass-1 entries (top byte)
template <bool kP2>
__device__ __forceinline__ uint32_t hist_digit(uint32_t x) { return kP2 ? x >> 24 : p1_digit(x); }

template <bool kP2>
__global__ __launch_bounds__(kPThreads) void k_hist_rep(const uint32_t* __restrict__ v,
                                                        const uint32_t* __restrict__ start,
                                                        const uint4* __restrict__ desc, uint32_t njobs,
                                                        const uint32_t* __restrict__ ncols_dev,
                                                        uint32_t* __restrict__ hist) {
  __shared__ uint32_t rc[256 * 32];
  const int tid = threadIdx.x;
  HistJob h;
  if (kP2) {
    const uint4 d = desc[blockIdx.x];
    h.s0 = d.x;
    h.s1 = d.y;
    h.col = d.w;
    if (h.s0 >= h.s1) return;
  } else {
    h.col = xcd_tile(blockIdx.x, njobs);
    h.s0 = start[h.col];
    h.s1 = start[h.col + 1];
  }
  const uint32_t ncols = kP2 ? *ncols_dev : njobs;
  HistRegs r;
  hist_load(v, h, tid, r);
#pragma unroll
  for (int k = 0; k < 256 * 32 / 4 / kPThreads; k++)
    reinterpret_cast<uint4*>(rc)[k * kPThreads + tid] = make_uint4(0, 0, 0, 0);
  __syncthreads();
  const uint32_t q0 = (h.s0 + 3) >> 2, q1 = h.s1 >> 2, cp = tid & 31;
#pragma unroll
  for (int k = 0; k <= kHistQ; k++)
    if (q0 + k * kPThreads + tid < q1) {
      atomicAdd(&rc[hist_digit<kP2>(r.x[k].x) * 32 + cp], 1u);
      atomicAdd(&rc[hist_digit<kP2>(r.x[k].y) * 32 + cp], 1u);
      atomicAdd(&rc[hist_digit<kP2>(r.x[k].z) * 32 + cp], 1u);
      atomicAdd(&rc[hist_digit<kP2>(r.x[k].w) * 32 + cp], 1u);
    }
  if (hist_edge(h, tid) != 0xFFFFFFFFu) atomicAdd(&rc[hist_digit<kP2>(r.y) * 32 + cp], 1u);
  __syncthreads();
  if (tid < 256) {
    uint32_t sum = 0;
#pragma unroll
    for (int k = 0; k < 32; k++) sum += rc[tid * 32 + ((k + tid) & 31)];
    hist[(uint64_t)tid * ncols + h.col] = sum;
  }
}

// Pass-2 histogram from the byte plane: hist[b * ncols + col] = count of
// byte b over the chunk's positions [s0, s1).  The chunk's <= kPT bytes are
// read as 16-B quads from s0 rounded down (<= kPT / 16 + 1 quads; the plane
// is padded), bytes outside [s0, s1) masked.  512 threads, 16 counter copies
// (the per-block zeroing and final sums are most of the work at 1 B per entry).
constexpr int kHBThreads = 512, kHBCopies = 16;
__global__ __launch_bounds__(kHBThreads) void k_hist_bytes(const uint8_t* __restrict__ v,
                                                            const uint4* __restrict__ desc,
                                                            const uint32_t* __restrict__ ncols_dev,
                                                            uint32_t* __restrict__ hist) {
  __shared__ uint32_t rc[256 * kHBCopies];
  const int tid = threadIdx.x;
  const uint4 d = desc[blockIdx.x];
  const uint32_t s0 = d.x, s1 = d.y, col = d.w;
  if (s0 >= s1) return;
  const uint32_t ncols = *ncols_dev;
  const uint32_t b0 = s0 & ~15u;
  constexpr int kQ = kPT / 16 / kHBThreads + 1;  // quads per thread (the last one only for the rounding)
  uint4 x[kQ];
#pragma unroll
  for (int k = 0; k < kQ; k++) {
    const uint32_t q = b0 + (uint32_t)(k * kHBThreads + tid) * 16u;
    x[k] = q < s1 ? *reinterpret_cast<const uint4*>(v + q) : make_uint4(0, 0, 0, 0);
  }
#pragma unroll
  for (int k = 0; k < 256 * kHBCopies / 4 / kHBThreads; k++)
    reinterpret_cast<uint4*>(rc)[k * kHBThreads + tid] = make_uint4(0, 0, 0, 0);
  __syncthreads();
  const uint32_t cp = tid & (kHBCopies - 1);
#pragma unroll
  for (int k = 0; k < kQ; k++) {
    const uint32_t q = b0 + (uint32_t)(k * kHBThreads + tid) * 16u;
    if (q < s1) {
      const uint32_t w[4] = {x[k].x, x[k].y, x[k].z, x[k].w};
#pragma unroll
      for (int j = 0; j < 16; j++) {
        const uint32_t pos = q + j;
        if (pos >= s0 && pos < s1) atomicAdd(&rc[((w[j >> 2] >> (8 * (j & 3))) & 0xFFu) * kHBCopies + cp], 1u);
      }
    }
  }
  __syncthreads();
  if (tid < 256) {
    uint32_t sum = 0;
#pragma unroll
    for (int k = 0; k < kHBCopies; k++) sum += rc[tid * kHBCopies + ((k + tid) & (kHBCopies - 1))];
    hist[(uint64_t)tid * ncols + col] = sum;
  }
}

// ------------------------------------------------ trace batches (set-exact) ---
// A batch given as raw per-call PC traces (the executor's KCOV buffers) is
// triaged with its edge signal computed in the pass-1 loads: entry e of a
// call is sig = pc[e] ^ hash(pc[e - 1]), pc[e] ^ 0 for the call's first PC
// (executor/executor.h:392-396), and a zero sig is not an entry (the
// executor's dedup reports 0 as seen, executor.h:507-515).  The executor
// also drops an edge its dedup table still holds; skipping that is exact for
// the triage: every non-zero edge is written at its first occurrence in the
// program (dedup returns false when no slot holds it, executor.h:516-525),
// i.e. in its first call, so the first record holding s and the union of the
// batch's signal -- all that decides the queued records and the set updates
// (fuzzer.go:665-691) -- are the same with or without the repeats.  The
// partition and the buckets are the sort and unique stage.
//
// Repeats inside a pass-1 tile (a hot edge recurs hundreds of times in one
// program's trace; the executor's table drops most of those) are dropped
// before the partition: each edge takes a 64-bit atomicMin of
// (tile position << 32 | sig) on an LDS slot hashed from sig, and an edge
// whose slot ends up holding the same sig at an earlier position is a
// repeat.  Exact: the earlier copy's record is not larger, so the first
// record holding sig and the union are unchanged; a slot taken by another
// edge only leaves a repeat in.  The histogram and the scatter drop the
// same entries (same positions, same hash).
constexpr uint32_t kTraceDedup = 1024;  // slots (8 KiB of LDS)
__device__ __forceinline__ uint32_t dedup_slot(uint32_t sig) { return (sig * 0x9E3779B1u) >> 22; }

// the previous PC of position e for lane-strided loads (x = this lane's PC,
// xp = pcs[e - 1] loaded by lane 0 of the wave)
__device__ __forceinline__ uint32_t trace_prev(uint32_t x, uint32_t xp) {
  return (uint32_t)__builtin_amdgcn_update_dpp((int)xp, (int)x, 0x138 /* wave_shr:1 */, 0xF, 0xF, false);
}

__device__ __forceinline__ uint32_t trace_sig(uint32_t pc, uint32_t prev, bool start) {
  return pc ^ (start ? 0u : sgd::exec_hash(prev));
}

// Pass-1 histogram of a trace batch: b2 counts of the tile's non-zero edges.
// It also records which entries are kept (non-zero, not an in-tile repeat):
// one ballot word per 64 tile positions (keep[t][p / 64], bit p % 64), which
// the scatter reads instead of repeating the dedup.
__global__ __launch_bounds__(kPThreads) void k_hist_trace(const uint32_t* __restrict__ pcs,
                                                          const uint64_t* __restrict__ rec_off, uint64_t nrec,
                                                          const uint32_t* __restrict__ tstart,
                                                          const uint32_t* __restrict__ trec, uint32_t T,
                                                          uint32_t* __restrict__ hist, uint64_t* __restrict__ keep) {
  __shared__ uint32_t rc[256 * 32];
  __shared__ alignas(16) uint32_t cs[kPT / 32];
  __shared__ unsigned long long dd[kTraceDedup];
  const int tid = threadIdx.x, lane = tid & 63;
  const uint32_t t = xcd_tile(blockIdx.x, T), s0 = tstart[t], s1 = tstart[t + 1];
  constexpr int kS = kPT / kPThreads;
  uint32_t x[kS], xp[kS];
#pragma unroll
  for (int k = 0; k < kS; k++) {
    const uint32_t e = s0 + k * kPThreads + tid;
    x[k] = e < s1 ? pcs[e] : 0u;
    xp[k] = lane == 0 && e < s1 && e > 0 ? pcs[e - 1] : 0u;
  }
  // the tile's record offsets, loaded with the PCs (one per thread), so their
  // round trip overlaps the PCs' instead of following the first barrier
  static_assert(kRecCap + 1 <= kPThreads, "one record offset per thread");
  const uint32_t r0 = trec[t];
  const uint32_t wn = (uint32_t)(nrec + 1 - r0 < kRecCap + 1 ? nrec + 1 - r0 : kRecCap + 1);
  const uint64_t ro = (uint32_t)tid < wn ? rec_off[r0 + tid] : ~0ull;
#pragma unroll
  for (int k = 0; k < 256 * 32 / 4 / kPThreads; k++)
    reinterpret_cast<uint4*>(rc)[k * kPThreads + tid] = make_uint4(0, 0, 0, 0);
  for (int i = tid; i < kPT / 32; i += kPThreads) cs[i] = 0;
  for (int i = tid; i < (int)kTraceDedup; i += kPThreads) dd[i] = ~0ull;
  __syncthreads();
  if (ro >= s0 && ro < s1) atomicOr(&cs[(ro - s0) >> 5], 1u << ((ro - s0) & 31));  // call starts in the tile
  __syncthreads();
  uint32_t live = 0;
#pragma unroll
  for (int k = 0; k < kS; k++) {
    const uint32_t p = k * kPThreads + tid, e = s0 + p;
    x[k] = trace_sig(x[k], trace_prev(x[k], xp[k]), (cs[p >> 5] >> (p & 31)) & 1u);
    if (e < s1 && x[k] != 0) {
      live |= 1u << k;
      atomicMin(&dd[dedup_slot(x[k])], ((unsigned long long)p << 32) | x[k]);
    }
  }
  __syncthreads();
  const uint32_t cp = tid & 31;
  uint32_t kmask = 0;  // kept steps of this thread (no cross-lane step in this loop)
#pragma unroll
  for (int k = 0; k < kS; k++) {
    const uint32_t p = k * kPThreads + tid;
    if ((live >> k) & 1u) {
      const unsigned long long v = dd[dedup_slot(x[k])];
      if ((uint32_t)v != x[k] || (uint32_t)(v >> 32) == p) {
        kmask |= 1u << k;
        atomicAdd(&rc[p1_digit(x[k]) * 32 + cp], 1u);
      }
    }
  }
  // the kept words through LDS (cs: the call starts are no longer needed),
  // then one coalesced 2 KiB store per tile
  unsigned long long* kw = reinterpret_cast<unsigned long long*>(cs);
#pragma unroll
  for (int k = 0; k < kS; k++) {
    const uint64_t b = __ballot((kmask >> k) & 1u);  // positions k kPThreads + 64 (tid / 64) ..
    if (lane == 0) kw[(k * kPThreads + tid) >> 6] = b;
  }
  __syncthreads();
  if (tid < 256) {
    uint32_t sum = 0;
#pragma unroll
    for (int k = 0; k < 32; k++) sum += rc[tid * 32 + ((k + tid) & 31)];
    hist[(uint64_t)tid * T + t] = sum;
    keep[(uint64_t)t * (kPT / 64) + tid] = kw[tid];
  }
}

// Counting sort of one tile held in registers (kSteps entries per lane) by an
// 8-bit digit, through LDS: counts, a one-wave exclusive scan, then every
// entry takes a slot with an LDS atomic (order within a digit is arbitrary).
// On return dstart[d] is the digit's first slot and pos[k] entry k's slot.
// cnt[] arrives holding the tile's digit counts (read from the histogram
// pass, not recounted); gbase[d] is lowered by the digit's first slot, so slot
// p of digit d goes to gbase[d] + p.
template <typename DigitF>
__device__ __forceinline__ void tile_rank(const uint32_t (&dv)[kSteps], DigitF digit, uint32_t vmask, uint32_t* cnt,
                                          uint32_t* gbase, uint32_t (&pos)[kSteps]) {
  const int tid = threadIdx.x, lane = tid & 63;
  if (tid < 64) {
    uint32_t carry = 0;
#pragma unroll
    for (int base = 0; base < 256; base += 64) {
      const uint32_t x = cnt[base + lane];
      const uint32_t incl = sgd::wave_incl_add(x);
      const uint32_t ex = carry + incl - x;
      gbase[base + lane] -= ex;
      cnt[base + lane] = ex;
      carry += __builtin_amdgcn_readlane(incl, 63);
    }
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < kSteps; k++)
    if ((vmask >> k) & 1u) pos[k] = atomicAdd(&cnt[digit(dv[k])], 1u);
}

// Write-out of a ranked tile: after tile_rank and the staging barrier, cnt[d]
// is the end of digit d's slots.  Each half-wave copies whole digit runs
// (16 half-waves, 16 digits each): 32 consecutive slots per store, and no
// per-slot digit array in LDS.
// With `top` (pass 1), the top byte of every entry also goes to the byte
// plane top[] at the same position: the pass-2 digit, which the pass-2
// histogram then reads at 1 B per entry instead of 4.
template <bool kTop>
__device__ __forceinline__ void tile_write(const uint32_t* stage, const uint32_t* cnt, const uint32_t* gbase,
                                           uint32_t* __restrict__ out, uint8_t* __restrict__ top, int tid) {
  const int hw = tid >> 5, hl = tid & 31;
  const bool wtop = kTop && top;  // (none when the M0 filter may end the partition after pass 1)
  for (int d = hw; d < 256; d += kPThreads / 32) {
    const uint32_t e = cnt[d], gb = gbase[d];
    for (uint32_t p = (d ? cnt[d - 1] : 0u) + hl; p < e; p += 32) {
      const uint32_t v = stage[p];
      out[gb + p] = v;
      if (wtop) top[gb + p] = (uint8_t)(v >> 24);
    }
  }
}

// O(1) "value of the segment holding p" inside one tile of <= kPT positions,
// for sorted segment starts st(0..m) given tile-relative and clamped to
// [0, kPT] (st(0) == 0) and segment values val(k) non-decreasing in k
// (< 2^16).  Non-empty segments that start inside the tile are marked: bit
// p of sbits <=> one starts at p > 0, sidx[p] = its value; wmax[w] = value of
// the segment holding position 32w + 31; kinit = that of position 0.
// Replaces a per-entry search (segments can be a few entries long: small
// records, thin slices).
template <typename IdxT>
struct SegLds {
  uint32_t sbits[kPT / 32];
  IdxT wmax[kPT / 32];
  uint32_t kinit;
};

template <typename IdxT>
__device__ __forceinline__ void seg_clear(SegLds<IdxT>& L, int tid) {
  for (int w = tid; w < kPT / 32; w += kPThreads) L.sbits[w] = 0;
  if (tid == 0) L.kinit = 0;
}

// one segment: start p, the next segment's start nx (0xFFFFFFFF: none), value v
template <typename IdxT>
__device__ __forceinline__ void seg_mark(SegLds<IdxT>& L, IdxT* sidx, uint32_t p, uint32_t nx, uint32_t v,
                                         uint32_t n) {
  if (p == 0) {
    if (nx > 0) atomicMax(&L.kinit, v);
  } else if (p < n && nx > p) {
    atomicOr(&L.sbits[p >> 5], 1u << (p & 31));
    sidx[p] = (IdxT)v;
  }
}

template <typename IdxT>
__device__ __forceinline__ void seg_finish(SegLds<IdxT>& L, IdxT* sidx, int tid);

// call after seg_clear + a barrier; ends with a barrier
template <typename IdxT, typename StF, typename ValF>
__device__ __forceinline__ void seg_build(SegLds<IdxT>& L, IdxT* sidx, StF st, ValF val, uint32_t m, uint32_t n,
                                          int tid) {
  for (uint32_t k = tid; k < m; k += kPThreads)
    seg_mark(L, sidx, st(k), k + 1 < m ? st(k + 1) : 0xFFFFFFFFu, val(k), n);
  seg_finish(L, sidx, tid);
}

// the segments' marks -> the per-word maxima (after seg_mark; ends with a barrier)
template <typename IdxT>
__device__ __forceinline__ void seg_finish(SegLds<IdxT>& L, IdxT* sidx, int tid) {
  __syncthreads();
  constexpr int kWL = kPT / 32 / 64;  // bitmap words per lane
  if (tid < 64) {  // prefix max over the kPT / 32 words
    int run = -1;
    int loc[kWL];
#pragma unroll
    for (int j = 0; j < kWL; j++) {
      const int w = tid * kWL + j;
      const uint32_t b = L.sbits[w];
      if (b) run = max(run, (int)sidx[w * 32 + 31 - __clz(b)]);
      loc[j] = run;
    }
    const int incl = sgd::wave_incl_max(run);
    int ex = __builtin_amdgcn_update_dpp(-1, incl, 0x138, 0xF, 0xF, false);  // wave_shr:1 (lane 0: -1)
    ex = max(ex, (int)L.kinit);
#pragma unroll
    for (int j = 0; j < kWL; j++) L.wmax[tid * kWL + j] = (IdxT)max(ex, loc[j]);
  }
  __syncthreads();
}

template <typename IdxT>
__device__ __forceinline__ uint32_t seg_lookup(const SegLds<IdxT>& L, const IdxT* sidx, uint32_t p) {
  const uint32_t w = p >> 5;
  const uint32_t m = L.sbits[w] & (0xFFFFFFFFu >> (31 - (p & 31)));
  return m ? sidx[(w << 5) + 31 - __clz(m)] : (w ? L.wmax[w - 1] : L.kinit);
}

// ---------------------------------------------------------------- pass 1 ---
struct P1Args {
  const uint32_t* vals;
  const uint64_t* rec_off;
  uint64_t nrec;
  const uint32_t* tstart;  // T + 1
  const uint32_t* trec;    // T
  uint32_t T;
  const uint32_t* goff1;   // scanned [slice][tile]
  const uint32_t* hist1;   // [slice][tile] counts
  uint32_t* out;           // s << 8 | rec_in_tile
  uint8_t* top;            // out's top bytes (the pass-2 digits)
  unsigned long long* dbg; // diagnostics (k_p1_scatter<true>): cycles per phase, summed over blocks
  const uint64_t* keep;    // trace batches: k_hist_trace's kept-entry words
};

// One tile.  Only the values and their records (four 8-bit records per
// register) stay live across the rank; digits and keys are recomputed from the
// values (1.85 -> 1.67 ms per C2 launch against keeping digits and keys in
// registers; an unpredicated path for full tiles, as pass 2 has, was slower
// here: 1.93 ms).
// kTrace: a.vals are raw per-call PC traces, each entry's signal computed here
// (see k_hist_trace) and zero edges skipped.
template <bool kDbg, bool kTrace>
__device__ __forceinline__ void p1_tile(const P1Args& a, uint32_t* stage, uint32_t* cnt, uint32_t* gbase,
                                        uint16_t* win, SegLds<uint8_t>& L, uint32_t t,
                                        uint32_t s0, uint32_t s1) {
  uint8_t* sidx = reinterpret_cast<uint8_t*>(stage);  // record-in-tile index; stage is free until the rank
  const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63;
  uint64_t tk = kDbg ? clock64() : 0;
  auto stamp = [&](int ph) {
    if (kDbg) {
      asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
      const uint64_t now = clock64();
      if (tid == 0) atomicAdd(&a.dbg[ph], (unsigned long long)(now - tk));
      tk = now;
    }
  };
  const uint32_t r0 = a.trec[t];
  const uint32_t wn = (uint32_t)(a.nrec + 1 - r0 < kRecCap + 1 ? a.nrec + 1 - r0 : kRecCap + 1);
  const uint32_t ebase = s0 + w * kPerWave;
  uint32_t sv[kSteps];
  uint32_t vmask = 0;
#pragma unroll
  for (int k = 0; k < kSteps; k++) {
    const uint32_t e = ebase + k * 64 + lane;
    const bool ok = e < s1;
    sv[k] = ok ? a.vals[e] : 0u;
    vmask |= (ok ? 1u : 0u) << k;
  }
  // trace batches: the PC before the wave's first position (lane 0; the rest
  // come from the wave itself)
  const uint32_t xp0 = kTrace && lane == 0 && ebase < s1 && ebase > 0 ? a.vals[ebase - 1] : 0u;
  const bool start0 = kTrace && a.rec_off[r0] == s0;  // does a call start at the tile's first position
  // trace batches: the kept-entry words of the wave's steps, loaded with the
  // tile (loaded where they are used, after the segment build, their round
  // trip was exposed: 2.38 -> 2.21 ms per C2 trace launch)
  uint64_t kwv[kTrace ? kSteps : 1];
  if (kTrace) {
    const uint64_t* kw = a.keep + (uint64_t)t * (kPT / 64) + __builtin_amdgcn_readfirstlane(w) * (kPerWave / 64);
#pragma unroll
    for (int k = 0; k < kSteps; k++) kwv[k] = kw[k];
  }
  for (uint32_t i = tid; i < wn; i += kPThreads) {
    const uint64_t o = a.rec_off[r0 + i];
    win[i] = (uint16_t)(o <= s0 ? 0 : (o - s0 >= (uint64_t)kPT ? kPT : o - s0));
  }
  for (int d = tid; d < 256; d += kPThreads) {
    gbase[d] = a.goff1[(uint64_t)d * a.T + t];
    cnt[d] = a.hist1[(uint64_t)d * a.T + t];
  }
  seg_clear(L, tid);
  __syncthreads();
  stamp(0);
  const uint32_t nt = s1 - s0;
  seg_build(
      L, sidx, [&](uint32_t k) { return (uint32_t)win[k]; }, [](uint32_t k) { return k; }, wn, nt, tid);
  uint32_t rp[kSteps / 4] = {};
  const uint32_t el0 = ebase + lane - s0;
  if (kTrace) {
    // entries -> edge signals: the previous PC is the lane before's (lane 0:
    // the previous step's lane 63, or xp0); a call start is a segment start
    // (seg_build marks every non-empty record starting inside the tile)
    uint32_t carry = xp0;
#pragma unroll
    for (int k = 0; k < kSteps; k++) {
      const uint32_t p = el0 + k * 64, pc = sv[k];
      const bool start = p ? ((L.sbits[p >> 5] >> (p & 31)) & 1u) != 0 : start0;
      const uint32_t prev = trace_prev(pc, carry);
      carry = (uint32_t)__builtin_amdgcn_readlane((int)pc, 63);
      sv[k] = trace_sig(pc, prev, start);
      asm volatile("" : "+v"(sv[k]));  // one step at a time (registers)
    }
    // kept entries (non-zero, not an in-tile repeat): the histogram's words,
    // one per 64 positions -- wave w's step k is positions w kPerWave + 64 k ..
#pragma unroll
    for (int k = 0; k < kSteps; k++)
      if (!((kwv[k] >> lane) & 1ull)) vmask &= ~(1u << k);
  }
#pragma unroll
  for (int k = 0; k < kSteps; k++) {
    const uint32_t r = ((vmask >> k) & 1u) ? seg_lookup(L, sidx, el0 + k * 64) : 0u;  // record in tile
    rp[k >> 2] |= r << (8 * (k & 3));
  }
  stamp(1);
  uint32_t pos[kSteps];
  tile_rank(sv, [](uint32_t v) { return p1_digit(v); }, vmask, cnt, gbase, pos);
  stamp(2);
#pragma unroll
  for (int k = 0; k < kSteps; k++)
    if ((vmask >> k) & 1u) stage[pos[k]] = (part_key(sv[k]) << 8) | ((rp[k >> 2] >> (8 * (k & 3))) & 0xFFu);
  __syncthreads();
  stamp(3);
  tile_write<true>(stage, cnt, gbase, a.out, a.top, tid);
  stamp(4);
  if (kDbg && tid == 0) atomicAdd(&a.dbg[5], 1ull);
}

template <bool kDbg, bool kTrace>
__global__ __launch_bounds__(kPThreads) __attribute__((amdgpu_waves_per_eu(8, 8))) void k_p1_scatter(P1Args a) {
  __shared__ uint32_t stage[kPT];
  __shared__ uint32_t cnt[256];
  __shared__ uint32_t gbase[256];
  __shared__ uint16_t win[kRecCap + 1];  // tile-relative record starts, clamped to [0, kPT]
  __shared__ SegLds<uint8_t> L;
  const uint32_t t = xcd_tile(blockIdx.x, gridDim.x);
  const uint32_t s0 = a.tstart[t], s1 = a.tstart[t + 1];
  if (s0 >= s1) return;
  p1_tile<kDbg, kTrace>(a, stage, cnt, gbase, win, L, t, s0, s1);
}

// ---------------------------------------------------------------- pass 2 ---
struct P2Args {
  const uint32_t* in;      // pass-1 output
  const uint4* desc;       // per-block chunk descriptors
  const uint2* dtile;      // per-block chunk tile ranges
  const uint32_t* g2;      // device: number of chunks G2 (the grid is an upper bound)
  const uint32_t* goff1;   // pass-1 run starts [slice][tile]
  const uint32_t* trec;    // first record of each pass-1 tile
  uint32_t T, NG;
  const uint32_t* goff2;   // scanned [byte][chunk]
  const uint32_t* hist2;   // [byte][chunk] counts
  uint32_t* out;           // (s & 0xFFFF) << 16 | record_in_group
  // a late pass 2 (P2Late, sg_part.h): win 1 = blocks [0, G1), win 2 = blocks [G1, ..) and only in its case of the
  // summary (4-byte entries: some record not flagged; k_p2_scatter16: all flagged); win 0 = every block
  uint32_t win;
  const uint32_t* bounds;
  const uint32_t* fs_cnt;
  uint32_t fs_nblk;
  uint32_t* fs_u16;
  const uint32_t* cstart;  // chunk starts (k_p2_scatter16 takes chunks by their number)
};

// One chunk; kFull: the chunk holds kPT entries (most do), so no entry is
// predicated (no exec-mask branch per entry and step: the scatters are bound
// by the instructions they issue).  As in pass 1, only the values and the
// records (two 16-bit records per register) stay live across the rank.
template <bool kFull>
__device__ __forceinline__ void p2_chunk(const P2Args& a, uint32_t* stage, uint32_t* cnt, uint32_t* gbase,
                                         SegLds<uint16_t>& L, uint32_t s0, uint32_t s1, uint32_t gov, uint32_t c,
                                         uint2 dt) {
  uint16_t* sidx = reinterpret_cast<uint16_t*>(stage);  // tile's first record in the group; stage is free until the rank
  const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63;
  const uint32_t G2 = *a.g2;
  const uint32_t d = gov / a.NG, rg0 = (gov % a.NG) << kGroupBits, tf = dt.x, m = dt.y - dt.x;
  const uint32_t ebase = s0 + w * kPerWave;
  uint32_t sv[kSteps];
  uint32_t vmask = kFull ? (1u << kSteps) - 1 : 0u;
#pragma unroll
  for (int k = 0; k < kSteps; k++) {
    const uint32_t e = ebase + k * 64 + lane;
    if (kFull) {
      sv[k] = a.in[e];
    } else {
      const bool ok = e < s1;
      sv[k] = ok ? a.in[e] : 0u;
      vmask |= (ok ? 1u : 0u) << k;
    }
  }
  for (int f = tid; f < 256; f += kPThreads) {
    gbase[f] = a.goff2[(uint64_t)f * G2 + c];
    cnt[f] = a.hist2[(uint64_t)f * G2 + c];
  }
  // segments = the chunk's tiles (runs of this slice); value = the tile's
  // first record relative to the group.  A chunk of at most kPThreads tiles
  // (nearly all) has thread k's tile loaded with the chunk's entries, so the
  // loads' round trip is not exposed after the barrier.
  const uint32_t* row = a.goff1 + (uint64_t)d * a.T + tf;
  auto clampst = [&](uint32_t o) { return o <= s0 ? 0u : (o - s0 >= (uint32_t)kPT ? (uint32_t)kPT : o - s0); };
  const bool one = m <= (uint32_t)kPThreads;  // (block-uniform)
  const uint32_t ku = (uint32_t)tid;
  uint32_t pst = 0, pnx = 0, pvl = 0;
  if (one && ku < m) {
    pst = row[ku];
    pnx = ku + 1 < m ? row[ku + 1] : 0u;
    pvl = a.trec[tf + ku];
  }
  seg_clear(L, tid);
  __syncthreads();
  const uint32_t nt = s1 - s0;
  if (one) {
    if (ku < m) seg_mark(L, sidx, clampst(pst), ku + 1 < m ? clampst(pnx) : 0xFFFFFFFFu, pvl - rg0, nt);
    seg_finish(L, sidx, tid);
  } else {
    seg_build(
        L, sidx, [&](uint32_t k) { return clampst(row[k]); }, [&](uint32_t k) { return a.trec[tf + k] - rg0; }, m,
        nt, tid);
  }
  const uint32_t el0 = ebase + lane - s0;
  uint32_t rp[kSteps / 2] = {};  // records in group, two 16-bit per register
#pragma unroll
  for (int k = 0; k < kSteps; k++) {
    const uint32_t r1 = ((vmask >> k) & 1u) ? seg_lookup(L, sidx, el0 + k * 64) : 0u;  // tile's record in group
    rp[k >> 1] |= (r1 + (sv[k] & (kRecCap - 1))) << (16 * (k & 1));
  }
  uint32_t pos[kSteps];
  tile_rank(sv, [](uint32_t v) { return v >> 24; }, vmask, cnt, gbase, pos);
#pragma unroll
  for (int k = 0; k < kSteps; k++)
    if ((vmask >> k) & 1u) stage[pos[k]] = (((sv[k] >> 8) & 0xFFFFu) << 16) | ((rp[k >> 1] >> (16 * (k & 1))) & 0xFFFFu);
  __syncthreads();
  tile_write<false>(stage, cnt, gbase, a.out, nullptr, tid);
}

__global__ __launch_bounds__(kPThreads) __attribute__((amdgpu_waves_per_eu(8, 8))) void k_p2_scatter(P2Args a) {
  __shared__ uint32_t stage[kPT];
  __shared__ uint32_t cnt[256];
  __shared__ uint32_t gbase[256];
  __shared__ SegLds<uint16_t> L;
  if (a.win) {
    if (a.win == 2 && *a.fs_cnt == a.fs_nblk) return;  // all-flagged: k_p2_scatter16 has this window
    if ((blockIdx.x < a.bounds[kLateChunks]) != (a.win == 1)) return;
  }
  const uint4 dsc = a.desc[blockIdx.x];
  const uint2 dt = a.dtile[blockIdx.x];
  const uint32_t s0 = dsc.x, s1 = dsc.y;
  if (s0 >= s1) return;
  if (s1 - s0 == (uint32_t)kPT)
    p2_chunk<true>(a, stage, cnt, gbase, L, s0, s1, dsc.z, dsc.w, dt);
  else
    p2_chunk<false>(a, stage, cnt, gbase, L, s0, s1, dsc.z, dsc.w, dt);
}

// The second window of a late pass 2 when every record is flagged (P2Late,
// sg_part.h): what is left of the launch is the set update, which uses no
// record, so an entry is its 16-bit signal (b3 b0) alone, a u16 at byte
// 2 * position of the same output buffer.  Same chunks, byte histogram, scan
// and digit runs as k_p2_scatter; no segments, no tile records.  The staging
// is 2 bytes per entry (32 KiB), and the write-out packs two entries per lane:
// a half-wave store covers 64 consecutive entries, 128 B, where a u16 per
// lane would issue the 4-byte form's stores for half their bytes (the
// scatters are bound by the instructions they issue).  A run's first and last
// entry, when it starts or ends at an odd position, go out as single u16
// stores: the other half of that word is a neighbouring run's.
// A block takes two consecutive chunks: the runs are laid out [byte][chunk],
// so chunk c + 1's run of a digit follows chunk c's, and the two go out as one
// run (two 64-entry runs of 2 bytes: 256 B, the 4-byte form's run length; a
// lone 128-B run pays as many partial lines as a 256-B one).  stage, cnt and
// gbase hold the first chunk's, then the second's (counts zero without one).
__device__ __forceinline__ void tile_write16(const uint16_t* stage, const uint32_t* cnt, const uint32_t* gbase,
                                             uint16_t* __restrict__ out, int tid) {
  const int hw = tid >> 5, hl = tid & 31;
  for (int d = hw; d < 256; d += kPThreads / 32) {
    // the output positions [g0, gm) of the first chunk's run and [gm, g1) of the second's, from its slot bs on
    const uint32_t gb = gbase[d], g0 = gb + (d ? cnt[d - 1] : 0u), gm = gb + cnt[d];
    const uint32_t bs = d ? cnt[256 + d - 1] : 0u, g1 = gm + (cnt[256 + d] - bs);
    const uint32_t ob = (uint32_t)kPT + bs - gm;  // second chunk: position p is stage[p + ob]
    for (uint32_t q = (g0 >> 1) + hl; 2 * q < g1; q += 32) {  // the pair of positions 2 q, 2 q + 1
      const uint32_t p0 = 2 * q, p1 = p0 + 1;
      const bool v0 = p0 >= g0, v1 = p1 < g1;  // (p0 < g1 holds; neither for an empty run at an odd position)
      const uint32_t x0 = v0 ? stage[p0 < gm ? p0 - gb : p0 + ob] : 0u;
      const uint32_t x1 = v1 ? stage[p1 < gm ? p1 - gb : p1 + ob] : 0u;
      if (v0 && v1)
        *reinterpret_cast<uint32_t*>(out + p0) = x0 | (x1 << 16);
      else if (v0)
        out[p0] = (uint16_t)x0;
      else if (v1)
        out[p1] = (uint16_t)x1;
    }
  }
}

// one chunk ranked and staged (ends without a barrier)
template <bool kFull>
__device__ __forceinline__ void p2_chunk16(const P2Args& a, uint16_t* stage, uint32_t* cnt, uint32_t* gbase,
                                           uint32_t s0, uint32_t s1, uint32_t c) {
  const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63;
  const uint32_t G2 = *a.g2;
  const uint32_t ebase = s0 + w * kPerWave;
  uint32_t sv[kSteps];
  uint32_t vmask = kFull ? (1u << kSteps) - 1 : 0u;
#pragma unroll
  for (int k = 0; k < kSteps; k++) {
    const uint32_t e = ebase + k * 64 + lane;
    if (kFull) {
      sv[k] = a.in[e];
    } else {
      const bool ok = e < s1;
      sv[k] = ok ? a.in[e] : 0u;
      vmask |= (ok ? 1u : 0u) << k;
    }
  }
  for (int f = tid; f < 256; f += kPThreads) {
    gbase[f] = a.goff2[(uint64_t)f * G2 + c];
    cnt[f] = a.hist2[(uint64_t)f * G2 + c];
  }
  __syncthreads();
  uint32_t pos[kSteps];
  tile_rank(sv, [](uint32_t v) { return v >> 24; }, vmask, cnt, gbase, pos);
#pragma unroll
  for (int k = 0; k < kSteps; k++)
    if ((vmask >> k) & 1u) stage[pos[k]] = (uint16_t)(sv[k] >> 8);
}

// (the grid is half the host's chunk bound, rounded up)
__global__ __launch_bounds__(kPThreads) __attribute__((amdgpu_waves_per_eu(8, 8))) void k_p2_scatter16(P2Args a) {
  __shared__ uint16_t stage[2 * kPT];
  __shared__ uint32_t cnt[2 * 256];
  __shared__ uint32_t gbase[2 * 256];
  if (*a.fs_cnt != a.fs_nblk) return;  // some record is not flagged yet: k_p2_scatter has this window
  if (blockIdx.x == 0 && threadIdx.x == 0) atomicAdd(a.fs_u16, 1u);  // "flag_skip_u16"
  const uint32_t G = *a.g2, G1 = min(a.bounds[kLateChunks], G), np = (G - G1 + 1) >> 1;  // chunk pairs of the window
  if (blockIdx.x >= np) return;
  const uint32_t c0 = G1 + 2 * xcd_tile(blockIdx.x, np);
#pragma unroll
  for (int h = 0; h < 2; h++) {
    const uint32_t c = c0 + h;
    if (c < G) {  // (block-uniform)
      const uint32_t s0 = a.cstart[c], s1 = a.cstart[c + 1];
      if (s1 - s0 == (uint32_t)kPT)
        p2_chunk16<true>(a, stage + h * kPT, cnt + h * 256, gbase + h * 256, s0, s1, c);
      else
        p2_chunk16<false>(a, stage + h * kPT, cnt + h * 256, gbase + h * 256, s0, s1, c);
    } else if (threadIdx.x < 256) {
      cnt[256 + threadIdx.x] = 0;
    }
  }
  __syncthreads();
  tile_write16(stage, cnt, gbase, reinterpret_cast<uint16_t*>(a.out), threadIdx.x);
}

// --------------------------------------------------------- bucket tables ---
// the list of non-empty buckets (lpos: k_bucket_desc's flags, scanned)
__global__ void k_bucket_compact(const uint4* __restrict__ bdesc, const uint32_t* __restrict__ lpos,
                                 uint32_t* __restrict__ blist_b, uint4* __restrict__ blist_q) {
  const uint32_t b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= kNumBuckets) return;
  const uint4 q = bdesc[b];
  if (q.x < q.y) {
    blist_b[lpos[b]] = b;
    blist_q[lpos[b]] = q;
  }
}

// {lo, hi, c0, nch} of every bucket, from the pass-2 scan, and its
// non-empty flag (scanned into list positions)
__global__ void k_bucket_desc(const uint32_t* __restrict__ goff2, const uint32_t* __restrict__ gcount,
                              const uint32_t* __restrict__ cfirst, uint4* __restrict__ bdesc, uint32_t* __restrict__ nz) {
  const uint32_t b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= kNumBuckets) return;
  const uint32_t d = b >> 8, f = b & 255, c0 = cfirst[d], nch = cfirst[d + 1] - c0;
  const uint32_t* row = goff2 + (uint64_t)f * *gcount + c0;
  const uint32_t lo = row[0], hi = row[nch];
  bdesc[b] = make_uint4(lo, hi, c0, nch);
  nz[b] = lo < hi ? 1u : 0u;
}

// gbnd[b * NG + g]: bucket b = (d, f) holds the runs of slice d's chunks in
// byte row f, chunk-ordered, so group g's entries start at the run of the
// first chunk of slice-group (d, g) (an empty slice-group: the next one's)
__global__ void k_bucket_groups(const uint32_t* __restrict__ goff2, const uint32_t* __restrict__ gcount,
                                const uint32_t* __restrict__ cbase, uint32_t NG, uint32_t* __restrict__ gbnd) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (uint64_t)kNumBuckets * NG) return;
  const uint32_t b = (uint32_t)(i / NG), g = (uint32_t)(i % NG);
  gbnd[i] = goff2[(uint64_t)(b & 255) * *gcount + cbase[(b >> 8) * NG + g]];
}

// the pass-2 digit plane of pass-1 entries (top byte of each), after a pass 1
// that did not write it: 4 entries per thread and step
__global__ void k_top_plane(const uint32_t* __restrict__ v1, uint64_t n, uint8_t* __restrict__ b1) {
  for (uint64_t i = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) * 4; i < n;
       i += (uint64_t)gridDim.x * blockDim.x * 4) {
    if (i + 4 <= n && ((uintptr_t)(v1 + i) & 15) == 0) {
      const uint4 q = *reinterpret_cast<const uint4*>(v1 + i);
      *reinterpret_cast<uint32_t*>(b1 + i) = (q.x >> 24) | ((q.y >> 24) << 8) | ((q.z >> 24) << 16) | (q.w & 0xFF000000u);
    } else {
      for (uint64_t k = i; k < i + 4 && k < n; k++) b1[k] = (uint8_t)(v1[k] >> 24);
    }
  }
}

// ------------------------------------------------------------------ scan ---
// Exclusive scan of u32 counts into u32 offsets (totals < 2^32), out[n] = total.
constexpr int kScanThreads = 1024;
constexpr int kScanPer = 16;
constexpr uint32_t kScanTile = kScanThreads * kScanPer;

__device__ __forceinline__ uint32_t block_excl_scan(uint32_t v, uint32_t* wsum, uint32_t* total) {
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  uint32_t incl = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const uint32_t y = __shfl_up(incl, o);
    if (lane >= o) incl += y;
  }
  if (lane == 63) wsum[w] = incl;
  __syncthreads();
  if (tid < 64) {
    const uint32_t x = tid < (int)(blockDim.x >> 6) ? wsum[tid] : 0u;
    uint32_t wi = x;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const uint32_t y = __shfl_up(wi, o);
      if (lane >= o) wi += y;
    }
    if (tid < (int)(blockDim.x >> 6)) wsum[tid] = wi - x;
    if (tid == 63) *total = wi;
  }
  __syncthreads();
  return wsum[w] + incl - v;
}

// n_dev (nullable): the element count is (*n_dev) * mul, <= the host bound n.
__device__ __forceinline__ uint64_t scan_n(uint64_t n, const uint32_t* n_dev, uint32_t mul) {
  return n_dev ? (uint64_t)(*n_dev) * mul : n;
}

__global__ __launch_bounds__(kScanThreads) void k_scan32_reduce(const uint32_t* __restrict__ in, uint64_t n,
                                                                const uint32_t* __restrict__ n_dev, uint32_t mul,
                                                                uint32_t* __restrict__ sums) {
  __shared__ uint32_t wsum[16];
  n = scan_n(n, n_dev, mul);
  const uint64_t base = (uint64_t)blockIdx.x * kScanTile;
  uint32_t s = 0;
  if (base < n) {
#pragma unroll
    for (int k = 0; k < kScanPer; k++) {
      const uint64_t i = base + (uint64_t)k * kScanThreads + threadIdx.x;
      s += i < n ? in[i] : 0u;
    }
  }
  for (int o = 32; o; o >>= 1) s += __shfl_down(s, o);
  if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t t = 0;
    for (int w = 0; w < kScanThreads / 64; w++) t += wsum[w];
    sums[blockIdx.x] = t;
  }
}

// in place, one block: exclusive scan of nb block sums
__global__ __launch_bounds__(kScanThreads) void k_scan32_top(uint32_t* __restrict__ sums, uint64_t nb) {
  __shared__ uint32_t wsum[16];
  __shared__ uint32_t tot;
  uint32_t carry = 0;
  for (uint64_t b0 = 0; b0 < nb; b0 += kScanThreads) {
    const uint64_t i = b0 + threadIdx.x;
    const uint32_t v = i < nb ? sums[i] : 0u;
    const uint32_t ex = block_excl_scan(v, wsum, &tot);
    if (i < nb) sums[i] = carry + ex;
    carry += tot;
    __syncthreads();
  }
}

__global__ __launch_bounds__(kScanThreads) void k_scan32_apply(const uint32_t* __restrict__ in, uint64_t n,
                                                               const uint32_t* __restrict__ n_dev, uint32_t mul,
                                                               const uint32_t* __restrict__ sums,
                                                               uint32_t* __restrict__ out) {
  __shared__ uint32_t wsum[16];
  __shared__ uint32_t tot;
  n = scan_n(n, n_dev, mul);
  const uint64_t b_last = n ? (n - 1) / kScanTile : 0;
  if (blockIdx.x > b_last) return;
  // each thread owns kScanPer consecutive counters
  const uint64_t base = (uint64_t)blockIdx.x * kScanTile + (uint64_t)threadIdx.x * kScanPer;
  const bool full = base + kScanPer <= n;  // in / out are 256-B aligned: 16-B accesses
  uint32_t v[kScanPer];
  uint32_t s = 0;
  if (full) {
#pragma unroll
    for (int k = 0; k < kScanPer; k += 4) {
      const uint4 q = *reinterpret_cast<const uint4*>(in + base + k);
      v[k] = q.x;
      v[k + 1] = q.y;
      v[k + 2] = q.z;
      v[k + 3] = q.w;
    }
  } else {
#pragma unroll
    for (int k = 0; k < kScanPer; k++) v[k] = base + k < n ? in[base + k] : 0u;
  }
#pragma unroll
  for (int k = 0; k < kScanPer; k++) s += v[k];
  uint32_t run = (sums ? sums[blockIdx.x] : 0u) + block_excl_scan(s, wsum, &tot);
  uint32_t o[kScanPer];
#pragma unroll
  for (int k = 0; k < kScanPer; k++) {
    o[k] = run;
    run += v[k];
  }
  if (full) {
#pragma unroll
    for (int k = 0; k < kScanPer; k += 4)
      *reinterpret_cast<uint4*>(out + base + k) = make_uint4(o[k], o[k + 1], o[k + 2], o[k + 3]);
  } else {
#pragma unroll
    for (int k = 0; k < kScanPer; k++)
      if (base + k < n) out[base + k] = o[k];
  }
  if (blockIdx.x == b_last && threadIdx.x == kScanThreads - 1) out[n] = run;
}

static size_t scan32_ws(uint64_t n) { return align256(((n + kScanTile - 1) / kScanTile) * 4); }

// n = host bound; with n_dev the count is (*n_dev) * mul (<= n)
static int scan32(sg_ctx* ctx, const uint32_t* in, uint32_t* out, uint64_t n, uint32_t* scratch,
                  const uint32_t* n_dev = nullptr, uint32_t mul = 1) {
  ScopedTimer tm(ctx, "scan");
  const uint64_t nb = (n + kScanTile - 1) / kScanTile;
  if (nb == 0) {
    SG_HIP(hipMemsetAsync(out, 0, 4, ctx->stream));
    return SG_OK;
  }
  if (nb == 1) {  // one tile: the apply pass alone
    hipLaunchKernelGGL(k_scan32_apply, dim3(1), dim3(kScanThreads), 0, ctx->stream, in, n, n_dev, mul,
                       (const uint32_t*)nullptr, out);
    SG_HIP(hipGetLastError());
    return SG_OK;
  }
  hipLaunchKernelGGL(k_scan32_reduce, dim3((uint32_t)nb), dim3(kScanThreads), 0, ctx->stream, in, n, n_dev, mul,
                     scratch);
  hipLaunchKernelGGL(k_scan32_top, dim3(1), dim3(kScanThreads), 0, ctx->stream, scratch, nb);
  hipLaunchKernelGGL(k_scan32_apply, dim3((uint32_t)nb), dim3(kScanThreads), 0, ctx->stream, in, n, n_dev, mul,
                     scratch, out);
  SG_HIP(hipGetLastError());
  return SG_OK;
}

// ------------------------------------------------------------------ host ---
// The regions' sizes, row by row as enum Region lists them (each 256-B
// aligned by WsPlan).
BucketPlan::BucketPlan(uint64_t n_, uint64_t nrec_) : n(n_), nrec(nrec_) {
  nA = (n + kPT - 1) / kPT;
  nB = nrec ? (nrec - 1) / kRecCap : 0;
  T = nA + nB;
  NG = nrec ? (nrec - 1) / kGroupRecs + 1 : 1;
  ng = 256 * NG;
  gmax = ng + nA;  // sum over slice-groups of ceil(size / kPT) <= ng + n / kPT
  const uint64_t nb = kNumBuckets;
  const size_t bytes[] = {
      (T + 1) * 4, (T + 1) * 4, (NG + 1) * 4,
      256 * T * 4, (256 * T + 1) * 4, n * 4, n + 64,  // (k_hist_bytes reads 16-B quads past the plane's end)
      ng * 4, (ng + 1) * 4,
      (gmax + 1) * 4, (gmax + 1) * 4, 257 * 4,
      gmax * 16, gmax * 8,
      nb * 16, nb * NG * 4,
      256 * gmax * 4, (256 * gmax + 1) * 4, n * 4 + 64,  // (the bucket kernel's 16-B loads may read past the end)
      (nb + 1) * 4, (kTkWords + kFsWords) * 4,
      nb * 4, (nb + 1) * 4,
      nb * 4, nb * 16,
      scan32_ws(256 * (gmax > T ? gmax : T)), T * (kPT / 8),
  };
  static_assert(sizeof(bytes) / sizeof(bytes[0]) == kRegions, "one size per region");
  for (size_t b : bytes) p.add(b);
}

size_t bucket_plan_bytes(uint64_t n, uint64_t nrec) { return BucketPlan(n, nrec).p.total; }

int partition_pass1(sg_ctx* ctx, const uint32_t* d_vals, const uint64_t* d_off, size_t ws_base, bool reserved,
                    BucketPlan& bp, bool trace, bool plane) {
  if (256 * bp.gmax >= 0xFFFFFFFFull || bp.NG > kMaxGroups) {
    set_error("bucket triage: batch too large");
    return SG_EINVAL;
  }
  int rc = reserved ? SG_OK : ws_reserve(ctx, ws_base + bp.p.total);
  if (rc) return rc;
  if (ctx->ws.cap < ws_base + bp.p.total) {
    set_error("bucket triage: workspace not reserved");
    return SG_EINVAL;
  }
  bp.rebase(ws_base);
  uint32_t* tstart = bp.at<uint32_t>(ctx, kTS);
  uint32_t* trec = bp.at<uint32_t>(ctx, kTR);
  uint32_t* hist1 = bp.at<uint32_t>(ctx, kH1);
  uint32_t* goff1 = bp.at<uint32_t>(ctx, kO1);
  uint64_t* keep = bp.at<uint64_t>(ctx, kKM);
  const uint32_t T = (uint32_t)bp.T, NG = (uint32_t)bp.NG;
  const bool dbg = ctx->debug_part;
  // pass-1 tiles
  const Cuts c1{bp.nA, kPT, bp.nB, bp.n, d_off, bp.nrec, tstart, trec};
  hipLaunchKernelGGL(k_cuts, dim3(div_up(bp.T + 1, 256)), dim3(256), 0, ctx->stream, c1);
  hipLaunchKernelGGL(k_group_tiles, dim3(div_up(bp.NG + 1, 256)), dim3(256), 0, ctx->stream, d_off, bp.nA, NG, T,
                     bp.at<uint32_t>(ctx, kGT));
  {
    ScopedTimer tm(ctx, "p1_hist");
    if (trace)
      hipLaunchKernelGGL(k_hist_trace, dim3(T), dim3(kPThreads), 0, ctx->stream, d_vals, d_off, bp.nrec,
                         (const uint32_t*)tstart, (const uint32_t*)trec, T, hist1, keep);
    else if (((uintptr_t)d_vals & 15) == 0)
      hipLaunchKernelGGL(k_hist_rep<false>, dim3(T), dim3(kPThreads), 0, ctx->stream, d_vals,
                         (const uint32_t*)tstart, (const uint4*)nullptr, T, (const uint32_t*)nullptr, hist1);
    else
      hipLaunchKernelGGL(k_p1_hist, dim3(T), dim3(kPThreads), 0, ctx->stream, d_vals,
                         (const uint32_t*)tstart, hist1);
  }
  rc = scan32(ctx, hist1, goff1, 256 * bp.T, bp.at<uint32_t>(ctx, kSC));
  if (rc) return rc;
  P1Args a1{d_vals, d_off, bp.nrec, tstart, trec, T, goff1, hist1, bp.at<uint32_t>(ctx, kV1),
            plane ? bp.at<uint8_t>(ctx, kB1) : nullptr, nullptr, keep};
  DevBuf<unsigned long long> p1dbg;
  if (dbg) {
    rc = p1dbg.grow_drop(8, nullptr);
    if (rc) return rc;
    SG_HIP(hipMemsetAsync(p1dbg.p, 0, 64, ctx->stream));
    a1.dbg = p1dbg.p;
  }
  {
    ScopedTimer tm(ctx, "p1_scatter");
    auto k1 = dbg ? (trace ? k_p1_scatter<true, true> : k_p1_scatter<true, false>)
                  : (trace ? k_p1_scatter<false, true> : k_p1_scatter<false, false>);
    hipLaunchKernelGGL(k1, dim3(T), dim3(kPThreads), 0, ctx->stream, a1);
  }
  if (dbg) {
    unsigned long long h[8];
    SG_HIP(hipMemcpy(h, p1dbg.p, 64, hipMemcpyDeviceToHost));
    fprintf(stderr, "sg p1_scatter per tile (cycles, wave 0): load+meta %.0f build+lookup %.0f rank %.0f stage %.0f "
            "write %.0f (tiles %llu)\n", (double)h[0] / h[5], (double)h[1] / h[5], (double)h[2] / h[5],
            (double)h[3] / h[5], (double)h[4] / h[5], h[5]);
  }
  return SG_OK;
}

int partition_pass2_tables(sg_ctx* ctx, const BucketPlan& bp, bool plane) {
  const uint32_t* gt = bp.at<uint32_t>(ctx, kGT);
  const uint32_t* goff1 = bp.at<uint32_t>(ctx, kO1);
  uint32_t* v1 = bp.at<uint32_t>(ctx, kV1);
  uint8_t* b1 = bp.at<uint8_t>(ctx, kB1);
  uint32_t* nch = bp.at<uint32_t>(ctx, kNC);
  uint32_t* cbase = bp.at<uint32_t>(ctx, kCB);
  uint32_t* cstart = bp.at<uint32_t>(ctx, kCS);
  uint32_t* cgov = bp.at<uint32_t>(ctx, kCG);
  uint32_t* cfirst = bp.at<uint32_t>(ctx, kCF);
  uint4* cdesc = bp.at<uint4>(ctx, kCD);
  uint2* dtile = bp.at<uint2>(ctx, kDT);
  uint32_t* hist2 = bp.at<uint32_t>(ctx, kH2);
  uint32_t* goff2 = bp.at<uint32_t>(ctx, kO2);
  uint32_t* scr = bp.at<uint32_t>(ctx, kSC);
  const uint32_t T = (uint32_t)bp.T, G = (uint32_t)bp.gmax, NG = (uint32_t)bp.NG;
  const uint32_t* gcount = cbase + bp.ng;  // device: number of pass-2 chunks
  if (!plane) {
    hipLaunchKernelGGL(k_top_plane, dim3((uint32_t)std::min<uint64_t>(4096, div_up(bp.n, 1024))), dim3(256), 0,
                       ctx->stream, (const uint32_t*)v1, bp.n, b1);
    SG_HIP(hipGetLastError());
  }
  // pass-2 chunks
  hipLaunchKernelGGL(k_group_chunks, dim3(div_up(bp.ng, 256)), dim3(256), 0, ctx->stream, goff1, T, NG, gt, bp.ng,
                     nch);
  int rc = scan32(ctx, nch, cbase, bp.ng, scr);
  if (rc) return rc;
  hipLaunchKernelGGL(k_chunk_list, dim3(div_up((bp.ng > bp.gmax ? bp.ng : bp.gmax) + 1, 256)), dim3(256), 0,
                     ctx->stream, goff1, T, NG, gt, bp.ng, (const uint32_t*)cbase, bp.gmax, cstart, cgov, cfirst);
  hipLaunchKernelGGL(k_chunk_desc, dim3(div_up(bp.gmax, 256)), dim3(256), 0, ctx->stream, (const uint32_t*)cstart,
                     (const uint32_t*)cgov, gcount, bp.gmax, goff1, T, NG, gt, (const uint32_t*)nullptr, cdesc, dtile);
  {
    ScopedTimer tm(ctx, "p2_hist");
    hipLaunchKernelGGL(k_hist_bytes, dim3(G), dim3(kHBThreads), 0, ctx->stream, (const uint8_t*)b1,
                       (const uint4*)cdesc, gcount, hist2);
  }
  return scan32(ctx, hist2, goff2, 256 * bp.gmax, scr, gcount, 256);
}

// The chunk descriptors again, each window's blocks contiguous (k_chunk_desc).
int partition_pass2_windows(sg_ctx* ctx, const BucketPlan& bp, const uint32_t* bounds) {
  const uint32_t* cbase = bp.at<uint32_t>(ctx, kCB);
  hipLaunchKernelGGL(k_chunk_desc, dim3(div_up(bp.gmax, 256)), dim3(256), 0, ctx->stream,
                     (const uint32_t*)bp.at<uint32_t>(ctx, kCS), (const uint32_t*)bp.at<uint32_t>(ctx, kCG),
                     cbase + bp.ng, bp.gmax, (const uint32_t*)bp.at<uint32_t>(ctx, kO1), (uint32_t)bp.T,
                     (uint32_t)bp.NG, (const uint32_t*)bp.at<uint32_t>(ctx, kGT), bounds, bp.at<uint4>(ctx, kCD),
                     bp.at<uint2>(ctx, kDT));
  SG_HIP(hipGetLastError());
  return SG_OK;
}

// The scatter over every chunk, or over one window of a late pass 2 in one of
// its forms (the grid is the host's bound either way: the blocks outside the
// window, and every block of the form that is not the launch's case, return
// at once).
int partition_pass2_scatter(sg_ctx* ctx, const BucketPlan& bp, const P2Late* late) {
  const uint32_t* cbase = bp.at<uint32_t>(ctx, kCB);
  P2Args a2{bp.at<uint32_t>(ctx, kV1), bp.at<uint4>(ctx, kCD), bp.at<uint2>(ctx, kDT), cbase + bp.ng,
            bp.at<uint32_t>(ctx, kO1), bp.at<uint32_t>(ctx, kTR), (uint32_t)bp.T, (uint32_t)bp.NG,
            bp.at<uint32_t>(ctx, kO2), bp.at<uint32_t>(ctx, kH2), bp.at<uint32_t>(ctx, kV2),
            0, nullptr, nullptr, 0, nullptr, bp.at<uint32_t>(ctx, kCS)};
  if (late) {
    a2.win = (uint32_t)late->win;
    a2.bounds = late->bounds;
    a2.fs_cnt = late->fs_cnt;
    a2.fs_nblk = late->fs_nblk;
    a2.fs_u16 = late->fs_u16;
  }
  {
    ScopedTimer tm(ctx, "p2_scatter");
    if (late && late->u16)
      hipLaunchKernelGGL(k_p2_scatter16, dim3((uint32_t)(bp.gmax / 2 + 1)), dim3(kPThreads), 0, ctx->stream, a2);
    else
      hipLaunchKernelGGL(k_p2_scatter, dim3((uint32_t)bp.gmax), dim3(kPThreads), 0, ctx->stream, a2);
  }
  SG_HIP(hipGetLastError());
  return SG_OK;
}

int partition_pass2_buckets(sg_ctx* ctx, const BucketPlan& bp) {
  uint32_t* cbase = bp.at<uint32_t>(ctx, kCB);
  uint32_t* cfirst = bp.at<uint32_t>(ctx, kCF);
  uint4* bdesc = bp.at<uint4>(ctx, kBD);
  uint32_t* goff2 = bp.at<uint32_t>(ctx, kO2);
  uint32_t* scr = bp.at<uint32_t>(ctx, kSC);
  uint32_t* bnz = bp.at<uint32_t>(ctx, kBN);
  uint32_t* blpos = bp.at<uint32_t>(ctx, kBP);
  const uint32_t NG = (uint32_t)bp.NG;
  const uint32_t* gcount = cbase + bp.ng;
  hipLaunchKernelGGL(k_bucket_desc, dim3(kNumBuckets / 256), dim3(256), 0, ctx->stream, (const uint32_t*)goff2,
                     gcount, (const uint32_t*)cfirst, bdesc, bnz);
  hipLaunchKernelGGL(k_bucket_groups, dim3(div_up((uint64_t)kNumBuckets * NG, 256)), dim3(256), 0, ctx->stream,
                     (const uint32_t*)goff2, gcount, (const uint32_t*)cbase, NG, bp.at<uint32_t>(ctx, kGB));
  const int rc = scan32(ctx, bnz, blpos, kNumBuckets, scr);
  if (rc) return rc;
  hipLaunchKernelGGL(k_bucket_compact, dim3(kNumBuckets / 256), dim3(256), 0, ctx->stream, (const uint4*)bdesc,
                     (const uint32_t*)blpos, bp.at<uint32_t>(ctx, kLB), bp.at<uint4>(ctx, kLQ));
  SG_HIP(hipGetLastError());
  return SG_OK;
}

int partition_pass2(sg_ctx* ctx, const BucketPlan& bp, bool plane) {
  int rc = partition_pass2_tables(ctx, bp, plane);
  if (!rc) rc = partition_pass2_scatter(ctx, bp, nullptr);
  if (!rc) rc = partition_pass2_buckets(ctx, bp);
  return rc;
}

int partition_one(sg_ctx* ctx, const uint32_t* d_vals, const uint64_t* d_off, size_t ws_base, bool reserved,
                  BucketPlan& bp, bool trace) {
  const int rc = partition_pass1(ctx, d_vals, d_off, ws_base, reserved, bp, trace, true);
  return rc ? rc : partition_pass2(ctx, bp);
}

}  // namespace sg
