// sg_triage_runs.hip -- triageInput's loop (syz-fuzzer/fuzzer.go:521-576) from
// the raw KCOV buffers of its re-executions, for a batch of candidates.
//
// Per candidate k the reference computes newSignal =
// Canonicalize(SignalDiff(corpusSignal, inp.signal)) (:526-532), then either
// takes the cover of the first run that has one (inp.minimized, :543-552) or
// runs three times, each run with a non-empty Signal taking newSignal =
// Intersection(newSignal, Canonicalize(Signal)) (:567) and folding Cover into
// inputCover by copy or Union (:571-575); a second run without Signal (:560-562)
// or an empty newSignal (:568-570) ends the candidate.
//
// Stages, all on the context's stream:
//  1. k_tr_select marks call[k] of every execution (an execution with fewer
//     calls is len(info) == 0); k_tr_trunc truncates the PCs (executor.h:394).
//     Both are sg_runs.h's, shared with sg_minimize_pred.hip.
//  2. Signal_i: the queued exec-signal path of sg_exec.hip (exec_signal_body
//     with the marks as its queued flags: each execution runs up to its call).
//     Cover_i: exec_cover (sg_exec_cover.hip) restricted to the marked calls.
//  3. k_tin_diff and canonicalize_dev give newSignal, as sg_triage_newsig.
//  4. One k_tr_round launch per run: a workgroup per candidate reads the
//     candidate's state word and newSignal's current length from device memory,
//     applies the "not executed" rule or tin_intersect (the body k_tin_intersect
//     runs), and writes both back.  No host round trip between runs.
//  5. k_tr_cover, a workgroup per candidate, folds the counted covers.  Lists
//     that are non-decreasing as u32 take the parallel route: one list is
//     copied (a copy keeps 0xFFFFFFFF); two or more have Union's result, every
//     value below the sentinel at its largest count over the lists, which is
//     the distinct (value, occurrence) pairs: keys value << 32 | occurrence are
//     sorted in LDS and their first occurrences written; with more than kTrSort
//     values each pair is written by the first list that has it, at its rank
//     (binary searches in the lists, a scan per list).  A candidate with a
//     list that is not non-decreasing (PCs that differ above bit 31: the
//     foreach merge is then order-dependent; counter "triage_runs_wide") or
//     with a list of sentinels only (Union can then return nothing and the
//     next run is copied) runs the two-pointer foreach itself on one lane,
//     bounded by the two lengths.  Each candidate with a cover adds one to
//     its route's device counter ("triage_runs_copied" / "_sorted" /
//     "_ranked" / "_foreach"), so a test can prove which route ran.
//  6. scan_counts gives new_off and cov_off; k_tr_pack writes each payload when
//     it fits its capacity.
#include "sg_runs.h"
#include "sg_tinput.h"

namespace sg {
namespace {

using namespace tin;

constexpr uint32_t kTrMaxRuns = 8;
constexpr uint64_t kTrPad = ~0ull;

// the per-candidate state word: done | status << 8 | skipped << 16 | counted << 24
// (counted: bit i = run i's Signal took part, so its Cover does)
__host__ __device__ inline uint32_t st_make(uint32_t done, uint32_t status, uint32_t skipped, uint32_t counted) {
  return done | (status << 8) | (skipped << 16) | (counted << 24);
}

struct RoundArgs {
  uint32_t run, nruns;
  const uint8_t* minimized;
  const uint32_t* selcall;
  const uint64_t* xsig_off;
  const uint32_t* xsig;
  uint32_t* diff;  // newSignal of candidate k at diff_off[k], cur_len[k] values
  const uint64_t* diff_off;
  uint64_t* cur_len;
  uint32_t* state;
};

// run `run` of every candidate (fuzzer.go:556-570)
__global__ __launch_bounds__(kTB) void k_tr_round(RoundArgs a) {
  __shared__ IntersectLds lds;
  __shared__ uint32_t s_st;
  __shared__ uint64_t s_len;
  const uint64_t k = blockIdx.x;
  if (threadIdx.x == 0) {
    s_st = a.state[k];
    s_len = a.cur_len[k];
  }
  __syncthreads();
  const uint32_t st = s_st;
  if ((st & 0xFF) || a.minimized[k]) return;
  const uint32_t c = a.selcall[k * a.nruns + a.run];
  const uint64_t r0 = c == kNoCall ? 0 : a.xsig_off[c], r1 = c == kNoCall ? 0 : a.xsig_off[c + 1];
  if (r1 <= r0) {  // :558-565 the call was not executed
    if (threadIdx.x == 0)
      a.state[k] = ((st >> 16) & 0xFF) ? st_make(1, SG_TIN_NOT_EXECUTED, 1, st >> 24) : (st | (1u << 16));
    return;
  }
  const uint64_t a0 = a.diff_off[k];
  const uint64_t kept = tin_intersect<true>(a.diff, a0, a0 + s_len, a.xsig, r0, r1, lds);  // :567
  if (threadIdx.x == 0) {
    a.cur_len[k] = kept;
    a.state[k] = kept == 0 ? st_make(1, SG_TIN_FLAKY, (st >> 16) & 0xFF, st >> 24)  // :568-570
                           : (st | (1u << (24 + a.run)));
  }
}

struct CoverArgs {
  uint32_t nruns;
  uint64_t ncalls, npcs;
  const uint8_t* minimized;
  const uint32_t* selcall;
  const uint64_t* prog_off;
  const uint64_t* call_off;
  const uint64_t* xcov_off;
  const uint32_t* xcov;
  const uint32_t* state;
  const uint64_t* cur_len;
  int32_t* status;
  uint32_t* newlen;
  uint32_t* covlen;
  uint8_t* covsrc;  // which of buf[0] / buf[1] holds the candidate's cover
  uint32_t* buf[2];  // [npcs] each: candidate k's slot starts at its first execution's first PC
  uint32_t* wide;
  uint32_t* routes;  // [kTrRoutes]: the candidates whose cover took each route
};

// Union (cover.go:63-70) through foreach (:81-102), literally, on one lane
__device__ uint32_t tr_union(const uint32_t* __restrict__ x, uint32_t nx, const uint32_t* __restrict__ y, uint32_t ny,
                             uint32_t* __restrict__ out, uint64_t cap) {
  uint32_t i0 = 0, i1 = 0, n = 0;
  for (uint64_t step = 0; step < (uint64_t)nx + ny && (i0 < nx || i1 < ny); step++) {
    const uint32_t v0 = i0 < nx ? x[i0] : kSentT, v1 = i1 < ny ? y[i1] : kSentT;
    if (v0 <= v1) i0++;
    if (v1 <= v0) i1++;
    const uint32_t v = v0 <= v1 ? v0 : v1;
    if (v != kSentT && n < cap) out[n++] = v;
  }
  return n;
}

// first i with x[i] >= v / x[i] > v in a non-decreasing x[0 .. n)
__device__ __forceinline__ uint32_t tr_lower(const uint32_t* __restrict__ x, uint32_t n, uint32_t v) {
  uint32_t lo = 0, hi = n;
  for (int step = 0; step < 32 && lo < hi; step++) {
    const uint32_t mid = lo + ((hi - lo) >> 1);
    if (x[mid] < v)
      lo = mid + 1;
    else
      hi = mid;
  }
  return lo;
}
__device__ __forceinline__ uint32_t tr_upper(const uint32_t* __restrict__ x, uint32_t n, uint32_t v) {
  uint32_t lo = 0, hi = n;
  for (int step = 0; step < 32 && lo < hi; step++) {
    const uint32_t mid = lo + ((hi - lo) >> 1);
    if (x[mid] <= v)
      lo = mid + 1;
    else
      hi = mid;
  }
  return lo;
}

// status, newSignal's length and inputCover of every candidate (fuzzer.go:543-552, :571-575)
__global__ __launch_bounds__(kTB) void k_tr_cover(CoverArgs a) {
  __shared__ unsigned long long keys[kTrSort];
  __shared__ uint32_t wsum[kTB / 64];
  __shared__ uint64_t s_lo[kTrMaxRuns];
  __shared__ uint32_t s_ln[kTrMaxRuns];
  __shared__ uint32_t s_m, s_alls;
  __shared__ uint32_t s_at[kTrMaxRuns], s_cnt[kTrMaxRuns];
  const uint64_t k = blockIdx.x;
  const uint32_t tid = threadIdx.x;
  const uint32_t st = a.state[k];
  const bool mini = a.minimized[k] != 0;
  const int32_t status = (st & 0xFF) ? (int32_t)((st >> 8) & 0xFF) : SG_TIN_OK;
  if (tid == 0) {
    a.status[k] = status;
    a.newlen[k] = status == SG_TIN_OK ? (uint32_t)a.cur_len[k] : 0u;
    a.covsrc[k] = 0;
    if (status != SG_TIN_OK) a.covlen[k] = 0;
  }
  if (status != SG_TIN_OK) return;
  // the candidate's slot and the lists that fold into its cover, in run order
  const uint64_t e0 = k * a.nruns;
  const uint64_t slot = min(a.call_off[min(a.prog_off[e0], a.ncalls)], a.npcs);
  const uint64_t send = min(max(a.call_off[min(a.prog_off[e0 + a.nruns], a.ncalls)], slot), a.npcs);
  const uint64_t cap = send - slot;
  if (tid == 0) {
    uint32_t m = 0, alls = 0;
    for (uint32_t i = 0; i < a.nruns; i++) {
      const uint32_t c = a.selcall[e0 + i];
      if (c == kNoCall) continue;
      const uint64_t lo = a.xcov_off[c], L = a.xcov_off[c + 1] - lo;
      // :547-551 the first run with any cover; :558-575 the runs whose Signal counted
      if (mini ? (m == 0 && L > 0) : (((st >> (24 + i)) & 1u) && L > 0)) {
        s_lo[m] = lo;
        s_ln[m] = (uint32_t)L;
        alls |= a.xcov[lo] == kSentT;
        m++;
      }
    }
    s_m = m;
    s_alls = alls;
  }
  __syncthreads();
  const uint32_t m = s_m;
  if (m == 0) {
    if (tid == 0) a.covlen[k] = 0;
    return;
  }
  uint64_t total = 0;
  bool bad = false;
  for (uint32_t q = 0; q < m; q++) {
    const uint32_t* __restrict__ x = a.xcov + s_lo[q];
    const uint32_t L = s_ln[q];
    for (uint32_t j = tid; j + 1 < L; j += kTB) bad |= x[j] > x[j + 1];
    total += L;
  }
  const bool wide = __syncthreads_or(bad) != 0;
  if (wide && tid == 0) atomicAdd(a.wide, 1u);
  uint32_t* out = a.buf[0] + slot;
  if (m == 1) {  // a copy (:550, :572): the sentinel stays
    const uint32_t* __restrict__ x = a.xcov + s_lo[0];
    const uint32_t L = (uint32_t)min<uint64_t>(s_ln[0], cap);
    for (uint32_t j = tid; j < L; j += kTB) out[j] = x[j];
    if (tid == 0) {
      a.covlen[k] = L;
      atomicAdd(a.routes + kTrCopied, 1u);
    }
    return;
  }
  if (wide || s_alls || total > cap) {  // foreach itself, one lane (total > cap: inconsistent offsets)
    if (tid == 0) {
      uint32_t src = 0, n = (uint32_t)min<uint64_t>(s_ln[0], cap);
      const uint32_t* __restrict__ x0 = a.xcov + s_lo[0];
      for (uint32_t j = 0; j < n; j++) out[j] = x0[j];
      for (uint32_t q = 1; q < m; q++) {
        const uint32_t* __restrict__ y = a.xcov + s_lo[q];
        if (n == 0) {  // :571-572 len(inputCover) == 0: a copy
          n = (uint32_t)min<uint64_t>(s_ln[q], cap);
          for (uint32_t j = 0; j < n; j++) a.buf[src][slot + j] = y[j];
        } else {
          n = tr_union(a.buf[src] + slot, n, y, s_ln[q], a.buf[src ^ 1] + slot, cap);
          src ^= 1;
        }
      }
      a.covlen[k] = n;
      a.covsrc[k] = (uint8_t)src;
      atomicAdd(a.routes + kTrForeach, 1u);
    }
    return;
  }
  if (total > kTrSort) {
    // More values than the LDS sort holds: by ranks.  A pair (value, occurrence)
    // is written by the first list that has it; its place is the number of
    // written pairs below it, a sum over the lists of the written elements
    // before the pair's lower bound there.  E: each element's count of written
    // elements before it in its list (in the second buffer's slot).
    uint32_t* E = a.buf[1] + slot;
    uint32_t at = 0;
    for (uint32_t q = 0; q < m; q++) {
      const uint32_t* __restrict__ x = a.xcov + s_lo[q];
      const uint32_t L = s_ln[q];
      uint32_t run = 0;
      for (uint32_t j0 = 0; j0 < L; j0 += kTB) {
        const uint32_t j = j0 + tid;
        bool emit = false;
        if (j < L) {
          const uint32_t v = x[j];
          if (v != kSentT) {
            const uint32_t t = j - tr_lower(x, j, v);
            emit = true;
            for (uint32_t p = 0; p < q; p++) {
              const uint32_t* __restrict__ y = a.xcov + s_lo[p];
              if (tr_upper(y, s_ln[p], v) - tr_lower(y, s_ln[p], v) > t) emit = false;
            }
          }
        }
        uint32_t tot;
        const uint32_t rk = block_rank(emit, wsum, &tot);
        if (j < L) E[at + j] = run + rk;
        run += tot;
      }
      if (tid == 0) {
        s_at[q] = at;
        s_cnt[q] = run;
      }
      at += L;
    }
    __syncthreads();  // E and the counts are visible to the workgroup
    uint32_t n = 0;
    for (uint32_t q = 0; q < m; q++) {
      const uint32_t* __restrict__ x = a.xcov + s_lo[q];
      const uint32_t L = s_ln[q], at_q = s_at[q];
      for (uint32_t j = tid; j < L; j += kTB) {
        const uint32_t before = E[at_q + j], upto = j + 1 < L ? E[at_q + j + 1] : s_cnt[q];
        if (upto == before) continue;  // not written by this list
        const uint32_t v = x[j], t = j - tr_lower(x, j, v);
        uint32_t pos = 0;
        for (uint32_t p = 0; p < m; p++) {
          const uint32_t* __restrict__ y = a.xcov + s_lo[p];
          const uint32_t lb = tr_lower(y, s_ln[p], v), ub = tr_upper(y, s_ln[p], v);
          const uint32_t idx = lb + min(t, ub - lb);  // the first element of list p at or above (v, t)
          pos += idx < s_ln[p] ? E[s_at[p] + idx] : s_cnt[p];
        }
        if (pos < cap) out[pos] = v;
      }
      n += s_cnt[q];
    }
    if (tid == 0) {
      a.covlen[k] = (uint32_t)min<uint64_t>(n, cap);
      atomicAdd(a.routes + kTrRanked, 1u);
    }
    return;
  }
  // the LDS sort: keys value << 32 | occurrence, the sentinel left out
  uint32_t P = 1;
  while (P < total) P <<= 1;  // <= kTrSort
  uint32_t at = 0;
  for (uint32_t q = 0; q < m; q++) {
    const uint32_t* __restrict__ x = a.xcov + s_lo[q];
    const uint32_t L = s_ln[q];
    for (uint32_t j = tid; j < L; j += kTB) {
      const uint32_t v = x[j];
      uint32_t lo = 0, hi = j;  // first i with x[i] >= v (x is non-decreasing): v's first copy
      for (int step = 0; step < 32 && lo < hi; step++) {
        const uint32_t mid = (lo + hi) >> 1;
        if (x[mid] < v)
          lo = mid + 1;
        else
          hi = mid;
      }
      keys[at + j] = v == kSentT ? kTrPad : ((unsigned long long)v << 32) | (j - lo);
    }
    at += L;
  }
  for (uint32_t i = (uint32_t)total + tid; i < P; i += kTB) keys[i] = kTrPad;
  __syncthreads();
  for (uint32_t kk = 2; kk <= P; kk <<= 1)
    for (uint32_t j = kk >> 1; j > 0; j >>= 1) {
      for (uint32_t t = tid; t < P / 2; t += kTB) {
        const uint32_t lo = ((t & ~(j - 1)) << 1) | (t & (j - 1)), hi = lo + j;
        const unsigned long long x = keys[lo], y = keys[hi];
        const bool up = (lo & kk) == 0;
        if (up ? y < x : x < y) {
          keys[lo] = y;
          keys[hi] = x;
        }
      }
      __syncthreads();
    }
  uint32_t n = 0;
  for (uint32_t j0 = 0; j0 < P; j0 += kTB) {
    const uint32_t j = j0 + tid;
    unsigned long long key = kTrPad;
    bool keep = false;
    if (j < P) {
      key = keys[j];
      keep = key != kTrPad && (j == 0 || keys[j - 1] != key);
    }
    uint32_t tot;
    const uint32_t rk = block_rank(keep, wsum, &tot);
    if (keep && n + rk < cap) out[n + rk] = (uint32_t)(key >> 32);
    n += tot;
  }
  if (tid == 0) {
    a.covlen[k] = (uint32_t)min<uint64_t>(n, cap);
    atomicAdd(a.routes + kTrSorted, 1u);
  }
}

struct PackArgs {
  uint64_t n, ncalls, npcs;
  uint32_t nruns;
  const uint64_t* prog_off;
  const uint64_t* call_off;
  const uint32_t* diff;
  const uint64_t* diff_off;
  const uint64_t* new_off;
  uint32_t* new_vals;
  uint64_t new_cap;
  const uint8_t* covsrc;
  const uint32_t* buf[2];
  const uint64_t* cov_off;
  uint32_t* cov_vals;
  uint64_t cov_cap;
};

// a wave per candidate: both payloads, each when it fits its capacity
__global__ __launch_bounds__(256) void k_tr_pack(PackArgs a) {
  const uint64_t k = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (k >= a.n) return;
  const uint32_t lane = threadIdx.x & 63;
  if (a.new_vals && a.new_off[a.n] <= a.new_cap) {
    const uint64_t d = a.new_off[k], L = a.new_off[k + 1] - d, s = a.diff_off[k];
    for (uint64_t i = lane; i < L; i += 64) a.new_vals[d + i] = a.diff[s + i];
  }
  if (a.cov_vals && a.cov_off[a.n] <= a.cov_cap) {
    const uint64_t slot = min(a.call_off[min(a.prog_off[k * a.nruns], a.ncalls)], a.npcs);
    const uint32_t* __restrict__ src = a.buf[a.covsrc[k] & 1] + slot;
    const uint64_t d = a.cov_off[k], L = a.cov_off[k + 1] - d;
    for (uint64_t i = lane; i < L; i += 64) a.cov_vals[d + i] = src[i];
  }
}

// the call's intermediates: regions of the caller's staging plan
struct TrPlan {
  size_t pcs32, sel, selcall, xsig_off, xsig, xcov_off, xcov, diff, diff_off, cnt, cur_len, state, newlen, covlen, covsrc,
      buf0, buf1;
  TrPlan(WsPlan& p, uint64_t n, uint64_t nexec, uint64_t ncalls, uint64_t npcs, uint64_t nsig) {
    pcs32 = p.add(npcs * 4 + 4);
    sel = p.add(ncalls + 1);
    selcall = p.add(nexec * 4 + 4);
    xsig_off = p.add((ncalls + 1) * 8);
    xsig = p.add(npcs * 4 + 4);
    xcov_off = p.add((ncalls + 1) * 8);
    xcov = p.add(npcs * 4 + 4);
    diff = p.add(nsig * 4 + 4);
    diff_off = p.add((n + 1) * 8);
    cnt = p.add(n * 4 + 4);
    cur_len = p.add(n * 8 + 8);
    state = p.add(n * 4 + 4);
    newlen = p.add(n * 4 + 4);
    covlen = p.add(n * 4 + 4);
    covsrc = p.add(n + 1);
    buf0 = p.add(npcs * 4 + 4);
    buf1 = p.add(npcs * 4 + 4);
  }
};

struct TrIo {
  const uint32_t* sig_vals;
  const uint64_t* sig_off;
  uint64_t n, nsig;
  const uint32_t* call;
  const uint8_t* minimized;
  uint32_t nruns;
  const uint64_t* pcs;
  const uint64_t* call_off;
  const uint64_t* prog_off;
  uint64_t ncalls, npcs;
  int32_t* status;
  uint64_t* new_off;
  uint32_t* new_vals;
  uint64_t new_cap;
  uint64_t* cov_off;
  uint32_t* cov_vals;
  uint64_t cov_cap;
};

int tr_limits(uint64_t n, uint32_t nruns, uint64_t ncalls, uint64_t npcs, uint64_t nsig) {
  if (nruns < 1 || nruns > kTrMaxRuns || n >= (1ull << 28) || ncalls >= (1ull << 31) || npcs >= (1ull << 32) ||
      nsig >= (1ull << 32)) {
    set_error("sg_triage_runs_from_kcov: %llu candidates x %u runs, %llu calls, %llu PCs, %llu signals (nruns is 1..8; "
              "the limits are 2^28 - 1, 2^31 - 1, 2^32 - 1 and 2^32 - 1)",
              (unsigned long long)n, nruns, (unsigned long long)ncalls, (unsigned long long)npcs,
              (unsigned long long)nsig);
    return SG_EINVAL;
  }
  return SG_OK;
}

// the body of both forms: every pointer of io is device memory, the
// intermediates are p's regions of the staging buffer (reserved by the
// caller); ctx lock held, the device ensured, n > 0
int triage_runs(sg_ctx* ctx, sg_set* corpus, const TrIo& io, const TrPlan& p) {
  const uint64_t n = io.n, nexec = n * io.nruns, ncalls = io.ncalls, npcs = io.npcs;
  uint32_t* pcs32 = dstage_at<uint32_t>(ctx, p.pcs32);
  uint8_t* sel = dstage_at<uint8_t>(ctx, p.sel);
  uint32_t* selcall = dstage_at<uint32_t>(ctx, p.selcall);
  uint64_t* xsig_off = dstage_at<uint64_t>(ctx, p.xsig_off);
  uint32_t* xsig = dstage_at<uint32_t>(ctx, p.xsig);
  uint64_t* xcov_off = dstage_at<uint64_t>(ctx, p.xcov_off);
  uint32_t* xcov = dstage_at<uint32_t>(ctx, p.xcov);
  uint32_t* diff = dstage_at<uint32_t>(ctx, p.diff);
  uint64_t* diff_off = dstage_at<uint64_t>(ctx, p.diff_off);
  uint32_t* cnt = dstage_at<uint32_t>(ctx, p.cnt);
  uint64_t* cur_len = dstage_at<uint64_t>(ctx, p.cur_len);
  uint32_t* state = dstage_at<uint32_t>(ctx, p.state);
  uint32_t* newlen = dstage_at<uint32_t>(ctx, p.newlen);
  uint32_t* covlen = dstage_at<uint32_t>(ctx, p.covlen);
  uint8_t* covsrc = dstage_at<uint8_t>(ctx, p.covsrc);
  uint32_t* buf0 = dstage_at<uint32_t>(ctx, p.buf0);
  uint32_t* buf1 = dstage_at<uint32_t>(ctx, p.buf1);
  uint32_t* wide = &ctx->dev.p->tr_wide;
  const dim3 b(256);
  int rc;
  SG_HIP(hipMemsetAsync(wide, 0, 4 * (1 + kTrRoutes), ctx->stream));  // (read by sg_ctx_counter only: no wait here)
  // 1. the calls that count, the truncated PCs
  SG_HIP(hipMemsetAsync(sel, 0, ncalls + 1, ctx->stream));
  hipLaunchKernelGGL(k_tr_select, dim3(div_up(nexec, 256)), b, 0, ctx->stream, io.prog_off, io.call, nexec, io.nruns,
                     ncalls, selcall, sel);
  if (npcs)
    hipLaunchKernelGGL(k_tr_trunc, dim3(std::min<uint64_t>(div_up(npcs, 256), 65536)), b, 0, ctx->stream, io.pcs, npcs,
                       pcs32);
  SG_HIP(hipGetLastError());
  // 2. Signal_i and Cover_i of those calls
  rc = exec_signal_body(ctx, pcs32, io.call_off, io.prog_off, nexec, ncalls, npcs, sel, xsig, xsig_off);
  if (rc) return rc;
  rc = exec_cover(ctx, io.pcs, io.call_off, ncalls, npcs, 1, xcov_off, xcov, npcs, sel);
  if (rc) return rc;
  // 3. newSignal = Canonicalize(SignalDiff(corpusSignal, inp.signal)) (fuzzer.go:526-532)
  rc = ws_reserve(ctx, scan_ws_bytes(n));
  if (rc) return rc;
  {
    ScopedTimer tm(ctx, "tinput_diff");
    hipLaunchKernelGGL(k_tin_diff<false>, dim3((uint32_t)n), dim3(kTB), 0, ctx->stream, corpus->words, io.sig_vals,
                       io.sig_off, cnt, nullptr, nullptr);
    rc = scan_counts(ctx, cnt, diff_off, n, 0);
    if (rc) return rc;
    hipLaunchKernelGGL(k_tin_diff<true>, dim3((uint32_t)n), dim3(kTB), 0, ctx->stream, corpus->words, io.sig_vals,
                       io.sig_off, nullptr, diff_off, diff);
  }
  SG_HIP(hipGetLastError());
  std::vector<uint64_t> hoff(n + 1), hlen(n, 0);
  std::vector<uint32_t> hstate(n);
  SG_HIP(hipMemcpyAsync(hoff.data(), diff_off, (n + 1) * 8, hipMemcpyDeviceToHost, ctx->stream));
  SG_HIP(hipStreamSynchronize(ctx->stream));  // the wait sg_triage_newsig has: Canonicalize is planned on the host
  if (hoff[n]) {
    rc = canonicalize_dev(ctx, diff, hoff.data(), n, hlen.data());  // (waits for the lengths)
    if (rc) return rc;
  }
  for (uint64_t k = 0; k < n; k++) hstate[k] = hlen[k] ? 0u : st_make(1, SG_TIN_NO_NEW, 0, 0);  // :529-531
  SG_HIP(hipMemcpyAsync(cur_len, hlen.data(), n * 8, hipMemcpyHostToDevice, ctx->stream));
  SG_HIP(hipMemcpyAsync(state, hstate.data(), n * 4, hipMemcpyHostToDevice, ctx->stream));
  SG_HIP(hipStreamSynchronize(ctx->stream));  // (the host vectors are read by the queued copies; the stream is idle)
  // 4. the runs
  {
    ScopedTimer tm(ctx, "triage_runs_round");
    RoundArgs ra{0, io.nruns, io.minimized, selcall, xsig_off, xsig, diff, diff_off, cur_len, state};
    for (uint32_t i = 0; i < io.nruns; i++) {
      ra.run = i;
      hipLaunchKernelGGL(k_tr_round, dim3((uint32_t)n), dim3(kTB), 0, ctx->stream, ra);
    }
  }
  // 5. status, lengths, inputCover
  {
    ScopedTimer tm(ctx, "triage_runs_cover");
    CoverArgs ca{io.nruns, ncalls,      npcs,   io.minimized, selcall, io.prog_off, io.call_off, xcov_off, xcov, state,
                 cur_len,  io.status,   newlen, covlen,       covsrc,  {buf0, buf1},
                 wide,     ctx->dev.p->tr_route};
    hipLaunchKernelGGL(k_tr_cover, dim3((uint32_t)n), dim3(kTB), 0, ctx->stream, ca);
  }
  SG_HIP(hipGetLastError());
  // 6. offsets and payloads
  rc = scan_counts(ctx, newlen, io.new_off, n, 0);
  if (rc) return rc;
  rc = scan_counts(ctx, covlen, io.cov_off, n, 0);
  if (rc) return rc;
  PackArgs pa{n,          ncalls,      npcs,         io.nruns, io.prog_off, io.call_off, diff, diff_off,
              io.new_off, io.new_vals, io.new_cap,   covsrc,   {buf0, buf1},
              io.cov_off, io.cov_vals, io.cov_cap};
  hipLaunchKernelGGL(k_tr_pack, dim3(div_up(n, 4)), b, 0, ctx->stream, pa);
  SG_HIP(hipGetLastError());
  return SG_OK;
}

}  // namespace
}  // namespace sg

using namespace sg;

extern "C" {

int sg_triage_runs_from_kcov_dev(sg_ctx* ctx, sg_set* corpus, const uint32_t* d_sig_vals, const uint64_t* d_sig_off,
                                 uint64_t n, uint64_t nsig, const uint32_t* d_call, const uint8_t* d_minimized,
                                 uint32_t nruns, const uint64_t* d_pcs, const uint64_t* d_call_off,
                                 const uint64_t* d_prog_off, uint64_t ncalls, uint64_t npcs, int32_t* d_status,
                                 uint64_t* d_new_off, uint32_t* d_new_vals, uint64_t new_cap, uint64_t* d_cov_off,
                                 uint32_t* d_cov_vals, uint64_t cov_cap) {
  if (!ctx || !corpus || corpus->ctx != ctx || !d_sig_off || !d_prog_off || !d_call_off || !d_new_off || !d_cov_off ||
      (n && (!d_call || !d_minimized || !d_status)) || (nsig && !d_sig_vals) || (npcs && !d_pcs) ||
      (new_cap && !d_new_vals) || (cov_cap && !d_cov_vals)) {
    set_error("sg_triage_runs_from_kcov_dev: invalid argument");
    return SG_EINVAL;
  }
  int rc = tr_limits(n, nruns, ncalls, npcs, nsig);
  if (rc) return rc;
  std::lock_guard<std::mutex> g(ctx->mu);
  rc = ensure_device(ctx);
  if (rc) return rc;
  if (n == 0) {
    SG_HIP(hipMemsetAsync(d_new_off, 0, 8, ctx->stream));
    SG_HIP(hipMemsetAsync(d_cov_off, 0, 8, ctx->stream));
    return SG_OK;
  }
  WsPlan plan;
  const TrPlan p(plan, n, n * nruns, ncalls, npcs, nsig);
  rc = dstage_reserve(ctx, plan);
  if (rc) return rc;
  const TrIo io{d_sig_vals, d_sig_off, n,        nsig,       d_call,  d_minimized, nruns,      d_pcs,     d_call_off, d_prog_off,
                ncalls,     npcs,      d_status, d_new_off,  d_new_vals, new_cap,  d_cov_off,  d_cov_vals, cov_cap};
  return triage_runs(ctx, corpus, io, p);
}

int sg_triage_runs_from_kcov(sg_ctx* ctx, sg_set* corpus, const uint32_t* sig_vals, const uint64_t* sig_off, size_t n,
                             const uint32_t* call, const uint8_t* minimized, uint32_t nruns, const uint64_t* pcs,
                             const uint64_t* call_off, const uint64_t* prog_off, int32_t* status, uint64_t* new_off,
                             uint32_t* new_vals, size_t new_cap, uint64_t* cov_off, uint32_t* cov_vals,
                             size_t cov_cap) {
  if (!ctx || !corpus || corpus->ctx != ctx || !sig_off || !prog_off || !call_off || !new_off || !cov_off ||
      (n && (!call || !minimized || !status)) || (new_cap && !new_vals) || (cov_cap && !cov_vals) || nruns < 1 ||
      nruns > kTrMaxRuns || n >= (1ull << 28)) {
    set_error("sg_triage_runs_from_kcov: invalid argument");
    return SG_EINVAL;
  }
  const uint64_t nexec = (uint64_t)n * nruns;
  if (!offsets_ok(sig_off, n) || !offsets_ok(prog_off, nexec)) return SG_EINVAL;
  const uint64_t nsig = sig_off[n], ncalls = prog_off[nexec];
  int rc = tr_limits(n, nruns, ncalls, 0, nsig);
  if (rc) return rc;
  if (!offsets_ok(call_off, ncalls)) return SG_EINVAL;
  const uint64_t npcs = call_off[ncalls];
  if ((nsig && !sig_vals) || (npcs && !pcs)) return SG_EINVAL;
  rc = tr_limits(n, nruns, ncalls, npcs, nsig);
  if (rc) return rc;
  if (n == 0) {
    new_off[0] = cov_off[0] = 0;
    return SG_OK;
  }
  // nsig and npcs values always suffice: a smaller cap is staged as it is
  const uint64_t ncap = new_cap < nsig ? new_cap : nsig, ccap = cov_cap < npcs ? cov_cap : npcs;
  WsPlan plan;
  const size_t o_sv = plan.add(nsig * 4 + 4), o_so = plan.add((n + 1) * 8), o_no = plan.add((n + 1) * 8),
               o_vo = plan.add((n + 1) * 8), o_call = plan.add(n * 4), o_min = plan.add(n),
               o_po = plan.add((nexec + 1) * 8), o_co = plan.add((ncalls + 1) * 8), o_pcs = plan.add(npcs * 8 + 8),
               o_st = plan.add(n * 4), o_nv = plan.add(ncap * 4 + 4), o_cv = plan.add(ccap * 4 + 4);
  const TrPlan p(plan, n, nexec, ncalls, npcs, nsig);
  std::lock_guard<std::mutex> g(ctx->mu);
  rc = ensure_device(ctx);
  if (rc) return rc;
  rc = dstage_reserve(ctx, plan);
  if (rc) return rc;
  uint32_t* dsv = dstage_at<uint32_t>(ctx, o_sv);
  uint64_t* dso = dstage_at<uint64_t>(ctx, o_so);
  uint64_t* dno = dstage_at<uint64_t>(ctx, o_no);
  uint64_t* dvo = dstage_at<uint64_t>(ctx, o_vo);
  uint32_t* dcall = dstage_at<uint32_t>(ctx, o_call);
  uint8_t* dmin = dstage_at<uint8_t>(ctx, o_min);
  uint64_t* dpo = dstage_at<uint64_t>(ctx, o_po);
  uint64_t* dco = dstage_at<uint64_t>(ctx, o_co);
  uint64_t* dpcs = dstage_at<uint64_t>(ctx, o_pcs);
  int32_t* dst = dstage_at<int32_t>(ctx, o_st);
  uint32_t* dnv = dstage_at<uint32_t>(ctx, o_nv);
  uint32_t* dcv = dstage_at<uint32_t>(ctx, o_cv);
  if ((rc = upload(ctx, dsv, sig_vals, nsig * 4))) return rc;
  if ((rc = upload(ctx, dso, sig_off, (n + 1) * 8))) return rc;
  if ((rc = upload(ctx, dcall, call, n * 4))) return rc;
  if ((rc = upload(ctx, dmin, minimized, n))) return rc;
  if ((rc = upload(ctx, dpo, prog_off, (nexec + 1) * 8))) return rc;
  if ((rc = upload(ctx, dco, call_off, (ncalls + 1) * 8))) return rc;
  if ((rc = upload(ctx, dpcs, pcs, npcs * 8))) return rc;
  const TrIo io{dsv,    dso,  n,   nsig, dcall, dmin, nruns, dpcs, dco, dpo,
                ncalls, npcs, dst, dno,  ncap ? dnv : nullptr, ncap, dvo, ccap ? dcv : nullptr, ccap};
  rc = triage_runs(ctx, corpus, io, p);
  if (rc) return rc;
  SG_HIP(hipMemcpyAsync(status, dst, n * 4, hipMemcpyDeviceToHost, ctx->stream));
  SG_HIP(hipMemcpyAsync(new_off, dno, (n + 1) * 8, hipMemcpyDeviceToHost, ctx->stream));
  SG_HIP(hipMemcpyAsync(cov_off, dvo, (n + 1) * 8, hipMemcpyDeviceToHost, ctx->stream));
  SG_HIP(hipStreamSynchronize(ctx->stream));
  if (new_off[n] && new_off[n] <= new_cap)
    SG_HIP(hipMemcpyAsync(new_vals, dnv, new_off[n] * 4, hipMemcpyDeviceToHost, ctx->stream));
  if (cov_off[n] && cov_off[n] <= cov_cap)
    SG_HIP(hipMemcpyAsync(cov_vals, dcv, cov_off[n] * 4, hipMemcpyDeviceToHost, ctx->stream));
  SG_HIP(hipStreamSynchronize(ctx->stream));
  return SG_OK;
}

}  // extern "C"
