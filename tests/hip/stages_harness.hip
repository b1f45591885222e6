// stages_harness.hip -- test-only entry points over the stages every feature of
// libsyzsig.so is built from: scan_counts, radix_sort_u64, radix_pass_runs, the
// distinct-and-rank stages, the device helpers of sg_internal.h and the line
// walk of sg_linewalk.h (tests/test_stages.py).  Built as syzkaller_amd/libsgstages_test.so and
// linked against libsyzsig.so: the sg:: functions called here are that
// library's own, the sgd:: helpers are the header's.  Nothing here is part of
// the product ABI.
//
// Every sgt_* call takes the context's lock, ensures the device, reserves the
// workspace, uploads its inputs, runs one stage on ctx->stream, waits and
// downloads.  It returns an SG_* code, and through `broken` a mask of the
// guards found damaged: every buffer handed to the stage is an allocation of
// its own between two kGuard-byte guards of kGuardByte, and the stage's
// workspace [ws_used + kGuard, ws_used + kGuard + bound) sits between two such
// guards inside the context's workspace.  Bit 0 is the workspace's lower guard,
// bit 1 its upper one, bits 2.. the buffers' in the order each call states.
#include "csrc/sg_internal.h"
#include "csrc/sg_linewalk.h"
#include "csrc/sg_rank.h"

#include <algorithm>
#include <cstring>
#include <vector>

namespace {

using namespace sg;

constexpr size_t kGuard = 4096;
constexpr int kGuardByte = 0xA5;
constexpr int kFillByte = 0xEE;  // what a payload holds before anything is written to it

int region_intact(sg_ctx* ctx, const char* d, bool* ok) {
  unsigned char h[kGuard];
  SG_HIP(hipMemcpyAsync(h, d, kGuard, hipMemcpyDeviceToHost, ctx->stream));
  SG_HIP(hipStreamSynchronize(ctx->stream));
  *ok = true;
  for (size_t i = 0; i < kGuard; i++)
    if (h[i] != kGuardByte) *ok = false;
  return SG_OK;
}

// A device block of `bytes` between two guards.
struct Guarded {
  char* base = nullptr;
  size_t bytes = 0;
  Guarded() = default;
  Guarded(const Guarded&) = delete;
  Guarded& operator=(const Guarded&) = delete;
  ~Guarded() {
    if (base) (void)hipFree(base);
  }
  int alloc(sg_ctx* ctx, size_t b, const void* h_init = nullptr) {
    bytes = b;
    SG_HIP(hipMalloc((void**)&base, b + 2 * kGuard));
    SG_HIP(hipMemsetAsync(base, kGuardByte, kGuard, ctx->stream));
    SG_HIP(hipMemsetAsync(base + kGuard + b, kGuardByte, kGuard, ctx->stream));
    if (b && h_init) return upload(ctx, base + kGuard, h_init, b);
    if (b) SG_HIP(hipMemsetAsync(base + kGuard, kFillByte, b, ctx->stream));
    return SG_OK;
  }
  template <typename T>
  T* p() const {
    return (T*)(base + kGuard);
  }
  int download(sg_ctx* ctx, void* h) const {
    if (bytes && h) SG_HIP(hipMemcpyAsync(h, base + kGuard, bytes, hipMemcpyDeviceToHost, ctx->stream));
    SG_HIP(hipStreamSynchronize(ctx->stream));
    return SG_OK;
  }
  // sets `bit` (lower guard) and `bit + 1` (upper guard) of *broken
  int check(sg_ctx* ctx, int bit, uint32_t* broken) const {
    bool lo = true, hi = true;
    int rc = region_intact(ctx, base, &lo);
    if (!rc) rc = region_intact(ctx, base + kGuard + bytes, &hi);
    if (!lo) *broken |= 1u << bit;
    if (!hi) *broken |= 2u << bit;
    return rc;
  }
};

// The stage's share of the context's workspace: `bound` bytes at at(), a guard
// on either side.
struct WsGuard {
  sg_ctx* ctx;
  size_t ws_used, bound;
  size_t at() const { return ws_used + kGuard; }
  int reserve(sg_ctx* c, size_t used, size_t b) {
    ctx = c;
    ws_used = used;
    bound = b;
    if (used % 256) {
      set_error("stages harness: ws_used is not a multiple of 256");
      return SG_EINVAL;
    }
    const int rc = ws_reserve(c, used + b + 2 * kGuard);
    if (rc) return rc;
    SG_HIP(hipMemsetAsync(ws_at(c, used), kGuardByte, kGuard, c->stream));
    SG_HIP(hipMemsetAsync(ws_at(c, used + kGuard + b), kGuardByte, kGuard, c->stream));
    if (b) SG_HIP(hipMemsetAsync(ws_at(c, used + kGuard), kFillByte, b, c->stream));
    return SG_OK;
  }
  int check(uint32_t* broken) const {
    bool lo = true, hi = true;
    int rc = region_intact(ctx, (const char*)ws_at(ctx, ws_used), &lo);
    if (!rc) rc = region_intact(ctx, (const char*)ws_at(ctx, ws_used + kGuard + bound), &hi);
    if (!lo) *broken |= 1u;
    if (!hi) *broken |= 2u;
    return rc;
  }
};

#define SGT_RC(call)        \
  do {                      \
    const int rc_ = (call); \
    if (rc_) return rc_;    \
  } while (0)

int sync_check(sg_ctx* ctx) {
  SG_HIP(hipGetLastError());
  SG_HIP(hipStreamSynchronize(ctx->stream));
  return SG_OK;
}

// ---- kernels over the device helpers ------------------------------------------
__global__ void k_t_bounds(const uint64_t* a, uint64_t n, const uint64_t* probe, uint64_t np, uint64_t* lb,
                           uint64_t* ub) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= np) return;
  lb[i] = sgd::lb64(a, n, probe[i]);
  ub[i] = sgd::ub64(a, n, probe[i]);
}

constexpr uint32_t kSegLds = 1024;  // offsets the LDS form holds
// query q = {lo, hi, i}; one workgroup, the queries strided over it
__global__ __launch_bounds__(256) void k_t_seg(const uint64_t* off, uint32_t noff, const uint64_t* q, uint64_t nq,
                                               uint64_t* out_global, uint64_t* out_lds) {
  __shared__ uint64_t s_off[kSegLds];
  for (uint32_t i = threadIdx.x; i < noff && i < kSegLds; i += blockDim.x) s_off[i] = off[i];
  __syncthreads();
  for (uint64_t k = threadIdx.x; k < nq; k += blockDim.x) {
    out_global[k] = sgd::seg_search(off, q[3 * k], q[3 * k + 1], q[3 * k + 2]);
    out_lds[k] = sgd::seg_search((const uint64_t*)s_off, q[3 * k], q[3 * k + 1], q[3 * k + 2]);
  }
}

// a full wave per row of 64 values
__global__ __launch_bounds__(64) void k_t_wave_add(const uint32_t* in, uint32_t* out) {
  const uint64_t i = (uint64_t)blockIdx.x * 64 + threadIdx.x;
  out[i] = sgd::wave_incl_add(in[i]);
}
__global__ __launch_bounds__(64) void k_t_wave_max(const int* in, int* out) {
  const uint64_t i = (uint64_t)blockIdx.x * 64 + threadIdx.x;
  out[i] = sgd::wave_incl_max(in[i]);
}

// sgd::walk_lines and sgd::LineGroup as the text scans use them: four waves a workgroup, a wave on a share of
// consecutive tiles of 1 << tile_log bytes over the segments of a CSR, the classes the first kClasses (0, 1 or 2)
// of the bytes cls[0] and cls[1].
// A tile's lines go through the store group into its per_tile records of {s, e, met, first0, first1} (met: bit k
// says class k was met; the first of a class not met is written as 0), their number into cnt.
struct WalkArgs {
  const uint8_t* text;
  uint64_t nbytes;
  const uint64_t* off;       // [nseg + 1]
  const uint64_t* tile_off;  // [nseg + 1]
  uint64_t nseg, ntiles, max_line;
  uint32_t tile_log, nwaves, per_tile;
  uint32_t cls[2];
  uint32_t* cnt;  // [ntiles]
  uint64_t* rec;  // [ntiles * per_tile * 5]
};
struct WalkRec {
  uint64_t s, e, met, first[2];
};
template <uint32_t kClasses>
__global__ __launch_bounds__(256) void k_t_walk(WalkArgs a) {
  const uint32_t lane = threadIdx.x & 63;
  const uint64_t wave = (uint64_t)blockIdx.x * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const uint64_t per = (a.ntiles + a.nwaves - 1) / a.nwaves;
  const uint64_t gend = min(a.ntiles, (wave + 1) * per);
  for (uint64_t g = wave * per; g < gend; g++) {
    const uint64_t p = sgd::seg_search(a.tile_off, (uint64_t)0, a.nseg - 1, g);
    uint64_t a0, a1;
    sgd::csr_range(a.off, p, a.nbytes, a0, a1);
    const uint64_t t = g - a.tile_off[p];
    const uint64_t tb = a0 + (t << a.tile_log);
    if (tb >= a1 || t > (a.nbytes >> a.tile_log)) {  // (never for a tile count made from the same offsets)
      if (lane == 0) a.cnt[g] = 0;
      continue;
    }
    const uint64_t te = min(a1, tb + (1ull << a.tile_log));
    sgd::LineGroup<WalkRec> lines;
    auto store = [&](uint32_t i0, const WalkRec& r) {
      const uint32_t i = i0 + lane;
      if (i >= a.per_tile) return;
      uint64_t* o = a.rec + (g * a.per_tile + i) * 5;
      o[0] = r.s;
      o[1] = r.e;
      o[2] = r.met;
      o[3] = r.first[0];
      o[4] = r.first[1];
    };
    sgd::walk_lines<kClasses>(
        a.text, a0, a1, tb, te, a.max_line, lane,
        [&](uint32_t c, uint64_t* m) {
#pragma unroll
          for (uint32_t k = 0; k < kClasses; k++) m[k] = __ballot(c == a.cls[k]);
        },
        [&](uint64_t s, uint64_t e, const bool* have, const uint64_t* first) {
          WalkRec r{s, e, 0, {0, 0}};
#pragma unroll
          for (uint32_t k = 0; k < kClasses; k++)
            if (have[k]) {
              r.met |= 1ull << k;
              r.first[k] = first[k];
            }
          lines.add(lane, r, store);
        });
    lines.flush(lane, store);
    if (lane == 0) a.cnt[g] = lines.n;
  }
}

// The RankWs of ng values behind the workspace's lower guard: rank_ws's regions, then the sort's and the scan's
// share, rank_ws_bytes(ng) in all.
int rank_setup(sg_ctx* ctx, uint64_t ng, uint64_t ws_used, WsGuard* ws, RankWs* g) {
  SGT_RC(ws->reserve(ctx, ws_used, rank_ws_bytes(ng)));
  WsPlan p;
  p.add(ws->at());
  *g = rank_ws(ctx, p, ng);
  return SG_OK;
}

struct Locked {
  std::lock_guard<std::mutex> g;
  explicit Locked(sg_ctx* ctx) : g(ctx->mu) {}
};

}  // namespace

extern "C" {

// The *_ws bounds, for the tests' own arithmetic.
uint64_t sgt_scan_ws_bytes(uint64_t n) { return scan_ws_bytes(n); }
uint64_t sgt_radix_sort_ws(uint64_t n) { return radix_sort_ws(n); }
uint64_t sgt_radix_pass_runs_ws(uint64_t n, uint64_t nruns) { return radix_pass_runs_ws(n, nruns); }
uint64_t sgt_rank_ws_bytes(uint64_t ng) { return rank_ws_bytes(ng); }
uint64_t sgt_bits_below(uint64_t n) { return bits_below(n); }

// scan_counts of in [n] into out [n + 1].  Guards: workspace, in, out.
int sgt_scan_counts(sg_ctx* ctx, const uint32_t* in, uint64_t n, uint64_t ws_used, uint64_t* out, uint32_t* broken) {
  if (!ctx || !out || !broken) return SG_EINVAL;
  Locked l(ctx);
  *broken = 0;
  SGT_RC(ensure_device(ctx));
  WsGuard ws;
  SGT_RC(ws.reserve(ctx, ws_used, scan_ws_bytes(n)));
  Guarded din, dout;
  SGT_RC(din.alloc(ctx, n * 4, in));
  SGT_RC(dout.alloc(ctx, (n + 1) * 8));
  SGT_RC(scan_counts(ctx, din.p<uint32_t>(), dout.p<uint64_t>(), n, ws.at()));
  SGT_RC(sync_check(ctx));
  SGT_RC(dout.download(ctx, out));
  SGT_RC(ws.check(broken));
  SGT_RC(din.check(ctx, 2, broken));
  return dout.check(ctx, 4, broken);
}

// radix_sort_u64 of keys [n].  out [n]: the result; which: 0 when *sorted is a, 1 when it is b, -1 otherwise;
// a_after [n]: what a holds afterwards.  Guards: workspace, a, b.
int sgt_radix_sort(sg_ctx* ctx, const uint64_t* keys, uint64_t n, uint64_t vary, uint64_t ws_used, uint64_t* out,
                   int* which, uint64_t* a_after, uint32_t* broken) {
  if (!ctx || !which || !broken) return SG_EINVAL;
  Locked l(ctx);
  *broken = 0;
  *which = -1;
  SGT_RC(ensure_device(ctx));
  WsGuard ws;
  SGT_RC(ws.reserve(ctx, ws_used, radix_sort_ws(n)));
  Guarded a, b;
  SGT_RC(a.alloc(ctx, n * 8, keys));
  SGT_RC(b.alloc(ctx, n * 8));
  uint64_t* sorted = nullptr;
  SGT_RC(radix_sort_u64(ctx, a.p<uint64_t>(), b.p<uint64_t>(), n, ws.at(), &sorted, vary));
  SGT_RC(sync_check(ctx));
  *which = sorted == a.p<uint64_t>() ? 0 : sorted == b.p<uint64_t>() ? 1 : -1;
  if (*which >= 0) SGT_RC((*which ? b : a).download(ctx, out));
  SGT_RC(a.download(ctx, a_after));
  SGT_RC(ws.check(broken));
  SGT_RC(a.check(ctx, 2, broken));
  return b.check(ctx, 4, broken);
}

// radix_pass_runs over the runs (run_start, run_cnt) [nruns] of src [src_len] into dst [n], n the runs' keys.
// Guards: workspace, src, dst.
int sgt_radix_pass_runs(sg_ctx* ctx, const uint64_t* src, uint64_t src_len, const uint64_t* run_start,
                        const uint64_t* run_cnt, uint64_t nruns, uint32_t shift, uint64_t ws_used, uint64_t* dst,
                        uint32_t* broken) {
  if (!ctx || !broken) return SG_EINVAL;
  Locked l(ctx);
  *broken = 0;
  SGT_RC(ensure_device(ctx));
  std::vector<uint64_t> rs(run_start, run_start + nruns), rc(run_cnt, run_cnt + nruns);
  uint64_t n = 0;
  for (uint64_t i = 0; i < nruns; i++) {
    if (rs[i] > src_len || rc[i] > src_len - rs[i]) return SG_EINVAL;  // (the harness's own bounds check)
    n += rc[i];
  }
  WsGuard ws;
  SGT_RC(ws.reserve(ctx, ws_used, radix_pass_runs_ws(n, nruns)));
  Guarded dsrc, ddst;
  SGT_RC(dsrc.alloc(ctx, src_len * 8, src));
  SGT_RC(ddst.alloc(ctx, n * 8));
  SGT_RC(radix_pass_runs(ctx, dsrc.p<uint64_t>(), rs, rc, shift, ddst.p<uint64_t>(), ws.at()));
  SGT_RC(sync_check(ctx));
  SGT_RC(ddst.download(ctx, dst));
  SGT_RC(ws.check(broken));
  SGT_RC(dsrc.check(ctx, 2, broken));
  return ddst.check(ctx, 4, broken);
}

// rank_runs of sorted [n] (n >= 1): flags [n], pos [n + 1], and with want_u the distinct keys u [n] (the places
// past pos[n] keep kFillByte).  Guards: workspace, sorted, flags, pos, u.
int sgt_rank_runs(sg_ctx* ctx, const uint64_t* sorted, uint64_t n, int want_u, uint64_t ws_used, uint32_t* flags,
                  uint64_t* pos, uint64_t* u, uint32_t* broken) {
  if (!ctx || !broken || !n) return SG_EINVAL;
  Locked l(ctx);
  *broken = 0;
  SGT_RC(ensure_device(ctx));
  WsGuard ws;
  SGT_RC(ws.reserve(ctx, ws_used, scan_ws_bytes(n)));
  Guarded ds, df, dp, du;
  SGT_RC(ds.alloc(ctx, n * 8, sorted));
  SGT_RC(df.alloc(ctx, n * 4));
  SGT_RC(dp.alloc(ctx, (n + 1) * 8));
  SGT_RC(du.alloc(ctx, n * 8));
  SGT_RC(rank_runs(ctx, ds.p<uint64_t>(), n, df.p<uint32_t>(), dp.p<uint64_t>(), want_u ? du.p<uint64_t>() : nullptr,
                   ws.at()));
  SGT_RC(sync_check(ctx));
  SGT_RC(df.download(ctx, flags));
  SGT_RC(dp.download(ctx, pos));
  SGT_RC(du.download(ctx, u));
  SGT_RC(ws.check(broken));
  SGT_RC(ds.check(ctx, 2, broken));
  SGT_RC(df.check(ctx, 4, broken));
  SGT_RC(dp.check(ctx, 6, broken));
  return du.check(ctx, 8, broken);
}

// rank_pack of hi, lo [ng]: what g.v and g.ka hold afterwards.  Guards: workspace, hi, lo.
int sgt_rank_pack(sg_ctx* ctx, const uint32_t* hi, const uint32_t* lo, uint64_t ng, uint64_t ws_used, uint64_t* v,
                  uint64_t* ka, uint32_t* broken) {
  if (!ctx || !broken || !ng) return SG_EINVAL;
  Locked l(ctx);
  *broken = 0;
  SGT_RC(ensure_device(ctx));
  WsGuard ws;
  RankWs g;
  SGT_RC(rank_setup(ctx, ng, ws_used, &ws, &g));
  Guarded dh, dl;
  SGT_RC(dh.alloc(ctx, ng * 4, hi));
  SGT_RC(dl.alloc(ctx, ng * 4, lo));
  SGT_RC(rank_pack(ctx, g, dh.p<uint32_t>(), dl.p<uint32_t>()));
  SGT_RC(sync_check(ctx));
  SG_HIP(hipMemcpyAsync(v, g.v, ng * 8, hipMemcpyDeviceToHost, ctx->stream));
  SG_HIP(hipMemcpyAsync(ka, g.ka, ng * 8, hipMemcpyDeviceToHost, ctx->stream));
  SG_HIP(hipStreamSynchronize(ctx->stream));
  SGT_RC(ws.check(broken));
  SGT_RC(dh.check(ctx, 2, broken));
  return dl.check(ctx, 4, broken);
}

// rank_values of v [ng] (uploaded to g.v and g.ka): u [ng] (the places past *nu keep kFillByte), *nu = g.pos[ng],
// rank [ng].  Guards: workspace, u, rank.
int sgt_rank_values(sg_ctx* ctx, const uint64_t* v, uint64_t ng, uint64_t vary, uint64_t ws_used, uint64_t* u,
                    uint64_t* nu, uint32_t* rank, uint32_t* broken) {
  if (!ctx || !broken || !ng || !nu) return SG_EINVAL;
  Locked l(ctx);
  *broken = 0;
  SGT_RC(ensure_device(ctx));
  WsGuard ws;
  RankWs g;
  SGT_RC(rank_setup(ctx, ng, ws_used, &ws, &g));
  SGT_RC(upload(ctx, g.v, v, ng * 8));
  SGT_RC(upload(ctx, g.ka, v, ng * 8));
  Guarded du, dr;
  SGT_RC(du.alloc(ctx, ng * 8));
  SGT_RC(dr.alloc(ctx, ng * 4));
  SGT_RC(rank_values(ctx, g, vary, du.p<uint64_t>(), dr.p<uint32_t>()));
  SGT_RC(sync_check(ctx));
  SG_HIP(hipMemcpyAsync(nu, g.pos + ng, 8, hipMemcpyDeviceToHost, ctx->stream));
  SGT_RC(du.download(ctx, u));
  SGT_RC(dr.download(ctx, rank));
  SGT_RC(ws.check(broken));
  SGT_RC(du.check(ctx, 2, broken));
  return dr.check(ctx, 4, broken);
}

// rank_flag_all over off [ngroups + 1] (ngroups >= 1), sel [ngroups] or null; flag and gbase start as zeroes, as
// the callers' first pass leaves them, and scal as {0, 0}.  Guards: off, sel (when given), flag, gbase, scal.
int sgt_rank_flag_all(sg_ctx* ctx, const uint64_t* off, uint64_t ngroups, uint64_t total, const uint8_t* sel,
                      uint8_t* flag, uint64_t* gbase, uint64_t* scal, uint32_t* broken) {
  if (!ctx || !broken || !ngroups) return SG_EINVAL;
  Locked l(ctx);
  *broken = 0;
  SGT_RC(ensure_device(ctx));
  std::vector<uint64_t> zero(ngroups + 2, 0);
  Guarded doff, dsel, dflag, dbase, dscal;
  SGT_RC(doff.alloc(ctx, (ngroups + 1) * 8, off));
  if (sel) SGT_RC(dsel.alloc(ctx, ngroups, sel));
  SGT_RC(dflag.alloc(ctx, ngroups, zero.data()));
  SGT_RC(dbase.alloc(ctx, ngroups * 8, zero.data()));
  SGT_RC(dscal.alloc(ctx, 16, zero.data()));
  SGT_RC(rank_flag_all(ctx, doff.p<uint64_t>(), ngroups, total, sel ? dsel.p<uint8_t>() : nullptr, dflag.p<uint8_t>(),
                       dbase.p<uint64_t>(), dscal.p<unsigned long long>()));
  SGT_RC(sync_check(ctx));
  SGT_RC(dflag.download(ctx, flag));
  SGT_RC(dbase.download(ctx, gbase));
  SGT_RC(dscal.download(ctx, scal));
  SGT_RC(doff.check(ctx, 2, broken));
  if (sel) SGT_RC(dsel.check(ctx, 4, broken));
  SGT_RC(dflag.check(ctx, 6, broken));
  SGT_RC(dbase.check(ctx, 8, broken));
  return dscal.check(ctx, 10, broken);
}

// rank_fill of ng places (ng >= 1) from flag, gbase [ngroups].  Guards: off, flag, gbase, gidx, ggroup.
int sgt_rank_fill(sg_ctx* ctx, const uint64_t* off, uint64_t ngroups, uint64_t total, const uint8_t* flag,
                  const uint64_t* gbase, uint64_t ng, uint32_t* gidx, uint32_t* ggroup, uint32_t* broken) {
  if (!ctx || !broken || !ngroups || !ng) return SG_EINVAL;
  Locked l(ctx);
  *broken = 0;
  SGT_RC(ensure_device(ctx));
  Guarded doff, dflag, dbase, didx, dgrp;
  SGT_RC(doff.alloc(ctx, (ngroups + 1) * 8, off));
  SGT_RC(dflag.alloc(ctx, ngroups, flag));
  SGT_RC(dbase.alloc(ctx, ngroups * 8, gbase));
  SGT_RC(didx.alloc(ctx, ng * 4));
  SGT_RC(dgrp.alloc(ctx, ng * 4));
  SGT_RC(rank_fill(ctx, doff.p<uint64_t>(), ngroups, total, dflag.p<uint8_t>(), dbase.p<uint64_t>(), ng,
                   didx.p<uint32_t>(), dgrp.p<uint32_t>()));
  SGT_RC(sync_check(ctx));
  SGT_RC(didx.download(ctx, gidx));
  SGT_RC(dgrp.download(ctx, ggroup));
  SGT_RC(doff.check(ctx, 2, broken));
  SGT_RC(dflag.check(ctx, 4, broken));
  SGT_RC(dbase.check(ctx, 6, broken));
  SGT_RC(didx.check(ctx, 8, broken));
  return dgrp.check(ctx, 10, broken);
}

// rank_group_first of ggroup, rank [ng] (ng >= 1) over ngroups groups (>= 1): first [ngroups], the sorted keys
// [ng], g.flags [ng] and g.pos [ng + 1].  Guards: workspace, ggroup, rank, first.
int sgt_rank_group_first(sg_ctx* ctx, const uint32_t* ggroup, const uint32_t* rank, uint64_t ng, uint64_t ngroups,
                         uint64_t ws_used, uint64_t* first, uint64_t* sorted_out, uint32_t* flags, uint64_t* pos,
                         uint32_t* broken) {
  if (!ctx || !broken || !ng || !ngroups) return SG_EINVAL;
  Locked l(ctx);
  *broken = 0;
  SGT_RC(ensure_device(ctx));
  WsGuard ws;
  RankWs g;
  SGT_RC(rank_setup(ctx, ng, ws_used, &ws, &g));
  Guarded dg, dr, df;
  SGT_RC(dg.alloc(ctx, ng * 4, ggroup));
  SGT_RC(dr.alloc(ctx, ng * 4, rank));
  SGT_RC(df.alloc(ctx, ngroups * 8));
  uint64_t* sorted = nullptr;
  SGT_RC(rank_group_first(ctx, g, dg.p<uint32_t>(), dr.p<uint32_t>(), ngroups, df.p<uint64_t>(), &sorted));
  SGT_RC(sync_check(ctx));
  if (sorted != g.ka && sorted != g.kb) {
    set_error("stages harness: rank_group_first's sorted keys are in neither key buffer");
    return SG_EINVAL;
  }
  SG_HIP(hipMemcpyAsync(sorted_out, sorted, ng * 8, hipMemcpyDeviceToHost, ctx->stream));
  SG_HIP(hipMemcpyAsync(flags, g.flags, ng * 4, hipMemcpyDeviceToHost, ctx->stream));
  SG_HIP(hipMemcpyAsync(pos, g.pos, (ng + 1) * 8, hipMemcpyDeviceToHost, ctx->stream));
  SGT_RC(df.download(ctx, first));
  SGT_RC(ws.check(broken));
  SGT_RC(dg.check(ctx, 2, broken));
  SGT_RC(dr.check(ctx, 4, broken));
  return df.check(ctx, 6, broken);
}

// lb64 and ub64 of every probe [np] (np >= 1) in a [n].  Guards: a, lb, ub.
int sgt_bounds(sg_ctx* ctx, const uint64_t* a, uint64_t n, const uint64_t* probe, uint64_t np, uint64_t* lb,
               uint64_t* ub, uint32_t* broken) {
  if (!ctx || !broken || !np) return SG_EINVAL;
  Locked l(ctx);
  *broken = 0;
  SGT_RC(ensure_device(ctx));
  Guarded da, dp, dl, du;
  SGT_RC(da.alloc(ctx, n * 8, a));
  SGT_RC(dp.alloc(ctx, np * 8, probe));
  SGT_RC(dl.alloc(ctx, np * 8));
  SGT_RC(du.alloc(ctx, np * 8));
  hipLaunchKernelGGL(k_t_bounds, dim3(div_up(np, 256)), dim3(256), 0, ctx->stream, da.p<uint64_t>(), n,
                     dp.p<uint64_t>(), np, dl.p<uint64_t>(), du.p<uint64_t>());
  SGT_RC(sync_check(ctx));
  SGT_RC(dl.download(ctx, lb));
  SGT_RC(du.download(ctx, ub));
  SGT_RC(da.check(ctx, 2, broken));
  SGT_RC(dl.check(ctx, 4, broken));
  return du.check(ctx, 6, broken);
}

// seg_search(off, lo, hi, i) of every query {lo, hi, i} of q [3 * nq] (nq >= 1, lo <= hi < noff <= 1024), through
// a global pointer and through an LDS copy of off.  Guards: off, out_global, out_lds.
int sgt_seg_search(sg_ctx* ctx, const uint64_t* off, uint32_t noff, const uint64_t* q, uint64_t nq,
                   uint64_t* out_global, uint64_t* out_lds, uint32_t* broken) {
  if (!ctx || !broken || !nq || !noff || noff > kSegLds) return SG_EINVAL;
  for (uint64_t k = 0; k < nq; k++)
    if (q[3 * k] > q[3 * k + 1] || q[3 * k + 1] >= noff) return SG_EINVAL;  // (the harness's own bounds check)
  Locked l(ctx);
  *broken = 0;
  SGT_RC(ensure_device(ctx));
  Guarded doff, dq, dg, dl;
  SGT_RC(doff.alloc(ctx, (size_t)noff * 8, off));
  SGT_RC(dq.alloc(ctx, nq * 24, q));
  SGT_RC(dg.alloc(ctx, nq * 8));
  SGT_RC(dl.alloc(ctx, nq * 8));
  hipLaunchKernelGGL(k_t_seg, dim3(1), dim3(256), 0, ctx->stream, doff.p<uint64_t>(), noff, dq.p<uint64_t>(), nq,
                     dg.p<uint64_t>(), dl.p<uint64_t>());
  SGT_RC(sync_check(ctx));
  SGT_RC(dg.download(ctx, out_global));
  SGT_RC(dl.download(ctx, out_lds));
  SGT_RC(doff.check(ctx, 2, broken));
  SGT_RC(dg.check(ctx, 4, broken));
  return dl.check(ctx, 6, broken);
}

// wave_incl_add / wave_incl_max of every row of 64 values of in [64 * rows] (rows >= 1), a full wave each.
// Guards: in, out.
int sgt_wave_add(sg_ctx* ctx, const uint32_t* in, uint64_t rows, uint32_t* out, uint32_t* broken) {
  if (!ctx || !broken || !rows) return SG_EINVAL;
  Locked l(ctx);
  *broken = 0;
  SGT_RC(ensure_device(ctx));
  Guarded di, dout;
  SGT_RC(di.alloc(ctx, rows * 256, in));
  SGT_RC(dout.alloc(ctx, rows * 256));
  hipLaunchKernelGGL(k_t_wave_add, dim3((uint32_t)rows), dim3(64), 0, ctx->stream, di.p<uint32_t>(), dout.p<uint32_t>());
  SGT_RC(sync_check(ctx));
  SGT_RC(dout.download(ctx, out));
  SGT_RC(di.check(ctx, 2, broken));
  return dout.check(ctx, 4, broken);
}
int sgt_wave_max(sg_ctx* ctx, const int32_t* in, uint64_t rows, int32_t* out, uint32_t* broken) {
  if (!ctx || !broken || !rows) return SG_EINVAL;
  Locked l(ctx);
  *broken = 0;
  SGT_RC(ensure_device(ctx));
  Guarded di, dout;
  SGT_RC(di.alloc(ctx, rows * 256, in));
  SGT_RC(dout.alloc(ctx, rows * 256));
  hipLaunchKernelGGL(k_t_wave_max, dim3((uint32_t)rows), dim3(64), 0, ctx->stream, di.p<int>(), dout.p<int>());
  SGT_RC(sync_check(ctx));
  SGT_RC(dout.download(ctx, out));
  SGT_RC(di.check(ctx, 2, broken));
  return dout.check(ctx, 4, broken);
}

// sgd::walk_lines over the segments off [nseg + 1] (nseg >= 1, clamped as csr_range clamps them) of text [nbytes],
// by nwaves waves (a multiple of 4) with the first nclasses (0, 1 or 2) of the class bytes: cnt [ntiles] the lines that start in each tile, rec [ntiles * per_tile * 5]
// their records, ntiles the segments' tiles of 1 << tile_log bytes (tile_log 6 .. 20) in segment order.
// Guards: text, off, tile_off, cnt, rec.
int sgt_walk_lines(sg_ctx* ctx, const uint8_t* text, uint64_t nbytes, const uint64_t* off, uint64_t nseg,
                   uint32_t tile_log, uint64_t max_line, uint32_t nclasses, uint32_t cls0, uint32_t cls1, uint32_t nwaves,
                   uint64_t ntiles, uint32_t per_tile, uint32_t* cnt, uint64_t* rec, uint32_t* broken) {
  if (!ctx || !broken || !off || !nseg || !ntiles || !per_tile || !nwaves || nwaves % 4 || tile_log < 6 || tile_log > 20 ||
      nclasses > 2)
    return SG_EINVAL;
  std::vector<uint64_t> tile_off(nseg + 1, 0);
  for (uint64_t p = 0; p < nseg; p++) {
    const uint64_t a0 = std::min(off[p], nbytes), a1 = std::min(std::max(off[p + 1], a0), nbytes);
    tile_off[p + 1] = tile_off[p] + ((a1 - a0 + ((1ull << tile_log) - 1)) >> tile_log);
  }
  if (tile_off[nseg] != ntiles) return SG_EINVAL;  // (the harness's own bounds check: cnt and rec hold ntiles)
  Locked l(ctx);
  *broken = 0;
  SGT_RC(ensure_device(ctx));
  Guarded dtext, doff, dtile, dcnt, drec;
  SGT_RC(dtext.alloc(ctx, nbytes, text));
  SGT_RC(doff.alloc(ctx, (nseg + 1) * 8, off));
  SGT_RC(dtile.alloc(ctx, (nseg + 1) * 8, tile_off.data()));
  SGT_RC(dcnt.alloc(ctx, ntiles * 4));
  SGT_RC(drec.alloc(ctx, ntiles * per_tile * 40));
  WalkArgs a{};
  a.text = dtext.p<uint8_t>();
  a.nbytes = nbytes;
  a.off = doff.p<uint64_t>();
  a.tile_off = dtile.p<uint64_t>();
  a.nseg = nseg;
  a.ntiles = ntiles;
  a.max_line = max_line;
  a.tile_log = tile_log;
  a.nwaves = nwaves;
  a.per_tile = per_tile;
  a.cls[0] = cls0;
  a.cls[1] = cls1;
  a.cnt = dcnt.p<uint32_t>();
  a.rec = drec.p<uint64_t>();
  const dim3 grid(nwaves / 4), block(256);
  if (nclasses == 0) hipLaunchKernelGGL(k_t_walk<0>, grid, block, 0, ctx->stream, a);
  if (nclasses == 1) hipLaunchKernelGGL(k_t_walk<1>, grid, block, 0, ctx->stream, a);
  if (nclasses == 2) hipLaunchKernelGGL(k_t_walk<2>, grid, block, 0, ctx->stream, a);
  SGT_RC(sync_check(ctx));
  SGT_RC(dcnt.download(ctx, cnt));
  SGT_RC(drec.download(ctx, rec));
  SGT_RC(dtext.check(ctx, 2, broken));
  SGT_RC(doff.check(ctx, 4, broken));
  SGT_RC(dtile.check(ctx, 6, broken));
  SGT_RC(dcnt.check(ctx, 8, broken));
  return drec.check(ctx, 10, broken);
}

}  // extern "C"
