// A hint seed's comparisons on the device: the executor's per-call comparison
// triples into the reader's AddComp pairs, and the fused call from raw
// KCOV_TRACE_CMP buffers and argument values to shrinkExpand's replacers.
//
// Pairs (sg_comps_pairs*): the reader's loop body (pkg/ipc/ipc_linux.go:290-302)
// over a triples CSR, at full operand width.  A wave per call, 64 triples per
// step (the shape of k_ec_emit):
//  - k_cp_count: each lane's triple yields 0, 1 or 2 pairs; a type above 7
//    anywhere in the call is the reader's :266-270 error and zeroes the call's
//    count (the reader assigns Comps after the loop, :304);
//  - scan_counts -> pair_off;
//  - k_cp_emit: the same walk; a DPP prefix of the lanes' counts plus a running
//    base gives the reader's order.
// The operands are extended as kcov_comparison_t::write does (executor.h:
// 632-645) on the way in: a no-op on sg_exec_comps' triples, and what lets the
// fused call feed the workspace's raw sorted keys.
//
// Fused (sg_hints_from_kcov*): exec_comps() stopped before k_ec_emit, the pairs
// kernels on its workspace keys, hints_replacers() on the pairs.  comp_off,
// pair_off and the pairs live in the device staging buffer: hints_replacers
// plans the context workspace from offset 0 and may move it.
// Every loop is bounded by the call's comparison count.
#include "sg_internal.h"

namespace sg {

constexpr int32_t kCpOk = 0, kCpType = 9;  // include/syzsig.h SG_IPC_OK, SG_IPC_COMPS_TYPE

struct CpArgs {
  const uint64_t* src;      // triples {type, arg1, arg2}: call c's at src + 3 * clamp(src_off[c])
  const uint64_t* src_off;  // [ncalls+1]
  uint64_t nsrc;            // triples src holds: the offsets are clamped to it (the device form cannot check them)
  const uint64_t* cnt_off;  // [ncalls+1] or null: call c has cnt_off[c+1] - cnt_off[c] triples, at most its range
  uint64_t ncalls;
};

// call c's triples: src + 3 * r0, n of them
__device__ __forceinline__ void cp_range(const CpArgs& a, uint64_t c, uint64_t& r0, uint64_t& n) {
  uint64_t r1;
  sgd::csr_range(a.src_off, c, a.nsrc, r0, r1);
  n = r1 - r0;
  if (a.cnt_off) {
    const uint64_t o0 = a.cnt_off[c], o1 = a.cnt_off[c + 1];
    n = min(n, o1 > o0 ? o1 - o0 : 0);
  }
}

// triple i of a call: its AddComp calls (0, 1 or 2) and its operands
__device__ __forceinline__ uint32_t cp_pairs(const uint64_t* __restrict__ t, uint64_t i, uint64_t& typ, uint64_t& op1,
                                             uint64_t& op2) {
  typ = t[3 * i];
  op1 = sgd::kcov_extend(typ, t[3 * i + 1]);
  op2 = sgd::kcov_extend(typ, t[3 * i + 2]);
  if (typ > 7 || op1 == op2) return 0;  // ipc_linux.go:266-270 (the call fails), :290-293
  return (typ & 1) ? 1u : 2u;           // :294-302: (op2, op1), and (op1, op2) unless one operand was const
}

// a wave per call: its pair count (0 when a type is bad) and its status
__global__ __launch_bounds__(256) void k_cp_count(CpArgs a, uint32_t* __restrict__ cnt, int32_t* __restrict__ status) {
  const uint64_t c = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (c >= a.ncalls) return;
  const uint32_t lane = threadIdx.x & 63;
  uint64_t r0, n;
  cp_range(a, c, r0, n);
  const uint64_t* __restrict__ t = a.src + 3 * r0;
  uint32_t mine = 0;
  bool bad = false;
  for (uint64_t i = lane; i < n; i += 64) {
    uint64_t typ, op1, op2;
    mine += cp_pairs(t, i, typ, op1, op2);
    bad = bad || typ > 7;
  }
  const uint32_t tot = __shfl(sgd::wave_incl_add(mine), 63);  // <= 2 n < 2^32
  const bool anybad = __ballot(bad) != 0;
  if (lane == 0) {
    cnt[c] = anybad ? 0u : tot;
    status[c] = anybad ? kCpType : kCpOk;
  }
}

// a wave per call: its pairs, in the reader's order, at pairs[pair_off[c] ..]
__global__ __launch_bounds__(256) void k_cp_emit(CpArgs a, const uint64_t* __restrict__ pair_off, uint64_t cap,
                                                 uint64_t* __restrict__ pairs) {
  const uint64_t c = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (c >= a.ncalls) return;
  if (pair_off[a.ncalls] > cap) return;
  const uint64_t o0 = pair_off[c], o1 = pair_off[c + 1];
  if (o0 >= o1) return;  // no pairs, or a bad type
  const uint32_t lane = threadIdx.x & 63;
  uint64_t r0, n;
  cp_range(a, c, r0, n);
  const uint64_t* __restrict__ t = a.src + 3 * r0;
  uint64_t run = o0;
  for (uint64_t base = 0; base < n; base += 64) {
    const uint64_t i = base + lane;
    uint64_t typ = 0, op1 = 0, op2 = 0;
    const uint32_t np = i < n ? cp_pairs(t, i, typ, op1, op2) : 0u;
    const uint32_t incl = sgd::wave_incl_add(np);
    const uint64_t at = run + incl - np;
    if (np >= 1 && at < o1) {
      pairs[2 * at] = op2;  // AddComp(op2, op1)
      pairs[2 * at + 1] = op1;
    }
    if (np == 2 && at + 1 < o1) {
      pairs[2 * at + 2] = op1;  // AddComp(op1, op2)
      pairs[2 * at + 3] = op2;
    }
    run += __shfl(incl, 63);
  }
}

// off[i] = min(off[i], cap): nothing changes when the call offsets are a CSR
// (then off[n - 1] <= cap); offsets the device form could not check may make
// ranges overlap, and whoever reads the pairs by these offsets stays in the buffer
__global__ void k_cp_clamp(uint64_t* __restrict__ off, uint64_t n, uint64_t cap) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n && off[i] > cap) off[i] = cap;
}

// The pairs of the triples `a` describes; ctx lock held.  cnt: ncalls u32 of
// scratch, scan_off: scan_counts' workspace for ncalls counts, both reserved by
// the caller.  clamp: pair_off is an intermediate, kept within cap.
static int comps_pairs(sg_ctx* ctx, const CpArgs& a, int32_t* d_status, uint64_t* d_pair_off, uint64_t* d_pairs,
                       uint64_t cap, uint32_t* cnt, size_t scan_off, bool clamp = false) {
  if (a.ncalls == 0) {
    SG_HIP(hipMemsetAsync(d_pair_off, 0, 8, ctx->stream));
    return SG_OK;
  }
  const dim3 g(div_up(a.ncalls, 4)), b(256);
  {
    ScopedTimer tm(ctx, "comps_pairs");
    hipLaunchKernelGGL(k_cp_count, g, b, 0, ctx->stream, a, cnt, d_status);
  }
  SG_HIP(hipGetLastError());
  int rc = scan_counts(ctx, cnt, d_pair_off, a.ncalls, scan_off);
  if (rc) return rc;
  if (clamp)
    hipLaunchKernelGGL(k_cp_clamp, dim3(div_up(a.ncalls + 1, 256)), dim3(256), 0, ctx->stream, d_pair_off, a.ncalls + 1,
                       cap);
  if (d_pairs) {
    ScopedTimer tm(ctx, "comps_pairs");
    hipLaunchKernelGGL(k_cp_emit, g, b, 0, ctx->stream, a, (const uint64_t*)d_pair_off, cap, d_pairs);
  }
  SG_HIP(hipGetLastError());
  return SG_OK;
}

static int cp_limits(uint64_t ncalls, uint64_t ncomps) {
  if (ncomps >= (1ull << 31) || ncalls >= (1ull << 31)) {
    set_error("sg_comps_pairs: %llu comparisons, %llu calls (the limit of each is 2^31 - 1)",
              (unsigned long long)ncomps, (unsigned long long)ncalls);
    return SG_EINVAL;
  }
  return SG_OK;
}

// sg_comps_pairs_dev's body; ctx lock held, the device ensured
static int comps_pairs_csr(sg_ctx* ctx, const uint64_t* d_comp_off, const uint64_t* d_comps, uint64_t ncalls,
                           uint64_t ncomps, int32_t* d_status, uint64_t* d_pair_off, uint64_t* d_pairs, uint64_t cap) {
  WsPlan p;
  const size_t o_cnt = p.add(ncalls * 4);
  int rc = ws_reserve(ctx, p.total + scan_ws_bytes(ncalls ? ncalls : 1));
  if (rc) return rc;
  CpArgs a{};
  a.src = d_comps;
  a.src_off = d_comp_off;
  a.nsrc = ncomps;
  a.ncalls = ncalls;
  return comps_pairs(ctx, a, d_status, d_pair_off, d_pairs, cap, (uint32_t*)ws_at(ctx, o_cnt), p.total);
}

static int hk_limits(uint64_t ncalls, uint64_t nrecs, uint64_t nvals) {
  // a call keeps at most its records, a comparison yields at most two pairs
  if (nrecs >= (1ull << 31) || ncalls >= (1ull << 31) || nvals >= (1ull << 32)) {
    set_error("sg_hints_from_kcov: %llu records, %llu calls, %llu value slots (the limits are 2^31 - 1, 2^31 - 1 and "
              "2^32 - 1)", (unsigned long long)nrecs, (unsigned long long)ncalls, (unsigned long long)nvals);
    return SG_EINVAL;
  }
  return ec_limits(ncalls, nrecs);
}

// The intermediates of the fused call: regions of the caller's staging plan
struct HkStage {
  size_t comp_off, pair_off, pairs;
  HkStage(WsPlan& p, uint64_t ncalls, uint64_t nrecs)
      : comp_off(p.add((ncalls + 1) * 8)),
        pair_off(p.add((ncalls + 1) * 8)),
        pairs(p.add(2 * nrecs * 16 + 16)) {}  // 2 nrecs pairs always suffice
};

// The three stages; ctx lock held, the device ensured, the staging plan of s reserved
static int hints_from_kcov(sg_ctx* ctx, const uint64_t* d_recs, const uint64_t* d_call_off, uint64_t ncalls,
                           uint64_t nrecs, const uint64_t* d_val_off, const uint64_t* d_vals, uint64_t nvals,
                           int32_t* d_status, const HkStage& s, uint64_t* d_rep_off, uint64_t* d_reps, uint64_t cap,
                           bool reps_in_ws, uint64_t** ws_reps) {
  uint64_t* d_comp_off = dstage_at<uint64_t>(ctx, s.comp_off);
  uint64_t* d_pair_off = dstage_at<uint64_t>(ctx, s.pair_off);
  uint64_t* d_pairs = dstage_at<uint64_t>(ctx, s.pairs);
  EcRaw raw;
  int rc = exec_comps(ctx, d_recs, d_call_off, ncalls, nrecs, d_comp_off, nullptr, 0, nullptr, nullptr, 0, &raw);
  if (rc) return rc;
  if (raw.tmp) {
    CpArgs a{};
    a.src = raw.tmp;
    a.src_off = d_call_off;
    a.nsrc = nrecs;
    a.cnt_off = d_comp_off;
    a.ncalls = ncalls;
    rc = comps_pairs(ctx, a, d_status, d_pair_off, d_pairs, 2 * nrecs, raw.cnt, raw.scan_off, true);
    if (rc) return rc;
  } else {  // no calls or no records: every CompMap is empty
    if (ncalls) SG_HIP(hipMemsetAsync(d_status, 0, ncalls * 4, ctx->stream));
    SG_HIP(hipMemsetAsync(d_pair_off, 0, (ncalls + 1) * 8, ctx->stream));
  }
  return hints_replacers(ctx, d_pair_off, d_pairs, ncalls, d_val_off, d_vals, nvals, d_rep_off, d_reps, cap, reps_in_ws,
                         ws_reps);
}

}  // namespace sg

using namespace sg;

extern "C" {

int sg_comps_pairs_dev(sg_ctx* ctx, const uint64_t* d_comp_off, const uint64_t* d_comps, uint64_t ncalls,
                       uint64_t ncomps, int32_t* d_status, uint64_t* d_pair_off, uint64_t* d_pairs, uint64_t cap) {
  if (!ctx || !d_comp_off || !d_status || !d_pair_off || (ncomps && !d_comps) || (cap && !d_pairs)) return SG_EINVAL;
  int rc = cp_limits(ncalls, ncomps);
  if (rc) return rc;
  std::lock_guard<std::mutex> g(ctx->mu);
  rc = ensure_device(ctx);
  if (rc) return rc;
  return comps_pairs_csr(ctx, d_comp_off, d_comps, ncalls, ncomps, d_status, d_pair_off, d_pairs, cap);
}

int sg_comps_pairs(sg_ctx* ctx, const uint64_t* comp_off, const uint64_t* comps, size_t ncalls, int32_t* status,
                   uint64_t* pair_off, uint64_t* pairs, size_t cap) {
  if (!ctx || !comp_off || !status || !pair_off || (cap && !pairs)) return SG_EINVAL;
  if (ncalls >= (1ull << 31)) return cp_limits(ncalls, 0);
  const uint64_t ncomps = comp_off[ncalls];
  if (!offsets_ok(comp_off, ncalls) || (ncomps && !comps)) return SG_EINVAL;
  int rc = cp_limits(ncalls, ncomps);
  if (rc) return rc;
  // 2 ncomps pairs always suffice: a smaller cap is staged as it is
  const uint64_t pcap = cap < 2 * ncomps ? cap : 2 * ncomps;
  WsPlan p;
  const size_t o_co = p.add((ncalls + 1) * 8), o_po = p.add((ncalls + 1) * 8), o_c = p.add(ncomps * 24 + 24),
               o_st = p.add(ncalls * 4 + 4), o_p = p.add(pcap * 16 + 16);
  std::lock_guard<std::mutex> g(ctx->mu);
  rc = ensure_device(ctx);
  if (rc) return rc;
  rc = dstage_reserve(ctx, p);
  if (rc) return rc;
  uint64_t* dco = dstage_at<uint64_t>(ctx, o_co);
  uint64_t* dpo = dstage_at<uint64_t>(ctx, o_po);
  uint64_t* dc = dstage_at<uint64_t>(ctx, o_c);
  int32_t* dst = dstage_at<int32_t>(ctx, o_st);
  uint64_t* dp = dstage_at<uint64_t>(ctx, o_p);
  if ((rc = upload(ctx, dco, comp_off, (ncalls + 1) * 8))) return rc;
  if ((rc = upload(ctx, dc, comps, ncomps * 24))) return rc;
  rc = comps_pairs_csr(ctx, dco, dc, ncalls, ncomps, dst, dpo, pcap ? dp : nullptr, pcap);
  if (rc) return rc;
  if (ncalls) SG_HIP(hipMemcpyAsync(status, dst, ncalls * 4, hipMemcpyDeviceToHost, ctx->stream));
  return csr_download(ctx, pair_off, dpo, ncalls, pairs, dp, 16, cap);
}

int sg_hints_from_kcov_dev(sg_ctx* ctx, const uint64_t* d_recs, const uint64_t* d_call_off, uint64_t ncalls,
                           uint64_t nrecs, const uint64_t* d_val_off, const uint64_t* d_vals, uint64_t nvals,
                           int32_t* d_status, uint64_t* d_rep_off, uint64_t* d_reps, uint64_t cap) {
  if (!ctx || !d_call_off || !d_val_off || !d_status || !d_rep_off || (nrecs && !d_recs) || (nvals && !d_vals) ||
      (cap && !d_reps))
    return SG_EINVAL;
  int rc = hk_limits(ncalls, nrecs, nvals);
  if (rc) return rc;
  std::lock_guard<std::mutex> g(ctx->mu);
  rc = ensure_device(ctx);
  if (rc) return rc;
  WsPlan p;
  const HkStage s(p, ncalls, nrecs);
  rc = dstage_reserve(ctx, p);  // grow-only: waits only when it has to grow
  if (rc) return rc;
  return hints_from_kcov(ctx, d_recs, d_call_off, ncalls, nrecs, d_val_off, d_vals, nvals, d_status, s, d_rep_off,
                         d_reps, cap, false, nullptr);
}

int sg_hints_from_kcov(sg_ctx* ctx, const uint64_t* recs, const uint64_t* call_off, size_t ncalls,
                       const uint64_t* val_off, const uint64_t* vals, int32_t* status, uint64_t* rep_off, uint64_t* reps,
                       size_t cap) {
  if (!ctx || !call_off || !val_off || !status || !rep_off || (cap && !reps)) return SG_EINVAL;
  if (ncalls >= (1ull << 31)) return hk_limits(ncalls, 0, 0);
  const uint64_t nrecs = call_off[ncalls], nvals = val_off[ncalls];
  if (!offsets_ok(call_off, ncalls) || !offsets_ok(val_off, ncalls) || (nrecs && !recs) || (nvals && !vals))
    return SG_EINVAL;
  int rc = hk_limits(ncalls, nrecs, nvals);
  if (rc) return rc;
  WsPlan p;
  const size_t o_recs = p.add(nrecs * 32 + 32), o_co = p.add((ncalls + 1) * 8), o_vo = p.add((ncalls + 1) * 8),
               o_v = p.add(nvals * 8 + 8), o_st = p.add(ncalls * 4 + 4), o_ro = p.add((nvals + 1) * 8);
  const HkStage s(p, ncalls, nrecs);
  std::lock_guard<std::mutex> g(ctx->mu);
  rc = ensure_device(ctx);
  if (rc) return rc;
  rc = dstage_reserve(ctx, p);
  if (rc) return rc;
  uint64_t* drecs = dstage_at<uint64_t>(ctx, o_recs);
  uint64_t* dco = dstage_at<uint64_t>(ctx, o_co);
  uint64_t* dvo = dstage_at<uint64_t>(ctx, o_vo);
  uint64_t* dv = dstage_at<uint64_t>(ctx, o_v);
  int32_t* dst = dstage_at<int32_t>(ctx, o_st);
  uint64_t* dro = dstage_at<uint64_t>(ctx, o_ro);
  if ((rc = upload(ctx, drecs, recs, nrecs * 32))) return rc;
  if ((rc = upload(ctx, dco, call_off, (ncalls + 1) * 8))) return rc;
  if ((rc = upload(ctx, dvo, val_off, (ncalls + 1) * 8))) return rc;
  if ((rc = upload(ctx, dv, vals, nvals * 8))) return rc;
  uint64_t* dreps = nullptr;
  rc = hints_from_kcov(ctx, drecs, dco, ncalls, nrecs, dvo, dv, nvals, dst, s, dro, nullptr, cap, true, &dreps);
  if (rc) return rc;
  if (ncalls) SG_HIP(hipMemcpyAsync(status, dst, ncalls * 4, hipMemcpyDeviceToHost, ctx->stream));
  return csr_download(ctx, rep_off, dro, nvals, reps, dreps, 8, cap);  // (dreps: set whenever a replacer was written)
}

}  // extern "C"
