// sg_minimize_pred.hip -- the predicate prog.Minimize calls in triageInput
// (syz-fuzzer/fuzzer.go:578-591, called from prog/mutation.go:256-450) from the
// raw KCOV buffers of the shortened programs' executions, for a batch of
// attempts.
//
// Per attempt e the reference runs execute() (:579), gives up when
// info[call1] does not exist or holds no Signal (:580-582), and otherwise
// answers len(Intersection(newSignal, Canonicalize(Signal))) == len(newSignal)
// (:584-590).  execute() itself runs the new-signal check of :665-691 on every
// call of the program.
//
// Stages, all on the context's stream:
//  1. k_tr_trunc truncates the PCs (executor.h:394).
//  2. With maxSignal: execute()'s check of all calls, bucket_triage on the
//     truncated traces (what sg_triage_traces_dev runs): rec_new and both sets.
//  3. k_tr_select with one execution per attempt marks call[e] on top of a
//     copy of rec_new and records it (sg_runs.h).
//  4. exec_signal_body with those marks as its queued flags: each execution
//     runs once, up to its last marked call, and the marked calls get their
//     executor-exact lists.  The table cannot be skipped: what a call's Signal
//     holds depends on the calls before it.
//  5. k_mp_pred, a workgroup per attempt, decides status[e]: the "not
//     executed" rule, else tin_intersect, the body of sg_triage_subset.  (A
//     second route, a wave per attempt for lists of at most 64 values, was
//     measured and not kept: DESIGN.md 4i.)
//  6. With maxSignal: k_mp_lists copies the lists out when they fit.
#include "sg_runs.h"
#include "sg_tinput.h"

namespace sg {
namespace {

using namespace tin;

struct PredArgs {
  uint64_t n, ncand, nnew;
  const uint32_t* new_vals;
  const uint64_t* new_off;
  const uint32_t* cand;
  const uint32_t* selcall;
  const uint64_t* xsig_off;
  const uint32_t* xsig;
  int32_t* status;
};

// status[e] (fuzzer.go:580-590): attempt e's list is new[a0 .. a1), its Signal xsig[r0 .. r1)
__global__ __launch_bounds__(kTB) void k_mp_pred(PredArgs a) {
  __shared__ IntersectLds lds;
  const uint64_t e = blockIdx.x;
  const uint64_t k = min<uint64_t>(a.cand[e], a.ncand - 1);
  uint64_t a0, a1;
  sgd::csr_range(a.new_off, k, a.nnew, a0, a1);
  const uint32_t c = a.selcall[e];
  const uint64_t r0 = c == kNoCall ? 0 : a.xsig_off[c], r1 = c == kNoCall ? 0 : a.xsig_off[c + 1];
  int32_t st = SG_MP_NOT_EXECUTED;  // :580-582
  if (r1 > r0) {
    const uint64_t kept = tin_intersect<false>(const_cast<uint32_t*>(a.new_vals), a0, a1, a.xsig, r0, r1, lds);
    st = kept == a1 - a0 ? SG_MP_OK : SG_MP_LOST;  // :587-589
  }
  if (threadIdx.x == 0) a.status[e] = st;
}

// the marked calls' lists to the caller's buffer, when they fit it
__global__ void k_mp_lists(const uint64_t* __restrict__ sig_off, uint64_t ncalls, uint64_t npcs,
                           const uint32_t* __restrict__ xsig, uint32_t* __restrict__ sig_vals, uint64_t cap) {
  const uint64_t total = min(sig_off[ncalls], npcs);
  if (total > cap) return;
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) sig_vals[i] = xsig[i];
}

// the call's intermediates: regions of the caller's staging plan
struct MpPlan {
  size_t pcs32, sel, selcall, xsig_off, xsig;
  MpPlan(WsPlan& p, uint64_t n, uint64_t ncalls, uint64_t npcs) {
    pcs32 = p.add(npcs * 4 + 4);
    sel = p.add(ncalls + 1);
    selcall = p.add(n * 4 + 4);
    xsig_off = p.add((ncalls + 1) * 8);
    xsig = p.add(npcs * 4 + 4);
  }
};

struct MpIo {
  const uint32_t* new_vals;
  const uint64_t* new_off;
  uint64_t ncand, nnew;
  const uint32_t* cand;
  const uint32_t* call;
  uint64_t n;
  const uint64_t* pcs;
  const uint64_t* call_off;
  const uint64_t* prog_off;
  uint64_t ncalls, npcs;
  int32_t* status;
  uint8_t* rec_new;  // the three list outputs: with maxsig only
  uint64_t* sig_off;
  uint32_t* sig_vals;
  uint64_t sig_cap;
};

int mp_limits(uint64_t n, uint64_t ncand, uint64_t nnew, uint64_t ncalls, uint64_t npcs) {
  if (n >= (1ull << 28) || ncand >= (1ull << 32) || nnew >= (1ull << 32) || ncalls >= (1ull << 31) ||
      npcs >= (1ull << 32) || (n && !ncand)) {
    set_error("sg_minimize_pred_from_kcov: %llu attempts on %llu lists of %llu values, %llu calls, %llu PCs (the limits "
              "are 2^28 - 1, 2^32 - 1, 2^32 - 1, 2^31 - 1 and 2^32 - 1; attempts need a list)",
              (unsigned long long)n, (unsigned long long)ncand, (unsigned long long)nnew, (unsigned long long)ncalls,
              (unsigned long long)npcs);
    return SG_EINVAL;
  }
  return SG_OK;
}

// the body of both forms: every pointer of io is device memory, the
// intermediates are p's regions of the staging buffer (reserved by the
// caller); ctx lock held, the device ensured, n > 0
int minimize_pred(sg_ctx* ctx, sg_set* maxsig, sg_set* newsig, const MpIo& io, const MpPlan& p) {
  const uint64_t n = io.n, ncalls = io.ncalls, npcs = io.npcs;
  uint32_t* pcs32 = dstage_at<uint32_t>(ctx, p.pcs32);
  uint8_t* sel = dstage_at<uint8_t>(ctx, p.sel);
  uint32_t* selcall = dstage_at<uint32_t>(ctx, p.selcall);
  uint64_t* xsig_off = maxsig ? io.sig_off : dstage_at<uint64_t>(ctx, p.xsig_off);  // offsets are always filled
  uint32_t* xsig = dstage_at<uint32_t>(ctx, p.xsig);
  const dim3 b(256);
  int rc;
  // 1. the truncated PCs
  if (npcs)
    hipLaunchKernelGGL(k_tr_trunc, dim3(std::min<uint64_t>(div_up(npcs, 256), 65536)), b, 0, ctx->stream, io.pcs, npcs,
                       pcs32);
  SG_HIP(hipGetLastError());
  // 2. execute()'s new-signal check of every call (fuzzer.go:665-691)
  if (maxsig && ncalls) {
    rc = bucket_triage(ctx, maxsig->words, newsig ? newsig->words : nullptr, pcs32, io.call_off, npcs, ncalls, io.rec_new,
                       true);
    if (rc) return rc;
    SG_HIP(hipMemcpyAsync(sel, io.rec_new, ncalls, hipMemcpyDeviceToDevice, ctx->stream));
  } else {
    SG_HIP(hipMemsetAsync(sel, 0, ncalls + 1, ctx->stream));
  }
  // 3. call1 of every execution, on top of the queued calls
  hipLaunchKernelGGL(k_tr_select, dim3(div_up(n, 256)), b, 0, ctx->stream, io.prog_off, io.call, n, 1u, ncalls, selcall,
                     sel);
  SG_HIP(hipGetLastError());
  // 4. the executor, once: the lists of the marked calls
  rc = exec_signal_body(ctx, pcs32, io.call_off, io.prog_off, n, ncalls, npcs, sel, xsig, xsig_off);
  if (rc) return rc;
  // 5. the predicate
  {
    ScopedTimer tm(ctx, "minimize_pred");
    const PredArgs pa{n, io.ncand, io.nnew, io.new_vals, io.new_off, io.cand, selcall, xsig_off, xsig, io.status};
    hipLaunchKernelGGL(k_mp_pred, dim3((uint32_t)n), dim3(kTB), 0, ctx->stream, pa);
  }
  SG_HIP(hipGetLastError());
  // 6. the lists
  if (maxsig && io.sig_vals && io.sig_cap && npcs)
    hipLaunchKernelGGL(k_mp_lists, dim3(std::min<uint64_t>(div_up(npcs, 256), 4096)), b, 0, ctx->stream, xsig_off, ncalls,
                       npcs, xsig, io.sig_vals, io.sig_cap);
  SG_HIP(hipGetLastError());
  return SG_OK;
}

}  // namespace
}  // namespace sg

using namespace sg;

extern "C" {

int sg_minimize_pred_from_kcov_dev(sg_ctx* ctx, sg_set* maxsig, sg_set* newsig, const uint32_t* d_new_vals,
                                   const uint64_t* d_new_off, uint64_t ncand, uint64_t nnew, const uint32_t* d_cand,
                                   const uint32_t* d_call, uint64_t n, const uint64_t* d_pcs, const uint64_t* d_call_off,
                                   const uint64_t* d_prog_off, uint64_t ncalls, uint64_t npcs, int32_t* d_status,
                                   uint8_t* d_rec_new, uint64_t* d_sig_off, uint32_t* d_sig_vals, uint64_t sig_cap) {
  if (!ctx || !d_new_off || !d_prog_off || !d_call_off || (n && (!d_cand || !d_call || !d_status)) ||
      (nnew && !d_new_vals) || (npcs && !d_pcs) || (newsig && !maxsig) ||
      (maxsig && (!d_sig_off || (ncalls && !d_rec_new) || (sig_cap && !d_sig_vals)))) {
    set_error("sg_minimize_pred_from_kcov_dev: invalid argument");
    return SG_EINVAL;
  }
  if ((maxsig && maxsig->ctx != ctx) || (newsig && newsig->ctx != ctx)) {
    set_error("sg_minimize_pred_from_kcov_dev: set belongs to another context");
    return SG_EINVAL;
  }
  int rc = mp_limits(n, ncand, nnew, ncalls, npcs);
  if (rc) return rc;
  std::lock_guard<std::mutex> g(ctx->mu);
  rc = ensure_device(ctx);
  if (rc) return rc;
  if (n == 0) {
    if (maxsig) SG_HIP(hipMemsetAsync(d_sig_off, 0, 8, ctx->stream));
    return SG_OK;
  }
  WsPlan plan;
  const MpPlan p(plan, n, ncalls, npcs);
  rc = dstage_reserve(ctx, plan);
  if (rc) return rc;
  const MpIo io{d_new_vals, d_new_off, ncand, nnew,     d_cand,    d_call,    n,          d_pcs,  d_call_off,
                d_prog_off, ncalls,    npcs,  d_status, d_rec_new, d_sig_off, d_sig_vals, sig_cap};
  return minimize_pred(ctx, maxsig, newsig, io, p);
}

int sg_minimize_pred_from_kcov(sg_ctx* ctx, sg_set* maxsig, sg_set* newsig, const uint32_t* new_vals,
                               const uint64_t* new_off, size_t ncand, const uint32_t* cand, const uint32_t* call, size_t n,
                               const uint64_t* pcs, const uint64_t* call_off, const uint64_t* prog_off, int32_t* status,
                               uint8_t* rec_new, uint64_t* sig_off, uint32_t* sig_vals, size_t sig_cap) {
  if (!ctx || !new_off || !prog_off || !call_off || (n && (!cand || !call || !status)) || (newsig && !maxsig) ||
      (maxsig && (!sig_off || (sig_cap && !sig_vals))) || n >= (1ull << 28) || ncand >= (1ull << 32)) {
    set_error("sg_minimize_pred_from_kcov: invalid argument");
    return SG_EINVAL;
  }
  if ((maxsig && maxsig->ctx != ctx) || (newsig && newsig->ctx != ctx)) {
    set_error("sg_minimize_pred_from_kcov: set belongs to another context");
    return SG_EINVAL;
  }
  if (!offsets_ok(new_off, ncand) || !offsets_ok(prog_off, n)) {
    set_error("sg_minimize_pred_from_kcov: offsets start at 0 and do not decrease");
    return SG_EINVAL;
  }
  const uint64_t nnew = new_off[ncand], ncalls = prog_off[n];
  int rc = mp_limits(n, ncand, nnew, ncalls, 0);
  if (rc) return rc;
  if (!offsets_ok(call_off, ncalls)) {
    set_error("sg_minimize_pred_from_kcov: offsets start at 0 and do not decrease");
    return SG_EINVAL;
  }
  const uint64_t npcs = call_off[ncalls];
  rc = mp_limits(n, ncand, nnew, ncalls, npcs);
  if (rc) return rc;
  if ((nnew && !new_vals) || (npcs && !pcs) || (maxsig && ncalls && !rec_new)) {
    set_error("sg_minimize_pred_from_kcov: invalid argument");
    return SG_EINVAL;
  }
  for (size_t e = 0; e < n; e++)
    if (cand[e] >= ncand) {
      set_error("sg_minimize_pred_from_kcov: attempt %zu tests list %u of %zu", e, cand[e], ncand);
      return SG_EINVAL;
    }
  for (size_t k = 0; k < ncand; k++)
    for (uint64_t i = new_off[k] + 1; i < new_off[k + 1]; i++)
      if (new_vals[i] < new_vals[i - 1]) {
        set_error("sg_minimize_pred_from_kcov: list %zu is not sorted", k);
        return SG_EINVAL;
      }
  if (n == 0) {
    if (maxsig) sig_off[0] = 0;
    return SG_OK;
  }
  // npcs values always suffice: a smaller cap is staged as it is
  const uint64_t scap = maxsig ? (sig_cap < npcs ? sig_cap : npcs) : 0;
  WsPlan plan;
  const size_t o_nv = plan.add(nnew * 4 + 4), o_no = plan.add((ncand + 1) * 8), o_cand = plan.add(n * 4),
               o_call = plan.add(n * 4), o_po = plan.add((n + 1) * 8), o_co = plan.add((ncalls + 1) * 8),
               o_pcs = plan.add(npcs * 8 + 8), o_st = plan.add(n * 4), o_rn = plan.add(ncalls + 1),
               o_so = plan.add((ncalls + 1) * 8), o_sv = plan.add(scap * 4 + 4);
  const MpPlan p(plan, n, ncalls, npcs);
  std::lock_guard<std::mutex> g(ctx->mu);
  rc = ensure_device(ctx);
  if (rc) return rc;
  rc = dstage_reserve(ctx, plan);
  if (rc) return rc;
  uint32_t* dnv = dstage_at<uint32_t>(ctx, o_nv);
  uint64_t* dno = dstage_at<uint64_t>(ctx, o_no);
  uint32_t* dcand = dstage_at<uint32_t>(ctx, o_cand);
  uint32_t* dcall = dstage_at<uint32_t>(ctx, o_call);
  uint64_t* dpo = dstage_at<uint64_t>(ctx, o_po);
  uint64_t* dco = dstage_at<uint64_t>(ctx, o_co);
  uint64_t* dpcs = dstage_at<uint64_t>(ctx, o_pcs);
  int32_t* dst = dstage_at<int32_t>(ctx, o_st);
  uint8_t* drn = dstage_at<uint8_t>(ctx, o_rn);
  uint64_t* dso = dstage_at<uint64_t>(ctx, o_so);
  uint32_t* dsv = dstage_at<uint32_t>(ctx, o_sv);
  if ((rc = upload(ctx, dnv, new_vals, nnew * 4))) return rc;
  if ((rc = upload(ctx, dno, new_off, (ncand + 1) * 8))) return rc;
  if ((rc = upload(ctx, dcand, cand, n * 4))) return rc;
  if ((rc = upload(ctx, dcall, call, n * 4))) return rc;
  if ((rc = upload(ctx, dpo, prog_off, (n + 1) * 8))) return rc;
  if ((rc = upload(ctx, dco, call_off, (ncalls + 1) * 8))) return rc;
  if ((rc = upload(ctx, dpcs, pcs, npcs * 8))) return rc;
  const MpIo io{dnv, dno,    ncand, nnew, dcand, dcall, n,   dpcs,
                dco, dpo,    ncalls, npcs, dst,   drn,   dso, scap ? dsv : nullptr,
                scap};
  rc = minimize_pred(ctx, maxsig, newsig, io, p);
  if (rc) return rc;
  SG_HIP(hipMemcpyAsync(status, dst, n * 4, hipMemcpyDeviceToHost, ctx->stream));
  if (!maxsig) {
    SG_HIP(hipStreamSynchronize(ctx->stream));
    return SG_OK;
  }
  if (ncalls) SG_HIP(hipMemcpyAsync(rec_new, drn, ncalls, hipMemcpyDeviceToHost, ctx->stream));
  return csr_download(ctx, sig_off, dso, ncalls, sig_vals, dsv, 4, sig_cap);
}

}  // extern "C"
