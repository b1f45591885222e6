// sg_hub_state.hip -- st.Corpus of syz-hub/state/state.go on the device:
// addInputs (state.go:310-336) and loadDB's loop (:83-110), pendingInputs
// (:265-308) and purgeCorpus (:338-354), which the reference runs under the
// hub's lock over the whole hub corpus for every manager's every sync
// (State.Sync, :175-195).
//
// A record is (key, seq, call ids).  The keys are an sg_sigset (its store and
// table, sg_sigset.hip), so a record's index is its store index and records
// are in insertion order; seq[] and the CSR call_off / ids run parallel to the
// store.  The ids come from the CallSet scan and the name dictionary
// (sg_call_set.hip) once, when the record enters: pending never sees a text.
//  * add: scan, lookup; any unknown name of a status-0 program ends the call
//    with the spans and nothing changed.  Otherwise SHA-1 of every program, the
//    status-0 ones' keys gathered dense, sg_sigset_add_new's kernels on mgr and
//    on the keys, and the new records' seqs and ids appended at the positions
//    the add's own scan gives.
//  * pending: a thread per record tests seq, the manager's set (k_ss_lookup)
//    and its ids against the mask; the selected (seq << 31 | index) keys are
//    sorted (radix_sort_u64) and one thread finds the cut of :286-300.
//  * purge: used[r] ORed over the managers' sets, then keys, seqs and ids are
//    gathered into the second halves (the key set's and the records': each
//    buffer owns its block and capacity, DevBuf of sg_buf.h, and grows from 1024
//    elements by doubling, rec_reserve), a fresh table is built and the halves
//    are swapped: nothing is ever
//    deleted from a table, so there are no tombstones and a probe never has to
//    step over a dead slot; the price is a rebuild per deleting call.
// Every index is checked against its buffer's capacity before it is used as
// an address.  No thread waits for another.
#include "sg_internal.h"

#include <algorithm>
#include <cstddef>

struct sg_hubcorpus {
  sg_ctx* ctx = nullptr;
  uint64_t count = 0;  // records (the keys' count; kept here too, for the checks made before the context is touched)
  sg_nametab* tab = nullptr;
  sg_sigset* keys = nullptr;
  uint64_t nids = 0;
  // the records beside the keys; purge gathers the kept ones into `next`, then swaps the halves
  struct Half {
    sg::DevBuf<uint64_t> seq;
    sg::DevBuf<uint64_t> call_off;  // [count + 1]
    sg::DevBuf<uint32_t> ids;
    void swap(Half& o) {
      seq.swap(o.seq);
      call_off.swap(o.call_off);
      ids.swap(o.ids);
    }
  } cur, next;
  // add's call lines: name_pos, name_len, name_id (bytes)
  sg::DevBuf<uint8_t> lines;
};
static_assert(offsetof(sg_hubcorpus, count) == 8, "tests/test_hub_state.py plants a count in a readable block");

namespace sg {
namespace {

constexpr uint32_t kHT = 256;
constexpr uint32_t kKeyDw = SG_SIG_BYTES / 4;
constexpr uint64_t kIdxBits = 31;
constexpr uint64_t kIdxMask = (1ull << kIdxBits) - 1;

__global__ __launch_bounds__(kHT) void k_hs_unk_flags(const uint32_t* __restrict__ name_id, uint64_t nl,
                                                       uint32_t* __restrict__ flag) {
  const uint64_t i = (uint64_t)blockIdx.x * kHT + threadIdx.x;
  if (i < nl) flag[i] = name_id[i] == SG_NAME_UNKNOWN;
}

__global__ __launch_bounds__(kHT) void k_hs_ok_flags(const uint8_t* __restrict__ status, uint64_t n,
                                                      uint32_t* __restrict__ flag) {
  const uint64_t k = (uint64_t)blockIdx.x * kHT + threadIdx.x;
  if (k < n) flag[k] = status[k] == SG_CALLSET_OK;
}

__global__ __launch_bounds__(kHT) void k_hs_unk_gather(const uint32_t* __restrict__ flag, const uint64_t* __restrict__ pos,
                                                        uint64_t nl, const uint64_t* __restrict__ name_pos,
                                                        const uint32_t* __restrict__ name_len, uint64_t cap,
                                                        uint64_t* __restrict__ out_pos, uint32_t* __restrict__ out_len) {
  const uint64_t i = (uint64_t)blockIdx.x * kHT + threadIdx.x;
  if (i >= nl || !flag[i] || pos[i] >= cap) return;
  out_pos[pos[i]] = name_pos[i];
  out_len[pos[i]] = name_len[i];
}

// program k: is_new[k], and for its dense index j the ids it brings
__global__ __launch_bounds__(kHT) void k_hs_new_counts(const uint32_t* __restrict__ okflag, const uint64_t* __restrict__ okpos,
                                                        uint64_t n, uint64_t m, const uint32_t* __restrict__ entered,
                                                        const uint64_t* __restrict__ line_off, uint8_t* __restrict__ is_new,
                                                        uint32_t* __restrict__ newcnt) {
  const uint64_t k = (uint64_t)blockIdx.x * kHT + threadIdx.x;
  if (k >= n) return;
  uint8_t nw = 0;
  if (okflag[k]) {
    const uint64_t j = okpos[k];
    if (j < m) {
      nw = entered[j] != 0;
      const uint64_t c = line_off[k + 1] - line_off[k];
      newcnt[j] = nw ? (uint32_t)min(c, (uint64_t)0xFFFFFFFFull) : 0u;
    }
  }
  is_new[k] = nw;
}

__global__ __launch_bounds__(kHT) void k_hs_append_recs(const uint32_t* __restrict__ okflag, const uint64_t* __restrict__ okpos,
                                                         uint64_t n, uint64_t m, const uint32_t* __restrict__ entered,
                                                         const uint64_t* __restrict__ newpos,
                                                         const uint64_t* __restrict__ idpos, const uint64_t* __restrict__ seqs,
                                                         uint64_t old, uint64_t nids, uint64_t* __restrict__ seq,
                                                         uint64_t seq_cap, uint64_t* __restrict__ call_off, uint64_t off_cap) {
  const uint64_t k = (uint64_t)blockIdx.x * kHT + threadIdx.x;
  if (k >= n || !okflag[k]) return;
  const uint64_t j = okpos[k];
  if (j >= m || !entered[j]) return;
  const uint64_t r = old + newpos[j];
  if (r >= seq_cap || r + 1 >= off_cap) return;
  seq[r] = seqs[k];
  call_off[r + 1] = nids + idpos[j + 1];
}

// call line i of the batch: to its record's ids when its program entered
__global__ __launch_bounds__(kHT) void k_hs_append_ids(const uint32_t* __restrict__ okflag, const uint64_t* __restrict__ okpos,
                                                        uint64_t n, uint64_t m, const uint32_t* __restrict__ entered,
                                                        const uint64_t* __restrict__ idpos,
                                                        const uint64_t* __restrict__ line_off, uint64_t nl,
                                                        const uint32_t* __restrict__ name_id, uint64_t nids,
                                                        uint32_t* __restrict__ ids, uint64_t ids_cap) {
  const uint64_t i = (uint64_t)blockIdx.x * kHT + threadIdx.x;
  if (i >= nl) return;
  const uint64_t k = sgd::seg_search(line_off, (uint64_t)0, n - 1, i);
  if (!okflag[k] || i < line_off[k]) return;
  const uint64_t j = okpos[k];
  if (j >= m || !entered[j]) return;
  const uint64_t dst = nids + idpos[j] + (i - line_off[k]);
  if (dst < ids_cap && dst < nids + idpos[j + 1]) ids[dst] = name_id[i];
}

// sel[r] &= seq[r] > mgr_seq and every id of r has its bit in mask
__global__ __launch_bounds__(kHT) void k_hs_pending_sel(uint32_t* __restrict__ sel, uint64_t c, const uint64_t* __restrict__ seq,
                                                         uint64_t mgr_seq, const uint64_t* __restrict__ call_off,
                                                         const uint32_t* __restrict__ ids, uint64_t nids,
                                                         const uint64_t* __restrict__ mask, uint64_t nwords) {
  const uint64_t r = (uint64_t)blockIdx.x * kHT + threadIdx.x;
  if (r >= c) return;
  bool ok = sel[r] && seq[r] > mgr_seq;
  if (ok) {
    const uint64_t b = call_off[r], e = min(call_off[r + 1], nids);
    for (uint64_t i = b; i < e && ok; i++) {
      const uint32_t id = ids[i];
      ok = (uint64_t)(id >> 6) < nwords && ((mask[id >> 6] >> (id & 63)) & 1);
    }
  }
  sel[r] = ok;
}

__global__ __launch_bounds__(kHT) void k_hs_pending_keys(const uint32_t* __restrict__ sel, const uint64_t* __restrict__ pos,
                                                          uint64_t c, const uint64_t* __restrict__ seq,
                                                          uint64_t* __restrict__ keys) {
  const uint64_t r = (uint64_t)blockIdx.x * kHT + threadIdx.x;
  if (r >= c || !sel[r] || pos[r] >= c) return;
  keys[pos[r]] = (seq[r] << kIdxBits) | r;
}

// state.go:292-298 on the sorted keys: cut[0] = maxSeq, cut[1] = pos
__global__ void k_hs_cut(const uint64_t* __restrict__ sorted, uint64_t n, uint64_t max_records, uint64_t* __restrict__ cut) {
  if (max_records >= n) {
    cut[0] = 0;
    cut[1] = n;
    return;
  }
  const uint64_t ms = sorted[max_records] >> kIdxBits;
  uint64_t lo = max_records, hi = n;  // the first key whose seq is above ms
  while (lo < hi) {
    const uint64_t mid = lo + (hi - lo) / 2;
    if ((sorted[mid] >> kIdxBits) > ms)
      hi = mid;
    else
      lo = mid + 1;
  }
  cut[0] = ms;
  cut[1] = lo;
}

__global__ __launch_bounds__(kHT) void k_hs_pending_out(const uint64_t* __restrict__ sorted, uint64_t keep,
                                                         const uint32_t* __restrict__ store, uint64_t c,
                                                         uint32_t* __restrict__ out_sigs, uint64_t* __restrict__ out_seqs) {
  const uint64_t i = (uint64_t)blockIdx.x * kHT + threadIdx.x;
  if (i >= keep) return;
  const uint64_t key = sorted[i], r = key & kIdxMask;
  out_seqs[i] = key >> kIdxBits;
  if (r >= c) return;
#pragma unroll
  for (uint32_t w = 0; w < kKeyDw; w++) out_sigs[i * kKeyDw + w] = store[r * kKeyDw + w];
}

__global__ __launch_bounds__(kHT) void k_hs_purge_flags(const uint32_t* __restrict__ used, uint64_t c,
                                                         const uint64_t* __restrict__ call_off, uint32_t* __restrict__ dead,
                                                         uint32_t* __restrict__ newcnt) {
  const uint64_t r = (uint64_t)blockIdx.x * kHT + threadIdx.x;
  if (r >= c) return;
  dead[r] = !used[r];
  const uint64_t n = call_off[r + 1] >= call_off[r] ? call_off[r + 1] - call_off[r] : 0;
  newcnt[r] = used[r] ? (uint32_t)min(n, (uint64_t)0xFFFFFFFFull) : 0u;
}

__global__ __launch_bounds__(kHT) void k_hs_purge_recs(const uint32_t* __restrict__ used, const uint64_t* __restrict__ keeppos,
                                                        const uint64_t* __restrict__ idpos, uint64_t c,
                                                        const uint64_t* __restrict__ seq, uint64_t* __restrict__ seq2,
                                                        uint64_t seq2_cap, uint64_t* __restrict__ call_off2,
                                                        uint64_t off2_cap) {
  const uint64_t r = (uint64_t)blockIdx.x * kHT + threadIdx.x;
  if (r == 0) call_off2[0] = 0;
  if (r >= c || !used[r]) return;
  const uint64_t nr = keeppos[r];
  if (nr >= seq2_cap || nr + 1 >= off2_cap) return;
  seq2[nr] = seq[r];
  call_off2[nr + 1] = idpos[r + 1];
}

__global__ __launch_bounds__(kHT) void k_hs_purge_ids(const uint32_t* __restrict__ used, const uint64_t* __restrict__ idpos,
                                                       uint64_t c, const uint64_t* __restrict__ call_off,
                                                       const uint32_t* __restrict__ ids, uint64_t nids,
                                                       uint32_t* __restrict__ ids2, uint64_t ids2_cap) {
  const uint64_t i = (uint64_t)blockIdx.x * kHT + threadIdx.x;
  if (i >= nids) return;
  const uint64_t r = sgd::seg_search(call_off, (uint64_t)0, c - 1, i);
  if (!used[r] || i < call_off[r]) return;
  const uint64_t dst = idpos[r] + (i - call_off[r]);
  if (dst < ids2_cap && dst < idpos[r + 1]) ids2[dst] = ids[i];
}

void hub_free(sg_hubcorpus* h) {
  sigset_delete(h->keys);
  delete h;
}

inline dim3 grid_of(uint64_t n) { return dim3(div_up(std::max<uint64_t>(n, 1), kHT)); }

bool foreign(const sg_hubcorpus* h, const sg_sigset* s) { return s && s->ctx != h->ctx; }

}  // namespace
}  // namespace sg

using namespace sg;

extern "C" {

int sg_hubcorpus_create(sg_ctx* ctx, sg_nametab* tab, sg_hubcorpus** out) {
  const char* fn = "sg_hubcorpus_create";
  if (!ctx || !tab || !out) {
    set_error("%s: invalid argument", fn);
    return SG_EINVAL;
  }
  *out = nullptr;
  if (nametab_ctx(tab) != ctx) {
    set_error("%s: the name table belongs to another context", fn);
    return SG_EINVAL;
  }
  std::lock_guard<std::mutex> g(ctx->mu);
  int rc = ensure_device(ctx);
  if (rc) return rc;
  sg_hubcorpus* h = new sg_hubcorpus();
  h->ctx = ctx;
  h->tab = tab;
  rc = sigset_new(ctx, 1, &h->keys);
  if (!rc) rc = rec_reserve(ctx, h->cur.seq, 1024, 0);
  if (!rc) rc = rec_reserve(ctx, h->cur.call_off, 1025, 0);
  if (!rc) rc = rec_reserve(ctx, h->cur.ids, 1024, 0);
  if (!rc) {
    hipError_t e = hipMemsetAsync(h->cur.call_off.p, 0, 8, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) rc = hip_fail(e, fn);
  }
  if (rc) {
    hub_free(h);
    return rc;
  }
  *out = h;
  return SG_OK;
}

void sg_hubcorpus_destroy(sg_hubcorpus* h) {
  if (!h) return;
  {
    std::lock_guard<std::mutex> g(h->ctx->mu);
    hipSetDevice(h->ctx->device);
    hipStreamSynchronize(h->ctx->stream);
  }
  hub_free(h);
}

int sg_hubcorpus_count(sg_hubcorpus* h, uint64_t* nrecs) {
  if (!h || !nrecs) {
    set_error("sg_hubcorpus_count: invalid argument");
    return SG_EINVAL;
  }
  std::lock_guard<std::mutex> g(h->ctx->mu);
  *nrecs = h->count;
  return SG_OK;
}

int sg_hubcorpus_export(sg_hubcorpus* h, uint8_t* sigs, uint64_t* seqs, uint64_t* call_off, uint32_t* call_ids,
                        size_t cap_recs, size_t cap_ids, size_t* nrecs, size_t* nids) {
  if (!h || !nrecs || !nids || !call_off || (cap_recs && (!sigs || !seqs)) || (cap_ids && !call_ids)) {
    set_error("sg_hubcorpus_export: invalid argument");
    return SG_EINVAL;
  }
  sg_ctx* ctx = h->ctx;
  std::lock_guard<std::mutex> g(ctx->mu);
  int rc = ensure_device(ctx);
  if (rc) return rc;
  const uint64_t c = h->count;
  *nrecs = c;
  *nids = h->nids;
  if (c > cap_recs || h->nids > cap_ids) return SG_OK;
  if (c) {
    SG_HIP(hipMemcpyAsync(sigs, h->keys->cur.keys(), c * SG_SIG_BYTES, hipMemcpyDeviceToHost, ctx->stream));
    SG_HIP(hipMemcpyAsync(seqs, h->cur.seq.p, c * 8, hipMemcpyDeviceToHost, ctx->stream));
  }
  SG_HIP(hipMemcpyAsync(call_off, h->cur.call_off.p, (c + 1) * 8, hipMemcpyDeviceToHost, ctx->stream));
  if (h->nids) SG_HIP(hipMemcpyAsync(call_ids, h->cur.ids.p, h->nids * 4, hipMemcpyDeviceToHost, ctx->stream));
  SG_HIP(hipStreamSynchronize(ctx->stream));
  return SG_OK;
}

int sg_hubcorpus_add(sg_hubcorpus* h, sg_sigset* mgr, const uint8_t* bytes, const uint64_t* off, size_t nprogs,
                     const uint64_t* seqs, uint8_t* status, uint8_t* is_new, uint8_t* sigs, uint64_t* unk_pos,
                     uint32_t* unk_len, size_t unk_cap, size_t* nunk) {
  const char* fn = "sg_hubcorpus_add";
  if (!h || !nunk || (nprogs && (!seqs || !status || !is_new)) || (unk_cap && (!unk_pos || !unk_len))) {
    set_error("%s: invalid argument", fn);
    return SG_EINVAL;
  }
  if (foreign(h, mgr)) {
    set_error("%s: the manager's set belongs to another context", fn);
    return SG_EINVAL;
  }
  int rc = prog_texts_ok(fn, bytes, off, nprogs);
  if (rc) return rc;
  if ((rc = call_sets_limits(fn, nprogs, off[nprogs]))) return rc;
  for (size_t k = 0; k < nprogs; k++)
    if (seqs[k] >= SG_HUB_SEQ_LIMIT) {
      set_error("%s: seq %llu of program %llu (the limit is 2^33 - 1)", fn, (unsigned long long)seqs[k],
                (unsigned long long)k);
      return SG_EINVAL;
    }
  if (h->count + nprogs >= kSigsetMaxKeys || (mgr && mgr->count + nprogs >= kSigsetMaxKeys)) {
    set_error("%s: the corpus or the manager's set would reach 2^31 records", fn);
    return SG_EINVAL;
  }
  sg_ctx* ctx = h->ctx;
  std::lock_guard<std::mutex> g(ctx->mu);
  rc = ensure_device(ctx);
  if (rc) return rc;
  *nunk = 0;
  if (nprogs == 0) return SG_OK;
  const uint64_t n = nprogs, nbytes = off[nprogs];
  WsPlan plan;
  const size_t o_bytes = plan.add(nbytes + 4), o_off = plan.add((n + 1) * 8), o_seqs = plan.add(n * 8),
               o_status = plan.add(n), o_line = plan.add((n + 1) * 8), o_keys = plan.add(n * SG_SIG_BYTES + 4),
               o_isnew = plan.add(n), o_upos = plan.add(unk_cap * 8 + 8), o_ulen = plan.add(unk_cap * 4 + 4);
  if ((rc = dstage_reserve(ctx, plan))) return rc;
  if ((rc = ws_reserve(ctx, call_sets_ws(n, nbytes)))) return rc;
  uint8_t* dbytes = dstage_at<uint8_t>(ctx, o_bytes);
  uint64_t* doff = dstage_at<uint64_t>(ctx, o_off);
  uint64_t* dseqs = dstage_at<uint64_t>(ctx, o_seqs);
  uint8_t* dstatus = dstage_at<uint8_t>(ctx, o_status);
  uint64_t* dline = dstage_at<uint64_t>(ctx, o_line);
  uint32_t* dkeys = dstage_at<uint32_t>(ctx, o_keys);
  uint8_t* disnew = dstage_at<uint8_t>(ctx, o_isnew);
  uint64_t* dupos = dstage_at<uint64_t>(ctx, o_upos);
  uint32_t* dulen = dstage_at<uint32_t>(ctx, o_ulen);
  if ((rc = upload(ctx, dbytes, bytes, nbytes))) return rc;
  if ((rc = upload(ctx, doff, off, (n + 1) * 8))) return rc;
  if ((rc = upload(ctx, dseqs, seqs, n * 8))) return rc;
  // the scan's count, then room for exactly its lines, then the spans and the ids
  if ((rc = call_sets_count(ctx, dbytes, doff, n, nbytes, dstatus, dline, 0, true))) return rc;
  uint64_t nl = 0;
  SG_HIP(hipMemcpyAsync(&nl, dline + n, 8, hipMemcpyDeviceToHost, ctx->stream));
  SG_HIP(hipMemcpyAsync(status, dstatus, n, hipMemcpyDeviceToHost, ctx->stream));
  SG_HIP(hipStreamSynchronize(ctx->stream));
  const uint64_t lcap = std::max<uint64_t>(nl, 1);
  if ((rc = rec_reserve(ctx, h->lines, align256(lcap * 8) + 2 * align256(lcap * 4), 0))) return rc;
  uint64_t* lpos = (uint64_t*)h->lines.p;
  uint32_t* llen = (uint32_t*)(h->lines.p + align256(lcap * 8));
  uint32_t* lid = (uint32_t*)(h->lines.p + align256(lcap * 8) + align256(lcap * 4));
  if (nl && (rc = call_sets_emit(ctx, h->tab, dbytes, doff, n, nbytes, dstatus, dline, lpos, llen, lid, nl, 0))) return rc;
  // (the scan's workspace is no longer needed: the plan below may move it)
  WsPlan wp;
  const size_t o_uflag = wp.add(nl * 4 + 4), o_upos2 = wp.add((nl + 1) * 8), o_okflag = wp.add(n * 4),
               o_okpos = wp.add((n + 1) * 8), o_okkeys = wp.add(n * SG_SIG_BYTES + 4), o_newcnt = wp.add(n * 4 + 4),
               o_idpos = wp.add((n + 1) * 8), o_dnew = wp.add(n), o_hash = wp.add(prog_hashes_ws(n)),
               o_add = wp.add(sigset_add_ws(n)), o_scan = wp.add(scan_ws_bytes(std::max(nl, n)));
  if ((rc = ws_reserve(ctx, wp))) return rc;
  uint32_t* uflag = (uint32_t*)ws_at(ctx, o_uflag);
  uint64_t* upos = (uint64_t*)ws_at(ctx, o_upos2);
  uint32_t* okflag = (uint32_t*)ws_at(ctx, o_okflag);
  uint64_t* okpos = (uint64_t*)ws_at(ctx, o_okpos);
  uint32_t* okkeys = (uint32_t*)ws_at(ctx, o_okkeys);
  uint32_t* newcnt = (uint32_t*)ws_at(ctx, o_newcnt);
  uint64_t* idpos = (uint64_t*)ws_at(ctx, o_idpos);
  uint8_t* dnew = (uint8_t*)ws_at(ctx, o_dnew);
  {
    ScopedTimer tm(ctx, "hub_add_flags");
    if (nl) hipLaunchKernelGGL(k_hs_unk_flags, grid_of(nl), dim3(kHT), 0, ctx->stream, (const uint32_t*)lid, nl, uflag);
    hipLaunchKernelGGL(k_hs_ok_flags, grid_of(n), dim3(kHT), 0, ctx->stream, (const uint8_t*)dstatus, n, okflag);
  }
  SG_HIP(hipGetLastError());
  if ((rc = scan_counts(ctx, uflag, upos, nl, o_scan))) return rc;
  if ((rc = scan_counts(ctx, okflag, okpos, n, o_scan))) return rc;
  if (nl && unk_cap) {
    hipLaunchKernelGGL(k_hs_unk_gather, grid_of(nl), dim3(kHT), 0, ctx->stream, (const uint32_t*)uflag,
                       (const uint64_t*)upos, nl, (const uint64_t*)lpos, (const uint32_t*)llen, (uint64_t)unk_cap, dupos,
                       dulen);
    SG_HIP(hipGetLastError());
  }
  uint64_t got[2] = {0, 0};  // unknown names, status-0 programs
  SG_HIP(hipMemcpyAsync(&got[0], upos + nl, 8, hipMemcpyDeviceToHost, ctx->stream));
  SG_HIP(hipMemcpyAsync(&got[1], okpos + n, 8, hipMemcpyDeviceToHost, ctx->stream));
  SG_HIP(hipStreamSynchronize(ctx->stream));
  const uint64_t nu = std::min(got[0], nl), m = std::min(got[1], n);
  *nunk = nu;
  if (nu) {
    const uint64_t w = std::min<uint64_t>(nu, unk_cap);
    if (w) {
      SG_HIP(hipMemcpyAsync(unk_pos, dupos, w * 8, hipMemcpyDeviceToHost, ctx->stream));
      SG_HIP(hipMemcpyAsync(unk_len, dulen, w * 4, hipMemcpyDeviceToHost, ctx->stream));
      SG_HIP(hipStreamSynchronize(ctx->stream));
    }
    return SG_OK;
  }
  if ((rc = prog_hashes(ctx, dbytes, doff, n, nbytes, (uint8_t*)dkeys, o_hash))) return rc;
  if (sigs) SG_HIP(hipMemcpyAsync(sigs, dkeys, n * SG_SIG_BYTES, hipMemcpyDeviceToHost, ctx->stream));
  uint64_t addids = 0;
  const uint64_t old = h->keys->count;
  SG_HIP(hipMemsetAsync(disnew, 0, n, ctx->stream));
  if (m) {
    if ((rc = sigset_gather_dev(ctx, dkeys, n, okflag, okpos, okkeys, m))) return rc;
    size_t o_newpos = 0;
    if (mgr && (rc = sigset_add_dev(mgr, okkeys, m, nullptr, o_add, &o_newpos))) return rc;
    if ((rc = sigset_add_dev(h->keys, okkeys, m, dnew, o_add, &o_newpos))) return rc;
    h->count = h->keys->count;
    const uint32_t* entered = (const uint32_t*)ws_at(ctx, o_add);
    const uint64_t* newpos = (const uint64_t*)ws_at(ctx, o_newpos);
    {
      ScopedTimer tm(ctx, "hub_add_counts");
      hipLaunchKernelGGL(k_hs_new_counts, grid_of(n), dim3(kHT), 0, ctx->stream, (const uint32_t*)okflag,
                         (const uint64_t*)okpos, n, m, entered, (const uint64_t*)dline, disnew, newcnt);
    }
    SG_HIP(hipGetLastError());
    if ((rc = scan_counts(ctx, newcnt, idpos, m, o_scan))) return rc;
    SG_HIP(hipMemcpyAsync(&addids, idpos + m, 8, hipMemcpyDeviceToHost, ctx->stream));
    SG_HIP(hipStreamSynchronize(ctx->stream));
    const uint64_t c = h->count;
    sg_hubcorpus::Half& cur = h->cur;
    if ((rc = rec_reserve(ctx, cur.seq, c, old))) return rc;
    if ((rc = rec_reserve(ctx, cur.call_off, c + 1, old + 1))) return rc;
    if ((rc = rec_reserve(ctx, cur.ids, h->nids + addids, h->nids))) return rc;
    {
      ScopedTimer tm(ctx, "hub_add_append");
      hipLaunchKernelGGL(k_hs_append_recs, grid_of(n), dim3(kHT), 0, ctx->stream, (const uint32_t*)okflag,
                         (const uint64_t*)okpos, n, m, entered, newpos, (const uint64_t*)idpos, (const uint64_t*)dseqs, old,
                         h->nids, cur.seq.p, (uint64_t)cur.seq.cap, cur.call_off.p, (uint64_t)cur.call_off.cap);
      if (nl)
        hipLaunchKernelGGL(k_hs_append_ids, grid_of(nl), dim3(kHT), 0, ctx->stream, (const uint32_t*)okflag,
                           (const uint64_t*)okpos, n, m, entered, (const uint64_t*)idpos, (const uint64_t*)dline, nl,
                           (const uint32_t*)lid, h->nids, cur.ids.p, (uint64_t)cur.ids.cap);
    }
    SG_HIP(hipGetLastError());
    h->nids += addids;
  }
  SG_HIP(hipMemcpyAsync(is_new, disnew, n, hipMemcpyDeviceToHost, ctx->stream));
  SG_HIP(hipStreamSynchronize(ctx->stream));
  return SG_OK;
}

int sg_hubcorpus_pending(sg_hubcorpus* h, sg_sigset* mgr, uint64_t mgr_seq, uint64_t hub_seq, const uint64_t* mask,
                         size_t nwords, uint64_t max_records, uint8_t* sigs, uint64_t* seqs, size_t cap, size_t* n,
                         uint64_t* max_seq, uint64_t* more) {
  const char* fn = "sg_hubcorpus_pending";
  if (!h || !mgr || !n || !max_seq || !more || (nwords && !mask) || (cap && (!sigs || !seqs))) {
    set_error("%s: invalid argument", fn);
    return SG_EINVAL;
  }
  if (foreign(h, mgr)) {
    set_error("%s: the manager's set belongs to another context", fn);
    return SG_EINVAL;
  }
  sg_ctx* ctx = h->ctx;
  std::lock_guard<std::mutex> g(ctx->mu);
  int rc = ensure_device(ctx);
  if (rc) return rc;
  *n = 0;
  *more = 0;
  *max_seq = hub_seq;
  const uint64_t c = h->count;
  if (mgr_seq == hub_seq || c == 0) return SG_OK;
  WsPlan plan;
  const size_t o_mask = plan.add(nwords * 8 + 8), o_sigs = plan.add(c * SG_SIG_BYTES), o_seqs = plan.add(c * 8);
  if ((rc = dstage_reserve(ctx, plan))) return rc;
  WsPlan wp;
  const size_t o_sel = wp.add(c * 4 + 4), o_pos = wp.add((c + 1) * 8), o_ka = wp.add(c * 8), o_kb = wp.add(c * 8),
               o_cut = wp.add(16), o_sort = wp.add(radix_sort_ws(c)), o_scan = wp.add(scan_ws_bytes(c));
  if ((rc = ws_reserve(ctx, wp))) return rc;
  uint64_t* dmask = dstage_at<uint64_t>(ctx, o_mask);
  uint32_t* dsigs = dstage_at<uint32_t>(ctx, o_sigs);
  uint64_t* dseqs = dstage_at<uint64_t>(ctx, o_seqs);
  uint32_t* sel = (uint32_t*)ws_at(ctx, o_sel);
  uint64_t* pos = (uint64_t*)ws_at(ctx, o_pos);
  uint64_t* ka = (uint64_t*)ws_at(ctx, o_ka);
  uint64_t* kb = (uint64_t*)ws_at(ctx, o_kb);
  uint64_t* cut = (uint64_t*)ws_at(ctx, o_cut);
  if ((rc = upload(ctx, dmask, mask, nwords * 8))) return rc;
  if ((rc = sigset_lookup_dev(mgr, h->keys->cur.keys(), c, 0u, sel))) return rc;
  {
    ScopedTimer tm(ctx, "hub_pending_select");
    hipLaunchKernelGGL(k_hs_pending_sel, grid_of(c), dim3(kHT), 0, ctx->stream, sel, c, (const uint64_t*)h->cur.seq.p,
                       mgr_seq, (const uint64_t*)h->cur.call_off.p, (const uint32_t*)h->cur.ids.p, h->nids,
                       (const uint64_t*)dmask, (uint64_t)nwords);
  }
  SG_HIP(hipGetLastError());
  if ((rc = scan_counts(ctx, sel, pos, c, o_scan))) return rc;
  hipLaunchKernelGGL(k_hs_pending_keys, grid_of(c), dim3(kHT), 0, ctx->stream, (const uint32_t*)sel, (const uint64_t*)pos, c,
                     (const uint64_t*)h->cur.seq.p, ka);
  SG_HIP(hipGetLastError());
  uint64_t nsel = 0;
  SG_HIP(hipMemcpyAsync(&nsel, pos + c, 8, hipMemcpyDeviceToHost, ctx->stream));
  SG_HIP(hipStreamSynchronize(ctx->stream));
  nsel = std::min(nsel, c);
  if (nsel == 0) return SG_OK;
  uint64_t* sorted = nullptr;
  {
    ScopedTimer tm(ctx, "hub_pending_sort");
    rc = radix_sort_u64(ctx, ka, kb, nsel, o_sort, &sorted, 0);
  }
  if (rc) return rc;
  uint64_t keep = nsel;
  if (nsel > max_records) {
    uint64_t got[2] = {0, 0};
    hipLaunchKernelGGL(k_hs_cut, dim3(1), dim3(1), 0, ctx->stream, (const uint64_t*)sorted, nsel, max_records, cut);
    SG_HIP(hipGetLastError());
    SG_HIP(hipMemcpyAsync(got, cut, 16, hipMemcpyDeviceToHost, ctx->stream));
    SG_HIP(hipStreamSynchronize(ctx->stream));
    keep = std::min(got[1], nsel);
    *max_seq = got[0];
    *more = nsel - keep;
  }
  *n = keep;
  if (keep > cap) return SG_OK;
  {
    ScopedTimer tm(ctx, "hub_pending_out");
    hipLaunchKernelGGL(k_hs_pending_out, grid_of(keep), dim3(kHT), 0, ctx->stream, (const uint64_t*)sorted, keep,
                       (const uint32_t*)h->keys->cur.keys(), c, dsigs, dseqs);
  }
  SG_HIP(hipGetLastError());
  SG_HIP(hipMemcpyAsync(sigs, dsigs, keep * SG_SIG_BYTES, hipMemcpyDeviceToHost, ctx->stream));
  SG_HIP(hipMemcpyAsync(seqs, dseqs, keep * 8, hipMemcpyDeviceToHost, ctx->stream));
  SG_HIP(hipStreamSynchronize(ctx->stream));
  return SG_OK;
}

int sg_hubcorpus_purge(sg_hubcorpus* h, sg_sigset* const* mgrs, size_t nmgrs, uint8_t* del_sigs, size_t del_cap,
                       size_t* ndel) {
  const char* fn = "sg_hubcorpus_purge";
  if (!h || !ndel || (nmgrs && !mgrs) || (del_cap && !del_sigs)) {
    set_error("%s: invalid argument", fn);
    return SG_EINVAL;
  }
  for (size_t i = 0; i < nmgrs; i++)
    if (!mgrs[i] || foreign(h, mgrs[i])) {
      set_error("%s: manager set %llu is NULL or belongs to another context", fn, (unsigned long long)i);
      return SG_EINVAL;
    }
  if ((uint64_t)del_cap < h->count) {
    set_error("%s: del_cap %llu below the corpus' %llu records", fn, (unsigned long long)del_cap,
              (unsigned long long)h->count);
    return SG_EINVAL;
  }
  sg_ctx* ctx = h->ctx;
  std::lock_guard<std::mutex> g(ctx->mu);
  int rc = ensure_device(ctx);
  if (rc) return rc;
  *ndel = 0;
  const uint64_t c = h->count;
  if (c == 0) return SG_OK;
  WsPlan plan;
  const size_t o_del = plan.add(c * SG_SIG_BYTES);
  if ((rc = dstage_reserve(ctx, plan))) return rc;
  WsPlan wp;
  const size_t o_used = wp.add(c * 4 + 4), o_keeppos = wp.add((c + 1) * 8), o_dead = wp.add(c * 4 + 4),
               o_deadpos = wp.add((c + 1) * 8), o_newcnt = wp.add(c * 4 + 4), o_idpos = wp.add((c + 1) * 8),
               o_scan = wp.add(scan_ws_bytes(c));
  if ((rc = ws_reserve(ctx, wp))) return rc;
  uint32_t* ddel = dstage_at<uint32_t>(ctx, o_del);
  uint32_t* used = (uint32_t*)ws_at(ctx, o_used);
  uint64_t* keeppos = (uint64_t*)ws_at(ctx, o_keeppos);
  uint32_t* dead = (uint32_t*)ws_at(ctx, o_dead);
  uint64_t* deadpos = (uint64_t*)ws_at(ctx, o_deadpos);
  uint32_t* newcnt = (uint32_t*)ws_at(ctx, o_newcnt);
  uint64_t* idpos = (uint64_t*)ws_at(ctx, o_idpos);
  SG_HIP(hipMemsetAsync(used, 0, c * 4 + 4, ctx->stream));
  for (size_t i = 0; i < nmgrs; i++)
    if ((rc = sigset_lookup_or_dev(mgrs[i], h->keys->cur.keys(), c, used))) return rc;
  {
    ScopedTimer tm(ctx, "hub_purge_flags");
    hipLaunchKernelGGL(k_hs_purge_flags, grid_of(c), dim3(kHT), 0, ctx->stream, (const uint32_t*)used, c,
                       (const uint64_t*)h->cur.call_off.p, dead, newcnt);
  }
  SG_HIP(hipGetLastError());
  if ((rc = scan_counts(ctx, used, keeppos, c, o_scan))) return rc;
  if ((rc = scan_counts(ctx, dead, deadpos, c, o_scan))) return rc;
  if ((rc = scan_counts(ctx, newcnt, idpos, c, o_scan))) return rc;
  uint64_t got[3] = {0, 0, 0};  // records kept, records deleted, ids kept
  SG_HIP(hipMemcpyAsync(&got[0], keeppos + c, 8, hipMemcpyDeviceToHost, ctx->stream));
  SG_HIP(hipMemcpyAsync(&got[1], deadpos + c, 8, hipMemcpyDeviceToHost, ctx->stream));
  SG_HIP(hipMemcpyAsync(&got[2], idpos + c, 8, hipMemcpyDeviceToHost, ctx->stream));
  SG_HIP(hipStreamSynchronize(ctx->stream));
  const uint64_t newc = std::min(got[0], c), nd = std::min(got[1], c), newids = std::min(got[2], h->nids);
  if (nd == 0) return SG_OK;
  if ((rc = sigset_gather_dev(ctx, h->keys->cur.keys(), c, dead, deadpos, ddel, c))) return rc;
  SG_HIP(hipMemcpyAsync(del_sigs, ddel, nd * SG_SIG_BYTES, hipMemcpyDeviceToHost, ctx->stream));
  sg_hubcorpus::Half &cur = h->cur, &nx = h->next;
  if ((rc = rec_reserve(ctx, nx.seq, std::max<uint64_t>(newc, 1), 0))) return rc;
  if ((rc = rec_reserve(ctx, nx.call_off, newc + 1, 0))) return rc;
  if ((rc = rec_reserve(ctx, nx.ids, std::max<uint64_t>(newids, 1), 0))) return rc;
  {
    ScopedTimer tm(ctx, "hub_purge_gather");
    hipLaunchKernelGGL(k_hs_purge_recs, grid_of(c), dim3(kHT), 0, ctx->stream, (const uint32_t*)used,
                       (const uint64_t*)keeppos, (const uint64_t*)idpos, c, (const uint64_t*)cur.seq.p, nx.seq.p,
                       (uint64_t)nx.seq.cap, nx.call_off.p, (uint64_t)nx.call_off.cap);
    if (h->nids)
      hipLaunchKernelGGL(k_hs_purge_ids, grid_of(h->nids), dim3(kHT), 0, ctx->stream, (const uint32_t*)used,
                         (const uint64_t*)idpos, c, (const uint64_t*)cur.call_off.p, (const uint32_t*)cur.ids.p, h->nids,
                         nx.ids.p, (uint64_t)nx.ids.cap);
  }
  SG_HIP(hipGetLastError());
  if ((rc = sigset_rebuild_dev(h->keys, used, keeppos, newc))) return rc;  // (waits)
  cur.swap(nx);
  h->count = h->keys->count;
  h->nids = newids;
  *ndel = nd;
  return SG_OK;
}

}  // extern "C"
