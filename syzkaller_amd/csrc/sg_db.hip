// sg_db.hip -- pkg/db's read side (pkg/db/db.go:38-52 Open, :167-249 the
// deserializers) and the hub's loadDB loop (syz-hub/state/state.go:83-110)
// from a database file's bytes.
//
// sg_db_scan is the framing: deserializeHeader and deserializeRecord without
// the inflate, on the host, a few loads per record.  sg_db_open uploads the
// file once and points sg_inflate.hip's passes at the framed values where they
// lie: every stream is counted and validated, the statuses and lengths are
// read back once, the host cuts the database at the first stream that is not
// OK, resolves the keys (last write wins, a deletion removes; a hash table over
// record indices -- host work as sg_nametab's is), zeroes the lengths
// of the streams nobody reads any more, and the write pass inflates the live
// ones into the database's own text buffer, where sg_prog_hashes_dev and
// sg_call_sets_dev take them.  sg_db_verify is those two over the resident
// texts and a 40-byte compare per record on the host.
//
// The write side (:95-116 compact, :132-165 serializeHeader and
// serializeRecord): sg_db_serialize and sg_db_compact point sg_deflate.hip's
// passes at the records' texts (uploaded, or an opened database's resident
// ones), zero the lengths of deletions and empty values, and assemble the file
// on the device: the host sends each record's prefix of bytes that are not
// streams, k_db_frames writes magic, key, seq and val_len a thread per record,
// the write phase puts every stream behind its frame, and one copy brings the
// file back.
#include "sg_internal.h"

#include <algorithm>
#include <cstring>
#include <vector>

struct sg_db {
  sg_ctx* ctx = nullptr;
  // the live records, in file order of their winning write
  std::vector<uint8_t> keys;
  std::vector<uint64_t> key_off{0};
  std::vector<uint64_t> seqs;
  std::vector<uint64_t> text_off{0};
  uint64_t uncompacted = 0;
  int end = 0;
  // the texts (exactly their bytes, at least one) and their offsets on the device
  sg::DevBuf<uint8_t> d_texts;
  sg::DevBuf<uint64_t> d_text_off;
};

namespace sg {
namespace {

constexpr uint32_t kDbMagic = 0xbaddb, kRecMagic = 0xfee1bad, kCurVersion = 1;

struct Rec {
  uint64_t key_pos, seq, val_pos;
  uint32_t key_len, val_len;
};

uint32_t le32(const uint8_t* p) {
  return (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24;
}
uint64_t le64(const uint8_t* p) { return (uint64_t)le32(p) | (uint64_t)le32(p + 4) << 32; }

// deserializeHeader, then deserializeRecord's framing until the file ends or
// a record does not parse.  Every length is compared with what is left of the
// file before anything is read through it.
template <class F>
int db_scan(const uint8_t* b, uint64_t n, F&& rec) {
  if (n == 0) return SG_DB_END_EOF;  // (:196-198: no header is the current version)
  if (n < 4) return SG_DB_END_TRUNCATED;
  if (le32(b) != kDbMagic) return SG_DB_END_MAGIC;
  if (n < 8) return SG_DB_END_TRUNCATED;
  const uint32_t ver = le32(b + 4);
  if (ver == 0 || ver > kCurVersion) return SG_DB_END_VERSION;
  uint64_t pos = 8;
  for (;;) {
    if (pos == n) return SG_DB_END_EOF;
    if (n - pos < 4) return SG_DB_END_TRUNCATED;
    if (le32(b + pos) != kRecMagic) return SG_DB_END_RECORD;
    if (n - pos < 8) return SG_DB_END_TRUNCATED;
    Rec r{};
    r.key_len = le32(b + pos + 4);
    r.key_pos = pos + 8;
    if (n - r.key_pos < (uint64_t)r.key_len + 8) return SG_DB_END_TRUNCATED;
    r.seq = le64(b + r.key_pos + r.key_len);
    pos = r.key_pos + r.key_len + 8;
    if (r.seq != SG_DB_SEQ_DELETED) {
      if (n - pos < 4) return SG_DB_END_TRUNCATED;
      r.val_len = le32(b + pos);
      pos += 4;
      if (n - pos < r.val_len) return SG_DB_END_TRUNCATED;
      r.val_pos = pos;
      pos += r.val_len;  // (whatever the stream inside consumes: the pinned choice)
    }
    rec(r);
  }
}

// ---- the write side: serializeHeader and serializeRecord (:132-165) ----------
// A record's bytes that are not its stream: magic, len(key), key, seq, and the
// value's length unless the record is a deletion.
uint64_t frame_bytes(uint64_t key_len, uint64_t seq) { return 4 + 4 + key_len + 8 + (seq == SG_DB_SEQ_DELETED ? 0 : 4); }

// A deletion and an empty value have no stream: their lengths are zeroed before the scan.
__global__ __launch_bounds__(256) void k_db_mask(const uint64_t* __restrict__ seqs, const uint64_t* __restrict__ text_off,
                                                  uint64_t n, uint32_t* __restrict__ olen) {
  const uint64_t k = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (k >= n) return;
  if (seqs[k] == SG_DB_SEQ_DELETED || text_off[k + 1] <= text_off[k]) olen[k] = 0;
}

__device__ __forceinline__ void put_le(uint8_t* out, uint64_t cap, uint64_t at, uint64_t v, uint32_t nbytes) {
  for (uint32_t j = 0; j < nbytes; j++)
    if (at + j < cap) out[at + j] = (uint8_t)(v >> (8 * j));
}

// Everything of the file but the streams, a thread per record: record k's
// stream starts at shift[k] + soff[k] (shift: the frames before it and its own,
// from the host), so its frame starts frame_bytes before that.  Every store is
// clamped to cap.
__global__ __launch_bounds__(256) void k_db_frames(const uint8_t* __restrict__ keys, const uint64_t* __restrict__ key_off,
                                                    const uint64_t* __restrict__ seqs, const uint64_t* __restrict__ shift,
                                                    const uint64_t* __restrict__ soff, uint64_t n, uint64_t nkeys,
                                                    int with_header, uint8_t* __restrict__ out, uint64_t cap) {
  const uint64_t k = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (k == 0 && with_header) {
    put_le(out, cap, 0, kDbMagic, 4);
    put_le(out, cap, 4, kCurVersion, 4);
  }
  if (k >= n) return;
  uint64_t k0, k1;
  sgd::csr_range(key_off, k, nkeys, k0, k1);
  const uint64_t seq = seqs[k], klen = k1 - k0;
  const bool del = seq == SG_DB_SEQ_DELETED;
  uint64_t at = shift[k] + soff[k] - (4 + 4 + klen + 8 + (del ? 0 : 4));
  put_le(out, cap, at, kRecMagic, 4);
  put_le(out, cap, at + 4, klen, 4);
  at += 8;
  for (uint64_t j = 0; j < klen; j++)
    if (at + j < cap) out[at + j] = keys[k0 + j];
  at += klen;
  put_le(out, cap, at, seq, 8);
  if (!del) put_le(out, cap, at + 8, soff[k + 1] - soff[k], 4);
}

// serializeHeader (with_header) and serializeRecord for n records whose texts
// are on the device already: keys and seqs from the host, the file assembled
// on the device and downloaded once.  ctx lock held, the device ensured, every
// argument checked.
int db_serialize_body(sg_ctx* ctx, const char* fn, const uint8_t* keys, const uint64_t* key_off, const uint64_t* seqs,
                      const uint8_t* d_texts, const uint64_t* d_text_off, uint64_t ntext, uint64_t n,
                      int with_header, uint8_t* out, size_t cap, size_t* nout) {
  const uint64_t head = with_header ? 8 : 0;
  if (n == 0) {
    *nout = head;
    if (head && head <= cap) {
      const uint32_t h[2] = {kDbMagic, kCurVersion};
      memcpy(out, h, 8);
    }
    return SG_OK;
  }
  // shift[k]: where record k's stream would start if no record before it had one
  std::vector<uint64_t> shift(n);
  uint64_t frames = head;
  for (uint64_t k = 0; k < n; k++) {
    frames += frame_bytes(key_off[k + 1] - key_off[k], seqs[k]);
    shift[k] = frames;
  }
  const uint64_t nkeys = key_off[n];
  WsPlan plan;
  const size_t o_keys = plan.add(nkeys + 4), o_koff = plan.add((n + 1) * 8), o_seqs = plan.add(n * 8),
               o_shift = plan.add(n * 8), o_olen = plan.add(n * 4), o_form = plan.add(n), o_soff = plan.add((n + 1) * 8);
  int rc;
  if ((rc = dstage_reserve(ctx, plan))) return rc;
  if ((rc = ws_reserve(ctx, deflate_ws(n)))) return rc;
  uint8_t* dkeys = dstage_at<uint8_t>(ctx, o_keys);
  uint64_t* dkoff = dstage_at<uint64_t>(ctx, o_koff);
  uint64_t* dseqs = dstage_at<uint64_t>(ctx, o_seqs);
  uint64_t* dshift = dstage_at<uint64_t>(ctx, o_shift);
  uint32_t* dolen = dstage_at<uint32_t>(ctx, o_olen);
  uint8_t* dform = dstage_at<uint8_t>(ctx, o_form);
  uint64_t* dsoff = dstage_at<uint64_t>(ctx, o_soff);
  if ((rc = upload(ctx, dkeys, keys, nkeys))) return rc;
  if ((rc = upload(ctx, dkoff, key_off, (n + 1) * 8))) return rc;
  if ((rc = upload(ctx, dseqs, seqs, n * 8))) return rc;
  if ((rc = upload(ctx, dshift, shift.data(), n * 8))) return rc;
  const uint64_t* sorted = nullptr;
  if ((rc = deflate_count(ctx, d_texts, d_text_off, d_text_off + 1, n, ntext, dolen, dform, 0, &sorted))) return rc;
  hipLaunchKernelGGL(k_db_mask, dim3(div_up(n, 256)), dim3(256), 0, ctx->stream, (const uint64_t*)dseqs, d_text_off, n,
                     dolen);
  SG_HIP(hipGetLastError());
  if ((rc = deflate_offsets(ctx, dolen, dsoff, n, 0))) return rc;
  uint64_t streams = 0;
  SG_HIP(hipMemcpyAsync(&streams, dsoff + n, 8, hipMemcpyDeviceToHost, ctx->stream));
  SG_HIP(hipStreamSynchronize(ctx->stream));  // (shift is this call's host memory, too)
  const uint64_t total = frames + streams;
  if (total >= kInflateMaxOut) {
    set_error("%s: a file of %llu bytes (the limit is 2^33 - 1)", fn, (unsigned long long)total);
    return SG_EINVAL;
  }
  *nout = total;
  if (total > cap) return SG_OK;
  if ((rc = ctx->inflate_out.grow_drop(grow_cap(ctx->inflate_out.cap, total, 16u << 20), ctx->stream))) return rc;
  uint8_t* dout = ctx->inflate_out.p;
  {
    ScopedTimer tm(ctx, "db_frames");
    hipLaunchKernelGGL(k_db_frames, dim3(div_up(n, 256)), dim3(256), 0, ctx->stream, (const uint8_t*)dkeys,
                       (const uint64_t*)dkoff, (const uint64_t*)dseqs, (const uint64_t*)dshift, (const uint64_t*)dsoff, n,
                       nkeys, with_header, dout, total);
  }
  SG_HIP(hipGetLastError());
  if ((rc = deflate_write(ctx, d_texts, d_text_off, d_text_off + 1, n, ntext, sorted, dsoff, dshift, frames, dout, total)))
    return rc;
  SG_HIP(hipMemcpyAsync(out, dout, total, hipMemcpyDeviceToHost, ctx->stream));
  SG_HIP(hipStreamSynchronize(ctx->stream));
  return SG_OK;
}

}  // namespace
}  // namespace sg

using namespace sg;

extern "C" {

int sg_db_serialize(sg_ctx* ctx, const uint8_t* keys, const uint64_t* key_off, const uint64_t* seqs, const uint8_t* texts,
                    const uint64_t* text_off, size_t n, int with_header, uint8_t* out, size_t cap, size_t* nout) {
  const char* fn = "sg_db_serialize";
  if (!ctx || !nout || (n && !seqs) || (cap && !out)) {
    set_error("%s: invalid argument", fn);
    return SG_EINVAL;
  }
  int rc = prog_texts_ok(fn, keys, key_off, n);
  if (rc) return rc;
  if ((rc = deflate_texts_ok(fn, texts, text_off, n))) return rc;
  for (size_t k = 0; k < n; k++) {
    if (key_off[k + 1] - key_off[k] >= (1ull << 32)) {
      set_error("%s: record %llu has a key of 2^32 bytes or more", fn, (unsigned long long)k);
      return SG_EINVAL;
    }
    if (seqs[k] == SG_DB_SEQ_DELETED && text_off[k + 1] != text_off[k]) {
      set_error("%s: record %llu is a deletion with a value", fn, (unsigned long long)k);
      return SG_EINVAL;
    }
  }
  std::lock_guard<std::mutex> g(ctx->mu);
  if ((rc = ensure_device(ctx))) return rc;
  const uint64_t ntext = n ? text_off[n] : 0;
  uint8_t* dtexts = nullptr;
  uint64_t* dtoff = nullptr;
  if (n) {  // the texts go to the workspace's tail, behind what the deflate passes take of it
    const size_t o_texts = deflate_ws(n), o_toff = o_texts + align256(ntext + 4);
    if ((rc = ws_reserve(ctx, o_toff + align256((n + 1) * 8)))) return rc;
    dtexts = (uint8_t*)ws_at(ctx, o_texts);
    dtoff = (uint64_t*)ws_at(ctx, o_toff);
    if ((rc = upload(ctx, dtexts, texts, ntext))) return rc;
    if ((rc = upload(ctx, dtoff, text_off, (n + 1) * 8))) return rc;
  }
  return db_serialize_body(ctx, fn, keys, key_off, seqs, dtexts, dtoff, ntext, n, with_header, out, cap, nout);
}

int sg_db_compact(sg_db* db, uint8_t* out, size_t cap, size_t* nout) {
  const char* fn = "sg_db_compact";
  if (!db || !nout || (cap && !out)) {
    set_error("%s: invalid argument", fn);
    return SG_EINVAL;
  }
  const uint64_t n = db->seqs.size();
  for (uint64_t k = 0; k < n; k++)
    if (db->text_off[k + 1] - db->text_off[k] > kDeflateMaxIn) {
      set_error("%s: record %llu has a value of more than 2^32 - 2^20 bytes", fn, (unsigned long long)k);
      return SG_EINVAL;
    }
  sg_ctx* ctx = db->ctx;
  std::lock_guard<std::mutex> g(ctx->mu);
  const int rc = ensure_device(ctx);
  if (rc) return rc;
  return db_serialize_body(ctx, fn, db->keys.data(), db->key_off.data(), db->seqs.data(), db->d_texts.p, db->d_text_off.p,
                           db->text_off.back(), n, 1, out, cap, nout);
}

int sg_db_scan(const uint8_t* bytes, size_t nbytes, uint64_t* key_pos, uint32_t* key_len, uint64_t* seq,
               uint64_t* val_pos, uint32_t* val_len, size_t cap, size_t* nrec, int* end) {
  if (!nrec || !end || (nbytes && !bytes) || (cap && (!key_pos || !key_len || !seq || !val_pos || !val_len))) {
    set_error("sg_db_scan: invalid argument");
    return SG_EINVAL;
  }
  size_t n = 0;
  *end = db_scan(bytes, nbytes, [&](const Rec&) { n++; });
  *nrec = n;
  if (n == 0 || n > cap) return SG_OK;
  size_t k = 0;
  db_scan(bytes, nbytes, [&](const Rec& r) {
    key_pos[k] = r.key_pos;
    key_len[k] = r.key_len;
    seq[k] = r.seq;
    val_pos[k] = r.val_pos;
    val_len[k] = r.val_len;
    k++;
  });
  return SG_OK;
}

int sg_db_open(sg_ctx* ctx, const uint8_t* bytes, size_t nbytes, sg_db** out) {
  const char* fn = "sg_db_open";
  if (!ctx || !out || (nbytes && !bytes)) {
    set_error("%s: invalid argument", fn);
    return SG_EINVAL;
  }
  *out = nullptr;
  std::vector<Rec> recs;
  const int end = db_scan(bytes, nbytes, [&](const Rec& r) { recs.push_back(r); });
  if (recs.size() >= (1ull << 32)) {
    set_error("%s: %llu records (the limit is 2^32 - 1)", fn, (unsigned long long)recs.size());
    return SG_EINVAL;
  }
  // the framed streams, in file order
  std::vector<uint64_t> ends;  // [beg ... | end ...]
  std::vector<uint32_t> stream_of(recs.size(), 0xFFFFFFFFu);
  uint64_t ns = 0;
  for (size_t k = 0; k < recs.size(); k++)
    if (recs[k].seq != SG_DB_SEQ_DELETED && recs[k].val_len) stream_of[k] = (uint32_t)ns++;
  ends.resize(2 * ns);
  for (size_t k = 0; k < recs.size(); k++)
    if (stream_of[k] != 0xFFFFFFFFu) {
      ends[stream_of[k]] = recs[k].val_pos;
      ends[ns + stream_of[k]] = recs[k].val_pos + recs[k].val_len;
    }
  std::lock_guard<std::mutex> g(ctx->mu);
  int rc = ensure_device(ctx);
  if (rc) return rc;
  sg_db* db = new sg_db();
  db->ctx = ctx;
  db->end = end;
  struct Drop {  // a failed open: wait for the copies in flight out of this call's host memory, then let go
    sg_db*& d;
    hipStream_t stream;
    ~Drop() {
      if (!d) return;
      hipStreamSynchronize(stream);
      delete d;
    }
  };
  sg_db* owned = db;
  Drop drop{owned, ctx->stream};
  std::vector<uint8_t> status(ns);
  std::vector<uint32_t> olen(ns);
  WsPlan plan;
  const size_t o_in = plan.add(nbytes + 4), o_ends = plan.add(2 * ns * 8 + 8), o_status = plan.add(ns + 1),
               o_cons = plan.add(ns * 8 + 8), o_olen = plan.add(ns * 4 + 4), o_oo = plan.add((ns + 1) * 8);
  uint8_t* din = nullptr;
  uint64_t* dends = nullptr;
  uint8_t* dstatus = nullptr;
  uint32_t* dolen = nullptr;
  uint64_t* doo = nullptr;
  const uint64_t* sorted = nullptr;
  if (ns) {
    if ((rc = dstage_reserve(ctx, plan))) return rc;
    if ((rc = ws_reserve(ctx, inflate_ws(ns)))) return rc;
    din = dstage_at<uint8_t>(ctx, o_in);
    dends = dstage_at<uint64_t>(ctx, o_ends);
    dstatus = dstage_at<uint8_t>(ctx, o_status);
    dolen = dstage_at<uint32_t>(ctx, o_olen);
    doo = dstage_at<uint64_t>(ctx, o_oo);
    if ((rc = upload(ctx, din, bytes, nbytes))) return rc;
    if ((rc = upload(ctx, dends, ends.data(), 2 * ns * 8))) return rc;
    if ((rc = inflate_count(ctx, din, dends, dends + ns, ns, nbytes, dstatus, dstage_at<uint64_t>(ctx, o_cons), dolen, 0,
                            &sorted)))
      return rc;
    SG_HIP(hipMemcpyAsync(status.data(), dstatus, ns, hipMemcpyDeviceToHost, ctx->stream));
    SG_HIP(hipMemcpyAsync(olen.data(), dolen, ns * 4, hipMemcpyDeviceToHost, ctx->stream));
    SG_HIP(hipStreamSynchronize(ctx->stream));
  }
  // deserializeDB's loop (:175-190): the first error ends it; the last write of a key wins.  The map is open
  // addressing over record indices, at most half of the slots used, a key compared where it lies in the file:
  // a slot holds the latest record of its key, a deletion included, so nothing is ever removed from it.
  size_t nslots = 16;
  while (nslots < 2 * recs.size()) nslots <<= 1;
  std::vector<uint32_t> slots(nslots, 0xFFFFFFFFu);
  uint64_t parsed = 0;
  for (; parsed < recs.size(); parsed++) {
    const Rec& r = recs[parsed];
    if (stream_of[parsed] != 0xFFFFFFFFu && status[stream_of[parsed]] != SG_INFLATE_OK) {
      db->end = SG_DB_END_VALUE;
      break;
    }
    uint64_t h = SG_FNV64_OFFSET;
    for (uint32_t j = 0; j < r.key_len; j++) h = (h ^ bytes[r.key_pos + j]) * SG_FNV64_PRIME;
    size_t s = (size_t)h & (nslots - 1);
    for (; slots[s] != 0xFFFFFFFFu; s = (s + 1) & (nslots - 1)) {
      const Rec& q = recs[slots[s]];
      if (q.key_len == r.key_len && (r.key_len == 0 || !memcmp(bytes + q.key_pos, bytes + r.key_pos, r.key_len))) break;
    }
    slots[s] = (uint32_t)parsed;
  }
  db->uncompacted = parsed;
  std::vector<uint8_t> live(parsed, 0);
  for (const uint32_t s : slots)
    if (s != 0xFFFFFFFFu && recs[s].seq != SG_DB_SEQ_DELETED) live[s] = 1;
  uint64_t total = 0;
  for (uint64_t k = 0; k < recs.size(); k++) {
    const bool keep = k < parsed && live[k];
    const uint32_t s = stream_of[k];
    if (s != 0xFFFFFFFFu && !keep) olen[s] = 0;  // a stream nobody reads: no span, no second decode
    if (!keep) continue;
    const Rec& r = recs[k];
    db->keys.insert(db->keys.end(), bytes + r.key_pos, bytes + r.key_pos + r.key_len);
    db->key_off.push_back(db->keys.size());
    db->seqs.push_back(r.seq);
    total += s != 0xFFFFFFFFu ? olen[s] : 0;
    db->text_off.push_back(total);
  }
  if (total >= kInflateMaxOut) {
    set_error("%s: %llu bytes of text (the limit is 2^33 - 1)", fn, (unsigned long long)total);
    return SG_EINVAL;
  }
  const uint64_t nlive = db->seqs.size();
  if ((rc = db->d_texts.grow_drop(total + 1, ctx->stream))) return rc;
  if ((rc = db->d_text_off.grow_drop(nlive + 1, ctx->stream))) return rc;
  if ((rc = upload(ctx, db->d_text_off.p, db->text_off.data(), (nlive + 1) * 8))) return rc;
  if (ns && total) {
    if ((rc = upload(ctx, dolen, olen.data(), ns * 4))) return rc;
    if ((rc = inflate_offsets(ctx, dolen, doo, ns, 0))) return rc;
    if ((rc = inflate_write(ctx, din, dends, dends + ns, ns, nbytes, sorted, dstatus, doo, db->d_texts.p, total)))
      return rc;
  }
  SG_HIP(hipStreamSynchronize(ctx->stream));  // (text_off and olen are this call's host memory)
  owned = nullptr;
  *out = db;
  return SG_OK;
}

void sg_db_destroy(sg_db* db) {
  if (!db) return;
  {
    std::lock_guard<std::mutex> g(db->ctx->mu);
    hipSetDevice(db->ctx->device);
    hipStreamSynchronize(db->ctx->stream);
  }
  delete db;
}

int sg_db_counts(sg_db* db, uint64_t counts[5]) {
  if (!db || !counts) {
    set_error("sg_db_counts: invalid argument");
    return SG_EINVAL;
  }
  counts[0] = db->seqs.size();
  counts[1] = db->uncompacted;
  counts[2] = db->text_off.back();
  counts[3] = db->keys.size();
  counts[4] = (uint64_t)db->end;
  return SG_OK;
}

int sg_db_export(sg_db* db, uint64_t* key_off, uint8_t* keys, uint64_t* seqs, uint64_t* text_off, uint8_t* texts) {
  if (!db) {
    set_error("sg_db_export: invalid argument");
    return SG_EINVAL;
  }
  const size_t n = db->seqs.size();
  if (key_off) memcpy(key_off, db->key_off.data(), (n + 1) * 8);
  if (keys && !db->keys.empty()) memcpy(keys, db->keys.data(), db->keys.size());
  if (seqs && n) memcpy(seqs, db->seqs.data(), n * 8);
  if (!text_off && !texts) return SG_OK;
  sg_ctx* ctx = db->ctx;
  std::lock_guard<std::mutex> g(ctx->mu);
  const int rc = ensure_device(ctx);
  if (rc) return rc;
  if (text_off) SG_HIP(hipMemcpyAsync(text_off, db->d_text_off.p, (n + 1) * 8, hipMemcpyDeviceToHost, ctx->stream));
  if (texts && db->text_off.back())
    SG_HIP(hipMemcpyAsync(texts, db->d_texts.p, db->text_off.back(), hipMemcpyDeviceToHost, ctx->stream));
  SG_HIP(hipStreamSynchronize(ctx->stream));
  return SG_OK;
}

int sg_db_device(sg_db* db, const uint8_t** d_texts, const uint64_t** d_text_off) {
  if (!db || !d_texts || !d_text_off) {
    set_error("sg_db_device: invalid argument");
    return SG_EINVAL;
  }
  *d_texts = db->d_texts.p;
  *d_text_off = db->d_text_off.p;
  return SG_OK;
}

int sg_db_verify(sg_db* db, sg_nametab* tab, uint8_t* bad, uint64_t* max_seq) {
  const char* fn = "sg_db_verify";
  if (!db || !max_seq || (!db->seqs.empty() && !bad)) {
    set_error("%s: invalid argument", fn);
    return SG_EINVAL;
  }
  sg_ctx* ctx = db->ctx;
  if (tab && nametab_ctx(tab) != ctx) {
    set_error("%s: the name table belongs to another context", fn);
    return SG_EINVAL;
  }
  const uint64_t n = db->seqs.size(), nbytes = db->text_off.back();
  int rc = call_sets_limits(fn, n, nbytes);
  if (rc) return rc;
  *max_seq = 0;
  if (n == 0) return SG_OK;
  std::lock_guard<std::mutex> g(ctx->mu);
  if ((rc = ensure_device(ctx))) return rc;
  WsPlan plan;
  const size_t o_status = plan.add(n), o_line = plan.add((n + 1) * 8), o_sigs = plan.add(n * SG_SIG_BYTES);
  if ((rc = dstage_reserve(ctx, plan))) return rc;
  if ((rc = ws_reserve(ctx, std::max(call_sets_ws(n, nbytes), prog_hashes_ws(n))))) return rc;
  uint8_t* dstatus = dstage_at<uint8_t>(ctx, o_status);
  uint8_t* dsigs = dstage_at<uint8_t>(ctx, o_sigs);
  // (the offsets are this library's own: they start at 0 and do not decrease)
  if ((rc = call_sets_count(ctx, db->d_texts.p, db->d_text_off.p, n, nbytes, dstatus, dstage_at<uint64_t>(ctx, o_line), 0,
                            true)))
    return rc;
  if ((rc = prog_hashes(ctx, db->d_texts.p, db->d_text_off.p, n, nbytes, dsigs, 0))) return rc;
  std::vector<uint8_t> sigs(n * SG_SIG_BYTES);
  SG_HIP(hipMemcpyAsync(bad, dstatus, n, hipMemcpyDeviceToHost, ctx->stream));
  SG_HIP(hipMemcpyAsync(sigs.data(), dsigs, sigs.size(), hipMemcpyDeviceToHost, ctx->stream));
  SG_HIP(hipStreamSynchronize(ctx->stream));
  static const char digits[] = "0123456789abcdef";
  for (uint64_t k = 0; k < n; k++) {
    if (bad[k]) {
      bad[k] = 1;
      continue;
    }
    const uint8_t* key = db->keys.data() + db->key_off[k];
    bool same = db->key_off[k + 1] - db->key_off[k] == 2 * SG_SIG_BYTES;
    for (uint32_t j = 0; same && j < SG_SIG_BYTES; j++) {
      const uint8_t h = sigs[k * SG_SIG_BYTES + j];
      same = key[2 * j] == (uint8_t)digits[h >> 4] && key[2 * j + 1] == (uint8_t)digits[h & 15];
    }
    if (!same)
      bad[k] = 2;
    else if (*max_seq < db->seqs[k])
      *max_seq = db->seqs[k];
  }
  return SG_OK;
}

}  // extern "C"
