// sg_prog_hash.hip -- pkg/hash on the GPU: SHA-1 (FIPS 180-4) of every program
// of a corpus (syz-manager/manager.go:777-781, :913, :1021-1025, :1053-1056;
// syz-fuzzer/fuzzer.go:480-484; syz-hub/state/state.go:91-101).
//
// SHA-1 is a serial chain of 80 rounds per 64-byte block, so the parallelism
// is across programs: a lane per program.
//
//  1. k_sha1_keys: a key per program, (class << 32) | program, class =
//     kMaxBlocks - its 64-byte blocks (padding included), kLongClass for a
//     program longer than SG_SHA1_LONG bytes.
//  2. radix_sort_u64 on the 11 class bits (two passes, stable): longest first,
//     the long programs last.  A wave takes 64 neighbours of that order, so its
//     lanes differ by at most the step between two neighbouring classes and
//     the wave that runs longest starts first.
//  3. k_sha1_short, a wave per 64 keys.  Per round r the wave stages block r of
//     each of its programs in LDS: 17 aligned dwords a program (a block starts
//     at any byte address).  In each of 16 steps 16 neighbouring lanes read
//     the first 16 dwords of one row, 64 contiguous bytes; a 17th step reads
//     every row's last dword.  All 17 loads are in flight together.  Only the
//     dwords that hold bytes of the program are read, and a dword that
//     straddles an end of the buffer is put together from its bytes inside.
//     Row stride 17 dwords: lanes l, l + 1 read banks 17 apart, and 17 is odd,
//     so the 32 lanes of a ds_read_b32 group hit 32 different banks; a write
//     step's 32 lanes cover two rows, banks 17 g + 0..15 and 17 g + 17..32:
//     32 different banks too.  Each lane funnel-shifts its row (v_alignbyte),
//     swaps to big-endian words, masks what lies past the message, sets the
//     0x80 byte and, in its last block, the 64-bit bit count (a full block
//     skips all of that), and runs the 80 rounds with the schedule in 16
//     registers.
//  4. k_sha1_long, a wave per long program, of any length: 64 consecutive
//     blocks are staged the same way, then compressed one after the other.
//     It keeps a 1 MiB program from holding 63 other programs' lanes; it is
//     there for correctness at any length, not for speed.
//  5. k_sha1_count: the long programs are the sorted keys' tail; one thread
//     finds where it starts and adds its length to "sha1_long_progs".
//
// No float, no atomics.
#include "sg_internal.h"

#include <algorithm>

namespace sg {
namespace {

constexpr uint32_t kMaxBlocks = (kSha1Long + 8) / 64 + 1;  // blocks of the longest short program
constexpr uint32_t kLongClass = 2047;
static_assert(kMaxBlocks < kLongClass, "the class field holds 11 bits");
constexpr uint64_t kClassBits = 0x7FFull << 32;
constexpr uint32_t kRowDw = 17;  // aligned dwords that hold 64 bytes at any alignment
constexpr uint32_t kHT = 64;     // one wave per workgroup: its LDS rows are its own

struct HashArgs {
  const uint8_t* base;  // bytes, aligned down to a dword
  uint64_t lo, hi;      // the buffer is base[lo, hi)
  const uint64_t* off;
  uint64_t nprogs, nbytes;
  const uint64_t* keys;  // sorted
  const uint32_t* safe;  // a dword that may always be read
  uint8_t* sigs;
};

// program p's bytes, clamped to the buffer: base[beg, beg + len)
__device__ __forceinline__ void text_range(const HashArgs& a, uint64_t p, uint64_t& beg, uint64_t& len) {
  uint64_t a0, a1;
  sgd::csr_range(a.off, p, a.nbytes, a0, a1);
  beg = a.lo + a0;
  len = a1 - a0;
}

__device__ __forceinline__ uint64_t sha1_blocks(uint64_t len) { return (len + 8) / 64 + 1; }

__global__ __launch_bounds__(256) void k_sha1_keys(const uint64_t* __restrict__ off, uint64_t nprogs, uint64_t nbytes,
                                                    uint64_t* __restrict__ keys) {
  const uint64_t p = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (p >= nprogs) return;
  uint64_t a0, a1;
  sgd::csr_range(off, p, nbytes, a0, a1);
  const uint64_t len = a1 - a0;
  const uint32_t cls = len > kSha1Long ? kLongClass : kMaxBlocks - (uint32_t)sha1_blocks(len);
  keys[p] = ((uint64_t)cls << 32) | p;
}

// The wave's rows: lane l asks for base[beg, beg + n), n <= 64, by writing s_q[l], the first aligned dword of
// that range, and s_w[l], the dwords that hold bytes of it (0..17).  load_rows makes rows[17 * l + j] dword
// s_q[l] + j, zero from s_w[l] on.
__device__ __forceinline__ void row_ask(uint64_t beg, uint32_t n, uint64_t* s_q, uint32_t* s_w, uint32_t lane) {
  s_q[lane] = beg >> 2;
  s_w[lane] = n ? (((uint32_t)beg & 3) + n + 3) >> 2 : 0;
}

// Step it < 16: lane l reads dword l % 16 of row 4 * it + l / 16, so 16 neighbouring lanes read 64 contiguous
// bytes; step 16: lane l reads dword 16 of row l.  The 17 loads are issued together; a row dword not wanted, or
// not wholly inside the buffer, reads a.safe instead, and the few of the second kind are then put together
// from their bytes inside.
__device__ __forceinline__ uint32_t edge_dword(const HashArgs& a, uint64_t q) {
  uint32_t e = 0;
  for (uint32_t t = 0; t < 4; t++)
    if (4 * q + t >= a.lo && 4 * q + t < a.hi) e |= (uint32_t)a.base[4 * q + t] << (8 * t);
  return e;
}

__device__ __forceinline__ void load_rows(const HashArgs& a, const uint64_t* s_q, const uint32_t* s_w, uint32_t* rows,
                                          uint32_t lane) {
  const uint64_t qlo = (a.lo + 3) >> 2, qhi = a.hi >> 2;  // the dwords wholly inside the buffer
  const uint32_t* words = reinterpret_cast<const uint32_t*>(a.base);
  const uint32_t sub = lane >> 4, j16 = lane & 15;
  uint32_t v[kRowDw];
  bool edge = false;
#pragma unroll
  for (uint32_t it = 0; it < kRowDw; it++) {
    const uint32_t p = it < 16 ? it * 4 + sub : lane, j = it < 16 ? j16 : 16;
    const bool need = j < s_w[p];
    const uint64_t q = s_q[p] + j;
    const bool whole = need && q >= qlo && q < qhi;
    edge = edge || (need && !whole);
    const uint32_t got = *(whole ? words + q : a.safe);
    v[it] = whole ? got : 0u;
  }
#pragma unroll
  for (uint32_t it = 0; it < kRowDw; it++) {
    const uint32_t p = it < 16 ? it * 4 + sub : lane, j = it < 16 ? j16 : 16;
    rows[p * kRowDw + j] = v[it];
  }
  if (edge) {
#pragma unroll 1
    for (uint32_t it = 0; it < kRowDw; it++) {
      const uint32_t p = it < 16 ? it * 4 + sub : lane, j = it < 16 ? j16 : 16;
      const uint64_t q = s_q[p] + j;
      if (j < s_w[p] && !(q >= qlo && q < qhi)) rows[p * kRowDw + j] = edge_dword(a, q);
    }
  }
}

// The 16 big-endian words of one block from its row: m message bytes (0..64),
// the 0x80 byte at m when mark, the bit count in the last block.
__device__ __forceinline__ void block_words(const uint32_t* row, uint32_t sh, uint32_t m, bool mark, bool last,
                                            uint64_t bits, uint32_t W[16]) {
  if (m == 64) {  // a full block (never the last one: that holds the 0x80 byte and the count): nothing to mask
#pragma unroll
    for (int j = 0; j < 16; j++) W[j] = __builtin_bswap32(__builtin_amdgcn_alignbyte(row[j + 1], row[j], sh));
    return;
  }
#pragma unroll
  for (int j = 0; j < 16; j++) {
    uint32_t w = __builtin_bswap32(__builtin_amdgcn_alignbyte(row[j + 1], row[j], sh));
    const int nv = (int)m - 4 * j;  // message bytes of this word
    w &= nv >= 4 ? 0xFFFFFFFFu : nv <= 0 ? 0u : ~(0xFFFFFFFFu >> (8 * nv));
    if (mark && (int)(m >> 2) == j) w |= 0x80u << (8 * (3 - (m & 3)));
    W[j] = w;
  }
  if (last) {
    W[14] = (uint32_t)(bits >> 32);
    W[15] = (uint32_t)bits;
  }
}

__device__ __forceinline__ uint32_t rotl(uint32_t x, int s) { return (x << s) | (x >> (32 - s)); }

__device__ __forceinline__ void sha1_block(uint32_t h[5], uint32_t W[16]) {
  uint32_t a = h[0], b = h[1], c = h[2], d = h[3], e = h[4];
#pragma unroll
  for (int t = 0; t < 80; t++) {
    uint32_t w;
    if (t < 16) {
      w = W[t];
    } else {
      w = rotl(W[(t - 3) & 15] ^ W[(t - 8) & 15] ^ W[(t - 14) & 15] ^ W[t & 15], 1);
      W[t & 15] = w;
    }
    uint32_t f, k;
    if (t < 20) {
      f = (b & c) | (~b & d);
      k = 0x5A827999u;
    } else if (t < 40) {
      f = b ^ c ^ d;
      k = 0x6ED9EBA1u;
    } else if (t < 60) {
      f = (b & c) | (b & d) | (c & d);
      k = 0x8F1BBCDCu;
    } else {
      f = b ^ c ^ d;
      k = 0xCA62C1D6u;
    }
    const uint32_t tmp = rotl(a, 5) + f + e + k + w;
    e = d;
    d = c;
    c = rotl(b, 30);
    b = a;
    a = tmp;
  }
  h[0] += a;
  h[1] += b;
  h[2] += c;
  h[3] += d;
  h[4] += e;
}

__device__ __forceinline__ void sha1_init(uint32_t h[5]) {
  h[0] = 0x67452301u;
  h[1] = 0xEFCDAB89u;
  h[2] = 0x98BADCFEu;
  h[3] = 0x10325476u;
  h[4] = 0xC3D2E1F0u;
}

// block r of a message of len bytes in nb blocks: what block_words needs
__device__ __forceinline__ void block_shape(uint64_t len, uint64_t nb, uint64_t r, uint32_t& m, bool& mark, bool& last) {
  const uint64_t done = r * 64;
  m = done >= len ? 0u : (uint32_t)min<uint64_t>(len - done, 64);
  mark = done <= len && len - done < 64;
  last = r + 1 == nb;
}

__device__ __forceinline__ void store_sig(uint8_t* sigs, uint64_t p, const uint32_t h[5]) {
  uint8_t* o = sigs + 20 * p;
  if (((uintptr_t)o & 3) == 0) {
#pragma unroll
    for (int i = 0; i < 5; i++) reinterpret_cast<uint32_t*>(o)[i] = __builtin_bswap32(h[i]);
  } else {
#pragma unroll
    for (int i = 0; i < 20; i++) o[i] = (uint8_t)(h[i >> 2] >> (8 * (3 - (i & 3))));
  }
}

__global__ __launch_bounds__(kHT) void k_sha1_short(HashArgs a) {
  __shared__ uint64_t s_q[64];
  __shared__ uint32_t s_w[64];
  __shared__ uint32_t rows[64 * kRowDw];
  const uint32_t lane = threadIdx.x;
  const uint64_t i = (uint64_t)blockIdx.x * 64 + lane;
  bool have = i < a.nprogs;
  uint64_t p = 0, beg = 0, len = 0;
  if (have) {
    const uint64_t key = a.keys[i];
    p = key & 0xFFFFFFFFull;
    have = (uint32_t)(key >> 32) != kLongClass && p < a.nprogs;
  }
  if (have) text_range(a, p, beg, len);
  have = have && len <= kSha1Long;
  const uint32_t nb = have ? (uint32_t)sha1_blocks(len) : 0;
  uint32_t maxnb = nb;
  for (int m = 32; m; m >>= 1) maxnb = max(maxnb, (uint32_t)__shfl_xor((int)maxnb, m));
  const uint32_t sh = (uint32_t)beg & 3;
  uint32_t h[5];
  sha1_init(h);
  for (uint32_t r = 0; r < maxnb; r++) {  // (maxnb is the wave's: the barriers are uniform)
    uint32_t m = 0;
    bool mark = false, last = false;
    if (r < nb) block_shape(len, nb, r, m, mark, last);
    row_ask(beg + (uint64_t)r * 64, m, s_q, s_w, lane);
    __syncthreads();
    load_rows(a, s_q, s_w, rows, lane);
    __syncthreads();
    if (r < nb) {
      uint32_t W[16];
      block_words(rows + lane * kRowDw, sh, m, mark, last, len * 8, W);
      sha1_block(h, W);
    }
  }
  if (have) store_sig(a.sigs, p, h);
}

__global__ __launch_bounds__(kHT) void k_sha1_long(HashArgs a) {
  __shared__ uint64_t s_q[64];
  __shared__ uint32_t s_w[64];
  __shared__ uint32_t rows[64 * kRowDw];
  const uint32_t lane = threadIdx.x;
  if (blockIdx.x >= a.nprogs) return;
  const uint64_t key = a.keys[a.nprogs - 1 - blockIdx.x];
  const uint64_t p = key & 0xFFFFFFFFull;
  if ((uint32_t)(key >> 32) != kLongClass || p >= a.nprogs) return;  // (the whole wave)
  uint64_t beg, len;
  text_range(a, p, beg, len);
  const uint64_t nb = sha1_blocks(len);
  const uint32_t sh = (uint32_t)beg & 3;
  uint32_t h[5];
  sha1_init(h);
  for (uint64_t r0 = 0; r0 < nb; r0 += 64) {
    const uint64_t r = r0 + lane;
    uint32_t m = 0;
    bool mark = false, last = false;
    if (r < nb) block_shape(len, nb, r, m, mark, last);
    row_ask(beg + r * 64, m, s_q, s_w, lane);
    __syncthreads();
    load_rows(a, s_q, s_w, rows, lane);
    __syncthreads();
    const uint32_t cnt = (uint32_t)min<uint64_t>(64, nb - r0);
#pragma unroll 1
    for (uint32_t k = 0; k < cnt; k++) {  // every lane the same block: the reads are LDS broadcasts
      block_shape(len, nb, r0 + k, m, mark, last);
      uint32_t W[16];
      block_words(rows + k * kRowDw, sh, m, mark, last, len * 8, W);
      sha1_block(h, W);
    }
    __syncthreads();
  }
  if (lane == 0) store_sig(a.sigs, p, h);
}

__global__ void k_sha1_count(const uint64_t* __restrict__ keys, uint64_t n, unsigned long long* __restrict__ ctr) {
  uint64_t lo = 0, hi = n;  // the first key of the long class
  while (lo < hi) {
    const uint64_t mid = lo + (hi - lo) / 2;
    if ((uint32_t)(keys[mid] >> 32) >= kLongClass)
      hi = mid;
    else
      lo = mid + 1;
  }
  *ctr += n - lo;  // (stream-ordered: one thread, one writer)
}

}  // namespace

size_t prog_hashes_ws(uint64_t nprogs) { return 2 * align256(nprogs * 8) + radix_sort_ws(nprogs); }

int prog_hashes(sg_ctx* ctx, const uint8_t* d_bytes, const uint64_t* d_off, uint64_t nprogs, uint64_t nbytes,
                uint8_t* d_sigs, size_t ws_used) {
  if (nprogs == 0) return SG_OK;
  uint64_t* ka = (uint64_t*)ws_at(ctx, ws_used);
  uint64_t* kb = (uint64_t*)ws_at(ctx, ws_used + align256(nprogs * 8));
  {
    ScopedTimer tm(ctx, "sha1_keys");
    hipLaunchKernelGGL(k_sha1_keys, dim3(div_up(nprogs, 256)), dim3(256), 0, ctx->stream, d_off, nprogs, nbytes, ka);
  }
  SG_HIP(hipGetLastError());
  uint64_t* sorted = nullptr;
  int rc;
  {
    ScopedTimer tm(ctx, "sha1_sort");  // (its scans are timed as "scan" as well)
    rc = radix_sort_u64(ctx, ka, kb, nprogs, ws_used + 2 * align256(nprogs * 8), &sorted, kClassBits);
  }
  if (rc) return rc;
  const uint64_t mis = (uintptr_t)d_bytes & 3;
  const HashArgs a{d_bytes - mis, mis, mis + nbytes, d_off, nprogs, nbytes, sorted, (const uint32_t*)sorted, d_sigs};
  {
    ScopedTimer tm(ctx, "sha1_short");
    hipLaunchKernelGGL(k_sha1_short, dim3(div_up(nprogs, 64)), dim3(kHT), 0, ctx->stream, a);
  }
  SG_HIP(hipGetLastError());
  const uint64_t nlong_max = std::min<uint64_t>(nprogs, nbytes / ((uint64_t)kSha1Long + 1));
  if (nlong_max) {
    ScopedTimer tm(ctx, "sha1_long");
    hipLaunchKernelGGL(k_sha1_long, dim3((uint32_t)nlong_max), dim3(kHT), 0, ctx->stream, a);
  }
  hipLaunchKernelGGL(k_sha1_count, dim3(1), dim3(1), 0, ctx->stream, (const uint64_t*)sorted, nprogs,
                     (unsigned long long*)&ctx->dev.p->sha1_long_progs);
  SG_HIP(hipGetLastError());
  return SG_OK;
}

int prog_texts_ok(const char* fn, const uint8_t* bytes, const uint64_t* off, size_t nprogs) {
  if (!off) {
    set_error("%s: invalid argument", fn);
    return SG_EINVAL;
  }
  if ((uint64_t)nprogs >= (1ull << 32)) {
    set_error("%s: %llu programs (the limit is 2^32 - 1)", fn, (unsigned long long)nprogs);
    return SG_EINVAL;
  }
  if (!offsets_ok(off, nprogs)) {
    set_error("%s: offsets start at 0 and do not decrease", fn);
    return SG_EINVAL;
  }
  if (off[nprogs] && !bytes) {
    set_error("%s: invalid argument", fn);
    return SG_EINVAL;
  }
  return SG_OK;
}

}  // namespace sg

using namespace sg;

extern "C" {

int sg_prog_hashes_dev(sg_ctx* ctx, const uint8_t* d_bytes, const uint64_t* d_off, uint64_t nprogs, uint64_t nbytes,
                       uint8_t* d_sigs) {
  const char* fn = "sg_prog_hashes_dev";
  if (!ctx || (nprogs && (!d_off || !d_sigs)) || (nbytes && !d_bytes)) {
    set_error("%s: invalid argument", fn);
    return SG_EINVAL;
  }
  if (nprogs >= (1ull << 32)) {
    set_error("%s: %llu programs (the limit is 2^32 - 1)", fn, (unsigned long long)nprogs);
    return SG_EINVAL;
  }
  std::lock_guard<std::mutex> g(ctx->mu);
  int rc = ensure_device(ctx);
  if (rc) return rc;
  if (nprogs == 0) return SG_OK;
  if ((rc = ws_reserve(ctx, prog_hashes_ws(nprogs)))) return rc;
  return prog_hashes(ctx, d_bytes, d_off, nprogs, nbytes, d_sigs, 0);
}

int sg_prog_hashes(sg_ctx* ctx, const uint8_t* bytes, const uint64_t* off, size_t nprogs, uint8_t* sigs, char* hex) {
  const char* fn = "sg_prog_hashes";
  if (!ctx) {
    set_error("%s: invalid argument", fn);
    return SG_EINVAL;
  }
  int rc = prog_texts_ok(fn, bytes, off, nprogs);
  if (rc) return rc;
  std::lock_guard<std::mutex> g(ctx->mu);
  rc = ensure_device(ctx);
  if (rc) return rc;
  if (nprogs == 0 || (!sigs && !hex)) return SG_OK;
  const uint64_t nbytes = off[nprogs];
  WsPlan plan;
  const size_t o_bytes = plan.add(nbytes + 4), o_off = plan.add((nprogs + 1) * 8), o_sig = plan.add(nprogs * SG_SIG_BYTES);
  if ((rc = dstage_reserve(ctx, plan))) return rc;
  if ((rc = ws_reserve(ctx, prog_hashes_ws(nprogs)))) return rc;
  if (!sigs && (rc = pin_reserve(ctx, nprogs * SG_SIG_BYTES))) return rc;
  uint8_t* dbytes = dstage_at<uint8_t>(ctx, o_bytes);
  uint64_t* doff = dstage_at<uint64_t>(ctx, o_off);
  uint8_t* dsig = dstage_at<uint8_t>(ctx, o_sig);
  if ((rc = upload(ctx, dbytes, bytes, nbytes))) return rc;
  if ((rc = upload(ctx, doff, off, (nprogs + 1) * 8))) return rc;
  if ((rc = prog_hashes(ctx, dbytes, doff, nprogs, nbytes, dsig, 0))) return rc;
  uint8_t* hs = sigs ? sigs : (uint8_t*)ctx->pin.p;
  SG_HIP(hipMemcpyAsync(hs, dsig, nprogs * SG_SIG_BYTES, hipMemcpyDeviceToHost, ctx->stream));
  SG_HIP(hipStreamSynchronize(ctx->stream));
  if (hex) {  // hex.EncodeToString
    static const char digits[] = "0123456789abcdef";
    for (size_t k = 0; k < nprogs * SG_SIG_BYTES; k++) {
      hex[2 * k] = digits[hs[k] >> 4];
      hex[2 * k + 1] = digits[hs[k] & 15];
    }
  }
  return SG_OK;
}

}  // extern "C"
