// sg_inflate.h -- one raw-DEFLATE (RFC 1951) decoder, written once for the
// host and the device: what pkg/db's deserializeRecord does to every value
// through compress/flate (pkg/db/db.go:241-247).  With SG_INFLATE_HD defined
// away (the default outside hipcc) this is plain C++.
//
// The decoder is parameterised by its sink (CountSink: the output's length;
// WriteSink: the bytes, clamped to a span) and by where its per-stream
// tables live (Tab: 812 bytes addressed through a dword stride, so the device
// can interleave the lanes of a wave in LDS and the host uses a flat block).
//
// Semantics are zlib 1.2.11's inflate over a raw stream (the oracle is
// zlib.decompressobj(-15)): SG_INFLATE_OK exactly when zlib reaches the end
// of the final block, `consumed` then the bytes up to and including the one
// that holds the final block's last bit; SG_INFLATE_CORRUPT where zlib raises;
// SG_INFLATE_TRUNCATED where the input ends first.  Rejected: block type 3,
// stored LEN != ~NLEN, HLIT > 286 or HDIST > 30 (once the 14 bits are there),
// a repeat with no previous length or past HLIT + HDIST, no end-of-block code,
// an over-subscribed code, an incomplete code other than the ones zlib takes
// (a literal/length or distance code with at most one code, of length 1;
// never the code-length code, except that an all-zero code-length code passes
// zlib's table builder and then reads every length as 0 from one bit each,
// which is restated here), literal/length symbols 286 and 287, distance
// symbols 30 and 31, a distance past the start of the output.  An error is
// reported only once every bit zlib would have asked for first is present,
// so the CORRUPT / TRUNCATED split is zlib's too.
//
// TERMINATION.  Every iteration of a decode loop (blocks, symbols, code
// lengths, the bits of one code) takes at least one bit out of the reader or
// returns; the reader holds at most 8 * len bits and never goes back.  Every
// other loop is bounded by a constant of the format: 19, 316 or 15 table
// entries, 138 repeats, 258 match bytes, 65535 stored bytes.  No loop reads
// anything another thread writes.
//
// BOUNDS.  The reader loads in[pos] only for pos < len; its 8-byte refill is
// taken only when len - pos >= 8, so no look-ahead crosses the end.  WriteSink
// stores out[n] only for n < cap and reads out[n - d] only for d <= n: it
// clamps by itself and trusts nothing the count pass said.  Table indices
// come from counts this code built (a symbol index is below the code's
// total, a length index below 316).
//
// No float, no atomics, no private arrays (a dynamically indexed one would go
// to scratch on the device): the 19 code-length lengths ride in one 64-bit
// register, the base/extra tables of lengths and distances are arithmetic.
#pragma once

#include <stdint.h>

#include "../../include/syzsig.h"

#ifndef SG_INFLATE_HD
#ifdef __HIPCC__
#define SG_INFLATE_HD __host__ __device__
#else
#define SG_INFLATE_HD
#endif
#endif

namespace sginf {

// A stream's tables, as logical byte offsets.  lit_end / dist_end: per code
// length l the index one past the last symbol of that length in canonical
// order (so length l holds end[l] - end[l - 1] codes, end[0] = 0); the
// symbols in canonical order; the 316 code lengths of a dynamic header as
// nibbles.  The code-length code's own tables live in the literal symbols'
// place: they are dead before those are built.
constexpr uint32_t kLitEnd = 0;     // u16 x 16
constexpr uint32_t kDistEnd = 32;   // u8 x 16
constexpr uint32_t kDistSym = 48;   // u8 x 32
constexpr uint32_t kLitSym = 80;    // u16 x 286
constexpr uint32_t kLens = 652;     // nibble x 316
constexpr uint32_t kTabBytes = 812;
constexpr uint32_t kTabDwords = kTabBytes / 4;  // 203
constexpr uint32_t kClEnd = kLitSym;            // u8 x 8
constexpr uint32_t kClSym = kLitSym + 8;        // u8 x 19
static_assert(kLens + 316 / 2 <= kTabBytes && kTabBytes % 4 == 0, "table layout");

// Logical dword w of the block is dword w * stride of base: stride 1 is a
// flat block; stride 64 with base = block + lane puts lane l's every dword in
// bank l mod 32 of the LDS whatever index each lane asks for.
struct Tab {
  uint8_t* base;
  uint32_t stride;
  SG_INFLATE_HD uint8_t* at(uint32_t b) const { return base + (uint64_t)(b >> 2) * stride * 4 + (b & 3); }
  SG_INFLATE_HD uint32_t r8(uint32_t b) const { return *at(b); }
  SG_INFLATE_HD void w8(uint32_t b, uint32_t v) const { *at(b) = (uint8_t)v; }
  SG_INFLATE_HD uint32_t r16(uint32_t b) const { return *reinterpret_cast<const uint16_t*>(at(b)); }  // (b even)
  SG_INFLATE_HD void w16(uint32_t b, uint32_t v) const { *reinterpret_cast<uint16_t*>(at(b)) = (uint16_t)v; }
  SG_INFLATE_HD uint32_t len(uint32_t i) const { return (r8(kLens + (i >> 1)) >> (4 * (i & 1))) & 15; }
  // (lengths are set in index order: an even index starts its byte)
  SG_INFLATE_HD void set_len(uint32_t i, uint32_t l) const {
    const uint32_t b = kLens + (i >> 1);
    w8(b, (i & 1) ? (r8(b) | (l << 4)) : l);
  }
};

// LSB-first bit reader over in[0, len).
struct Bits {
  const uint8_t* in;
  uint64_t len, pos = 0, buf = 0;
  uint32_t nb = 0;
  SG_INFLATE_HD Bits(const uint8_t* p, uint64_t n) : in(p), len(n) {}
  // At least 48 bits afterwards, or every byte of the input taken.  Bits of
  // buf above nb are bits of the bytes at pos and on, or zero: they are
  // OR-ed in again, at the same places, by the next refill.
  SG_INFLATE_HD void refill() {
    if (nb >= 48) return;
    if (len - pos >= 8) {
      uint64_t w = 0;
      for (uint32_t k = 0; k < 8; k++) w |= (uint64_t)in[pos + k] << (8 * k);
      buf |= w << nb;
      const uint32_t adv = (63 - nb) >> 3;
      pos += adv;
      nb += 8 * adv;
    } else {
      while (nb <= 56 && pos < len) {
        buf |= (uint64_t)in[pos++] << nb;
        nb += 8;
      }
    }
  }
  SG_INFLATE_HD uint32_t take(uint32_t n) {  // n <= nb, n <= 16
    const uint32_t v = (uint32_t)buf & ((1u << n) - 1);
    buf >>= n;
    nb -= n;
    return v;
  }
  // whole unread bytes go back to the input: the reader is empty afterwards
  SG_INFLATE_HD void rewind() {
    pos -= nb >> 3;
    buf = 0;
    nb = 0;
  }
};

struct CountSink {
  uint64_t n = 0;
  SG_INFLATE_HD void lit(uint32_t) { n++; }
  SG_INFLATE_HD void match(uint32_t, uint32_t l) { n += l; }
  SG_INFLATE_HD void stored(const uint8_t*, uint32_t l) { n += l; }
};

struct WriteSink {
  uint8_t* out;
  uint64_t cap;
  uint64_t n = 0;
  SG_INFLATE_HD WriteSink(uint8_t* o, uint64_t c) : out(o), cap(c) {}
  SG_INFLATE_HD void lit(uint32_t b) {
    if (n < cap) out[n] = (uint8_t)b;
    n++;
  }
  SG_INFLATE_HD void match(uint32_t d, uint32_t l) {
    for (uint32_t i = 0; i < l; i++, n++)
      if (n < cap && d <= n) out[n] = out[n - d];
  }
  SG_INFLATE_HD void stored(const uint8_t* p, uint32_t l) {
    for (uint32_t i = 0; i < l; i++, n++)
      if (n < cap) out[n] = p[i];
  }
};

// One code of a canonical Huffman code with `total` symbols and lengths up to
// maxlen, a bit at a time: end(l) and sym(k) read the tables.  The bits are
// taken only once a code is found, or once no longer code exists (which zlib
// reports from its one-bit invalid entry).
template <class EndF, class SymF>
SG_INFLATE_HD int decode(Bits& s, uint32_t maxlen, uint32_t total, EndF end, SymF sym, uint32_t& out) {
  uint32_t code = 0, first = 0, index = 0;
  const uint32_t bits = (uint32_t)s.buf;
  for (uint32_t l = 1; l <= maxlen; l++) {
    if (l > s.nb) return SG_INFLATE_TRUNCATED;
    code |= (bits >> (l - 1)) & 1;
    const uint32_t e = end(l), cnt = e - index;
    if (code - first < cnt) {
      s.take(l);
      out = sym(index + (code - first));
      return SG_INFLATE_OK;
    }
    index = e;
    first += cnt;
    if (index >= total) {
      s.take(l);
      return SG_INFLATE_CORRUPT;
    }
    first <<= 1;
    code <<= 1;
  }
  return SG_INFLATE_CORRUPT;
}

// zlib's inflate_table as counts: the code of n symbols with lengths len(i)
// into end / sym.  `codes`: the code-length code, which may not be incomplete.
template <class LenF, class RdF, class WrF, class SymF>
SG_INFLATE_HD int construct(uint32_t n, uint32_t maxlen, bool codes, LenF len, RdF rd, WrF wr, SymF put,
                            uint32_t& total) {
  for (uint32_t l = 0; l <= maxlen; l++) wr(l, 0);
  for (uint32_t i = 0; i < n; i++) {
    const uint32_t l = len(i);
    if (l) wr(l, rd(l) + 1);
  }
  int32_t left = 1;
  uint32_t maxl = 0;
  for (uint32_t l = 1; l <= maxlen; l++) {
    const uint32_t c = rd(l);
    left = (left << 1) - (int32_t)c;
    if (left < 0) return SG_INFLATE_CORRUPT;  // over-subscribed
    if (c) maxl = l;
  }
  if (left > 0 && (codes ? maxl != 0 : maxl > 1)) return SG_INFLATE_CORRUPT;  // incomplete
  uint32_t run = 0;
  for (uint32_t l = 1; l <= maxlen; l++) {  // counts to starts ...
    const uint32_t c = rd(l);
    wr(l, run);
    run += c;
  }
  total = run;
  for (uint32_t i = 0; i < n; i++) {  // ... which placing the symbols turns into ends
    const uint32_t l = len(i);
    if (l) {
      const uint32_t k = rd(l);
      put(k, i);
      wr(l, k + 1);
    }
  }
  return SG_INFLATE_OK;
}

// the fixed code (RFC 1951 3.2.6) as closed forms, the same for every lane
SG_INFLATE_HD inline uint32_t fixed_lit_end(uint32_t l) { return l < 7 ? 0u : l == 7 ? 24u : l == 8 ? 176u : 288u; }
SG_INFLATE_HD inline uint32_t fixed_lit_sym(uint32_t k) {
  return k < 24 ? 256 + k : k < 168 ? k - 24 : k < 176 ? 280 + (k - 168) : 144 + (k - 176);
}
SG_INFLATE_HD inline uint32_t fixed_dist_end(uint32_t l) { return l < 5 ? 0u : 32u; }

struct Codes {
  uint32_t lit_total = 0, dist_total = 0;
};

// the order of the code-length code's lengths, five bits each
constexpr uint64_t kClOrdLo = 16ull | 17ull << 5 | 18ull << 10 | 0ull << 15 | 8ull << 20 | 7ull << 25 | 9ull << 30 |
                              6ull << 35 | 10ull << 40 | 5ull << 45 | 11ull << 50 | 4ull << 55;
constexpr uint64_t kClOrdHi = 12ull | 3ull << 5 | 13ull << 10 | 2ull << 15 | 14ull << 20 | 1ull << 25 | 15ull << 30;

// a dynamic block's header, after its three type bits
SG_INFLATE_HD inline int dynamic_header(Bits& s, const Tab& t, Codes& c) {
  s.refill();
  if (s.nb < 14) return SG_INFLATE_TRUNCATED;
  const uint32_t nlen = s.take(5) + 257, ndist = s.take(5) + 1, ncode = s.take(4) + 4;
  if (nlen > 286 || ndist > 30) return SG_INFLATE_CORRUPT;
  uint64_t cl = 0;  // the 19 lengths, three bits each
  for (uint32_t i = 0; i < ncode; i++) {
    s.refill();
    if (s.nb < 3) return SG_INFLATE_TRUNCATED;
    const uint32_t o = (uint32_t)((i < 12 ? kClOrdLo >> (5 * i) : kClOrdHi >> (5 * (i - 12))) & 31);
    cl |= (uint64_t)s.take(3) << (3 * o);
  }
  uint32_t cl_total = 0;
  int rc = construct(
      19, 7, true, [&](uint32_t i) { return (uint32_t)(cl >> (3 * i)) & 7; }, [&](uint32_t l) { return t.r8(kClEnd + l); },
      [&](uint32_t l, uint32_t v) { t.w8(kClEnd + l, v); }, [&](uint32_t k, uint32_t v) { t.w8(kClSym + k, v); }, cl_total);
  if (rc) return rc;
  const uint32_t n = nlen + ndist;
  uint32_t have = 0, prev = 0;
  while (have < n) {
    s.refill();
    uint32_t v = 0;
    if (cl_total == 0) {  // zlib's table of invalid entries: one bit, length 0
      if (s.nb < 1) return SG_INFLATE_TRUNCATED;
      s.take(1);
    } else if ((rc = decode(
                    s, 7, cl_total, [&](uint32_t l) { return t.r8(kClEnd + l); },
                    [&](uint32_t k) { return t.r8(kClSym + k); }, v))) {
      return rc;
    }
    if (v < 16) {
      t.set_len(have++, v);
      prev = v;
      continue;
    }
    const uint32_t eb = v == 16 ? 2 : v == 17 ? 3 : 7;
    if (s.nb < eb) return SG_INFLATE_TRUNCATED;
    uint32_t l = 0, rep;
    if (v == 16) {
      if (have == 0) return SG_INFLATE_CORRUPT;
      l = prev;
      rep = 3 + s.take(2);
    } else {
      rep = (v == 17 ? 3 : 11) + s.take(eb);
    }
    if (have + rep > n) return SG_INFLATE_CORRUPT;
    for (; rep; rep--) t.set_len(have++, l);
    prev = l;
  }
  if (t.len(256) == 0) return SG_INFLATE_CORRUPT;  // no end-of-block code
  rc = construct(
      nlen, 15, false, [&](uint32_t i) { return t.len(i); }, [&](uint32_t l) { return t.r16(kLitEnd + 2 * l); },
      [&](uint32_t l, uint32_t v) { t.w16(kLitEnd + 2 * l, v); }, [&](uint32_t k, uint32_t v) { t.w16(kLitSym + 2 * k, v); },
      c.lit_total);
  if (rc) return rc;
  return construct(
      ndist, 15, false, [&](uint32_t i) { return t.len(nlen + i); }, [&](uint32_t l) { return t.r8(kDistEnd + l); },
      [&](uint32_t l, uint32_t v) { t.w8(kDistEnd + l, v); }, [&](uint32_t k, uint32_t v) { t.w8(kDistSym + k, v); },
      c.dist_total);
}

// the symbols of one Huffman block, to its end-of-block code
template <bool kFixed, class Sink>
SG_INFLATE_HD int block_codes(Bits& s, const Tab& t, const Codes& c, Sink& o) {
  for (;;) {
    s.refill();  // 48 bits: a length (15 + 5) and a distance (15 + 13)
    uint32_t sym = 0;
    int rc;
    if constexpr (kFixed)
      rc = decode(
          s, 9, 288, [](uint32_t l) { return fixed_lit_end(l); }, [](uint32_t k) { return fixed_lit_sym(k); }, sym);
    else
      rc = decode(
          s, 15, c.lit_total, [&](uint32_t l) { return t.r16(kLitEnd + 2 * l); },
          [&](uint32_t k) { return t.r16(kLitSym + 2 * k); }, sym);
    if (rc) return rc;
    if (sym < 256) {
      o.lit(sym);
    } else if (sym == 256) {
      return SG_INFLATE_OK;
    } else {
      if (sym >= 286) return SG_INFLATE_CORRUPT;
      sym -= 257;  // length 3 + ((4 + sym % 4) << extra), extra = sym / 4 - 1; 3..10 and 258 plain
      uint32_t eb = sym < 8 || sym == 28 ? 0 : (sym >> 2) - 1;
      if (s.nb < eb) return SG_INFLATE_TRUNCATED;
      const uint32_t length = sym < 8 ? 3 + sym : sym == 28 ? 258 : 3 + ((4 + (sym & 3)) << eb) + s.take(eb);
      uint32_t ds = 0;
      if constexpr (kFixed)
        rc = decode(
            s, 5, 32, [](uint32_t l) { return fixed_dist_end(l); }, [](uint32_t k) { return k; }, ds);
      else
        rc = decode(
            s, 15, c.dist_total, [&](uint32_t l) { return t.r8(kDistEnd + l); },
            [&](uint32_t k) { return t.r8(kDistSym + k); }, ds);
      if (rc) return rc;
      if (ds >= 30) return SG_INFLATE_CORRUPT;
      eb = ds < 4 ? 0 : (ds >> 1) - 1;  // distance 1 + ((2 + ds % 2) << extra); 1..4 plain
      if (s.nb < eb) return SG_INFLATE_TRUNCATED;
      const uint32_t dist = ds < 4 ? 1 + ds : 1 + ((2 + (ds & 1)) << eb) + s.take(eb);
      if (dist > o.n) return SG_INFLATE_CORRUPT;  // before the start of the output
      o.match(dist, length);
    }
    if (o.n >> 32) return SG_INFLATE_TOO_LARGE;
  }
}

// The stream in[0, len) through sink o.  consumed is set on SG_INFLATE_OK.
template <class Sink>
SG_INFLATE_HD int inflate(const uint8_t* in, uint64_t len, const Tab& t, Sink& o, uint64_t& consumed) {
  Bits s(in, len);
  Codes c;
  for (;;) {
    s.refill();
    if (s.nb < 3) return SG_INFLATE_TRUNCATED;
    const uint32_t last = s.take(1), type = s.take(2);
    int rc = SG_INFLATE_OK;
    if (type == 3) return SG_INFLATE_CORRUPT;
    if (type == 0) {
      s.take(s.nb & 7);  // to the byte boundary
      s.refill();
      if (s.nb < 32) return SG_INFLATE_TRUNCATED;
      const uint32_t n = s.take(16), nn = s.take(16);
      if (n != (nn ^ 0xFFFFu)) return SG_INFLATE_CORRUPT;
      s.rewind();
      if (len - s.pos < n) return SG_INFLATE_TRUNCATED;
      o.stored(in + s.pos, n);
      s.pos += n;
      if (o.n >> 32) return SG_INFLATE_TOO_LARGE;
    } else if (type == 1) {
      rc = block_codes<true>(s, t, c, o);
    } else {
      rc = dynamic_header(s, t, c);
      if (!rc) rc = block_codes<false>(s, t, c, o);
    }
    if (rc) return rc;
    if (last) break;
  }
  consumed = s.pos - (s.nb >> 3);
  return SG_INFLATE_OK;
}

}  // namespace sginf
