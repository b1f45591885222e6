// sg_deflate.h -- one raw-DEFLATE (RFC 1951) encoder, written once for the
// host and the device: what pkg/db's serializeRecord does to every value
// through compress/flate (pkg/db/db.go:151-163), and so what compact()
// (:95-116) does to every live record.  With SG_DEFLATE_HD defined away (the
// default outside hipcc) this is plain C++.
//
// A stream is ONE block, fixed (BTYPE 01) or dynamic (BTYPE 10), or a chain of
// stored blocks of at most 65,535 bytes; the last block carries BFINAL; there
// is no sync-flush marker and no trailing empty block.  The empty input is the
// fixed block that holds only end-of-block: 03 00.
//
// The matcher is LZ77, greedy, one probe: a table of kHashSize last positions
// keyed by a hash of three bytes, positions kept as 16-bit values.  The
// distance is derived modulo 65,536, taken only when 1 <= dist <= 32768 and
// dist <= pos, and every candidate is compared with the input, every byte of
// it, before it is used: a stale or aliased entry costs compression, never
// correctness.  Positions inside a match are not entered.
//
// Two phases over the same deterministic parse.  plan(): tokenise, count the
// 286 + 30 frequencies, derive the dynamic code lengths, and from them the
// exact length of all three forms; the smallest wins, and of forms of equal
// length in bytes the first of STORED, FIXED, DYNAMIC (the cheapest to read).
// encode(): plan(), then tokenise again from the same starting table and emit.
//
// Dynamic code lengths are Shannon's, not Huffman's: with every used frequency
// raised to m = ceil(total / 2^14) the length of a symbol is the smallest l
// with f << l >= total', which is at most 15 (total' / f <= total / m + 286 <
// 2^15) and has a Kraft sum of at most 1.  The deficit is then handed out in
// units of 2^-15: level by level from the shortest lengths (the most frequent
// symbols) a symbol is shortened by one when its 2^-l fits, and one last pass
// in index order shortens whatever still fits.  After it the sum is exactly 1:
// the deficit is a multiple of 2^-Lmax, so while it is not zero the symbol of
// length Lmax > 1 fits it, and that pass would have shortened it.  A code of
// one symbol gets length 1 (zlib's special case), one of none no length at
// all.  The code-length code is fixed and complete: symbols 0..12 at 4 bits,
// 13..18 at 5; runs go through 16, 17 and 18.
//
// TERMINATION.  The parse loop advances pos by at least one byte per
// iteration; the stored chain by at least one byte per block (the empty input
// has one block).  Every other loop is bounded by a constant of the format:
// 258 match bytes, 316 symbols (286, 30), 19 code-length symbols, 15 lengths,
// 65535 stored bytes, or by the table's own size (kHashSize).  No loop reads
// anything another thread writes.
//
// BOUNDS.  in[pos] is loaded only for pos < len; the three bytes of a hash only
// when len - pos >= 3, as one 4-byte load only when len - pos >= 4; a match is
// compared only over min(258, len - pos) bytes, eight at a time only while
// eight of those remain, and its source lies dist <= pos bytes back.
// Every table index is masked (the hash), a symbol of the format (below 316), a
// length (below 16), or below a count this code built.  WriteSink stores
// out[n] only for n < cap: it clamps by itself and trusts nothing plan() said.
//
// DETERMINISM.  A stream's bytes are a function of its input bytes alone: the
// table is reset at the start of every parse, nothing is read from another
// stream, the arithmetic is integer arithmetic of fixed width, and the host
// and the device run this same source.  Its place in a batch, its neighbours
// in a wave and the side that ran it do not enter.
//
// No floating point, no read-modify-write shared with another thread, no
// private arrays (a dynamically indexed one would go to scratch on the
// device): the base/extra tables of lengths and distances are arithmetic.
#pragma once

#include <stdint.h>

#include "../../include/syzsig.h"

#ifndef SG_DEFLATE_HD
#ifdef __HIPCC__
#define SG_DEFLATE_HD __host__ __device__
#else
#define SG_DEFLATE_HD
#endif
#endif

namespace sgdef {

constexpr uint32_t kHashBits = 9;
constexpr uint32_t kHashSize = 1u << kHashBits;
constexpr uint32_t kNLit = 286, kNDist = 30, kNSym = kNLit + kNDist;  // distance symbol d is symbol 286 + d
constexpr int kStored = 0, kFixed = 1, kDynamic = 2, kAuto = -1;      // a form is its BTYPE

// A stream's tables, as logical byte offsets.  The frequencies of the count
// become, in encode(), each symbol's code (bit-reversed, ready to emit) and
// length; the lengths are nibbles; kNext is build_codes' count per length.
constexpr uint32_t kFreq = 0;      // u32 x 316
constexpr uint32_t kLens = 1264;   // nibble x 316
constexpr uint32_t kNext = 1424;   // u16 x 16
constexpr uint32_t kHash = 1456;   // u16 x kHashSize
constexpr uint32_t kTabBytes = kHash + 2 * kHashSize;  // 2480
constexpr uint32_t kTabDwords = kTabBytes / 4;         // 620
static_assert(kLens == 4 * kNSym && kLens + kNSym / 2 <= kNext && kNext + 32 == kHash && kTabBytes % 4 == 0,
              "table layout");

// Logical dword w of the block is dword w * stride of base (sg_inflate.h Tab).
struct Tab {
  uint8_t* base;
  uint32_t stride;
  SG_DEFLATE_HD uint8_t* at(uint32_t b) const { return base + (uint64_t)(b >> 2) * stride * 4 + (b & 3); }
  SG_DEFLATE_HD uint32_t r8(uint32_t b) const { return *at(b); }
  SG_DEFLATE_HD void w8(uint32_t b, uint32_t v) const { *at(b) = (uint8_t)v; }
  SG_DEFLATE_HD uint32_t r16(uint32_t b) const { return *reinterpret_cast<const uint16_t*>(at(b)); }  // (b even)
  SG_DEFLATE_HD void w16(uint32_t b, uint32_t v) const { *reinterpret_cast<uint16_t*>(at(b)) = (uint16_t)v; }
  SG_DEFLATE_HD uint32_t r32(uint32_t b) const { return *reinterpret_cast<const uint32_t*>(at(b)); }  // (b % 4 == 0)
  SG_DEFLATE_HD void w32(uint32_t b, uint32_t v) const { *reinterpret_cast<uint32_t*>(at(b)) = v; }
  SG_DEFLATE_HD uint32_t freq(uint32_t s) const { return r32(kFreq + 4 * s); }
  SG_DEFLATE_HD uint32_t len(uint32_t s) const { return (r8(kLens + (s >> 1)) >> (4 * (s & 1))) & 15; }
  SG_DEFLATE_HD void set_len(uint32_t s, uint32_t l) const {
    const uint32_t b = kLens + (s >> 1), sh = 4 * (s & 1);
    w8(b, (r8(b) & ~(15u << sh)) | (l << sh));
  }
};

struct CountSink {
  uint64_t n = 0;
  SG_DEFLATE_HD void put(uint32_t) { n++; }
};

struct WriteSink {
  uint8_t* out;
  uint64_t cap;
  uint64_t n = 0;
  SG_DEFLATE_HD WriteSink(uint8_t* o, uint64_t c) : out(o), cap(c) {}
  SG_DEFLATE_HD void put(uint32_t b) {
    if (n < cap) out[n] = (uint8_t)b;
    n++;
  }
};

// LSB-first bit writer over a sink; fewer than 8 bits wait between calls
template <class Sink>
struct Bits {
  Sink& o;
  uint64_t buf = 0;
  uint32_t nb = 0;
  SG_DEFLATE_HD explicit Bits(Sink& s) : o(s) {}
  SG_DEFLATE_HD void put(uint32_t v, uint32_t n) {  // n <= 16, v < 2^n
    buf |= (uint64_t)v << nb;
    nb += n;
    while (nb >= 8) {
      o.put((uint32_t)buf & 0xFF);
      buf >>= 8;
      nb -= 8;
    }
  }
  SG_DEFLATE_HD void finish() {
    if (nb) o.put((uint32_t)buf & 0xFF);
    buf = 0;
    nb = 0;
  }
};

SG_DEFLATE_HD inline uint32_t bit_len(uint64_t x) { return x ? 64u - (uint32_t)__builtin_clzll(x) : 0u; }

// the low n bits of c, reversed (Huffman codes go out most significant bit first); 1 <= n <= 15
SG_DEFLATE_HD inline uint32_t rev_bits(uint32_t c, uint32_t n) {
  c = ((c & 0x5555u) << 1) | ((c >> 1) & 0x5555u);
  c = ((c & 0x3333u) << 2) | ((c >> 2) & 0x3333u);
  c = ((c & 0x0F0Fu) << 4) | ((c >> 4) & 0x0F0Fu);
  c = ((c & 0x00FFu) << 8) | ((c >> 8) & 0x00FFu);
  return c >> (16 - n);
}

// A length 3..258 and a distance 1..32768 as symbol, extra bits and their
// value: the inverse of block_codes' closed forms in sg_inflate.h.
struct Sym {
  uint32_t sym, eb, ev;
};
SG_DEFLATE_HD inline Sym length_sym(uint32_t l) {
  if (l == 258) return {285, 0, 0};
  const uint32_t x = l - 3;
  if (x < 8) return {257 + x, 0, 0};
  const uint32_t eb = bit_len(x) - 3;  // x = (4 + m) << eb | ev
  return {257 + 4 * (eb + 1) + ((x >> eb) & 3), eb, x & ((1u << eb) - 1)};
}
SG_DEFLATE_HD inline Sym dist_sym(uint32_t d) {
  const uint32_t y = d - 1;
  if (y < 4) return {y, 0, 0};
  const uint32_t eb = bit_len(y) - 2;  // y = (2 + m) << eb | ev
  return {2 * (eb + 1) + ((y >> eb) & 1), eb, y & ((1u << eb) - 1)};
}

// the fixed code (RFC 1951 3.2.6)
SG_DEFLATE_HD inline uint32_t fixed_len(uint32_t s) { return s < 144 ? 8u : s < 256 ? 9u : s < 280 ? 7u : 8u; }
SG_DEFLATE_HD inline uint32_t fixed_code(uint32_t s) {
  return s < 144 ? 0x30 + s : s < 256 ? 0x190 + (s - 144) : s < 280 ? s - 256 : 0xC0 + (s - 280);
}
// the code-length code: symbols 0..12 at 4 bits (codes 0..12), 13..18 at 5 (codes 26..31): 13/16 + 6/32 = 1
SG_DEFLATE_HD inline uint32_t cl_len(uint32_t s) { return s < 13 ? 4u : 5u; }
SG_DEFLATE_HD inline uint32_t cl_code(uint32_t s) { return s < 13 ? s : 26 + (s - 13); }
// the order in which a header sends the code-length code's lengths, five bits each
constexpr uint64_t kClOrdLo = 16ull | 17ull << 5 | 18ull << 10 | 0ull << 15 | 8ull << 20 | 7ull << 25 | 9ull << 30 |
                              6ull << 35 | 10ull << 40 | 5ull << 45 | 11ull << 50 | 4ull << 55;
constexpr uint64_t kClOrdHi = 12ull | 3ull << 5 | 13ull << 10 | 2ull << 15 | 14ull << 20 | 1ull << 25 | 15ull << 30;

SG_DEFLATE_HD inline uint64_t stored_bytes(uint64_t len) {
  const uint64_t blocks = len ? (len + 65534) / 65535 : 1;
  return len + 5 * blocks;
}

// Unaligned little-endian loads (both sides are little-endian); the caller has seen that so many bytes remain.
SG_DEFLATE_HD inline uint32_t load4(const uint8_t* p) {
  uint32_t v;
  __builtin_memcpy(&v, p, 4);
  return v;
}
SG_DEFLATE_HD inline uint64_t load8(const uint8_t* p) {
  uint64_t v;
  __builtin_memcpy(&v, p, 8);
  return v;
}

// The parse: tok.lit(byte) and tok.match(length, distance) in order.  The
// table starts from zeros every time, so two parses of one input agree.
template <class Tok>
SG_DEFLATE_HD void tokenise(const uint8_t* in, uint64_t len, const Tab& t, Tok& tok) {
  for (uint32_t i = 0; i < kHashSize / 2; i++) t.w32(kHash + 4 * i, 0);
  uint64_t pos = 0;
  while (pos < len) {
    if (len - pos >= 3) {
      const uint32_t w = len - pos >= 4
                             ? load4(in + pos) & 0xFFFFFFu
                             : (uint32_t)in[pos] | (uint32_t)in[pos + 1] << 8 | (uint32_t)in[pos + 2] << 16;
      const uint32_t h = (w * 0x9E3779B1u) >> (32 - kHashBits);  // (below kHashSize)
      const uint32_t cand = t.r16(kHash + 2 * h);
      t.w16(kHash + 2 * h, (uint32_t)pos & 0xFFFFu);
      const uint32_t dist = ((uint32_t)pos - cand) & 0xFFFFu;
      if (dist >= 1 && dist <= 32768 && dist <= pos) {
        const uint64_t rem = len - pos;
        const uint32_t maxl = rem < 258 ? (uint32_t)rem : 258u;
        const uint8_t* src = in + (pos - dist);
        uint32_t l = 0;
        bool differ = false;
        while (!differ && maxl - l >= 8) {  // eight bytes at a time while eight remain of the match's reach
          const uint64_t x = load8(src + l) ^ load8(in + pos + l);
          if (x) {
            l += (uint32_t)__builtin_ctzll(x) >> 3;
            differ = true;
          } else {
            l += 8;
          }
        }
        while (!differ && l < maxl && src[l] == in[pos + l]) l++;
        if (l >= 3) {
          tok.match(l, dist);
          pos += l;
          continue;
        }
      }
    }
    tok.lit(in[pos]);
    pos++;
  }
}

struct FreqTok {
  const Tab& t;
  uint64_t extra = 0;  // the extra bits of every length and distance
  SG_DEFLATE_HD void inc(uint32_t s) { t.w32(kFreq + 4 * s, t.r32(kFreq + 4 * s) + 1); }
  SG_DEFLATE_HD void lit(uint32_t b) { inc(b); }
  SG_DEFLATE_HD void match(uint32_t l, uint32_t d) {
    const Sym ls = length_sym(l), ds = dist_sym(d);
    inc(ls.sym);
    inc(kNLit + ds.sym);
    extra += ls.eb + ds.eb;
  }
};

// Lengths of the symbols [first, first + n) from their frequencies (see the
// top of the file).  Returns one past the last used symbol.
SG_DEFLATE_HD inline uint32_t build_lengths(const Tab& t, uint32_t first, uint32_t n) {
  uint64_t total = 0;
  uint32_t used = 0, last = 0;
  for (uint32_t i = 0; i < n; i++) {
    const uint32_t f = t.freq(first + i);
    total += f;
    if (f) {
      used++;
      last = i + 1;
    }
  }
  if (used < 2) {
    for (uint32_t i = 0; i < n; i++) t.set_len(first + i, t.freq(first + i) ? 1 : 0);
    return last;
  }
  const uint64_t m = (total + 16383) >> 14;
  uint64_t tp = 0;
  for (uint32_t i = 0; i < last; i++) {
    const uint64_t f = t.freq(first + i);
    if (f) tp += f < m ? m : f;
  }
  const uint32_t bt = bit_len(tp);
  uint32_t kraft = 0, present = 0;  // in units of 2^-15; bit l: some symbol has length l
  for (uint32_t i = 0; i < n; i++) {
    const uint64_t f = t.freq(first + i);
    uint32_t l = 0;
    if (f) {
      const uint64_t fp = f < m ? m : f;
      l = bt - bit_len(fp);
      if ((fp << l) < tp) l++;
      if (l > 15) l = 15;  // (never: see the top of the file)
      kraft += 1u << (15 - l);
      present |= 1u << l;
    }
    t.set_len(first + i, l);
  }
  uint32_t left = kraft < 32768 ? 32768 - kraft : 0;
  for (uint32_t lv = 2; lv <= 15 && left; lv++) {
    const uint32_t w = 1u << (15 - lv);
    if (!((present >> lv) & 1) || w > left) continue;
    for (uint32_t i = 0; i < last && left >= w; i++)
      if (t.len(first + i) == lv) {
        t.set_len(first + i, lv - 1);
        left -= w;
      }
  }
  for (uint32_t i = 0; i < last && left; i++) {
    uint32_t l = t.len(first + i);
    if (l < 2) continue;
    while (l > 1 && (1u << (15 - l)) <= left) {
      left -= 1u << (15 - l);
      l--;
    }
    t.set_len(first + i, l);
  }
  return last;
}

// The nlit + ndist lengths of a dynamic header as code-length symbols:
// emit(symbol, extra value, extra bits).
template <class LenF, class Emit>
SG_DEFLATE_HD void header_runs(uint32_t n, LenF len, Emit emit) {
  uint32_t i = 0;
  while (i < n) {
    const uint32_t v = len(i);
    uint32_t c = 1;
    while (i + c < n && len(i + c) == v) c++;
    i += c;
    if (v == 0) {
      while (c >= 11) {
        const uint32_t r = c < 138 ? c : 138;
        emit(18, r - 11, 7);
        c -= r;
      }
      if (c >= 3) {
        emit(17, c - 3, 3);
        c = 0;
      }
    } else {
      emit(v, 0, 0);
      c--;
      while (c >= 3) {
        const uint32_t r = c < 6 ? c : 6;
        emit(16, r - 3, 2);
        c -= r;
      }
    }
    for (; c; c--) emit(v, 0, 0);
  }
}

struct Plan {
  int form = kFixed;
  uint64_t bytes = 0;  // of the chosen form
  uint64_t stored = 0, fixed = 0, dynamic = 0;  // of each form (0: not computed, the form was forced)
  uint32_t nlit = 257, ndist = 1;
};

// The count phase.  Leaves the dynamic code's lengths in t (unless stored was forced).
SG_DEFLATE_HD inline Plan plan(const uint8_t* in, uint64_t len, const Tab& t, int force = kAuto) {
  Plan p;
  p.stored = stored_bytes(len);
  if (force == kStored) {
    p.form = kStored;
    p.bytes = p.stored;
    return p;
  }
  for (uint32_t s = 0; s < kNSym; s++) t.w32(kFreq + 4 * s, 0);
  t.w32(kFreq + 4 * 256, 1);  // end of block
  FreqTok ft{t};
  tokenise(in, len, t, ft);
  uint64_t fixed_bits = 3 + ft.extra;
  for (uint32_t s = 0; s < kNLit; s++) fixed_bits += (uint64_t)t.freq(s) * fixed_len(s);
  for (uint32_t s = 0; s < kNDist; s++) fixed_bits += (uint64_t)t.freq(kNLit + s) * 5;
  p.fixed = (fixed_bits + 7) >> 3;
  p.nlit = build_lengths(t, 0, kNLit);
  if (p.nlit < 257) p.nlit = 257;
  p.ndist = build_lengths(t, kNLit, kNDist);
  if (p.ndist < 1) p.ndist = 1;
  uint64_t dyn_bits = 3 + 14 + 19 * 3 + ft.extra;
  for (uint32_t s = 0; s < p.nlit; s++) dyn_bits += (uint64_t)t.freq(s) * t.len(s);
  for (uint32_t s = 0; s < p.ndist; s++) dyn_bits += (uint64_t)t.freq(kNLit + s) * t.len(kNLit + s);
  const uint32_t nlit = p.nlit;
  header_runs(
      p.nlit + p.ndist, [&](uint32_t i) { return t.len(i < nlit ? i : kNLit + (i - nlit)); },
      [&](uint32_t s, uint32_t, uint32_t eb) { dyn_bits += cl_len(s) + eb; });
  p.dynamic = (dyn_bits + 7) >> 3;
  if (force == kFixed || force == kDynamic) {
    p.form = force;
    p.bytes = force == kFixed ? p.fixed : p.dynamic;
    return p;
  }
  p.form = kStored;
  p.bytes = p.stored;
  if (p.fixed < p.bytes) {
    p.form = kFixed;
    p.bytes = p.fixed;
  }
  if (p.dynamic < p.bytes) {
    p.form = kDynamic;
    p.bytes = p.dynamic;
  }
  return p;
}

// The canonical codes of the symbols [first, first + n) from their lengths,
// into the frequencies' place: code (reversed) | length << 16.
SG_DEFLATE_HD inline void build_codes(const Tab& t, uint32_t first, uint32_t n) {
  for (uint32_t l = 0; l < 16; l++) t.w16(kNext + 2 * l, 0);
  for (uint32_t i = 0; i < n; i++) {
    const uint32_t l = t.len(first + i);
    if (l) t.w16(kNext + 2 * l, t.r16(kNext + 2 * l) + 1);
  }
  uint32_t code = 0, before = 0;
  for (uint32_t l = 1; l < 16; l++) {  // counts to first codes
    const uint32_t c = t.r16(kNext + 2 * l);
    code = (code + before) << 1;
    t.w16(kNext + 2 * l, code);
    before = c;
  }
  for (uint32_t i = 0; i < n; i++) {
    const uint32_t l = t.len(first + i);
    uint32_t v = 0;
    if (l) {
      const uint32_t c = t.r16(kNext + 2 * l);
      t.w16(kNext + 2 * l, c + 1);
      v = rev_bits(c, l) | l << 16;
    }
    t.w32(kFreq + 4 * (first + i), v);
  }
}

template <class Sink, bool kFixedCode>
struct EmitTok {
  Bits<Sink>& w;
  const Tab& t;
  SG_DEFLATE_HD void sym(uint32_t s) {
    if (kFixedCode) {
      w.put(rev_bits(fixed_code(s), fixed_len(s)), fixed_len(s));
    } else {
      const uint32_t v = t.r32(kFreq + 4 * s);
      w.put(v & 0xFFFFu, v >> 16);
    }
  }
  SG_DEFLATE_HD void lit(uint32_t b) { sym(b); }
  SG_DEFLATE_HD void match(uint32_t l, uint32_t d) {
    const Sym ls = length_sym(l), ds = dist_sym(d);
    sym(ls.sym);
    w.put(ls.ev, ls.eb);
    if (kFixedCode)
      w.put(rev_bits(ds.sym, 5), 5);
    else
      sym(kNLit + ds.sym);
    w.put(ds.ev, ds.eb);
  }
};

// The write phase: the stream of in[0, len) through sink o (o.n is its length
// afterwards, whatever the sink kept).  Returns the plan it followed.
template <class Sink>
SG_DEFLATE_HD Plan encode(const uint8_t* in, uint64_t len, const Tab& t, Sink& o, int force = kAuto) {
  const Plan p = plan(in, len, t, force);
  if (p.form == kStored) {
    uint64_t pos = 0;
    do {
      const uint64_t rem = len - pos;
      const uint32_t n = rem < 65535 ? (uint32_t)rem : 65535u;
      o.put(pos + n == len ? 1 : 0);
      o.put(n & 0xFF);
      o.put(n >> 8);
      o.put(~n & 0xFF);
      o.put((~n >> 8) & 0xFF);
      for (uint32_t i = 0; i < n; i++) o.put(in[pos + i]);
      pos += n;
    } while (pos < len);
    return p;
  }
  Bits<Sink> w(o);
  w.put(1, 1);
  w.put((uint32_t)p.form, 2);
  if (p.form == kFixed) {
    EmitTok<Sink, true> et{w, t};
    tokenise(in, len, t, et);
    et.sym(256);
  } else {
    w.put(p.nlit - 257, 5);
    w.put(p.ndist - 1, 5);
    w.put(19 - 4, 4);
    for (uint32_t i = 0; i < 19; i++) {
      const uint32_t s = (uint32_t)((i < 12 ? kClOrdLo >> (5 * i) : kClOrdHi >> (5 * (i - 12))) & 31);
      w.put(cl_len(s), 3);
    }
    const uint32_t nlit = p.nlit;
    header_runs(
        p.nlit + p.ndist, [&](uint32_t i) { return t.len(i < nlit ? i : kNLit + (i - nlit)); },
        [&](uint32_t s, uint32_t ev, uint32_t eb) {
          w.put(rev_bits(cl_code(s), cl_len(s)), cl_len(s));
          w.put(ev, eb);
        });
    build_codes(t, 0, p.nlit);
    build_codes(t, kNLit, p.ndist);
    EmitTok<Sink, false> et{w, t};
    tokenise(in, len, t, et);
    et.sym(256);
  }
  w.finish();
  return p;
}

}  // namespace sgdef
