"""Inputs for the corpus database's write side (tests/test_db_write.py): the encoder's case file, seeded random
inputs, a bit-exact reader that lists a stream's blocks, tokens and last bit, and a database with a history.

The copies that force a length or a distance code are a random source of non-zero bytes, a filler of zeros, and the
copy at the chosen distance: the matcher (syzkaller_amd/csrc/sg_deflate.h) is one probe into 512 last positions and
enters no position inside a match, so a run of zeros leaves the source's slot alone while a random filler of a few
hundred bytes would have overwritten it.  The source itself is drawn again until no later three bytes of it share
the slot of its first three (slot() restates the encoder's hash for that; if the hash changes, test_case_file says
which code went missing).  The same copies behind a random prefix are in the file as well; of those only validity
is asked."""
import random
import struct

from tests import db_cases as K

DEFLATE_LONG = 65536  # SG_DEFLATE_LONG
STORED, FIXED, DYNAMIC = 0, 1, 2
CLASS_BYTES = 64      # the kernels sort by input length / 64


def bound(n):
    """sg_deflate_bound."""
    return n + 5 * max(1, -(-n // 65535))


def form_of(stream):
    return (stream[0] >> 1) & 3


# ---- a reader that keeps what zlib throws away -----------------------------------
class _Bits:
    def __init__(self, data):
        self.data, self.pos = data, 0

    def bits(self, n):
        v = 0
        for k in range(n):
            v |= ((self.data[self.pos >> 3] >> (self.pos & 7)) & 1) << k
            self.pos += 1
        return v

    def sym(self, table):
        code = 0
        for ln in range(1, 16):
            code = (code << 1) | self.bits(1)
            s = table.get((ln, code))
            if s is not None:
                return s
        raise ValueError("no such code")


def _table(lens):
    return {(ln, code): s for s, (code, ln) in K.canonical(lens).items()}


_FIXED_LIT = _table([8] * 144 + [9] * 112 + [7] * 24 + [8] * 8)
_FIXED_DIST = _table([5] * 32)


def read_stream(stream):
    """(blocks, tokens, end_bit): each block's (type, lit_lens, dist_lens); the literals as ints and the matches
    as (length, distance) in order; the bit position behind the final block's last bit."""
    r = _Bits(bytes(stream))
    blocks, toks = [], []
    while True:
        last, typ = r.bits(1), r.bits(2)
        if typ == 0:
            r.pos = (r.pos + 7) & ~7
            n, nn = r.bits(16), r.bits(16)
            assert n == nn ^ 0xFFFF
            toks += list(r.data[r.pos >> 3:(r.pos >> 3) + n])
            r.pos += 8 * n
            blocks.append((0, n, None))
        else:
            if typ == 1:
                lit, dist, ll, dl = _FIXED_LIT, _FIXED_DIST, None, None
            else:
                assert typ == 2
                nlit, ndist, ncode = r.bits(5) + 257, r.bits(5) + 1, r.bits(4) + 4
                cl = [0] * 19
                for k in range(ncode):
                    cl[K.CL_ORDER[k]] = r.bits(3)
                clt, lens = _table(cl), []
                while len(lens) < nlit + ndist:
                    s = r.sym(clt)
                    if s < 16:
                        lens.append(s)
                    elif s == 16:
                        lens += [lens[-1]] * (3 + r.bits(2))
                    elif s == 17:
                        lens += [0] * (3 + r.bits(3))
                    else:
                        lens += [0] * (11 + r.bits(7))
                assert len(lens) == nlit + ndist
                ll, dl = lens[:nlit], lens[nlit:]
                lit, dist = _table(ll), _table(dl)
            blocks.append((typ, ll, dl))
            while True:
                s = r.sym(lit)
                if s < 256:
                    toks.append(s)
                elif s == 256:
                    break
                else:
                    k = s - 257
                    length = K.LBASE[k] + r.bits(K.LEXT[k])
                    d = r.sym(dist)
                    toks.append((length, K.DBASE[d] + r.bits(K.DEXT[d])))
        if last:
            return blocks, toks, r.pos


def kraft(lens):
    """(number of codes, Kraft sum in units of 2^-15)."""
    used = [ln for ln in lens if ln]
    return len(used), sum(1 << (15 - ln) for ln in used)


# ---- the case file ---------------------------------------------------------------
def _nonzero(rng, n):
    return bytes(rng.randrange(1, 256) for _ in range(n))


def _rand(rng, n):
    return rng.randbytes(n)


def slot(b):
    """The matcher's table slot of three bytes (sg_deflate.h tokenise)."""
    return (((b[0] | b[1] << 8 | b[2] << 16) * 0x9E3779B1) & 0xFFFFFFFF) >> 23


def _copy(prefix, length, dist):
    buf = bytearray(prefix)
    for _ in range(length):
        buf.append(buf[len(buf) - dist])
    buf.append(buf[len(buf) - dist] ^ 0xFF)
    return bytes(buf)


def copy_case(seed, length, dist, quiet=True):
    """A source, a filler up to `dist` bytes, `length` bytes copied from `dist` back, and a byte that ends the copy.
    quiet: the source is min(length, dist) non-zero bytes and the filler zeros, and when the parse reaches the copy
    the slot of its first three bytes still holds the source's position; else the whole prefix is random."""
    rng = random.Random(seed)
    if not quiet:
        return _copy(_rand(rng, dist), length, dist)
    while True:
        src = _nonzero(rng, min(length, dist))
        buf = _copy(src + bytes(dist - len(src)), length, dist)
        if dist < 3:
            return buf
        later = {buf[j:j + 3] for j in range(1, min(dist, len(src) + 3))} | ({bytes(3)} if dist - len(src) >= 3 else set())
        if all(slot(g) != slot(buf[:3]) for g in later):
            return buf


def no_repeats(k=8):
    """Every three bytes over k values exactly once (a de Bruijn sequence, unrolled): nothing for a matcher."""
    a, seq = [0] * (3 * k), []

    def db(t, p):
        if t > 3:
            if 3 % p == 0:
                seq.extend(a[1:p + 1])
        else:
            a[t] = a[t - p]
            db(t + 1, p)
            for j in range(a[t - p] + 1, k):
                a[t] = j
                db(t + 1, t)

    db(1, 1)
    return bytes(97 + v for v in seq + seq[:2])


def length_ends():
    """(length code, length) at both ends of every code's extra-bit range."""
    out = []
    for k in range(29):
        lo = K.LBASE[k]
        hi = min(lo + (1 << K.LEXT[k]) - 1, 257 if k < 28 else 258)
        out += [(257 + k, lo)] + ([(257 + k, hi)] if hi != lo else [])
    return out


def dist_ends():
    out = []
    for k in range(30):
        lo = K.DBASE[k]
        hi = lo + (1 << K.DEXT[k]) - 1
        out += [(k, lo)] + ([(k, hi)] if hi != lo else [])
    return out


LINE40 = b"r0 = openat(0xffffff9c, &(0x7f0000)=0)\n\n"
assert len(LINE40) == 40
PROG_SIZES = (40, 64, 100, 128, 200, 500, 1000, 2048, 4096, 10000, 30000, 65536)
PHASE_SIZES = tuple(range(40, 121, 2))   # enough sizes that the streams end on every bit phase


def cases():
    """[(name, input bytes)]."""
    out = []

    def add(name, data):
        out.append((name, bytes(data)))

    for n in range(4):
        add("len_%d" % n, b"abc"[:n])
    for n in (3, 4, 257, 258, 259, 260, 517):
        add("run_%d" % n, b"z" * n)
    for sym, length in length_ends():
        add("length_code_%d_len_%d" % (sym, length), copy_case(1000 + length, length, 300))
        add("length_code_%d_len_%d_random_prefix" % (sym, length), copy_case(2000 + length, length, 300, quiet=False))
    for sym, dist in dist_ends():
        add("dist_code_%d_dist_%d" % (sym, dist), copy_case(3000 + dist, 10, dist))
        add("dist_code_%d_dist_%d_random_prefix" % (sym, dist), copy_case(4000 + dist, 10, dist, quiet=False))
    add("repeat_at_32768", copy_case(32768, 20, 32768))
    add("repeat_at_32769", copy_case(32769, 20, 32769))
    rng = random.Random(65536)
    block = _rand(rng, 65536)
    add("block_65536_twice", block + block)
    add("repeat_across_65536", (LINE40 * 1639)[:65536 + 3])
    for n in (1, 100, 65535, 65536, 131071):
        add("random_%d" % n, _rand(rng, n))
    add("literals_above_143", bytes(rng.randrange(144, 256) for _ in range(12)))
    add("literals_above_143_long", bytes(rng.randrange(144, 256) for _ in range(16)) * 40)
    add("two_symbols", bytes(rng.choice(b"ab") for _ in range(4000)))
    add("one_symbol", b"q" * 60000)                 # distances 1 and then 258: a complete code of two
    add("one_distance", _rand(rng, 258) * 200)      # every match 258 bytes long and 258 back: a single code
    add("no_repeats_8_symbols", no_repeats())
    add("all_256_values", b"".join(bytes(rng.sample(range(256), 256)) for _ in range(16)))
    for size in PROG_SIZES:
        add("prog_%d" % size, K.prog_text(size, size))
    for size in PHASE_SIZES:
        add("phase_%d" % size, K.prog_text(7000 + size, size))
    add("line40_65536", (LINE40 * 1639)[:65536])
    return out


def random_inputs(count=300, seed=951):
    """Seeded inputs of mixed kinds: random bytes over alphabets of 1 to 256 values, with copies spliced in."""
    rng = random.Random(seed)
    out = []
    for _ in range(count):
        n = rng.choice((rng.randrange(0, 40), rng.randrange(0, 400), rng.randrange(0, 4000)))
        alpha = rng.choice((1, 2, 4, 16, 64, 256))
        buf = bytearray(rng.randrange(alpha) * (255 // max(alpha - 1, 1)) for _ in range(n))
        for _ in range(rng.randrange(0, 6)):
            if len(buf) < 4:
                break
            src = rng.randrange(len(buf))
            ln = rng.randrange(3, 300)
            at = rng.randrange(len(buf) + 1)
            piece = bytes(buf[src:src + ln])
            buf[at:at] = piece
        out.append(bytes(buf))
    return out


# ---- a database with a history -----------------------------------------------------
def history_records(hash_keys=True):
    """About 300 writes as (key, val or None, seq): overwrites, deletions, empty values and one long value.  With
    hash_keys a value's key is its text's SHA-1 in hex, as the hub and the manager name programs (a rewritten key
    then keeps its text: only the seq changes)."""
    import hashlib

    rng = random.Random(300)
    texts = [K.prog_text(900 + k, 60 + 23 * (k % 37)) for k in range(240)]
    texts[17] = K.prog_text(917, 70000)   # the long value: past SG_DEFLATE_LONG

    def key(k):
        return hashlib.sha1(texts[k]).hexdigest().encode() if hash_keys else b"key%d" % k

    recs = [(key(k), texts[k], k + 1) for k in range(240)]
    for k in rng.sample(range(240), 30):
        recs.append((key(k), texts[k], 1000 + k))          # overwritten: the later seq wins
    for k in rng.sample([k for k in range(240) if k != 17], 25):
        recs.append((key(k), None, K.SEQ_DELETED))         # deleted (never the long one)
    for k in range(5):
        recs.append((b"empty%d" % k, b"", 2000 + k))       # empty values (their keys are no hashes)
    return recs


def record_bytes(key, val, seq, stream=None):
    """serializeRecord with this library's stream swapped in."""
    if val is None:
        return K.db_record(key, None, seq)
    return K.db_record(key, val, seq, stream=stream if len(val) else b"")
