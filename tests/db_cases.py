"""Streams and databases for the corpus-database tests (tests/test_db.py): a bit writer for
the fixed code and for dynamic headers, so that edge streams are built exactly, the hand-built cases with the
status each must get, seeded mutations, and database files.  Every expectation here is checked against zlib
(tests/db_oracle.py) by a CPU test before a GPU test relies on it."""
import random
import struct
import zlib

OK, CORRUPT, TRUNCATED = 0, 1, 2
INFLATE_LONG = 65536  # SG_INFLATE_LONG
FINAL_EMPTY = b"\x01\x00\x00\xff\xff"
CL_ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)


def go_stream(data, level=9):
    """A value as pkg/db writes it (db.go:154-162): flate.NewWriter(BestCompression), Write, Flush, Close -- read
    from compress/flate's source as a sync flush followed by the final empty stored block.  Unpinned: that source
    is not among this repository's references."""
    c = zlib.compressobj(level, zlib.DEFLATED, -15)
    return c.compress(bytes(data)) + c.flush(zlib.Z_SYNC_FLUSH) + FINAL_EMPTY


def raw_stream(data, level=9, strategy=zlib.Z_DEFAULT_STRATEGY):
    c = zlib.compressobj(level, zlib.DEFLATED, -15, 9, strategy)
    return c.compress(bytes(data)) + c.flush()


class BitWriter:
    """DEFLATE's bit order: values LSB first, Huffman codes MSB first."""

    def __init__(self):
        self.out = bytearray()
        self.acc = 0
        self.n = 0

    def bits(self, v, n):
        assert 0 <= v < (1 << n)
        self.acc |= v << self.n
        self.n += n
        while self.n >= 8:
            self.out.append(self.acc & 0xFF)
            self.acc >>= 8
            self.n -= 8
        return self

    def code(self, c, n):
        for k in range(n - 1, -1, -1):
            self.bits((c >> k) & 1, 1)
        return self

    def header(self, last, typ):
        return self.bits(last, 1).bits(typ, 2)

    def align(self):
        if self.n:
            self.bits(0, 8 - self.n)
        return self

    def stored(self, last, data, nlen=None):
        self.header(last, 0).align()
        n = len(data)
        self.bits(n, 16).bits((n ^ 0xFFFF) if nlen is None else nlen, 16)
        self.out += bytes(data)
        return self

    def done(self):
        return bytes(self.align().out)

    # ---- the fixed code ----
    def flit(self, s):
        if s < 144:
            return self.code(0x30 + s, 8)
        if s < 256:
            return self.code(0x190 + s - 144, 9)
        if s < 280:
            return self.code(s - 256, 7)
        return self.code(0xC0 + s - 280, 8)

    def fmatch(self, length, dist):
        ls, lb, le = length_symbol(length)
        self.flit(ls).bits(length - lb, le)
        ds, db_, de = dist_symbol(dist)
        return self.code(ds, 5).bits(dist - db_, de)

    def feob(self):
        return self.flit(256)


LBASE = (3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258)
LEXT = (0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0)
DBASE = (1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097,
         6145, 8193, 12289, 16385, 24577)
DEXT = (0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13)


def length_symbol(length):
    if length == 258:
        return 285, 258, 0
    k = max(i for i in range(28) if LBASE[i] <= length)
    return 257 + k, LBASE[k], LEXT[k]


def dist_symbol(dist):
    k = max(i for i in range(30) if DBASE[i] <= dist)
    return k, DBASE[k], DEXT[k]


def canonical(lens):
    """symbol -> (code, length) of the canonical code with these lengths (any lengths: the writer does not judge)."""
    codes, code = {}, 0
    for ln in range(1, 16):
        for s, l in enumerate(lens):
            if l == ln:
                codes[s] = (code, ln)
                code += 1
        code <<= 1
    return codes


def dynamic_header(w, last, lit_lens, dist_lens, cl_lens=None, hlit=None, hdist=None, ncode=19, ops=None):
    """A dynamic block's header.  cl_lens: the code-length code's 19 lengths (default: symbols 0..12 at length 4 and
    13..18 at length 5, which is complete).  ops: the code-length symbols to send as (symbol, extra value) pairs;
    default one plain length per symbol."""
    if cl_lens is None:
        cl_lens = [4] * 13 + [5] * 6  # 13/16 + 6/32 = 1
    w.header(last, 2)
    w.bits((len(lit_lens) if hlit is None else hlit) - 257, 5)
    w.bits((len(dist_lens) if hdist is None else hdist) - 1, 5)
    w.bits(ncode - 4, 4)
    for k in range(ncode):
        w.bits(cl_lens[CL_ORDER[k]], 3)
    cl = canonical(cl_lens)
    if ops is None:
        ops = [(l, None) for l in list(lit_lens) + list(dist_lens)]
    for s, extra in ops:
        w.code(*cl[s])
        if s >= 16:
            w.bits(extra, {16: 2, 17: 3, 18: 7}[s])
    return w


def _lens(n, table):
    out = [0] * n
    for s, l in table.items():
        out[s] = l
    return out


def hand_cases():
    """[(name, stream, status)]: each rejection, and its accepted neighbours."""
    cases = []

    def add(name, stream, status):
        cases.append((name, bytes(stream), status))

    add("final_empty_stored", FINAL_EMPTY, OK)
    add("one_byte_text", go_stream(b"a"), OK)
    add("empty_text_go", go_stream(b""), OK)
    add("block_type_3", BitWriter().header(1, 3).done() + b"\0" * 8, CORRUPT)
    add("stored_len_nlen", BitWriter().stored(1, b"hello", nlen=0x1234).done(), CORRUPT)
    add("stored_len_0", BitWriter().stored(0, b"").stored(1, b"xy").done(), OK)
    add("stored_len_65535", BitWriter().stored(1, bytes(range(256)) * 255 + bytes(255)).done(), OK)
    add("stored_short_body", BitWriter().stored(1, b"hello").done()[:-1], TRUNCATED)
    for j in range(8):  # the stored block's header at bit (2 + j) % 8 of its byte
        w = BitWriter().header(0, 1)
        for k in range(j):
            w.flit(200 + k)
        add("stored_at_bit_%d" % ((2 + j) % 8), w.feob().stored(1, b"stored %d" % j).done(), OK)
    # HLIT / HDIST, checked once the 14 bits are there
    add("hlit_287", BitWriter().header(1, 2).bits(30, 5).bits(0, 5).bits(0, 4).done() + b"\0" * 4, CORRUPT)
    add("hdist_31", BitWriter().header(1, 2).bits(0, 5).bits(30, 5).bits(0, 4).done() + b"\0" * 4, CORRUPT)
    add("hlit_287_short", BitWriter().header(1, 2).bits(30, 5).done()[:1], TRUNCATED)
    # the code-length code
    two = _lens(19, {0: 1, 16: 1})
    add("repeat_without_previous", dynamic_header(BitWriter(), 1, [0] * 257, [0], cl_lens=two, ops=[(16, 0)]).done()
        + b"\0" * 4, CORRUPT)
    z18 = _lens(19, {0: 1, 18: 1})
    add("repeat_past_the_end", dynamic_header(BitWriter(), 1, [0] * 257, [0], cl_lens=z18,
                                              ops=[(18, 127), (18, 127)]).done() + b"\0" * 4, CORRUPT)
    add("no_end_of_block", dynamic_header(BitWriter(), 1, [0] * 257, [0], cl_lens=z18,
                                          ops=[(18, 127), (18, 109)]).done() + b"\0" * 4, CORRUPT)
    add("cl_oversubscribed", dynamic_header(BitWriter(), 1, [0] * 257, [0], cl_lens=_lens(19, {0: 1, 1: 1, 2: 1}),
                                            ops=[]).done() + b"\0" * 8, CORRUPT)
    add("cl_incomplete_single", dynamic_header(BitWriter(), 1, [0] * 257, [0], cl_lens=_lens(19, {0: 1}),
                                               ops=[]).done() + b"\0" * 8, CORRUPT)
    add("cl_all_zero", dynamic_header(BitWriter(), 1, [0] * 257, [0], cl_lens=[0] * 19, ops=[]).done() + b"\0" * 40,
        CORRUPT)
    add("cl_all_zero_short", dynamic_header(BitWriter(), 1, [0] * 257, [0], cl_lens=[0] * 19, ops=[]).done() + b"\0" * 8,
        TRUNCATED)
    # literal/length and distance codes
    add("lit_oversubscribed", dynamic_header(BitWriter(), 1, _lens(257, {0: 1, 1: 1, 256: 1}), [0]).done() + b"\0" * 4,
        CORRUPT)
    add("lit_incomplete", dynamic_header(BitWriter(), 1, _lens(257, {0: 2, 256: 2}), [0]).done() + b"\0" * 4, CORRUPT)
    add("dist_oversubscribed", dynamic_header(BitWriter(), 1, _lens(257, {0: 1, 256: 1}), [1, 1, 1]).done() + b"\0" * 4,
        CORRUPT)
    add("dist_incomplete", dynamic_header(BitWriter(), 1, _lens(257, {0: 1, 256: 1}), [2, 2]).done() + b"\0" * 4, CORRUPT)
    lit3 = _lens(258, {97: 1, 256: 2, 257: 2})
    c3 = canonical(lit3)
    w = dynamic_header(BitWriter(), 1, lit3, [1])       # one distance code of length 1: accepted
    add("dist_single_code", w.code(*c3[97]).code(*c3[257]).code(0, 1).code(*c3[256]).done(), OK)
    w = dynamic_header(BitWriter(), 1, lit3, [1])       # ... and its other, unused, bit pattern
    add("dist_single_code_invalid_bit", w.code(*c3[97]).code(*c3[257]).code(1, 1).done() + b"\0" * 4, CORRUPT)
    w = dynamic_header(BitWriter(), 1, lit3, [0])       # no distance code at all, literals only
    add("dist_none_literals_only", w.code(*c3[97]).code(*c3[97]).code(*c3[256]).done(), OK)
    w = dynamic_header(BitWriter(), 1, lit3, [0])
    add("dist_none_but_used", w.code(*c3[97]).code(*c3[257]).code(0, 1).done() + b"\0" * 4, CORRUPT)
    w = dynamic_header(BitWriter(), 1, _lens(257, {256: 1}), [0])  # one literal/length code of length 1
    add("lit_single_code", w.code(0, 1).done(), OK)
    w = dynamic_header(BitWriter(), 1, _lens(257, {256: 1}), [0])
    add("lit_single_code_invalid_bit", w.code(1, 1).done() + b"\0" * 4, CORRUPT)
    # symbols the fixed code has and the format does not
    add("lit_symbol_286", BitWriter().header(1, 1).flit(97).flit(286).done() + b"\0" * 4, CORRUPT)
    add("lit_symbol_287", BitWriter().header(1, 1).flit(97).flit(287).done() + b"\0" * 4, CORRUPT)
    for ds in (30, 31):
        add("dist_symbol_%d" % ds, BitWriter().header(1, 1).flit(97).flit(257).code(ds, 5).done() + b"\0" * 4, CORRUPT)
    # matches
    add("match_len_3", BitWriter().header(1, 1).flit(97).flit(98).flit(99).fmatch(3, 3).feob().done(), OK)
    add("match_len_258", BitWriter().header(1, 1).flit(97).flit(98).fmatch(258, 2).feob().done(), OK)
    add("match_overlap", BitWriter().header(1, 1).flit(97).flit(98).flit(99).fmatch(10, 2).feob().done(), OK)
    add("match_before_start", BitWriter().header(1, 1).flit(97).flit(98).fmatch(3, 3).feob().done(), CORRUPT)
    add("match_at_start", BitWriter().header(1, 1).fmatch(3, 1).feob().done(), CORRUPT)
    rng = random.Random(32768)
    w = BitWriter().header(1, 1)
    for _ in range(32768):
        w.flit(rng.randrange(256))
    far = w.fmatch(3, 32768).feob().done()
    add("match_dist_32768", far, OK)
    w = BitWriter().header(1, 1)
    for _ in range(32767):
        w.flit(rng.randrange(256))
    add("match_dist_32768_before_start", w.fmatch(3, 32768).feob().done(), CORRUPT)
    add("zeros_100000", raw_stream(bytes(100000)), OK)
    # block types
    add("only_stored", raw_stream(b"stored text " * 9, level=0), OK)
    add("only_fixed", raw_stream(b"fixed fixed text", strategy=zlib.Z_FIXED), OK)
    add("only_dynamic", raw_stream(prog_text(7, 900)), OK)
    add("three_blocks", three_blocks(), OK)
    add("tail_ignored", go_stream(b"tail") + b"\x07garbage", OK)
    return cases


def too_large():
    """A stream whose output passes 2^32 bytes: a dynamic block in which a match of length 258 at distance 1 is
    two zero bits (symbol 285 and distance symbol 0 are both the one-bit code 0), so the zero bytes behind the first
    literal are four matches each.  zlib would write 4 GiB; the decoder stops with SG_INFLATE_TOO_LARGE."""
    lit = _lens(286, {285: 1, 0: 2, 256: 2})
    w = dynamic_header(BitWriter(), 1, lit, [1, 1])
    w.code(*canonical(lit)[0])
    need = (1 << 32) // 258 + 1
    return w.done() + bytes(need // 4 + 8)


def three_blocks():
    """Stored, fixed and dynamic blocks in one stream: chunks joined by Z_FULL_FLUSH."""
    rng = random.Random(3)
    parts = ((bytes(rng.randrange(256) for _ in range(120)), zlib.Z_DEFAULT_STRATEGY),
             (b"short text", zlib.Z_FIXED),
             (b"".join(b"r%d = openat(0x%x, &(0x7f0000000000)='./file0\\x00', 0x0)\n" % (k, k) for k in range(40)),
              zlib.Z_DEFAULT_STRATEGY))
    out = b""
    for data, strategy in parts:
        c = zlib.compressobj(9, zlib.DEFLATED, -15, 9, strategy)
        out += c.compress(data) + c.flush(zlib.Z_FULL_FLUSH)
    return out + FINAL_EMPTY


CALLS =(b"openat", b"read", b"write", b"mmap", b"ioctl$KVM_RUN", b"socket$inet6", b"sendmsg$nl_route", b"close",
         b"bpf$PROG_LOAD", b"setsockopt$inet_tcp_int", b"getpid", b"futex", b"epoll_ctl$EPOLL_CTL_ADD", b"pipe2")


def prog_text(seed, size):
    """A synthetic program of about `size` bytes, in the shape of a serialized syzkaller program."""
    rng = random.Random(seed)
    lines, total, k = [], 0, 0
    while total < size:
        call = CALLS[rng.randrange(len(CALLS))]
        ln = b"r%d = %s(0x%x, &(0x7f0000%06x)={0x%x, 0x%x}, 0x%x)\n" % (k, call, rng.randrange(1 << 16),
                                                                        rng.randrange(1 << 24), rng.randrange(1 << 32),
                                                                        rng.randrange(256), rng.randrange(64))
        lines.append(ln)
        total += len(ln)
        k += 1
    return b"".join(lines)


def valid_streams():
    out = [go_stream(prog_text(s, 40 + 37 * s)) for s in range(12)]
    out += [s for name, s, st in hand_cases() if st == OK and len(s) < 600]
    return out


def mutations(count=20000, seed=20170):
    """Seeded damage of valid streams: bit flips, byte truncations, spliced tails."""
    rng = random.Random(seed)
    base = valid_streams()
    out = []
    while len(out) < count:
        s = bytearray(base[rng.randrange(len(base))])
        kind = rng.randrange(3)
        if kind == 0:
            for _ in range(rng.randrange(1, 4)):
                s[rng.randrange(len(s))] ^= 1 << rng.randrange(8)
        elif kind == 1:
            s = s[:rng.randrange(len(s))]
        else:
            t = base[rng.randrange(len(base))]
            s = s[:rng.randrange(len(s) + 1)] + t[rng.randrange(len(t) + 1):]
        out.append(bytes(s))
    return out


# ---- database files (db.go:125-165) --------------------------------------------
DB_MAGIC, REC_MAGIC, CUR_VERSION, SEQ_DELETED = 0xBADDB, 0xFEE1BAD, 1, (1 << 64) - 1


def db_header(magic=DB_MAGIC, version=CUR_VERSION):
    return struct.pack("<II", magic, version)


def db_record(key, val, seq, stream=None, magic=REC_MAGIC):
    """serializeRecord: val None is a deletion; stream overrides the value's bytes (and so its length field)."""
    out = struct.pack("<II", magic, len(key)) + bytes(key)
    if val is None and stream is None:
        return out + struct.pack("<Q", SEQ_DELETED)
    out += struct.pack("<Q", seq)
    if stream is None:
        stream = go_stream(val) if len(val) else b""
    return out + struct.pack("<I", len(stream)) + stream


def db_file(records):
    """records: (key, val or None, seq) tuples."""
    return db_header() + b"".join(db_record(*r) for r in records)


# The reference's own pkg/db/db_test.go, restated as data: the writes of TestBasic and TestModify in order (val None: a
# Delete), and what their checkContents expects of db.Records after the reopen.
DB_TEST_BASIC = ((b"", b"", 0), (b"1", b"ab", 1), (b"23", b"abcd", 2))
DB_TEST_BASIC_WANT = {b"": (b"", 0), b"1": (b"ab", 1), b"23": (b"abcd", 2)}
DB_TEST_MODIFY = ((b"1", b"ab", 0), (b"23", b"", 1), (b"456", b"abcd", 1), (b"7890", b"a", 0), (b"23", None, 0),
                  (b"1", b"", 5), (b"456", b"ef", 6), (b"7890", None, 0), (b"456", b"efg", 0), (b"7890", b"bc", 0))
DB_TEST_MODIFY_WANT = {b"1": (b"", 5), b"456": (b"efg", 0), b"7890": (b"bc", 0)}
DB_TEST_LARGE_RECORDS = 1000   # TestLarge: keys "0".."999", one random 1000-byte value, seq 0
