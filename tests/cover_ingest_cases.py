"""The case families of the cover ingest (sg_cover_ingest.hip): `objdump -d` and `nm -nS` texts placed on the edges
of the scan's walk, and `addr2line -afi` texts with every failure, the oddities that are legal, random adversarial
sequences and a world of more than 65,536 names (with a2l_model, the kernels' parallel reading restated).  The few constants a case sits on are restated here (tests/test_cover_ingest.py checks them
against the kernel file by regex):

  a text is cut into tiles of TILE bytes; nwaves = min(tiles rounded up to 4, MAX_WAVES), a wave's share is
  ceil(tiles / nwaves) consecutive tiles; a wave walks STEP bytes a step and stores GROUP kept lines at once; a
  line whose content is MAX_LINE bytes or more fails the call.
"""
TILE = 1024                  # kCiTile
STEP = 64
GROUP = 64                   # lines held before a store
MAX_WAVES = 1 << 13          # kCiMaxWaves
MAX_LINE = 65536             # SG_INGEST_MAX_LINE
MAX_NEEDLE = 64              # SG_INGEST_MAX_NEEDLE

CALL = b"callq "
FUNC = b" <__sanitizer_cov_trace_pc>"


def ntiles(nbytes):
    return (nbytes + TILE - 1) // TILE


def nwaves(tiles):
    return min((tiles + 3) & ~3, MAX_WAVES)


class Text:
    """A text under construction: filler lines steer what follows to an absolute position."""

    def __init__(self, filler=b"#"):
        self.b = bytearray()
        self.filler = filler

    def pad_to(self, pos):
        """filler lines (they match nothing) up to exactly `pos`, which starts a line"""
        need = pos - len(self.b)
        assert need >= 0 and (need != 0 or not self.b or self.b[-1] == 10), (pos, len(self.b))
        while need > 0:
            n = min(need, 200)
            if need - n == 1:
                n -= 1
            self.b += self.filler * (n - 1) + b"\n"
            need -= n
        return self

    def add(self, line):
        self.b += line
        return self

    def bytes(self):
        return bytes(self.b)


def site(pc, call=CALL, func=FUNC, pre=b"       ", mid=b" ffffffff815cc1d0", tail=b"\n"):
    """a call-site line as objdump prints it"""
    return b"%x:" % pc + pre + call + mid + func + tail


def other(k):
    """an objdump line that is no call site"""
    return (b"%x:       mov    %%rax,0x%x(%%rbp)\n" % (0xffffffff81000000 + 4 * k, k % 4096),
            b"%x:       callq  ffffffff81%06x <schedule>\n" % (0xffffffff81000000 + 4 * k, k),
            b"\n", b"ffffffff81%06x <func_%d>:\n" % (k, k))[k % 4]


# ---- the line rule, for either scanner ------------------------------------------------------------
def long_line(kind, content):
    """a kept line of exactly `content` bytes"""
    if kind == "objdump":
        head, tail = b"1f:", CALL + b"x" + FUNC
        return head + b" " * (content - len(head) - len(tail)) + tail
    head = b"00000000000000aa 0000000000000010 t "
    return head + b"n" * (content - len(head))


def short_line(kind, k):
    return site(0x100 + k, tail=b"") if kind == "objdump" else b"%016x %016x T sym_%d" % (0x1000 + 32 * k, 7 + k, k)


def line_rule_texts(kind):
    """[(name, text)]: no trailing '\\n', "\\r\\n", empty lines, the empty text, and a line of MAX_LINE - 1 and of
    MAX_LINE content bytes at the start, in the middle and at the end (with and without its '\\n')."""
    s = [short_line(kind, k) for k in range(6)]
    out = [("empty", b""), ("newline_only", b"\n"), ("no_trailing_newline", s[0] + b"\n" + s[1]),
           ("crlf", s[0] + b"\r\n" + s[1] + b"\r\n" + s[2] + b"\r"), ("empty_lines", b"\n\n" + s[0] + b"\n\n\r\n" + s[1] + b"\n\n"),
           ("cr_only_lines", b"\r\n\r\r\n" + s[0] + b"\r\r\n" + s[1] + b"\n")]
    for content in (MAX_LINE - 1, MAX_LINE):
        ln = long_line(kind, content)
        assert len(ln) == content
        front, back = s[0] + b"\n" + s[1] + b"\n", s[2] + b"\n" + s[3] + b"\n"
        out += [("start_%d" % content, ln + b"\n" + back), ("middle_%d" % content, front + ln + b"\n" + back),
                ("end_nl_%d" % content, front + ln + b"\n"), ("end_%d" % content, front + ln),
                ("cr_%d" % content, front + ln[:-1] + b"\r\n" + back)]  # the '\r' counts
    out.append(("two_long", s[0] + b"\n" + b"x" * (MAX_LINE + 5) + b"\n" + s[1] + b"\n" + b"y" * (3 * MAX_LINE) + b"\n"))
    return out


# ---- objdump ------------------------------------------------------------------------------------
def objdump_offsets():
    """(text, expected PCs): the call needle, then the trace needle, starting at every offset of a 64-byte step
    and at every place across a tile boundary; line k's PC is k + 1."""
    t, want = Text(), []

    def place(at, which):
        pc = len(want) + 1
        ln = site(pc)
        start = at - ln.index(CALL if which == 0 else FUNC)
        t.pad_to(start).add(ln)
        assert t.b.index(CALL if which == 0 else FUNC, start) == at
        want.append(pc)

    at = 256
    for which in (0, 1):
        for o in range(STEP):
            place(at + o, which)
            at += 256
        at = (at // TILE + 2) * TILE
        for j in range(len(FUNC) + 2):  # the needle's first byte from TILE - len - 1 up to TILE
            place(at - j, which)
            at += 2 * TILE
    return t.pad_to(len(t.b) + 300).bytes(), want


def objdump_rules():
    """[(line, kept PC or None)]: the per-line rule, one reason a line."""
    z = b"ffffffff8100206a"
    rest = b"       " + CALL + b" ffffffff815cc1d0" + FUNC
    return [
        (z + b":" + rest, 0xffffffff8100206a),
        (z + b":   " + CALL + b"x " + CALL + b"y" + FUNC, 0xffffffff8100206a),          # the call needle twice
        (z + b": " + FUNC + b" " + CALL + b"ffffffff815cc1d0 <other>", None),           # the trace needle only before pos
        (z + b": " + FUNC + b" " + CALL + b"q" + FUNC, 0xffffffff8100206a),             # ... and again behind it
        (z + b": " + CALL[:-1] + b"\t" + FUNC, None),                                    # "callq\t": no call needle
        (z + rest, None),                                                                # no ':'
        (z + rest + b":", None),                                                         # the ':' behind: ln[:colon] is no number
        (b":" + rest, None),                                                             # an empty field
        (b"ab:cd:" + rest, 0xab),                                                        # the first ':' counts
        (b"1:" + rest, 1),
        (b"0123456789abcdef:" + rest, 0x0123456789abcdef),                               # 16 digits
        (b"ffffffffffffffff:" + rest, 0xffffffffffffffff),
        (b"00123456789abcdef:" + rest, 0x0123456789abcdef),                              # 17 digits, a leading zero
        (b"0" * 24 + b"fedcba9876543210:" + rest, 0xfedcba9876543210),                   # 40 digits
        (b"0" * 100 + b"7:" + rest, 7),                                                  # a field longer than a step
        (b"10000000000000000:" + rest, None),                                            # 17 significant digits
        (b"0" * 30 + b"1" + b"0" * 16 + b":" + rest, None),
        (b"FFFFFFFF8100ABCD:" + rest, 0xffffffff8100abcd),                               # upper case
        (b"aBcDeF:" + rest, 0xabcdef),
        (b"  10:" + rest, None),                                                         # as objdump indents small addresses
        (b"0x10:" + rest, None), (b"+10:" + rest, None), (b"-10:" + rest, None), (b"1_0:" + rest, None),
        (b"10 :" + rest, None), (b"1g:" + rest, None), (b"1\x00:" + rest, None), (b"\xff1:" + rest, None),
        (b"12:" + rest[:-1], None),                                                      # the trace needle cut short
        (b"13:" + rest + b"\r", 0x13),
    ]


def objdump_rules_text():
    rules = objdump_rules()
    text = b"".join(other(k) + ln + b"\n" for k, (ln, _) in enumerate(rules))
    return text, sorted(pc for _, pc in rules if pc is not None)


def objdump_tile_edge():
    """(text, PCs): a call-site line starting in a tile's last byte, in its first byte, and one whose '\\n' is a
    tile's last byte; a '\\r' as a tile's last byte."""
    t, want = Text(), []
    for k, (at, cr) in enumerate([(TILE - 1, False), (2 * TILE, False), (4 * TILE - 1, False), (6 * TILE, False)]):
        ln = site(0x40 + k)
        t.pad_to(at).add(ln)
        want.append(0x40 + k)
    ln = site(0x50)
    t.pad_to(9 * TILE - len(ln)).add(ln)             # its '\n' at 9 * TILE - 1
    ln = site(0x51, tail=b"\r\n")
    t.pad_to(11 * TILE - len(ln) + 1).add(ln)        # its '\r' at 11 * TILE - 1
    want += [0x50, 0x51]
    return t.bytes(), want


def objdump_order():
    """descending PCs with repeats: the output is sorted and keeps them"""
    pcs = [0xffffffff81000000 + 16 * ((977 * k) % 300) for k in range(700)] + [5, 5, 0xffffffffffffffff, 0, 0]
    pcs = sorted(pcs, reverse=True)[:350] + pcs
    return b"".join(site(pc) + other(k) for k, pc in enumerate(pcs)), sorted(pcs)


DENSE_CALL, DENSE_FUNC = b"c", b"f"


def objdump_dense():
    """(text, PCs) under one-byte needles: five-byte call sites, 204 to a tile, so every tile fills three store
    groups and a part of a fourth"""
    pcs = [(7 * k) % 16 for k in range(1500)]
    return b"".join(b"%x:cf\n" % pc for pc in pcs), sorted(pcs)


def objdump_many_tiles():
    """(text, PCs): more tiles than MAX_WAVES, so a wave walks several; sites sparse and in descending order"""
    block = b"".join(other(k) for k in range(0, 64)) + b"ffffffff81000000:       nopw   0x0(%rax,%rax,1)" + b" " * 120 + b"\n"
    reps = (MAX_WAVES + 500) * TILE // (len(block) + 60) + 1
    parts, pcs = [], []
    for r in range(reps):
        parts.append(block)
        if r % 3 == 0:
            pcs.append(0xffffffff90000000 - 5 * r)
            parts.append(site(pcs[-1]))
    return b"".join(parts), sorted(pcs)


# ---- nm --------------------------------------------------------------------------------------
def nm_rules():
    """[(line, kept (addr, size field, name) or None)]"""
    a, z = b"ffffffff8104db90", b"0000000000000059"
    return [
        (a + b" " + z + b" t snb_uncore_msr_enable_box", (0xffffffff8104db90, 0x59, b"snb_uncore_msr_enable_box")),
        (a + b" " + z + b" T _stext", (0xffffffff8104db90, 0x59, b"_stext")),
        (b"0000000000401000 T _init", None),                                   # no size: ln[sp2:] is " _init"
        (b"0000000000401000 T t x", None),                                     # ... even when " t " follows
        (a + b" " + z + b" D has t in name", None),                            # " t " only inside the name
        (a + b" " + z + b" d x", None), (a + b" " + z + b" W x", None), (a + b" " + z + b" r x", None),
        (a + b" " + z + b" b x", None), (a + b" " + z + b" A x", None), (a + b" " + z + b" U x", None),
        (a + b" " + z + b" t", None),                                          # no blank behind the letter
        (a + b" " + z + b" t ", (0xffffffff8104db90, 0x59, b"")),              # an empty name
        (a + b" " + z + b" T a name with blanks ", (0xffffffff8104db90, 0x59, b"a name with blanks ")),
        (a + b" " + z + b" t  t ", (0xffffffff8104db90, 0x59, b" t ")),
        (a + b"  " + z + b" t x", None),                                       # two blanks: an empty size field
        (b" " + a + b" " + z + b" t x", None),                                 # a leading blank: an empty addr field
        (a + b" 0 t size0", (0xffffffff8104db90, 0, b"size0")),
        (a + b" 1 t size1", (0xffffffff8104db90, 1, b"size1")),
        (a + b" 10 t size16", (0xffffffff8104db90, 16, b"size16")),
        (a + b" 11 t size17", (0xffffffff8104db90, 17, b"size17")),
        (a + b" ffffffffffffffff t wraps", (0xffffffff8104db90, 0xffffffffffffffff, b"wraps")),
        (a + b" fffffffffffffff1 t wraps_to_zero", (0xffffffff8104db90, 0xfffffffffffffff1, b"wraps_to_zero")),
        (a + b" fffffffffffffff0 t minus_one", (0xffffffff8104db90, 0xfffffffffffffff0, b"minus_one")),
        (a + b" 8000000000000000 t negative", (0xffffffff8104db90, 1 << 63, b"negative")),
        (a + b" 7ffffffffffffff1 t flips_sign", (0xffffffff8104db90, 0x7ffffffffffffff1, b"flips_sign")),
        (b"fffffffffffffff0 0000000000000020 T end_wraps", (0xfffffffffffffff0, 0x20, b"end_wraps")),
        (b"10000000000000000 10 t x", None), (a + b" 10000000000000000 t x", None),
        (b"0" * 70 + b"FFFF 0" + b"0" * 90 + b"1f t long_fields", (0xffff, 0x1f, b"long_fields")),
        (b"0x10 10 t x", None), (a + b" +10 t x", None), (a + b" 1g t x", None), (a + b"\t10 t x", None),
        (a + b" " + z + b" T crlf\r", (0xffffffff8104db90, 0x59, b"crlf")),
        (a + b" " + z + b" t \r", (0xffffffff8104db90, 0x59, b"")),
        (a + b" " + z + b" t\r", None),
    ]


def nm_rules_text():
    return b"".join(ln + b"\n" for ln, _ in nm_rules())


def nm_ties():
    """symbols in a scrambled order with equal starts: the pinned order is (start, text order)"""
    lines = []
    for k in range(900):
        start = 0xffffffff81000000 + 64 * ((613 * k) % 200)   # 200 starts, each four or five times
        lines.append(b"%016x %016x %c dup_%d\n" % (start, (k * 37) % 300, b"tT"[k % 2], k))
    return b"".join(lines)


def nm_dense():
    """seven-byte symbols, 146 to a tile"""
    return b"".join(b"%x %x t \n" % ((5 * k) % 16, k % 16) for k in range(1200))


def nm_tile_edge():
    """a symbol line starting in a tile's last byte, its blanks and its letter on both sides of a boundary, and a
    name longer than a tile"""
    t = Text(filler=b"-")
    ln = b"%016x %016x t edge_%d\n"
    for k, at in enumerate([TILE - 1, 2 * TILE - 16, 3 * TILE - 17, 4 * TILE - 33, 5 * TILE - 34, 6 * TILE - 35, 7 * TILE - 36]):
        t.pad_to(at).add(ln % (0x2000 - 16 * k, 16 + k, k))
    t.pad_to(9 * TILE - 100).add(b"%016x %016x T " % (0x10, 0x20) + b"N" * (2 * TILE + 77) + b"\n")
    return t.add(ln % (1, 2, 99)).bytes()


# ---- getVmOffset ------------------------------------------------------------------------------
READELF = (b"There are 40 section headers, starting at offset 0x1a2b3c8:\n\nSection Headers:\n"
           b"  [Nr] Name              Type            Address          Off    Size   ES Flg Lk Inf Al\n"
           b"  [ 0]                   NULL            0000000000000000 000000 000000 00      0   0  0\n"
           b"  [ 1] .text             PROGBITS        ffffffff81000000 200000 e00000 00  AX  0   0 4096\n"
           b"  [ 2] .notes            NOTE            ffffffff81e00000 1000000 0001bc 00   A  0   0  4\n"
           b"  [ 3] .rodata           PROGBITS        ffffffff82000000 1200000 3fa000 00  WA  0   0 4096\n"
           b"  [ 4] .comment          PROGBITS        0000000000000000 2600000 00002c 01  MS  0   0  1\n"
           b"  [ 5] .bss              NOBITS          ffffffff83000000 2600000 500000 00  WA  0   0 4096\n")


def vm_offset_cases():
    """[(text, offset or None for an error)]"""
    bad = READELF + b"  [ 6] .user             PROGBITS        0000000000400000 2600000 000010 00  WA  0   0 1\n"
    return [
        (READELF, 0xffffffff), (b"", 0), (READELF.replace(b"\n", b"\r\n"), 0xffffffff),
        (bad, None),                                                         # different section offsets
        (b" [ 1] .a PROGBITS 0000000000400000 0\n [ 2] .b PROGBITS ffffffff81000000 0\n", 0xffffffff),  # addr stays 0
        (READELF + b"  [ 6] .x PROGBITS", None),                             # the reference's index panic
        (READELF + b"  [ 6] .x PROGBITS zz 0\n", None), (READELF + b"  [ 6] .x PROGBITS 0x10 0\n", None),
        (b"x PROGBITS ffff_ffff_8100_0000 0\n", 0xffffffff), (b"x PROGBITS _ffffffff81000000 0\n", 0xffffffff),
        (b"x PROGBITS ffffffff81000000_ 0\n", None), (b"x PROGBITS ff__ff 0\n", None),
        (b"x PROGBITS 1ffffffff81000000 0\n", None),                         # out of range
        (b"x\tPROGBITS\x0bffffffff81000000\x0c0\n", 0xffffffff),
        (b"x PROGBITS PROGBITS 1\n", None),                                  # "0xPROGBITS"
        (READELF + b"y" * MAX_LINE + b"\n" + bad, 0xffffffff),               # the scan ends at the long line, unreported
    ]


# ---- addr2line ----------------------------------------------------------------------------------
def a2l_model(text, nrec, OR):
    """The parallel reading of an addr2line output that the kernels take (sg_cover_ingest.hip k_al_*), restated
    line by line: (status, pos, records).  tests/test_cover_ingest.py holds it against the sequential oracle."""
    n = len(text)
    if n == 0:
        return OR.A2L_EMPTY, 0, None
    starts, s = [], 0
    while s < n:
        starts.append(s)
        e = text.find(b"\n", s)
        s = n if e < 0 else e + 1
    L = len(starts)
    lines = []
    for i, s in enumerate(starts):
        e = starts[i + 1] - 1 if i + 1 < L else (n - 1 if text.endswith(b"\n") else n)
        lng = e - s >= MAX_LINE
        ln = None if lng else (text[s:e - 1] if text[s:e].endswith(b"\r") else text[s:e])
        shaped = (not lng) and len(ln) > 3 and ln[:2] == b"0x"
        colon = -1 if lng else ln.rfind(b":")
        lines.append((s, ln, lng, shaped, colon, i == 0 or (shaped and colon < 0)))
    rline = [i for i in range(L) if lines[i][5]] + [L]
    nr = len(rline) - 1
    rec_of, r = [], -1
    for i in range(L):
        r += lines[i][5]
        rec_of.append(r)
    term = L
    if 1 <= nrec <= nr:
        term = rline[nrec]
        for i in range(rline[nrec - 1] + 1, rline[nrec], 2):
            if lines[i][3]:
                term = i
                break
    fails, recs = [], [[None, []] for _ in range(min(nrec, nr))]
    if nr < nrec:
        fails.append((n, OR.A2L_TOO_FEW))
    for i in range(L):
        s, ln, lng, shaped, colon, start = lines[i]
        r = rec_of[i]
        if nrec == 0:
            if i == 0 and lng:
                fails.append((s, OR.A2L_TOO_LONG))
            continue
        if start and 1 <= r <= nrec and (r < nrec or term == i) and (i - rline[r - 1] - 1) & 1:
            fails.append((s, OR.A2L_NO_COLON))
            continue                      # read as a file line, it is never parsed as a PC
        if r >= nrec or (r == nrec - 1 and i >= term):
            continue
        if lng:
            fails.append((s, OR.A2L_TOO_LONG))
            continue
        place = i - rline[r]
        if place == 0:
            pc = OR.parse_uint0(ln)
            if pc is None:
                fails.append((s, OR.A2L_BAD_PC))
            recs[r][0] = pc
        elif place % 2 == 0:
            if colon < 0:
                fails.append((s, OR.A2L_NO_COLON))
        elif shaped:
            fails.append((s, OR.A2L_BAD_PC))
        else:
            rend = min(rline[r + 1], term) if r == nrec - 1 else rline[r + 1]
            if i + 1 >= rend:
                if i + 1 == L:
                    fails.append((s, OR.A2L_NO_FILE_LINE))
                continue
            s2, ln2, lng2, _, colon2, _ = lines[i + 1]
            if lng2 or colon2 < 0:
                continue
            end = colon2 + 1
            while end < len(ln2) and 0x30 <= ln2[end] <= 0x39:
                end += 1
            digits, file = ln2[colon2 + 1:end], ln2[:colon2]
            if not digits or not 0 < int(digits) <= OR.INT_MAX or ln in (b"", b"??") or file in (b"", b"??"):
                continue
            recs[r][1].append((ln, file, int(digits), s, s2))
    if fails:
        pos, status = min(fails)
        return status, pos, None
    return OR.A2L_OK, 0, [(pc, fr) for pc, fr in recs]


A2L_LINES = [b"0xffffffff81000010", b"0x10", b"0x1", b"0x", b"0xzz", b"0x10:3", b"0x1f:x", b"main", b"??", b"", b"a b",
             b"/k/a.c:10", b"/k/a.c:0", b"??:0", b"??:7", b"/k/b.h:588 (discriminator 3)", b"C:/x.c:5", b":9", b"nocolon",
             b"/k/c.c:", b"/k/c.c:007", b"/k/c.c:99999999999999999999", b"0x10\r", b"/k/a.c:10\r", b"main\r", b"017", b"12",
             b"0X1F", b"0b101", b"0o17", b"1_0", b"0x_1f", b"0x1__f", b"f:9223372036854775807", b"f:9223372036854775808"]


def a2l_random_texts(seed, count):
    """adversarial sequences of A2L_LINES, some well formed at their start"""
    import random

    rng = random.Random(seed)
    out = []
    for _ in range(count):
        k = rng.randrange(0, 14)
        if rng.random() < 0.5:       # a well-formed prefix: records of whole frames
            parts = []
            for _ in range(rng.randrange(1, 4)):
                parts.append(rng.choice(A2L_LINES[:2]))
                for _ in range(rng.randrange(0, 3)):
                    parts += [rng.choice(A2L_LINES[7:11]), rng.choice(A2L_LINES[11:17] + A2L_LINES[5:7])]
            parts += [rng.choice(A2L_LINES) for _ in range(rng.randrange(0, 4))]
        else:
            parts = [rng.choice(A2L_LINES) for _ in range(k)]
        text = b"\n".join(parts) + (b"\n" if rng.random() < 0.8 and parts else b"")
        out.append((text, rng.randrange(0, 5)))
    return out


def a2l_render(records, sentinel=True):
    """records [(pc, [(func, file, line)])] as `addr2line -afi` prints them, with the sentinel's record"""
    out = []
    for pc, frames in records:
        out.append(b"0x%016x" % pc)
        for fn, file, line in frames or [(b"??", b"??", 0)]:
            out += [fn, b"%s:%d" % (file, line) if file != b"??" else b"??:0"]
    if sentinel:
        out += [b"0xffffffffffffffff", b"??", b"??:0"]
    return b"\n".join(out) + b"\n"


def a2l_world(nrec=700, nfiles=90, nfuncs=70000, seed=3):
    """records with 0, 1 and up to 70 frames, more than 65,536 distinct function names, names shared across
    records so that first-occurrence order is not hash order"""
    import random

    rng = random.Random(seed)
    recs, k = [], 0
    for r in range(nrec):
        nf = (0, 1, 1, 2, 3, 70, 200)[r % 7] if r % 50 else 0
        frames = []
        for _ in range(nf):
            if rng.random() < 0.3 and k:
                f = rng.randrange(k)
            else:
                f, k = k, k + 1
            frames.append((b"fn_%d" % (f * 7919 % 1000003), b"/src/dir%d/file_%d.c" % (f % 7, f % nfiles), 1 + f % 5000))
        recs.append((0xffffffff81000000 + 16 * r, frames))
    # pad with single-frame records until the function names pass 65,536
    while k < nfuncs:
        recs.append((0xffffffff82000000 + 16 * k, [(b"g%d" % k, b"/src/gen/%d.h" % (k % 40000), 1 + k % 99)]))
        k += 1
    return recs


def a2l_failure_cases():
    """[(name, text, nrec)]: every failure kind at the first record, at the last one and with the failing line
    across a tile boundary; what lies behind the last record and must not fail; legal oddities."""
    ok = [(0x10 + r, [(b"fn%d" % r, b"/s/f%d.c" % (r % 3), 5 + r)]) for r in range(40)]
    good = a2l_render(ok)
    lines = good.split(b"\n")[:-1]
    out = [("ok", good, 40), ("ok_fewer", good, 7), ("ok_with_sentinel", good, 41), ("too_few", good, 42),
           ("too_few_far", good, 100000), ("nrec_0", good, 0), ("empty", b"", 3), ("empty_nrec_0", b"", 0),
           ("only_newline", b"\n", 1), ("no_sentinel_end_of_text", a2l_render(ok, sentinel=False), 40),
           ("no_final_newline", good[:-1], 41)]

    def edit(name, idx, new, nrec=40):
        ls = list(lines)
        ls[idx:idx + 1] = new
        out.append((name, b"\n".join(ls) + b"\n", nrec))

    for where, rec in (("first", 0), ("last", 39)):
        edit("bad_pc_" + where, 3 * rec, [b"0xnothex"])
        edit("bad_pc_colon_" + where, 3 * rec + 1, [b"0x12:3"] if rec else [b"fn", b"/s/x.c:1", b"0x12:3"])
        edit("no_colon_" + where, 3 * rec + 2, [b"no colon here"])
        edit("odd_lines_" + where, 3 * rec + 2, [])                     # the next start is read as a file line
        edit("too_long_" + where, 3 * rec + 1, [b"L" * MAX_LINE])
        edit("long_ok_" + where, 3 * rec + 1, [b"L" * (MAX_LINE - 1)])  # a name of 64 tiles
    edit("too_long_line0", 0, [b"0x" + b"1" * MAX_LINE])
    edit("long_ok_line0", 0, [b"0" * (MAX_LINE - 3) + b"17"])             # octal 15 behind 65,532 zeros
    for k, rec in enumerate((13, 26)):                                    # in the middle: a function and a file line
        edit("too_long_middle_%d" % k, 3 * rec + 1 + k, [b"M" * MAX_LINE])
        edit("long_ok_middle_%d" % k, 3 * rec + 1 + k, [(b"M" * (MAX_LINE - 3) + b":7")[:MAX_LINE - 1]])
    edit("bad_pc_line0_empty", 0, [b""])
    edit("pc_octal", 0, [b"017"])
    edit("pc_decimal", 0, [b"12345"])
    edit("pc_binary_underscore", 0, [b"0b1_01"])
    edit("pc_0x1_is_no_start", 3, [b"0x1", b"/s/q.c:3"])               # len 3: a function name
    edit("shaped_file_line", 2, [b"0x10:77"])                           # legal: file "0x10"
    edit("colon_in_file", 2, [b"C:/dir:x/y.c:12:34"])                   # the last ':' counts: file "C:/dir:x/y.c:12"
    edit("discriminator", 2, [b"/s/d.c:588 (discriminator 3)"])
    edit("dropped_frames", 1, [b"??", b"/s/a.c:1", b"f", b"??:3", b"", b"/s/a.c:2", b"g", b":4", b"h", b"/s/a.c:0",
                               b"i", b"/s/a.c:", b"j", b"/s/a.c:x", b"k", b"/s/a.c:00012", b"l", b"/s/a.c:9223372036854775808",
                               b"m", b"/s/a.c:9223372036854775807", b"n\r", b"/s/a.c:5\r", b"z"])
    edit("eof_after_function", 3 * 39 + 1, [b"fn", b"/s/a.c:1", b"dangling"], nrec=40)
    out[-1] = (out[-1][0], b"\n".join(out[-1][1].split(b"\n")[:3 * 39 + 4]) + b"\n", 40)   # cut: the text ends there
    # behind the last record: none of it is read
    tail = b"\n".join([b"0xnothex", b"f", b"no colon", b"L" * MAX_LINE, b"0x5:5"]) + b"\n"
    out.append(("garbage_behind_last", b"\n".join(lines[:3 * 7]) + b"\n" + b"0x999\n" + tail, 7))
    out.append(("garbage_in_sentinel", b"\n".join(lines[:3 * 7]) + b"\n0xffffffffffffffff\nf\nno colon\n" + tail, 7))
    out.append(("last_record_ends_at_colon_line", b"\n".join(lines[:3 * 7]) + b"\n0x12:3\n" + tail, 7))
    out.append(("colon_line_before_last", b"\n".join(lines[:3 * 7]) + b"\n0x12:3\n" + tail, 8))
    out.append(("too_long_reached", b"\n".join(lines[:3 * 7]) + b"\n" + b"L" * MAX_LINE + b"\n0x999\n", 7))
    # the failing line across a tile boundary
    pad = [(0x1000 + r, [(b"p" * 50, b"/p/" + b"q" * 40 + b".c", 1)]) for r in range(9)]
    body = a2l_render(pad, sentinel=False)
    for name, bad in (("tile_no_colon", b"x\n" + b"y" * 30 + b"\n"), ("tile_bad_pc", b"0x" + b"g" * 30 + b"\n"),
                      ("tile_too_long", b"T" * MAX_LINE + b"\n/t/z.c:9\n"), ("tile_no_file_line", b"d" * 30),
                      ("tile_ok", b"fn\n/t/" + b"z" * 30 + b".c:9\n")):
        cut = TILE - 16
        assert len(body) > cut
        k = body.rfind(b"\n0x", 0, cut) + 1
        head = body[:k]
        fill = b"0x77\n" + b"w" * (cut - len(head) - 5 - 6 - 1) + b"\n" + b"/w:1\n"
        text = head + fill + (b"0x78\n" if name != "tile_bad_pc" else b"") + bad
        text += b"0x79\n??\n??:0\n" if name != "tile_no_file_line" else b""      # (that one: the text ends there)
        out.append((name, text, text.count(b"\n0x") + (name == "tile_no_file_line")))   # every record but the sentinel's
    return out
