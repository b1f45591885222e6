"""Cases of tests/test_call_set_edges.py: program texts at the edges of the CallSet scan that the cases of
tests/hub_state_cases.py do not reach -- the 64-lines-a-store groups of a dense tile, the tile boundary, lines
longer than a tile, a wave with more than one tile, wide tiles of the device form, and the long-line limit at
every place of a step.

What is restated here from sg_call_set.hip and from the walk it runs (sgd::walk_lines and sgd::LineGroup of
sg_linewalk.h), and nothing else of them:
  a tile is TILE << shift bytes of a program, counted from the program's start, and owns the lines that start
      in it;
  tile_bound = nbytes // TILE + 1 + nprogs, nwaves = min(tile_bound rounded up to 4, MAX_WAVES), a wave's share
      is per = ceil(total tiles / nwaves) consecutive tiles of the batch;
  the device form takes the least shift at which sum(max(ceil(len / (TILE << shift)) - 1, 0)) + nprogs is at
      most tile_bound (the host forms take shift 0);
  a wave stores the call lines of a tile GROUP at a time.
The expected values never come from these: they are the oracle's (tests/hub_state_oracle.py), and the
restatement only shows, on the CPU, that a case is where it claims to be."""
import numpy as np

from tests import hub_state_cases as K
from tests import hub_state_oracle as OR

MAX_LINE = K.MAX_LINE
STEP, TILE = K.STEP, K.TILE
GROUP = 64                   # call lines a wave holds before it stores them
MAX_WAVES = 1 << 16          # kCsMaxWaves
DENSE_COUNTS = (63, 64, 65, 85, 86)
LETTERS = [bytes([c]) for c in range(ord("a"), ord("z") + 1)]
TABLE_LETTERS = LETTERS[::3] + [b"z"]          # the name table of the dense family: some letters, not all


# ---- the restatement -----------------------------------------------------------
def ntiles(length, tile=TILE):
    return (length + tile - 1) // tile


def tile_bound(nprogs, nbytes):
    return nbytes // TILE + 1 + nprogs


def nwaves(bound):
    return min((bound + 3) & ~3, MAX_WAVES)


def shares(lengths, nbytes=None, tile=TILE):
    """(tile_off, per, nwaves) of a batch of programs of these lengths."""
    lengths = [int(x) for x in lengths]
    nbytes = sum(lengths) if nbytes is None else nbytes
    tile_off = np.concatenate([[0], np.cumsum([ntiles(x, tile) for x in lengths])]).astype(np.int64)
    nw = nwaves(tile_bound(len(lengths), nbytes))
    total = min(int(tile_off[-1]), tile_bound(len(lengths), nbytes))
    return tile_off, (total + nw - 1) // nw, nw


def pick_shift(lengths, nbytes):
    """The shift the device form takes for programs of these (clamped) lengths over nbytes of text."""
    n = len(lengths)
    for k in range(33):
        if sum(max(ntiles(x, TILE << k) - 1, 0) for x in lengths) + n <= tile_bound(n, nbytes) or k == 32:
            return k


def tile_profile(progs, tile=TILE):
    """For each program the number of call lines that start in each of its tiles (the oracle's call lines: a
    failing program has none)."""
    out = []
    for p in progs:
        p = bytes(p)
        counts = np.zeros(ntiles(len(p), tile), np.int64)
        st, lines = OR.call_lines(p)
        if lines:
            nl = np.flatnonzero(np.frombuffer(p, np.uint8) == 10)
            pos = np.array([a for a, _ in lines], np.int64)
            at = np.searchsorted(nl, pos)                      # the '\n's in front of each name
            start = np.where(at > 0, nl[np.maximum(at, 1) - 1] + 1, 0)
            counts += np.bincount(start // tile, minlength=counts.size)
        out.append(counts.tolist())
    return out


def comment(n):
    """A comment line of n bytes, its '\\n' counted (n == 1: an empty line)."""
    assert n >= 1
    return b"#" * (n - 1) + b"\n" if n > 1 else b"\n"


# ---- 1: dense tiles ----------------------------------------------------------------
def dense_tile(n, first=0):
    """n call lines `x(\\n` from a tile's first byte, x cycling through the letters from LETTERS[first], and a
    comment up to the tile's end (the 86th line starts on the tile's last byte and ends in the next tile)."""
    body = b"".join(LETTERS[(first + k) % 26] + b"(\n" for k in range(n))
    return body + (comment(TILE - len(body)) if len(body) < TILE else b"")


def dense_progs():
    """[(text, tile that is dense, its call lines)]: each count of DENSE_COUNTS in a first tile and in a second
    one, a few call lines behind it; then twelve dense tiles in a row."""
    out = []
    for k, n in enumerate(DENSE_COUNTS):
        out.append((dense_tile(n, k) + b"y(\nr1 = zz(\nq(\n", 0, n))
        lead = b"r0 = open(0x1)\nclose(\nb(\n"
        lead += comment(TILE - len(lead))
        out.append((lead + dense_tile(n, 2 * k + 1) + b"y(\nr1 = zz(\nq(\n", 1, n))
    out.append((b"a(\n" * 1000, 0, 86))
    return out


def dense_batch():
    """(progs, indices of the dense ones): short and empty programs between the dense ones."""
    progs, at = [b"", b"open(0x1)\n"], []
    short = K.mixed(40, 77)
    for k, (text, _, _) in enumerate(dense_progs()):
        at.append(len(progs))
        progs.append(text)
        progs += [short[3 * k], b"", b"", b"x", short[3 * k + 1], b""][:1 + k % 6]
    return progs, at


# ---- 2: tile boundaries ------------------------------------------------------------
BOUNDARY_OFFSETS = (tuple(range(180, 331)), tuple(range(436, 591)))
BOUNDARY_WINDOWS = (range(253, 260), range(509, 516))
PROGRAM_LENGTHS = (255, 256, 257, 511, 512, 513)


def sized(n, tail):
    """A program of n bytes: a call line, a comment up to the tail, the tail."""
    head = b"f(0x1)\n"
    return head + comment(n - len(head) - len(tail)) + tail


def length_progs():
    """[(text, status, note)]: programs whose length is a tile, or a byte less or more, with each ending."""
    out = []
    for n in PROGRAM_LENGTHS:
        out.append((sized(n, b"g()\n"), 0, "the final newline is the last byte"))
        out.append((sized(n, b"g()"), 0, "a call line ended by the program's end"))
        out.append((sized(n, b"g()\r\n"), 0, "CR LF the last two bytes"))
    for n in (257, 513):
        out.append((sized(n, b"x"), 1, "a last tile of one byte, a line without a bracket"))
        out.append((sized(n, b"\n"), 0, "a last tile that holds only an empty line's newline"))
        out.append((sized(n, b"\r"), 0, "a last tile that holds only a line of one CR"))
        out.append((sized(n, b"g()\r"), 0, "a last tile that holds only the CR that ends a call line"))
        out.append((sized(n - 1, b"\n") + b"(", 2, "a last tile of one byte, an empty name"))
    return out


# ---- 3: lines that span tiles --------------------------------------------------------
SPAN_STARTS = (0, 1, 254, 255, 256, 257)
SPAN_LENGTHS = (255, 256, 257, 511, 512, 513, 1023, 1024, 1025)
PAREN_PLACES = ("near", "last", "next", "two_on", "absent")
EQ_PLACES = ("other_side", "none")


def span_line(o, length, paren, eq, cr=False):
    """A line of `length` bytes (its '\\n' not counted) that starts at offset o of its program, with its first '('
    and its '=' at the named places: (line, status, name).  `other_side`: the `r0 = ` at the line's start when the
    '(' lies behind the start tile's end, and an '=' behind that end (so behind the '(') when it does not."""
    end = (o // TILE + 1) * TILE                 # the first byte of the next tile
    at = {"near": o + 9, "last": end - 1, "next": end, "two_on": end + TILE + 7, "absent": None}[paren]
    if at is not None and not o <= at < o + length - (2 if cr else 1):
        return None
    line = bytearray(b"n" * length)
    if cr:
        line[-1] = 0x0D
    q = None
    if eq == "other_side":
        if at is not None and at >= end:
            head = b"r0 = "[:max(min(len(b"r0 = "), end - o), 1)]    # as much of it as the start tile has room for
            if b"=" not in head:
                head = b"="
            line[:len(head)] = head
            q = o + head.index(b"=")
        else:
            q = min(end + 3, o + length - (2 if cr else 1))
            if q < end or (at is not None and q <= at):       # (the line ends in its start tile)
                return None
            line[q - o] = ord("=")
    elif eq == "before":
        line[:5] = b"r0 = "
        q = o + 3
    if at is None:
        return bytes(line), 1, None
    line[at - o] = ord("(")
    ns = o
    if q is not None and q < at:
        ns = q + 1
        while ns < at and line[ns - o] == 0x20:
            ns += 1
    if ns == at:
        return bytes(line), 2, None
    return bytes(line), 0, bytes(line[ns - o:at - o])


def span_progs():
    """[(text, status, names, note)]: filler up to the start offset, one long line, then `z()`."""
    out = []

    def add(o, length, paren, eq, cr=False):
        made = span_line(o, length, paren, eq, cr)
        if made is None:
            return
        line, st, name = made
        text = (comment(o) if o else b"") + line + b"\nz()\n"
        out.append((text, st, [name, b"z"] if st == 0 else [], (o, length, paren, eq, cr)))

    for o in SPAN_STARTS:
        for length in SPAN_LENGTHS:
            for paren in PAREN_PLACES:
                for eq in EQ_PLACES:
                    add(o, length, paren, eq)
            add(o, length, "near", "before")
        # CR LF with the CR on a tile's last byte
        for paren in ("near", "next"):
            add(o, (o // TILE + 2) * TILE - o, paren, "other_side", cr=True)
            add(o, (o // TILE + 3) * TILE - o, paren, "none", cr=True)
    return out


def failure_order_progs():
    """[(text, status)]: a status-2 line in tile 1 and a status-1 line in tile 3, and the reverse."""
    def prog(first, second):
        text = b"ok()\n"
        text += comment(TILE + 10 - len(text)) + first
        text += comment(3 * TILE + 10 - len(text)) + second
        return text + b"z()\n"
    return [(prog(b"r1 = (x\n", b"no bracket\n"), 2), (prog(b"no bracket\n", b"r1 = (x\n"), 1)]


# ---- 4: more than MAX_WAVES tiles -----------------------------------------------------
EMPTY_RUNS = (1, 2, 3, 17, 64, 65, 150, 300)
WIDE_PROGRAMS = 70000


def wide_batch():
    """WIDE_PROGRAMS programs, most of one short call line: runs of empty programs, a failing program every 97th,
    two-tile and three-tile programs, a dense one and the two of failure_order_progs()."""
    progs = [K.NAMES[k % len(K.NAMES)] + b"(0x%x)\n" % (k * 2654435761 % 9973) for k in range(WIDE_PROGRAMS)]
    for k in range(7, WIDE_PROGRAMS, 97):
        progs[k] = (b"ok()\nbroken line\n", b"r0 = (\n", b"# only\n")[k % 3]
    two = b"read(0x1)\n" + comment(TILE) + b"write(0x2)\n"
    three = b"mmap(0x1)\n" + comment(2 * TILE - 3) + b"r1 = getpid()\n" + comment(100) + b"close$foo(r1)"
    assert ntiles(len(two)) == 2 and ntiles(len(three)) == 3
    for j in range(12):
        progs[1000 + 5003 * j + j % 2] = two + b"# %d\n" % j
        progs[3000 + 5003 * j + j % 2] = three + b"# %d\n" % j
    progs[40000] = dense_progs()[-1][0]
    (a, _), (b, _) = failure_order_progs()
    progs[20001], progs[50002] = a, b
    at = 500
    for j in range(40):
        run = EMPTY_RUNS[j % len(EMPTY_RUNS)]
        progs[at:at + run] = [b""] * run
        at += 1500 + j + run
    assert len(progs) == WIDE_PROGRAMS and at < WIDE_PROGRAMS
    return progs


# ---- 5: high shifts in the device form ---------------------------------------------------
HIGH_SHIFT_BYTES = 16384
HIGH_SHIFT_STARTS = 300


def high_shift_case():
    """(text, offsets, ranges): HIGH_SHIFT_STARTS programs that each run from a start of their own to the end of
    one buffer of short call lines.  An offset is both a program's end and the next one's start, so a program
    that is to end at the buffer's end is followed by an empty one: every second offset is at or past nbytes."""
    lines, size = [], 0
    names = K.NAMES[:5] + [b"brk", b"x"]
    while size < HIGH_SHIFT_BYTES - 40:
        ln = (b"r%d = " % (len(lines) % 3) if len(lines) % 4 == 0 else b"") + names[len(lines) % len(names)] + b"(%d)\n" % (len(lines) % 10)
        lines.append(ln)
        size += len(ln)
    text = b"".join(lines) + comment(HIGH_SHIFT_BYTES - size)
    assert len(text) == HIGH_SHIFT_BYTES
    line_starts = np.concatenate([[0], np.cumsum([len(x) for x in lines])])[:-1]
    rng = np.random.default_rng(55)
    low = line_starts[line_starts < HIGH_SHIFT_BYTES // 2]
    high = line_starts[line_starts >= HIGH_SHIFT_BYTES // 2]
    starts = np.concatenate([rng.choice(low, 60, replace=False), rng.choice(high, HIGH_SHIFT_STARTS - 60, replace=False)])
    rng.shuffle(starts)
    starts[1::2] += rng.integers(1, 4, size=starts[1::2].size)        # every second one starts inside a line
    past = (HIGH_SHIFT_BYTES, HIGH_SHIFT_BYTES + 1000, 1 << 63, (1 << 64) - 1)
    offs = []
    for k, s in enumerate(starts.tolist()):
        offs += [s, past[k % len(past)]]
    offs = np.array(offs, np.uint64)
    return text, offs, line_starts


# ---- 6: the long-line limit at step positions ----------------------------------------------
LONG_STARTS = (0, 1, 62, 63, 255, 256)


def long_step_cases():
    """[(text, status, names)]: a line of MAX_LINE - 1 bytes and one of MAX_LINE bytes at each start of
    LONG_STARTS, ended by a '\\n' and by the program's end."""
    def line(n):
        return b"r0 = big(" + b"x" * (n - 9)
    out = []
    for o in LONG_STARTS:
        head = comment(o) if o else b""
        out.append((head + line(MAX_LINE - 1) + b"\nz()\n", 0, [b"big", b"z"]))
        out.append((head + line(MAX_LINE - 1), 0, [b"big"]))
        out.append((head + line(MAX_LINE) + b"\nz()\n", 3, []))
        out.append((head + line(MAX_LINE), 3, []))
    return out
