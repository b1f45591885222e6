"""Cases of tests/test_hub_state.py: program texts for the rules of CallSet, a call line at every place of the
scan's 64-byte step, lines at the long-line limit, names crafted for the dictionary's probe paths, and corpora
for the hub's add, pending and purge.  What each case relies on is asserted on the case itself by the CPU
tests.  The edges of the scan's 256-byte tiles, of its 64-line stores and of a wave's share of the tiles are
not met here: tests/call_set_cases.py has the cases for those."""
import json
import os

import numpy as np

from tests import hub_state_oracle as OR

MAX_LINE = 262144            # SG_CALLSET_MAX_LINE
STEP, TILE = 64, 256         # bytes of a wave's step and of a tile of the scan
OFFSETS = tuple(range(0, 131))
BATCH_SIZES = (0, 1, 63, 64, 65, 4097)
TABLE_MASK_BITS = 16         # a table of 5,000 names has 2^14 slots; the crafted names agree in 16 bits


def kats():
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "callset_kats.json")) as f:
        return [(c["text"].encode(), c["ok"], [n.encode() for n in c["names"]]) for c in json.load(f)["cases"]]


def offset_batch(offsets=OFFSETS):
    """One call line `rN = name(` at every start offset of `offsets` in its program, the program at every start
    misalignment 0..3 of the buffer: (progs, [(index, misalignment, offset, name)]).  With OFFSETS the line's
    '=', '(' and '\\n' so each fall on both sides of every 64-byte step."""
    progs, marks, pos = [], [], 0
    for a in range(4):
        for o in offsets:
            fill = (a - pos) % 4 or 4
            progs.append(b"f(\n\n"[:fill])
            pos += fill
            name = b"nm%03d_%d" % (o, a)
            head = b"" if o == 0 else b"#" * (o - 1) + b"\n"
            p = head + b"r%d = " % (o % 10) + name + b"(0x0)\nq()"
            marks.append((len(progs), a, o, name))
            progs.append(p)
            pos += len(p)
    return progs, marks


# (text, status, names in line order): every rule of the pinned semantics once
EDGES = (
    (b"a(b=c)\n", 0, [b"a"]),                                  # '=' after the '(' is ignored
    (b"r0 = r1 = foo(\n", 0, [b"r1 = foo"]),                   # two '=' before it: the first counts
    (b"r0 =foo(", 0, [b"foo"]),
    (b"r0 = foo(", 0, [b"foo"]),
    (b"r0 =   foo(", 0, [b"foo"]),
    (b"r0 =\tfoo(", 0, [b"\tfoo"]),                            # a tab is part of the name
    (b"r0 =  (foo)", 2, []),
    (b"ok()\nno bracket here\n", 1, []),
    (b"ok()\nr1 = (x\nno bracket\n", 2, []),                   # 2 on line 2 wins over 1 on line 3
    (b"ok()\nno bracket\nr1 = (x\n", 1, []),                   # and the reverse
    (b"a()\r\nb()\r\n", 0, [b"a", b"b"]),
    (b"a()\n\r\nb()\n", 0, [b"a", b"b"]),                      # a line that is only '\r'
    (b"a()\nb()\r", 0, [b"a", b"b"]),                          # a final '\r' without '\n'
    (b"#c()\na()\n# (\n", 0, [b"a"]),
    (b" #x(\n", 0, [b" #x"]),                                  # '#' is a comment only as the first byte
    (b"", 4, []),
    (b"#a()\n#b()\n", 4, []),
    (b"\n\n\r\n\n", 4, []),
    (b"a()\nb()", 0, [b"a", b"b"]),                            # no trailing newline
    (b"a\x00b(\n\xff\x80(\nx \t(\n", 0, [b"a\x00b", b"\xff\x80", b"x \t"]),
    (b"a(\na(\nb(\na(\n", 0, [b"a", b"a", b"b", b"a"]),        # repeats kept, in line order
    (b"=(", 2, []),
    (b"= =(", 0, [b"=" ]),
    (b"r0 = (", 2, []),
    (b"(", 2, []),
    (b"x", 1, []),
    (b"\r", 4, []),
    (b"#", 4, []),
)


def long_cases():
    """Lines at the long-line limit, the '(' early: (text, status)."""
    def line(n):
        return b"r0 = big(" + b"x" * (n - 9)
    assert len(line(MAX_LINE)) == MAX_LINE
    return [
        (line(MAX_LINE - 1) + b"\n", 0),
        (line(MAX_LINE) + b"\n", 3),
        (b"a()\n" + line(MAX_LINE - 1), 0),                     # the same as the last line, no '\n'
        (b"a()\n" + line(MAX_LINE), 3),
        (b"a()\nno bracket\n" + line(MAX_LINE) + b"\n", 1),     # a status-1 line before a too-long one
        (line(MAX_LINE) + b"\nno bracket\n", 3),                # and after it
        (line(MAX_LINE - 2) + b"\r\n", 0),                      # the '\r' counts: 262,143 with it
        (line(MAX_LINE - 1) + b"\r\n", 3),
        (b"#" * (MAX_LINE + 5) + b"\na()\n", 3),                # a comment is scanned like any line
    ]


NAMES = [b"open", b"openat", b"open$x", b"read", b"write", b"close$foo", b"mmap", b"ioctl$A", b"ioctl$B", b"getpid"]


def synth_prog(rng, names, nlines=None):
    n = int(rng.integers(1, 6)) if nlines is None else nlines
    out = []
    for k in range(n):
        nm = names[int(rng.integers(0, len(names)))]
        form = int(rng.integers(0, 4))
        if form == 0:
            out.append(nm + b"(0x%x)" % int(rng.integers(0, 1 << 30)))
        elif form == 1:
            out.append(b"r%d = " % k + nm + b"(0x%x, &(0x7f0000000000)=0x%x)" % (int(rng.integers(0, 99)), k))
        elif form == 2:
            out.append(b"# comment (\n" + nm + b"()")
        else:
            out.append(nm + b"(&(0x7f0000001000)={0x1, 0x2, " + b"0x0, " * int(rng.integers(0, 30)) + b"0x3})")
    return b"\n".join(out) + (b"\n" if rng.integers(0, 2) else b"")


def mixed(nprogs, seed, names=NAMES):
    """Valid programs of 1..5 lines, with runs of empty programs and a few failing ones."""
    rng = np.random.default_rng(seed)
    progs = [synth_prog(rng, names) for _ in range(nprogs)]
    for start in rng.integers(0, max(nprogs, 1), size=max(nprogs // 50, 1)):
        for k in range(int(start), min(int(start) + 5, nprogs)):
            progs[k] = b""
    for k in range(7, nprogs, 97):
        progs[k] = (b"ok()\nbroken line\n", b"r0 = (\n", b"# only\n")[k % 3]
    return progs


def big_among_short(seed=5):
    """A 1 MiB program of short lines among 200 short programs: (progs, index of the big one)."""
    rng = np.random.default_rng(seed)
    lines, size = [], 0
    while size < (1 << 20):
        ln = b"r%d = " % (len(lines) % 7) + NAMES[len(lines) % len(NAMES)] + b"(0x%x)" % (len(lines) * 2654435761 % 997)
        lines.append(ln)
        size += len(ln) + 1
    progs = mixed(100, seed) + [b"\n".join(lines) + b"\n"] + mixed(100, seed + 1)
    return progs, 100


# ---- names ----------------------------------------------------------------------
def low_bits(name, bits=TABLE_MASK_BITS):
    return OR.fnv1a(name) & ((1 << bits) - 1)


def colliding_pair():
    """Two names whose 64-bit FNV-1a hashes agree in their low TABLE_MASK_BITS bits (and differ above), found by
    search."""
    seen = {}
    for k in range(1 << 20):
        name = b"coll$%d" % k
        lb = low_bits(name)
        if lb in seen:
            return seen[lb], name
        seen[lb] = name
    raise AssertionError("no pair")


def slot_sharers(present, n):
    """n names that are not in `present` and share the low TABLE_MASK_BITS hash bits with one that is."""
    want = {low_bits(p) for p in present}
    out, have = [], set(present)
    k = 0
    while len(out) < n:
        name = b"absent$%d" % k
        k += 1
        if name not in have and low_bits(name) in want:
            out.append(name)
    return out


def many_names(n=5000, seed=11):
    """n distinct names of lengths 1..200, bytes 1..255 except '(' '=' '\\n' '\\r' ' ' and '#'."""
    rng = np.random.default_rng(seed)
    alphabet = np.array([c for c in range(1, 256) if c not in b"(=\n\r #"], np.uint8)
    names = {}
    while len(names) < n:
        ln = 1 + len(names) % 200
        names[alphabet[rng.integers(0, alphabet.size, size=ln)].tobytes()] = True
    return list(names)


# ---- corpora ----------------------------------------------------------------------
def pool(n=400, seed=21, names=NAMES):
    rng = np.random.default_rng(seed)
    out = {}
    while len(out) < n:
        out[synth_prog(rng, names)] = True
    return list(out)


POOL = pool()


def one_name_progs(n, name, tag):
    """n distinct programs that call only `name`."""
    return [name + b"(0x%x) # %s" % (k, tag) for k in range(n)]


def pending_steps():
    """Batches for the cut of pendingInputs: (batches as (seq, progs), max_records).  Seq 1 has 3 records, seq 2
    has 4, seq 3 has 3: with max_records = 5 index 5 lies inside seq 2 (indices 3..6), so the tie straddles the
    cut and pos runs to 7."""
    return [(1, one_name_progs(3, b"read", b"s1")), (2, one_name_progs(4, b"read", b"s2")),
            (3, one_name_progs(3, b"write", b"s3"))], 5
