"""Inputs of the cover-report page tests (tests/test_cover_pages.py): source
files with parseFile's expected lines and hand-written reports with their
expected bodies written out, the worlds that put a chosen list of lines into a
report (on tests/cover_lines_cases.py's World), the shapes that walk a listed
line across the copy's tile and chunk boundaries, and a seeded random report."""
import functools

import numpy as np

from tests import cover_lines_cases as K
from tests import cover_pages_oracle as OP

U8, U64 = np.uint8, np.uint64
T, F = True, False
LAST = 0xFFFFFFFF  # the largest line number a frame can carry
ANCHOR = "anchor.c"

# ---- parseFile: (source, its lines) -----------------------------------------------------
ESCAPES = ((b">", b"&gt;"), (b"<", b"&lt;"), (b"&", b"&amp;"), (b"\t", b"        "))
PARSE = [
    (b"", []),
    (b"a", [b"a"]),
    (b"\n", [b""]),
    (b"a\n", [b"a"]),
    (b"a\nb<&>\t", [b"a", b"b<&>\t"]),            # the fragment stays raw
    (b"\n\n", [b"", b""]),
    (b"\r\n", [b"\r"]),
    (b"&amp;\n", [b"&amp;amp;"]),                 # escaped again: the replacer knows no entities
    (b"<&\n", [b"&lt;&amp;"]),                    # ... and does not look at what it wrote
    (b"a\x00b\x80\xff\n\x00", [b"a\x00b\x80\xff", b"\x00"]),
]
for _e, _r in ESCAPES:
    PARSE += [(_e + b"\n", [_r]), (_e + b"abc\n", [_r + b"abc"]), (b"abc" + _e + b"\n", [b"abc" + _r]),
              (b"abc\n" + _e, [b"abc", _e]), (b"abc" + _e, [b"abc" + _e]), (_e, [_e]),
              (b"abc" + _e + b"\nx", [b"abc" + _r, b"x"])]
LINE_LENGTHS = [0, 1, 3, 4, 5, 15, 16, 17, 63, 64, 65, 255, 256, 257]


def parse_shapes(tile):
    """Sources whose lines the oracle gives: a line of 4,096 tabs, every byte value, the line lengths around the
    16-byte chunk, the wave's 64 and 256 and the copy's tile, one line of three tiles with no newline at all."""
    every = bytes(b for b in range(256) if b != 10)
    out = [b"\t" * 4096 + b"\n", every + b"\n" + every, b"".join(b"x" * n + b"\n" for n in LINE_LENGTHS),
           b"".join(b"<" * n + b"\n" for n in LINE_LENGTHS), b"q" * (3 * tile)]
    out += [b"y" * n + b"\n" + b"z" * n for n in (tile - 1, tile, tile + 1)]
    out += [b"y" * n for n in LINE_LENGTHS[1:]]
    return out


def src_arrays(datas):
    """sg_src_table_create's (have, bytes, off) for a list of sources, None being a file that cannot be read."""
    have = np.array([d is not None for d in datas], dtype=U8)
    off = np.zeros(len(datas) + 1, dtype=U64)
    off[1:] = np.cumsum([len(d) if d is not None else 0 for d in datas])
    return have, np.frombuffer(b"".join(d for d in datas if d is not None), dtype=U8), off


# ---- reports ----------------------------------------------------------------------------------
def marks_world(spec, unseen=(), extra_cov=()):
    """A world whose report lists exactly spec = [(file, [(line, covered), ...]), ...]: one symbol of func "f" with
    a call site per listed line, the cover the PCs of the covered ones (an uncovered site of a touched function is
    an uncovered PC).  Without any covered line a covered site in ANCHOR line 1 comes first.  Files are interned in
    spec order.  `unseen` names files that the table holds and no report does: sites of a function "g" that is
    never covered.  extra_cov: more cover PCs.  Returns (world, cover, file names by id)."""
    frames, sites, cov = {}, [], []
    pc = K.K + 0x110
    spec = list(spec)
    if not any(c for _, marks in spec for _, c in marks):
        spec = [(ANCHOR, [(1, T)])] + spec
    for name, marks in spec:
        for line, c in marks:
            frames[pc] = [("f", name, line)]
            sites.append(pc)
            if c:
                cov.append(pc)
            pc += 16
    syms = [(K.K + 0x100, pc - 1)]
    if unseen:
        start = pc = pc + 0x100
        for name in unseen:
            frames[pc] = [("g", name, 1)]
            sites.append(pc)
            pc += 16
        syms.append((start, pc - 1))
    names = [name for name, _ in spec] + list(unseen)
    assert len(set(names)) == len(names)
    return K.World(syms, sites, frames), K.cov_of(cov + list(extra_cov)), names


def spec_file_set(spec):
    """What fileSet gives for marks_world(spec)."""
    if not any(c for _, marks in spec for _, c in marks):
        spec = [(ANCHOR, [(1, T)])] + list(spec)
    return {name: sorted(marks) for name, marks in spec}


# (name, source, listed lines, the body, Coverage)
HAND = [
    ("first_and_last.c", b"one\ntwo\nthree\n", [(1, T), (3, F)],
     b"<span id='covered'>one</span> /*covered*/\ntwo\n<span id='uncovered'>three</span>\n", 1),
    ("raw_fragment.c", b"a<b\n\tx&y", [(2, T)],
     b"a&lt;b\n<span id='covered'>\tx&y</span> /*covered*/\n", 1),
    ("past_the_end.c", b"p\nq\n", [(2, F), (3, T), (LAST, T)],
     b"p\n<span id='uncovered'>q</span>\n", 0),
    ("all_past.c", b"only\n", [(2, T), (9, F)], b"only\n", 0),
    ("every_line.c", b"\n\t\n&\n", [(1, T), (2, F), (3, T)],
     b"<span id='covered'></span> /*covered*/\n<span id='uncovered'>        </span>\n"
     b"<span id='covered'>&amp;</span> /*covered*/\n", 2),
    ("no_lines.c", b"", [(1, T)], b"", 0),
    ("escapes.c", b"if (a < b && c > d)\t{\n", [(1, F)],
     b"<span id='uncovered'>if (a &lt; b &amp;&amp; c &gt; d)        {</span>\n", 0),
    ("untouched_lines.c", b"1\n2\n3\n4", [(4, F)], b"1\n2\n3\n<span id='uncovered'>4</span>\n", 0),
]
HAND_UNSEEN = {"unseen_gone.c": None, "unseen_here.c": b"never rendered\n"}


def hand():
    spec = [(name, marks) for name, _, marks, _, _ in HAND]
    sources = {name: src for name, src, _, _, _ in HAND}
    sources.update(HAND_UNSEEN)
    return spec, sources, list(HAND_UNSEEN)


MARKED = b"marked-line-text"


def straddle(tile):
    """A file per (pair of literals, part of the wrapped line, cut): a first line as long as it takes to put the cut
    of the second line's prefix, text or suffix on a tile boundary of the bodies.  Returns (spec, sources)."""
    spec, sources, pos = [], {}, 0
    for covered in (T, F):
        pre, suf = OP.COVERED if covered else OP.UNCOVERED
        for part, (start, size) in enumerate(((0, len(pre)), (len(pre), len(MARKED)), (len(pre) + len(MARKED), len(suf)))):
            for cut in (1, size // 2, size - 1):
                fill = (-(pos + 1 + start + cut)) % tile  # the first line and its '\n' come before the listed one
                name = "straddle_%d_%d_%d.c" % (covered, part, cut)
                spec.append((name, [(2, covered)]))
                sources[name] = b"." * fill + b"\n" + MARKED + b"\nafter\n"
                pos += fill + 1 + len(pre) + len(MARKED) + len(suf) + 6
    return spec, sources


def alignments():
    """The file under test behind a file whose body has 0 to 16 bytes; its own body has 128, so it starts at every
    offset mod 16 (the triangular numbers)."""
    spec, sources = [], {}
    for k in range(17):
        small, under = "small%02d.c" % k, "under%02d.c" % k
        sources[small] = b"a" * (k - 1) + b"\n" if k else b""
        spec.append((small, [(2 if k else 1, F)]))  # past its end: the body is the stored text
        sources[under] = b"first\nsecond<\nthirdx"
        spec.append((under, [(1, T), (2, F), (3, T)]))
    return spec, sources


def mark_ranges(file_set, names, sources):
    """The bodies' byte ranges (prefix, text, suffix) of every wrapped line of the report, and each file's start."""
    pos, out, starts = 0, [], {}
    for name in names:
        if name not in file_set:
            continue
        starts[name] = pos
        cov = list(file_set[name])
        for i, ln in enumerate(OP.parse_file(sources[name])):
            if cov and cov[0][0] == i + 1:
                pre, suf = OP.COVERED if cov[0][1] else OP.UNCOVERED
                a, b, c = pos + len(pre), pos + len(pre) + len(ln), pos + len(pre) + len(ln) + len(suf)
                out.append(((pos, a), (a, b), (b, c)))
                pos, cov = c, cov[1:]
            else:
                pos += len(ln) + 1
    return out, starts


# ---- random -----------------------------------------------------------------------------------------
ALPHABET = np.frombuffer(b"abcdefghijklmnop      (){};=<>&\t\t\n\n\n\r\x00\x80\xff", dtype=U8)
SEEDS = (1, 2)


@functools.lru_cache(maxsize=None)
def random_report(seed, nfiles=200, maxlen=4096):
    """(spec, sources, unseen): up to nfiles files of up to maxlen bytes over ALPHABET, a quarter of them outside the
    report (half of those unreadable), the others with a twentieth, a third or all of their lines listed and now
    and then lines past their end.  The first files are written by hand so that no seed lacks what
    tests/test_cover_pages.py asserts of the generator."""
    rng = np.random.default_rng(seed)
    spec = [("r/forced0.c", [(2, T), (3, F)]), ("r/forced1.c", [(1, T), (3, F)]), ("r/forced2.c", [(2, T), (5, F)])]
    sources = {"r/forced0.c": b"alpha\n<tag> & \t end\nraw tail <&>", "r/forced1.c": b"x\ny\n", "r/forced2.c": b"z\n",
               "r/unseen0.c": None}
    unseen = ["r/unseen0.c"]
    for i in range(nfiles - 4):
        name = "r/%03d.c" % i
        n = 0 if rng.random() < 0.05 else int(rng.integers(0, maxlen + 1))
        data = rng.choice(ALPHABET, size=n).tobytes()
        if rng.random() < 0.3:
            data = data[:-1] + b"\n" if data else data
        if rng.random() < 0.25:
            sources[name] = None if rng.random() < 0.5 else data
            unseen.append(name)
            continue
        sources[name] = data
        nl = len(OP.parse_file(data))
        p = (0.05, 0.34, 1.0)[int(rng.integers(0, 3))]
        marks = [(ln, bool(rng.random() < 0.5)) for ln in range(1, nl + 1) if rng.random() < p]
        r = rng.random()
        if r < 0.2 or not marks:
            marks.append((nl + 1, bool(rng.random() < 0.5)))
        if r < 0.1:
            marks += [(nl + 1 + int(rng.integers(1, 1000)), F), (LAST, T)]
        spec.append((name, marks))
    return spec, sources, unseen
