"""The cover report's file bodies (syz-manager/cover.go:122-156, :198-217):
sg_src_table_*, sg_cover_pages, sg_cover_pages_set and the Python mirror.  On
the CPU the boundary, every rejected argument, the no-device result, the test
oracle (tests/cover_pages_oracle.py) on the hand-written cases and the
conditions the generated cases must hold; on the GPU parseFile through the
exported lines and both report forms bit-exact against the oracle: every byte
of every body, body_off, coverage, bad_file, the line tables of the same
call, and the output buffers' tails."""
import os
import re
import subprocess

import numpy as np
import pytest

from tests import cover_lines_cases as K
from tests import cover_lines_oracle as OR
from tests import cover_pages_cases as P
from tests import cover_pages_oracle as OP
from tests.conftest import ROOT

U32, U64, U8 = np.uint32, np.uint64, np.uint8
BASE = K.BASE
FILL64, FILL32, FILL8 = 0xA5A5A5A5A5A5A5A5, 0xA5A5A5A5, 0xEE
NAMES = ("sg_src_table_create", "sg_src_table_destroy", "sg_src_table_counts", "sg_src_table_export", "sg_cover_pages",
         "sg_cover_pages_set")
TILE = 4096  # the CPU tests' stand-in; the GPU tests read the counter


def _has_gpu():
    try:
        import torch

        return torch.cuda.device_count() > 0
    except Exception:
        return False


# ---- CPU: the boundary ---------------------------------------------------------
def test_header_binding_and_library():
    from syzkaller_amd import _lib
    from syzkaller_amd import cover as C

    text = open(os.path.join(ROOT, "include", "syzsig.h")).read()
    for cite in ("syz-manager/cover.go:122-156", "syz-manager/cover.go:198-217", "cover.go:133-135", "cover.go:138-140"):
        assert cite in text, cite
    src = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r" T (sg_[a-z0-9_]+)$", out, flags=re.M))
    for name in NAMES:
        assert re.search(r"\b(int|void) %s\s*\(" % name, src), name
        assert name in _lib.SIGNATURES and name in exported, name
    assert callable(C.SourceTable) and callable(C.cover_pages) and callable(C.CoverReport.pages)


def _outs(n=8):
    """sg_cover_pages' output arguments after base, and what keeps them alive."""
    from syzkaller_amd import _lib
    from syzkaller_amd.cover import _p8, _p32, _p64

    by = _lib.ctypes.byref
    keep = [np.zeros(n, U64), np.zeros(n, U32), np.zeros(n, U8), np.zeros(n, U8), _lib.c_uint64(), np.zeros(n, U64),
            _lib.c_size_t(), np.zeros(n, U64), np.zeros(n, U32), np.zeros(n, U8), _lib.c_size_t(), _lib.c_uint32()]
    fo, ln, cv, fs, ncf, ms, nm, bo, cg, bd, nb, bad = keep
    return [_p64(fo), _p32(ln), _p8(cv), _p8(fs), by(ncf), _p64(ms), by(nm), _p64(bo), _p32(cg), _p8(bd), n, by(nb),
            by(bad)], keep


def test_invalid_arguments_are_einval():
    """Every check the calls make before they touch the context or a table: a context (a table, a set) that is only
    a readable block of memory is enough."""
    from syzkaller_amd import _lib
    from syzkaller_amd.cover import _p8, _p32, _p64

    lib, E = _lib.lib, _lib.SG_EINVAL
    block = np.zeros(1 << 16, U8)
    fake = block.ctypes.data_as(_lib.c_void_p)  # never used: each case below returns first
    have, data, off = P.src_arrays([b"ab\n", None, b"c"])
    out = _lib.c_void_p()
    good = [_p8(have), _p8(data), _p64(off), 3, _lib.ctypes.byref(out)]

    def create(i=None, v=None, ctx=fake):
        a = list(good)
        if i is not None:
            a[i] = v
        return lib.sg_src_table_create(ctx, *a)

    assert create(ctx=None) == E
    for i in (0, 1, 2, 4):  # null have, bytes, off, out
        assert create(i, None) == E, i
    for bad_off in ([1, 3, 3, 4], [0, 3, 2, 4], [0, 3, 4, 4]):  # not from 0, decreasing, an unreadable file with bytes
        assert create(2, _p64(np.array(bad_off, U64))) == E, bad_off
        assert lib.sg_last_error()
    big = [_p8(np.ones(1, U8)), _p8(data), _p64(np.array([0, 1 << 32], U64)), 1, _lib.ctypes.byref(out)]
    assert lib.sg_src_table_create(fake, *big) == E  # 2^32 raw bytes
    assert b"2^32" in lib.sg_last_error() and not out.value
    tot, flo = np.zeros(3, U64), np.zeros(4, U64)
    assert lib.sg_src_table_counts(None, _p64(flo), _p64(tot)) == E
    assert lib.sg_src_table_counts(fake, None, _p64(tot)) == E and lib.sg_src_table_counts(fake, _p64(flo), None) == E
    assert lib.sg_src_table_export(None, _p64(flo), _p8(data)) == E and lib.sg_src_table_export(fake, None, _p8(data)) == E
    lib.sg_src_table_destroy(None)

    # the report calls: sg_cover_lines' checks, then their own
    outs, keep = _outs()
    cov = np.zeros(4, U32)
    assert lib.sg_cover_pages(None, fake, _p32(cov), 4, BASE, *outs) == E
    assert lib.sg_cover_pages_set(None, fake, fake, BASE, *outs) == E
    assert lib.sg_cover_pages(fake, None, _p32(cov), 4, BASE, *outs) == E
    assert lib.sg_cover_pages_set(fake, None, fake, BASE, *outs) == E
    assert lib.sg_cover_pages_set(fake, fake, None, BASE, *outs) == E
    assert lib.sg_cover_pages(fake, fake, None, 4, BASE, *outs) == E
    assert lib.sg_cover_pages(fake, fake, _p32(cov), 0xFFFFFFFF, BASE, *outs) == E
    for i in (0, 1, 2, 4, 5, 6, 7, 8, 11, 12):  # every output but the nullable file_seen, and bodies
        o = list(outs)
        o[i] = None
        assert lib.sg_cover_pages(fake, fake, _p32(cov), 4, BASE, *o) == E, i
        assert lib.sg_cover_pages_set(fake, fake, fake, BASE, *o) == E, i
    o = list(outs)
    o[9] = None  # null bodies with a capacity
    assert lib.sg_cover_pages(fake, fake, _p32(cov), 4, BASE, *o) == E and b"null bodies" in lib.sg_last_error()
    # (a table without a context: the source table cannot share it)
    assert lib.sg_cover_pages(fake, fake, _p32(cov), 4, BASE, *outs) == E and b"context" in lib.sg_last_error()


@pytest.mark.skipif(_has_gpu(), reason="checks the no-GPU failure path")
def test_no_device_is_enodev():
    """Valid arguments and no device: the first thing the call asks of the context fails."""
    from syzkaller_amd import _lib
    from syzkaller_amd.cover import _p8, _p64

    have, data, off = P.src_arrays([b"ab\n", None, b"c"])
    out = _lib.c_void_p()
    block = np.zeros(1 << 16, U8)  # a zeroed sg_ctx: device 0, an unlocked mutex
    rc = _lib.lib.sg_src_table_create(block.ctypes.data_as(_lib.c_void_p), _p8(have), _p8(data), _p64(off), 3,
                                      _lib.ctypes.byref(out))
    assert rc == _lib.SG_ENODEV and not out.value


# ---- CPU: the oracle and the generated cases ---------------------------------------------
def _expected(spec, sources, unseen=(), extra_cov=()):
    """(world, cover, names, the line-table oracle's result, the page oracle's result)."""
    w, cov, names = P.marks_world(spec, unseen, extra_cov)
    rep = OR.report(cov, BASE, w)
    return w, cov, names, rep, OP.pages(rep[0], names, sources)


def test_oracle_hand_cases():
    for src, lines in P.PARSE:
        assert OP.parse_file(src) == lines, src
    for name, src, marks, body, coverage in P.HAND:
        assert OP.render(OP.parse_file(src), sorted(marks)) == (body, coverage), name
    spec, sources, unseen = P.hand()
    _, _, names, rep, (body_off, bodies, coverage, bad) = _expected(spec, sources, unseen)
    assert rep[0] == P.spec_file_set(spec) and rep[3] == [] and bad is None
    assert names == [h[0] for h in P.HAND] + unseen
    for f, (name, _, _, body, cg) in enumerate(P.HAND):
        assert bodies[body_off[f]:body_off[f + 1]] == body and coverage[f] == cg, name
    assert body_off[len(P.HAND):] == [len(bodies)] * (len(unseen) + 1) and coverage[len(P.HAND):] == [0, 0]
    # an unreadable file inside the report stops everything; the lowest id is named
    sources = dict(sources, **{"all_past.c": None, "escapes.c": None})
    assert OP.pages(rep[0], names, sources) == ([0] * (len(names) + 1), b"", [0] * len(names), 3)
    # no covered line at all: the anchor is the report's first file
    spec = [("u.c", [(1, F)])]
    _, _, names, rep, pg = _expected(spec, {"u.c": b"x\n", P.ANCHOR: b"anchor\n"})
    assert names == [P.ANCHOR, "u.c"] and rep[0] == P.spec_file_set(spec)
    assert pg[1] == b"<span id='covered'>anchor</span> /*covered*/\n<span id='uncovered'>x</span>\n" and pg[2] == [1, 0]
    # the string level: the prefix of one file is the file (its name stays, the others lose as many bytes), names
    # starting with '.' go last
    assert OP.common_prefix(["/src/a.c"]) == "/src/a.c" and OP.common_prefix(["/src/a.c", "/src/inc/h.h", "/src/a.c"]) == "/src/"
    assert OP.common_prefix([]) == ""
    fs = {"/src/b.c": [(1, T)], "/src/.hid.h": [(1, F)], "/src/a.c": [(2, T)]}
    src = {name: b"l1\nl2\n" for name in fs}
    assert [f[0] for f in OP.files(fs, "/src/", src)] == ["a.c", "b.c", ".hid.h"]
    assert [f[0] for f in OP.files(fs, "/src/b.c", src)] == ["/src/a.c", "/src/b.c", "d.h"]  # (the guard: not longer)
    with pytest.raises(OSError):
        OP.files(fs, "", dict(src, **{"/src/a.c": None}))


T, F = True, False


def _straddling(ranges, tile):
    return [sum(1 for r in ranges if r[part][1] > r[part][0] and r[part][0] // tile != (r[part][1] - 1) // tile)
            for part in range(3)]


def test_generated_case_conditions():
    """What the generated cases must contain for the GPU comparison to mean something."""
    # the tile boundary inside each part of a wrapped line, at its first byte, its middle and its last byte
    spec, sources = P.straddle(TILE)
    _, _, names, rep, pg = _expected(spec, sources)
    ranges, _ = P.mark_ranges(rep[0], names, sources)
    assert len(ranges) == 18
    for i, r in enumerate(ranges):
        part, cut = (i % 9) // 3, (1, None, -1)[i % 3]
        a, b = r[part]
        at = a + 1 if cut == 1 else b - 1 if cut == -1 else a + (b - a) // 2
        assert at % TILE == 0 and a < at < b, (i, r)
    assert _straddling(ranges, TILE) == [6, 6, 6]
    # every destination alignment mod 16 behind bodies of 0 to 16 bytes
    spec, sources = P.alignments()
    _, _, names, rep, (body_off, _, _, _) = _expected(spec, sources)
    small = [body_off[f + 1] - body_off[f] for f in range(0, 34, 2)]
    assert small == list(range(17))
    assert {body_off[f] % 16 for f in range(1, 34, 2)} == set(range(16))
    # the random reports
    for seed in P.SEEDS:
        spec, sources, unseen = P.random_report(seed)
        assert len(spec) + len(unseen) <= 200 and max(len(s) for s in sources.values() if s is not None) <= 4096
        w, cov, names, rep, (body_off, bodies, coverage, bad) = _expected(spec, sources, unseen)
        fs = rep[0]
        assert fs == P.spec_file_set(spec) and bad is None and len(bodies) > 100000
        nl = {name: len(OP.parse_file(sources[name])) for name in fs}
        raw = {name: sources[name] != b"" and not sources[name].endswith(b"\n") for name in fs}
        assert any(raw[n] and (nl[n], c) in m for n, m in fs.items() for c in (T, F)), "a marked raw last fragment"
        assert any(ln == nl[n] + 1 for n, m in fs.items() for ln, _ in m), "a listed line one past the end"
        assert any(m and all(ln > nl[n] for ln, _ in m) for n, m in fs.items()), "all listed lines past the end"
        assert any(sources[n] is None for n in unseen), "an unreadable file outside the report"
        assert all(n not in fs for n in unseen)
        assert any(a[0] + 1 == b[0] and a[1] != b[1] and b[0] <= nl[n] for n, m in fs.items() for a, b in zip(m, m[1:])), \
            "a covered and an uncovered mark on adjacent lines"
        four = lambda ln: all(x in ln for x in (b"&gt;", b"&lt;", b"&amp;", b"        "))
        assert any(four(ln) for n in fs for ln in OP.parse_file(sources[n])[:-1 if raw[n] else None]), \
            "a line holding all four escaped bytes"
        assert sum(_straddling(P.mark_ranges(fs, names, sources)[0], TILE)) > 0


# ---- GPU --------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tile(ctx):
    t = ctx.counter("cover_pages_tile")
    assert t >= 256 and t % 16 == 0
    return t


def _source_table(ctx, datas):
    from syzkaller_amd import cover as C

    have, data, off = P.src_arrays(datas)
    return C.SourceTable(have, data, off, ctx=ctx)


def _check_lines(ctx, datas):
    """parseFile through the table: the lines, the counts and the stored text."""
    t = _source_table(ctx, datas)
    exp = [OP.parse_file(d) if d is not None else [] for d in datas]
    flo, nlines, stored, raw = t.counts()
    assert flo.tolist() == np.concatenate([[0], np.cumsum([len(e) for e in exp])]).tolist()
    assert nlines == sum(len(e) for e in exp) and raw == sum(len(d) for d in datas if d is not None)
    assert stored == sum(len(ln) + 1 for e in exp for ln in e)
    got = t.lines()
    t.close()
    assert len(got) == len(exp)
    for f, (g, e) in enumerate(zip(got, exp)):
        assert g == e, f


@pytest.mark.gpu
def test_parse_file_hand_cases(ctx):
    datas = [src for src, _ in P.PARSE]
    _check_lines(ctx, datas)
    t = _source_table(ctx, datas)
    assert t.lines() == [lines for _, lines in P.PARSE]
    t.close()
    # each alone in a table, and with unreadable files between the present ones
    for src, lines in P.PARSE[:10]:
        t = _source_table(ctx, [src])
        assert t.lines() == [lines]
        t.close()
    mixed = [x for src, _ in P.PARSE for x in (None, src)] + [None, None]
    _check_lines(ctx, mixed)


@pytest.mark.gpu
def test_parse_file_shapes(ctx, tile):
    _check_lines(ctx, P.parse_shapes(tile))
    _check_lines(ctx, [None] + P.parse_shapes(tile)[::-1] + [b""])


@pytest.mark.gpu
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65])
def test_parse_file_counts(ctx, n):
    rng = np.random.default_rng(n)
    datas = [None if i % 7 == 3 else rng.choice(P.ALPHABET, size=int(rng.integers(0, 40))).tobytes() for i in range(n)]
    _check_lines(ctx, datas)


def _tables(ctx, world, names, sources, frames=None):
    from syzkaller_amd import cover as C

    tab, off, ff, fl, fn, files, funcs = K.intern(world, frames)
    assert files == names[: len(files)]
    t = C.CoverTable(world.sym_start, world.sym_end, world.sites, tab, off, ff, fl, fn, len(names), len(funcs), ctx=ctx)
    return t, _source_table(ctx, [sources.get(name) for name in names])


def _run(table, src, cov, cap=None, lines_too=True):
    """One report through the C call itself, every output buffer longer than needed and prefilled: nothing past
    what the call reports is written.  cov: an array, or a SignalSet for the set form.  cap: the bodies' capacity
    (default: ample).  Returns (sg_cover_lines' outputs, body_off, bodies or None when they did not fit, coverage,
    bad_file, nbytes)."""
    from syzkaller_amd import _lib
    from syzkaller_amd import cover as C
    from syzkaller_amd.cover import _p8, _p32, _p64

    nf, ns, pad = table.nfiles, table.nslots, 8
    is_set = isinstance(cov, C.SignalSet)
    ncov = len(cov) if is_set else cov.size
    fo, ln = np.full(nf + 1 + pad, FILL64, U64), np.full(ns + pad, FILL32, U32)
    cv, fs, ms = np.full(ns + pad, FILL8, U8), np.full(nf + pad, FILL8, U8), np.full(ncov + pad, FILL64, U64)
    bo, cg = np.full(nf + 1 + pad, FILL64, U64), np.full(nf + pad, FILL32, U32)
    cap = (1 << 21) if cap is None else cap
    bd = np.full(cap + pad, FILL8, U8)
    ncf, nm, nb, bad = _lib.c_uint64(), _lib.c_size_t(), _lib.c_size_t(), _lib.c_uint32(7)
    by = _lib.ctypes.byref
    outs = (_p64(fo), _p32(ln), _p8(cv), _p8(fs), by(ncf), _p64(ms), by(nm), _p64(bo), _p32(cg), _p8(bd), cap, by(nb),
            by(bad))
    if is_set:
        _lib.call("sg_cover_pages_set", table.h, src.h, cov.h, BASE, *outs)
    else:
        c = np.ascontiguousarray(cov, dtype=U32)
        _lib.call("sg_cover_pages", table.h, src.h, _p32(c), c.size, BASE, *outs)
    total, nbytes = int(fo[nf]), nb.value
    assert total <= ns and nm.value <= ncov
    assert (fo[nf + 1:] == FILL64).all() and (ln[total:] == FILL32).all() and (cv[total:] == FILL8).all()
    assert (fs[nf:] == FILL8).all() and (ms[nm.value:] == FILL64).all()
    assert (bo[nf + 1:] == FILL64).all() and (cg[nf:] == FILL32).all()
    assert int(bo[nf]) == nbytes and (np.diff(bo[: nf + 1].astype(np.int64)) >= 0).all()
    fits = nbytes <= cap
    assert (bd[nbytes if fits else 0:] == FILL8).all()
    lines = (fo[: nf + 1].tolist(), ln[:total].tolist(), cv[:total].tolist(), fs[:nf].tolist(), ncf.value,
             ms[: nm.value].tolist())
    if lines_too:  # the line tables of the same call are those of a plain sg_cover_lines call
        plain = C.cover_lines(table, cov, BASE)
        assert lines == tuple(x.tolist() if isinstance(x, np.ndarray) else x for x in plain)
    return (lines, bo[: nf + 1].tolist(), bd[:nbytes].tobytes() if fits else None, cg[:nf].tolist(),
            None if bad.value == 0xFFFFFFFF else bad.value, nbytes)


def _same(got, rep, pg, names):
    """got: _run's result; rep: the line-table oracle's; pg: the page oracle's."""
    lines, body_off, bodies, coverage, bad, nbytes = got
    fo, ln, cv, fs, ncf, ms = lines
    res = {names[f]: [(ln[i], bool(cv[i])) for i in range(fo[f], fo[f + 1])] for f in range(len(names)) if fo[f + 1] > fo[f]}
    assert res == rep[0] and {names[f]: b for f, b in enumerate(fs) if b} == rep[1] and ncf == rep[2] and ms == rep[3]
    assert bad == pg[3] and body_off == pg[0] and coverage == pg[2] and nbytes == len(pg[1])
    if bodies != pg[1]:  # (not one assert on the pair: a failure would print both in full)
        at = next(i for i, (x, y) in enumerate(zip(bodies, pg[1])) if x != y)
        f = int(np.searchsorted(np.array(body_off), at, side="right")) - 1
        raise AssertionError("byte %d (file %d %s, +%d): %r, expected %r" % (
            at, f, names[f], at - body_off[f], bodies[max(at - 24, 0):at + 24], pg[1][max(at - 24, 0):at + 24]))


def _report(ctx, spec, sources, unseen=()):
    w, cov, names, rep, pg = _expected(spec, sources, unseen)
    t, s = _tables(ctx, w, names, sources)
    got = _run(t, s, cov)
    t.close()
    s.close()
    _same(got, rep, pg, names)
    return got, pg


@pytest.mark.gpu
def test_hand_cases(ctx):
    spec, sources, unseen = P.hand()
    got, _ = _report(ctx, spec, sources, unseen)
    _, body_off, bodies, coverage, bad, _ = got
    for f, (name, _, _, body, cg) in enumerate(P.HAND):  # the literals of the case file
        assert bodies[body_off[f]:body_off[f + 1]] == body and coverage[f] == cg, name
    assert bad is None
    # each alone: a report of one file (and the anchor where no line is covered)
    for name, src, marks, body, cg in P.HAND:
        got, _ = _report(ctx, [(name, marks)], {name: src, P.ANCHOR: b"anchor\n"})
        assert got[2].endswith(body) and got[3][-1] == cg, name


@pytest.mark.gpu
def test_tile_boundaries_and_alignments(ctx, tile):
    spec, sources = P.straddle(tile)
    w, cov, names, rep, pg = _expected(spec, sources)
    assert _straddling(P.mark_ranges(rep[0], names, sources)[0], tile) == [6, 6, 6]
    _report(ctx, spec, sources)
    _report(ctx, *P.alignments())
    # a listed line of three tiles, one of a tile - 1, + 0, + 1 bytes, and an unlisted one as long
    big = b"s" * (3 * tile) + b"\n" + b"".join(b"<" * ((tile + d) // 4) + b"\n" + b"u" * (tile + d) + b"\n" for d in (-1, 0, 1))
    _report(ctx, [("big.c", [(1, T), (2, F), (4, T), (6, F)])], {"big.c": big + b"t" * (3 * tile)})
    _report(ctx, [("frag.c", [(1, F)])], {"frag.c": b"t" * (3 * tile), P.ANCHOR: b"anchor\n"})


@pytest.mark.gpu
def test_every_line_and_alternating(ctx):
    src = b"".join(b"line %d <&>\t.\n" % i for i in range(700)) + b"tail"
    _report(ctx, [("all.c", [(i, T) for i in range(1, 702)])], {"all.c": src})
    _report(ctx, [("alt.c", [(i, i % 2 == 0) for i in range(1, 702)])], {"alt.c": src})
    _report(ctx, [("none.c", [(702, F), (P.LAST, T)]), ("empty.c", [(1, T)])], {"none.c": src, "empty.c": b""})


@pytest.mark.gpu
def test_two_reports_capacity_and_bad_file(ctx):
    spec, sources, unseen = P.hand()
    w, cov, names, rep, pg = _expected(spec, sources, unseen)
    t, s = _tables(ctx, w, names, sources)
    # two reports on one pair of tables: nothing is left of the first
    cov2 = cov[:1]
    rep2 = OR.report(cov2, BASE, w)
    pg2 = OP.pages(rep2[0], names, sources)
    assert pg2[1] != pg[1] and len(pg2[1]) > 0
    _same(_run(t, s, cov), rep, pg, names)
    _same(_run(t, s, cov2), rep2, pg2, names)
    _same(_run(t, s, cov), rep, pg, names)
    # a capacity one byte short: the total is reported, the bodies are untouched (checked by _run); exact: written
    n = len(pg[1])
    got = _run(t, s, cov, cap=n - 1)
    assert got[2] is None and got[5] == n and got[1] == pg[0] and got[3] == pg[2]
    _same(_run(t, s, cov, cap=n), rep, pg, names)
    got = _run(t, s, cov, cap=0)
    assert got[2] is None and got[5] == n
    # ncov == 0: all-empty outputs
    got = _run(t, s, np.zeros(0, U32))
    assert got[1:] == ([0] * (len(names) + 1), b"", [0] * len(names), None, 0) and got[0][0] == [0] * (len(names) + 1)
    s.close()
    # unreadable files inside the report: nothing is rendered, the lowest id is named, the line tables stand
    for gone in (["escapes.c"], ["escapes.c", "all_past.c"], ["first_and_last.c", "no_lines.c"]):
        src2 = dict(sources, **{name: None for name in gone})
        s2 = _source_table(ctx, [src2.get(name) for name in names])
        pg3 = OP.pages(rep[0], names, src2)
        assert pg3[3] == min(names.index(g) for g in gone) and pg3[1] == b""
        _same(_run(t, s2, cov), rep, pg3, names)
        s2.close()
    # a source table of another size is refused
    from syzkaller_amd._lib import SG_EINVAL, SyzSigError

    s3 = _source_table(ctx, [b"x\n"])
    with pytest.raises(SyzSigError) as e:
        _run(t, s3, cov)
    assert e.value.rc == SG_EINVAL
    s3.close()
    t.close()


@pytest.mark.gpu
def test_missing_pcs_and_rebuilt_tables(ctx):
    spec, sources, unseen = P.hand()
    stray = K.K + 0x108  # inside the symbol, no site, not in the table
    w, cov, names, rep, pg = _expected(spec, sources, unseen, extra_cov=[stray])
    assert rep[3] == [stray]
    t, s = _tables(ctx, w, names, sources)
    _same(_run(t, s, cov), rep, pg, names)  # the bodies match the line tables of the call
    t.close()
    s.close()
    full = dict(w.frames)
    full[stray] = [("f", "new.c", 2)]
    names2, sources2 = K.intern(w, full)[5], dict(sources, **{"new.c": b"n1\nn2\n"})  # (the lowest PC: file id 0)
    rep2 = OR.report(cov, BASE, w, full)
    pg2 = OP.pages(rep2[0], names2, sources2)
    t, s = _tables(ctx, w, names2, sources2, full)
    got = _run(t, s, cov)
    _same(got, rep2, pg2, names2)
    assert rep2[3] == [] and got[2].count(b"<span id='covered'>n2</span>") == 1
    t.close()
    s.close()


@pytest.mark.gpu
def test_set_form(ctx):
    """The corpus cover as sg_accept_batch maintains it, rendered without an upload."""
    from syzkaller_amd import cover as C

    spec, sources, unseen = P.random_report(P.SEEDS[0])
    w, cov, names, rep, pg = _expected(spec, sources, unseen)
    t, s = _tables(ctx, w, names, sources)
    sig, cset = C.SignalSet(ctx), C.SignalSet(ctx)
    parts = np.array_split(cov, 5)
    off = np.concatenate([[0], np.cumsum([p.size for p in parts])]).astype(U64)
    assert C.accept_batch(sig, cset, cov, off, cov, off, ctx=ctx)[0]
    uniq = cset.export()
    assert uniq.size >= parts[0].size and np.isin(uniq, cov).all()
    rep2 = OR.report(uniq, BASE, w)
    pg2 = OP.pages(rep2[0], names, sources)
    got = _run(t, s, cset)
    _same(got, rep2, pg2, names)
    assert got == _run(t, s, uniq)
    cset.clear()
    assert _run(t, s, cset)[5] == 0
    sig.close()
    cset.close()
    t.close()
    s.close()


@pytest.mark.gpu
@pytest.mark.parametrize("seed", P.SEEDS)
def test_random_reports(ctx, seed):
    from syzkaller_amd import cover as C

    spec, sources, unseen = P.random_report(seed)
    w, cov, names, rep, pg = _expected(spec, sources, unseen)
    t, s = _tables(ctx, w, names, sources)
    got = _run(t, s, cov)
    _same(got, rep, pg, names)
    # the Python call: its tuple is cover_lines' plus the pages
    res = C.cover_pages(t, s, cov, BASE)
    assert res[6].tolist() == pg[0] and res[7].tobytes() == pg[1] and res[8].tolist() == pg[2] and res[9] is None
    for x, y in zip(res[:6], C.cover_lines(t, cov, BASE)):
        assert np.array_equal(x, y)
    t.close()
    s.close()


@pytest.mark.gpu
def test_mirror_pages(ctx):
    from syzkaller_amd import cover as C

    src = b"l1\nl2 <\nl3"
    for unc_files in (["/src/a.c"], ["/src/a.c", "/src/inc/long.h"]):
        spec = [("/src/a.c", [(1, T), (2, F)]), ("/src/inc/long.h", [(2, T), (3, "/src/inc/long.h" not in unc_files)]),
                ("/src/.hid.h", [(1, T)]), ("/src/b.c", [(3, T), (4, T)])]
        sources = {name: src for name, _ in spec}
        w, cov, names = P.marks_world(spec)
        calls = []

        def symbolize(pcs):
            calls.append(list(pcs))
            return w.symbolize(pcs)

        r = C.CoverReport(w.sym_start, w.sym_end, w.sites, symbolize, ctx=ctx, read_file=sources.get)
        fs, seen, _, _, unc = OR.report(cov, BASE, w)
        prefix = OP.common_prefix([fl for pc in unc for _, fl, _ in w.frames.get(pc, [])])
        assert prefix == ("/src/a.c" if len(unc_files) == 1 else "/src/")
        exp = OP.files(fs, prefix, sources)
        got = r.pages(cov, BASE)
        assert got == exp
        if prefix == "/src/":
            assert [f[0] for f in got] == ["a.c", "b.c", "inc/long.h", ".hid.h"]
        else:  # the one file as long as the prefix keeps its name; the others lose as many bytes
            assert [f[0] for f in got] == ["/long.h", "/src/a.c", "/src/b.c", "d.h"]
        assert r.file_set(cov, BASE) == fs and len(calls) == 1
        with pytest.raises(ValueError, match=OR.NO_DATA):
            r.pages([], BASE)
        r.close()
    # a file of the report that cannot be read
    gone = dict(sources, **{"/src/b.c": None})
    r = C.CoverReport(w.sym_start, w.sym_end, w.sites, w.symbolize, ctx=ctx, read_file=gone.get)
    with pytest.raises(OSError, match="b.c"):
        r.pages(cov, BASE)
    r.close()
    # covered PCs the table does not know: one more symbolize call, then the source table of the larger file list
    stray = K.K + 0x108
    w2, cov2, _ = P.marks_world(spec, extra_cov=[stray])
    full = dict(w2.frames)
    full[stray] = [("f", "/src/new.c", 1)]
    sources2 = dict(sources, **{"/src/new.c": b"fresh\n"})
    calls = []

    def symbolize2(pcs):
        calls.append(list(pcs))
        return [(pc, fn, fl, ln) for pc in pcs for fn, fl, ln in full.get(int(pc), [])]

    r = C.CoverReport(w2.sym_start, w2.sym_end, w2.sites, symbolize2, ctx=ctx, read_file=sources2.get)
    fs, _, _, _, unc = OR.report(cov2, BASE, w2, full)
    exp = OP.files(fs, OP.common_prefix([fl for pc in unc for _, fl, _ in full.get(pc, [])]), sources2)
    assert r.pages(cov2, BASE) == exp and len(calls) == 2 and calls[1] == [stray]
    assert ("new.c", b"<span id='covered'>fresh</span> /*covered*/\n", 1) in exp
    assert r.pages(cov2, BASE) == exp and len(calls) == 2
    r.close()
