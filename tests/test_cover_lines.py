"""The cover report's line tables (syz-manager/cover.go:91-120, :165-196):
sg_cover_table_create, sg_cover_lines, sg_cover_lines_set.  On the CPU the
boundary, every rejected argument, the no-device result, the test oracle
(tests/cover_lines_oracle.py) on hand-written cases and the conditions the
random generator must hold; on the GPU both report forms bit-exact against
the oracle: the hand-written cases, missing PCs and the rebuilt table, the
compaction's and the bitmaps' unit edges, the set form, both query regimes of
the shared report body, and the output buffers' tails."""
import functools
import os
import re
import subprocess

import numpy as np
import pytest

from oracle import pyoracle as O
from tests import cover_lines_cases as K
from tests import cover_lines_oracle as OR
from tests.conftest import ROOT

U32, U64, U8 = np.uint32, np.uint64, np.uint8
BASE = K.BASE
FILL64, FILL32, FILL8 = 0xA5A5A5A5A5A5A5A5, 0xA5A5A5A5, 0xEE
NAMES = ("sg_cover_table_create", "sg_cover_table_destroy", "sg_cover_table_slots", "sg_cover_lines",
         "sg_cover_lines_set")


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
    for cite in ("syz-manager/cover.go:91-120", "syz-manager/cover.go:165-196", "syz-manager/html.go:169-194"):
        assert cite in text, cite
    assert "equal strings MUST get" in text  # the interning rule
    src = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r" T (sg_[a-z0-9_]+)$", out, flags=re.M))
    for name in NAMES:
        assert re.search(r"\b(int|void) %s\s*\(" % name, src), name
        assert name in _lib.SIGNATURES and name in exported, name
    assert callable(C.CoverTable) and callable(C.cover_lines) and callable(C.CoverReport)


def _create_args(world=None):
    """sg_cover_table_create's ctypes arguments after ctx (the last is the out pointer), and the arrays behind them."""
    from syzkaller_amd import _lib
    from syzkaller_amd.cover import _p32, _p64

    w = K.hand_world() if world is None else world
    tab, off, ff, fl, fn, files, funcs = K.intern(w)
    out = _lib.c_void_p()
    keep = [w.sym_start, w.sym_end, w.sites, tab, off, ff, fl, fn, out]
    return [_p64(w.sym_start), _p64(w.sym_end), w.sym_start.size, _p64(w.sites), w.sites.size, _p64(tab), tab.size,
            _p64(off), _p32(ff), _p32(fl), _p32(fn), len(files), len(funcs), _lib.ctypes.byref(out)], keep


def test_invalid_arguments_are_einval():
    """Every check the calls make before they touch the context or the table: a context (a table, a set) that is
    only a readable block of memory is enough."""
    from syzkaller_amd import _lib
    from syzkaller_amd.cover import _p8, _p32, _p64

    lib, E = _lib.lib, _lib.SG_EINVAL
    good, keep = _create_args()
    block = np.zeros(1 << 16, U8)
    fake = block.ctypes.data_as(_lib.c_void_p)  # never used: each case below returns first

    def create(i=None, v=None):
        a = list(good)
        if i is not None:
            a[i] = v
        return lib.sg_cover_table_create(fake, *a)

    assert lib.sg_cover_table_create(None, *good) == E
    for i in (0, 1, 3, 5, 7, 8, 9, 10, 13):  # null pointers: symbols, call sites, table PCs, frame arrays, out
        assert create(i, None) == E, i
    for i in (2, 4, 6, 11, 12):              # counts at 2^32 - 1
        assert create(i, 0xFFFFFFFF) == E, i
    w = keep[0:8]

    def arr(k, j, v):
        a = w[k].copy()
        a[j] = v
        return (_p64 if a.dtype == U64 else _p32)(a), a

    for i, k, j, v in ((0, 0, 1, 0), (1, 1, 1, 0),               # symbol starts, ends out of order
                       (3, 2, 1, int(w[2][0])), (5, 3, 2, 0),    # a repeated call site, table PCs out of order
                       (7, 4, 0, 1), (7, 4, 3, 0),               # frame_off not from 0, decreasing
                       (8, 5, 0, good[11]), (10, 7, 0, good[12]), (9, 6, 0, 0),  # file, func out of range, line 0
                       (3, 2, 0, int(w[2][0]) - 1)):             # a call site the table does not hold
        p, a = arr(k, j, v)
        assert create(i, p) == E, (i, k, j)
        assert _lib.lib.sg_last_error()
    big = np.array([0, 0xFFFFFFFF], U64)                          # too many frames in all
    a = list(good)
    a[4], a[6], a[7] = 0, 1, _p64(big)
    assert lib.sg_cover_table_create(fake, *a) == E

    # the report calls
    fo, ln, cv, fs = np.zeros(8, U64), np.zeros(8, U32), np.zeros(8, U8), np.zeros(8, U8)
    ncf, ms, nm = _lib.c_uint64(), np.zeros(8, U64), _lib.c_size_t()
    cov = np.zeros(4, U32)
    outs = [_p64(fo), _p32(ln), _p8(cv), _p8(fs), _lib.ctypes.byref(ncf), _p64(ms), _lib.ctypes.byref(nm)]
    assert lib.sg_cover_lines(None, _p32(cov), 4, BASE, *outs) == E
    assert lib.sg_cover_lines_set(None, fake, BASE, *outs) == E
    assert lib.sg_cover_lines_set(fake, None, BASE, *outs) == E
    assert lib.sg_cover_lines(fake, None, 4, BASE, *outs) == E
    assert lib.sg_cover_lines(fake, _p32(cov), 0xFFFFFFFF, BASE, *outs) == E
    for i in (0, 1, 2, 4, 5, 6):  # every output but the nullable file_seen
        o = list(outs)
        o[i] = None
        assert lib.sg_cover_lines(fake, _p32(cov), 4, BASE, *o) == E, i
        assert lib.sg_cover_lines_set(fake, fake, BASE, *o) == E, i
    assert lib.sg_cover_table_slots(None, _lib.ctypes.byref(ncf)) == E and lib.sg_cover_table_slots(fake, None) == E
    lib.sg_cover_table_destroy(None)


@pytest.mark.skipif(_has_gpu(), reason="checks the no-GPU failure path")
def test_no_device_is_enodev():
    """Valid arguments and no device: the first thing the call asks of the context fails."""
    from syzkaller_amd import _lib

    good, keep = _create_args()
    block = np.zeros(1 << 16, U8)  # a zeroed sg_ctx: device 0, an unlocked mutex
    assert _lib.lib.sg_cover_table_create(block.ctypes.data_as(_lib.c_void_p), *good) == _lib.SG_ENODEV
    assert not keep[-1].value


# ---- CPU: the oracle ---------------------------------------------------------------
def test_oracle_hand_cases():
    w = K.hand_world()
    for name, pcs, exp, ncf in K.HAND:
        res, seen, got_ncf, missing, _ = OR.report(K.hand_cov(pcs), BASE, w)
        assert res == exp, name
        assert got_ncf == ncf and missing == [], name
    # file_seen: h.h appears in uncovered frames that the funcs filter drops
    _, seen, _, _, unc = OR.report(K.hand_cov([0x1010]), BASE, w)
    assert seen == {"a.c": 3, "h.h": 2} and sorted(unc) == [K.K + 0x1020, K.K + 0x1030]
    _, _, _, _, unc = OR.report(K.hand_cov([0x6090, 0x6100]), BASE, w)
    assert K.K + 0x6090 in unc
    with pytest.raises(ValueError, match=OR.NO_DATA):
        OR.generate([], BASE, w)
    with pytest.raises(ValueError, match=OR.NO_DEBUG):
        OR.generate(K.hand_cov([0x1020]), BASE, w)
    assert OR.generate(K.hand_cov([0x1010]), BASE, w) == K.HAND[0][2]
    # a PC the frame dict does not hold: reported, no frames
    res, _, ncf, missing, _ = OR.report(K.hand_cov([0x7000, 0x1010, 0x7000]), BASE, w)
    assert res == K.HAND[0][2] and ncf == 1 and missing == [K.K + 0x7000]


@functools.lru_cache(maxsize=None)
def _random_oracle(nq=100000, missing=0, order="random"):
    cov = K.random_cover(nq=nq, missing=missing)
    if order == "sorted":
        cov = np.sort(cov)
    return cov, OR.report(cov, BASE, K.random_world())


def test_generator_conditions():
    """What the random case must contain for the GPU comparison to mean something."""
    w = K.random_world()
    nfr = sum(len(f) for f in w.frames.values())
    assert 100000 < w.sites.size <= 200000 and 150000 < nfr <= 300000
    cov, (res, seen, ncf, missing, unc) = _random_oracle()
    assert cov.size == 100000 and missing == [] and ncf > 0
    assert any(any(c for _, c in v) and any(not c for _, c in v) for v in res.values())  # a file with both kinds
    pcs = set((((BASE << 32) + int(c)) - 5) & OR.M64 for c in cov.tolist())
    assert pcs & set(unc)                                                               # both covered and uncovered
    sym_of = lambda pc: int(np.searchsorted(w.sym_start, np.uint64(pc), side="right")) - 1
    funcs, outer, inl_syms = set(), set(), {}
    covered_lines = set()
    for pc in pcs:
        fr = w.frames.get(pc, [])
        for i, (fn, fl, ln) in enumerate(fr):
            funcs.add(fn)
            covered_lines.add((fl, ln))
            if i == len(fr) - 1:
                outer.add(fn)
            else:
                inl_syms.setdefault(fn, set()).add(sym_of(pc))
    dropped = kept_inline = both = 0
    for pc in unc:
        for fn, fl, ln in w.frames.get(pc, []):
            if fn not in funcs:
                dropped += 1
                continue
            both += (fl, ln) in covered_lines
            kept_inline += fn not in outer and sym_of(pc) not in inl_syms[fn]
    assert dropped > 0 and kept_inline > 0 and both > 0, (dropped, kept_inline, both)
    # the cover with missing PCs: some of them twice
    cov, (_, _, _, missing, _) = _random_oracle(20000, 300)
    assert len(missing) == 200


# ---- GPU -----------------------------------------------------------------------------
def _table(ctx, world, frames=None):
    from syzkaller_amd import cover as C

    tab, off, ff, fl, fn, files, funcs = K.intern(world, frames)
    t = C.CoverTable(world.sym_start, world.sym_end, world.sites, tab, off, ff, fl, fn, len(files), len(funcs), ctx=ctx)
    return t, files


def _run(table, files, cov):
    """One report through the C call itself, every output buffer longer than needed and prefilled: nothing past
    file_off[nfiles] entries and *nmissing is written.  cov: an array, or a SignalSet for the set form."""
    from syzkaller_amd import _lib
    from syzkaller_amd import cover as C
    from syzkaller_amd.cover import _p8, _p32, _p64

    nf, ns, pad = table.nfiles, table.nslots, 8
    is_set = isinstance(cov, C.SignalSet)
    ncov = len(cov) if is_set else cov.size
    fo, ln = np.full(nf + 1 + pad, FILL64, U64), np.full(ns + pad, FILL32, U32)
    cv, fs, ms = np.full(ns + pad, FILL8, U8), np.full(nf + pad, FILL8, U8), np.full(ncov + pad, FILL64, U64)
    ncf, nm = _lib.c_uint64(), _lib.c_size_t()
    outs = (_p64(fo), _p32(ln), _p8(cv), _p8(fs), _lib.ctypes.byref(ncf), _p64(ms), _lib.ctypes.byref(nm))
    if is_set:
        _lib.call("sg_cover_lines_set", table.h, cov.h, BASE, *outs)
    else:
        c = np.ascontiguousarray(cov, dtype=U32)
        _lib.call("sg_cover_lines", table.h, _p32(c), c.size, BASE, *outs)
    total = int(fo[nf])
    assert total <= ns and nm.value <= ncov
    assert (fo[nf + 1:] == FILL64).all() and (ln[total:] == FILL32).all() and (cv[total:] == FILL8).all()
    assert (fs[nf:] == FILL8).all() and (ms[nm.value:] == FILL64).all()
    assert (np.diff(fo[: nf + 1].astype(np.int64)) >= 0).all() and set(cv[:total].tolist()) <= {0, 1}
    res = {}
    for f in range(nf):
        a, b = int(fo[f]), int(fo[f + 1])
        if b > a:
            res[files[f]] = [(int(x), bool(y)) for x, y in zip(ln[a:b], cv[a:b])]
    seen = {files[f]: int(b) for f, b in enumerate(fs[:nf]) if b}
    return res, seen, ncf.value, ms[: nm.value].tolist()


def _same(got, exp):
    assert got[0] == exp[0]
    assert got[1] == exp[1] and got[2] == exp[2] and got[3] == exp[3]


@pytest.fixture(scope="module")
def hand(ctx):
    t, files = _table(ctx, K.hand_world())
    yield t, files
    t.close()


@pytest.fixture(scope="module")
def rand(ctx):
    t, files = _table(ctx, K.random_world())
    yield t, files
    t.close()


@pytest.mark.gpu
def test_hand_cases(ctx, hand):
    t, files = hand
    w = K.hand_world()
    assert t.nslots == 15
    for name, pcs, exp, ncf in K.HAND:
        got = _run(t, files, K.hand_cov(pcs))
        assert got[0] == exp and got[2] == ncf and got[3] == [], name
        _same(got, OR.report(K.hand_cov(pcs), BASE, w)[:4])
    assert _run(t, files, K.hand_cov([0x1010]))[1] == {"a.c": 3, "h.h": 2}
    # covered PCs outside every symbol and off every site change nothing
    got = _run(t, files, K.hand_cov([0x1010, 0x5000]))
    assert got[0] == {"a.c": [(10, True), (12, False)], "s.c": [(1, True)]}
    # ncov == 0: all-empty outputs
    assert _run(t, files, np.zeros(0, U32)) == ({}, {}, 0, [])


@pytest.mark.gpu
def test_mirror_errors_and_file_set(ctx):
    from syzkaller_amd import cover as C

    w = K.hand_world()
    calls = []

    def symbolize(pcs):
        calls.append(list(pcs))
        return w.symbolize(pcs)

    r = C.CoverReport(w.sym_start, w.sym_end, w.sites, symbolize, ctx=ctx)
    assert len(calls) == 1
    for name, pcs, exp, ncf in K.HAND:
        if ncf and name != "stray_and_non_site":  # (that one is for the rebuild below)
            assert r.file_set(K.hand_cov(pcs), BASE) == exp, name
    assert len(calls) == 1
    with pytest.raises(ValueError, match=OR.NO_DATA):
        r.file_set([], BASE)
    with pytest.raises(ValueError, match=OR.NO_DEBUG):
        r.file_set(K.hand_cov([0x1020]), BASE)
    # table PCs that are no call sites are unknown to the mirror's first table: exactly one more symbolize call
    n = len(calls)
    assert r.file_set(K.hand_cov([0x5000, 0x1018, 0x5000]), BASE) == K.HAND[2][2]
    assert len(calls) == n + 1 and calls[-1] == [K.K + 0x1018, K.K + 0x5000]
    assert r.file_set(K.hand_cov([0x5000, 0x1018]), BASE) == K.HAND[2][2] and len(calls) == n + 1
    r.close()


@pytest.mark.gpu
def test_missing_pcs_and_rebuilt_table(ctx, hand):
    t, files = hand
    w = K.hand_world()
    cov = K.hand_cov([0x7000, 0x1010, 0x0500, 0x7000, 0x9000, 0x0500])
    got = _run(t, files, cov)
    assert got[3] == [K.K + 0x0500, K.K + 0x7000, K.K + 0x9000]       # distinct, ascending
    _same(got, OR.report(cov, BASE, w)[:4])                              # ... and no frames
    assert got[0] == K.HAND[0][2]
    full = dict(w.frames)
    full.update({K.K + 0x0500: [("low", "low.c", 1)], K.K + 0x7000: [("f1", "x.c", 2), ("hi", "x.c", 3)], K.K + 0x9000: []})
    t2, files2 = _table(ctx, w, full)
    got = _run(t2, files2, cov)
    _same(got, OR.report(cov, BASE, w, full)[:4])
    assert got[3] == [] and got[0]["x.c"] == [(2, True), (3, True)] and got[0]["low.c"] == [(1, True)]
    t2.close()
    # the random world
    cov, exp = _random_oracle(20000, 300)
    tr, fr = _table(ctx, K.random_world())
    got = _run(tr, fr, cov)
    _same(got, exp[:4])
    assert len(got[3]) == 200
    tr.close()


@pytest.mark.gpu
def test_random_case(ctx, rand):
    t, files = rand
    cov, exp = _random_oracle()
    _same(_run(t, files, cov), exp[:4])
    # a second report on the same table with another cover: nothing is left of the first one's bit sets
    cov2, exp2 = _random_oracle(20000, 300)
    _same(_run(t, files, cov2), exp2[:4])
    _same(_run(t, files, cov), exp[:4])


@pytest.mark.gpu
def test_both_query_regimes(ctx, rand, ctx_option):
    """The shared report body's chunked path (queries in random order, and in PC order) and its global-search path
    (option report_direct) through the new call."""
    t, files = rand
    for order in ("random", "sorted"):
        cov, exp = _random_oracle(20000, 0, order)
        assert ctx.get_option("report_direct") == 0
        got = _run(t, files, cov)
        _same(got, exp[:4])
        ctx_option(ctx, "report_direct", 1)
        assert _run(t, files, cov) == got
        ctx.set_option("report_direct", 0)


@pytest.mark.gpu
def test_cover_uncovered_unchanged_by_a_table(ctx):
    from syzkaller_amd import cover as C

    w = K.random_world()
    cov, exp = _random_oracle(20000, 0)
    before = C.cover_uncovered(cov, BASE, w.sym_start, w.sym_end, w.sites, ctx=ctx)
    t, files = _table(ctx, K.hand_world())
    _run(t, files, K.hand_cov([0x1010]))
    after = C.cover_uncovered(cov, BASE, w.sym_start, w.sym_end, w.sites, ctx=ctx)
    t.close()
    assert np.array_equal(before, after) and np.array_equal(before, np.sort(np.array(exp[4], dtype=U64)))


@pytest.mark.gpu
def test_set_form(ctx, rand):
    """The corpus cover as sg_accept_batch maintains it, reported without an upload: equal to the host form on the
    sorted distinct cover."""
    from syzkaller_amd import cover as C

    t, files = rand
    cov, _ = _random_oracle(20000, 300)
    sig, cset = C.SignalSet(ctx), C.SignalSet(ctx)
    parts = np.array_split(cov, 7)
    off = np.concatenate([[0], np.cumsum([p.size for p in parts])]).astype(U64)
    acc = C.accept_batch(sig, cset, cov, off, cov, off, ctx=ctx)
    assert acc[0]
    uniq = cset.export()  # ascending, distinct: the accepted inputs' cover
    assert uniq.size >= parts[0].size // 2 and np.isin(uniq, cov).all() and (np.diff(uniq.astype(np.int64)) > 0).all()
    got = _run(t, files, cset)
    assert got == _run(t, files, uniq)
    _same(got, OR.report(uniq, BASE, K.random_world())[:4])
    # an empty set
    cset.clear()
    assert _run(t, files, cset) == ({}, {}, 0, [])
    sig.close()
    cset.close()


@pytest.mark.gpu
@pytest.mark.parametrize("n", K.SLOT_COUNTS)
def test_slot_count_edges(ctx, n):
    """Slot counts one below, at and one above the compaction's units: the 64-bit mask word, the wave's chunk of
    256 slots, the workgroup's tile of 1024."""
    w = K.slots_world(n)
    t, files = _table(ctx, w)
    assert t.nslots == n
    rng = np.random.default_rng(n)
    for cov in K.slots_cover(n, rng):
        _same(_run(t, files, cov), OR.report(cov, BASE, w)[:4])
    t.close()


@pytest.mark.gpu
def test_id_and_frame_edges(ctx):
    # func and file ids at bits 31, 32 and 33
    w = K.ids_world()
    t, files = _table(ctx, w)
    assert files[31] == "file31.c" and files[33] == "file33.c"
    for ks in ([31], [32], [33], [0, 31, 32, 33, 39]):
        cov = K.cov_of([K.K + 0x100 * k + 0x10 for k in ks])
        got = _run(t, files, cov)
        _same(got, OR.report(cov, BASE, w)[:4])
        assert sorted(got[0]) == sorted("file%d.c" % k for k in ks)
        assert all(v == [(1, True), (2, False)] for v in got[0].values())
    t.close()
    # sites of 0, 1, 2, 3, 64 and 65 frames
    w = K.frames_world()
    t, files = _table(ctx, w)
    for i in range(8):
        cov = K.cov_of([K.K + 0x10 + 16 * i])
        _same(_run(t, files, cov), OR.report(cov, BASE, w)[:4])
    cov = K.cov_of([K.K + 0x10 + 16 * i for i in (5, 1, 5)])
    _same(_run(t, files, cov), OR.report(cov, BASE, w)[:4])
    t.close()


@pytest.mark.gpu
def test_one_row_table_and_queries_outside_it(ctx):
    pc = K.K + 0x100
    w = K.World([(K.K, K.K + 0xfff)], [pc], {pc: [("f", "a.c", 7)]})
    t, files = _table(ctx, w)
    assert t.nslots == 1
    assert _run(t, files, K.cov_of([pc])) == ({"a.c": [(7, True)]}, {"a.c": 1}, 1, [])
    # below the first and above the last table PC, inside the symbol: the site stays uncovered, func f never covered
    cov = K.cov_of([pc - 16, pc + 16, pc - 16])
    got = _run(t, files, cov)
    assert got == ({}, {"a.c": 2}, 0, [pc - 16, pc + 16])
    _same(got, OR.report(cov, BASE, w)[:4])
    got = _run(t, files, K.cov_of([pc + 16, pc]))
    assert got == ({"a.c": [(7, True)]}, {"a.c": 1}, 1, [pc + 16])
    t.close()
    # a table with nothing in it: every covered PC is missing
    w0 = K.World([], [], {})
    t, files = _table(ctx, w0)
    assert t.nslots == 0 and _run(t, files, K.cov_of([pc, pc])) == ({}, {}, 0, [pc])
    t.close()
