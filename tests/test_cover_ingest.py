"""The cover report's ingest (sg_cover_ingest.hip): sg_objdump_pcs, sg_nm_symbols and sg_addr2line_frames against a
sequential restatement of the Go lines they replace (tests/cover_ingest_oracle.py), the table and the report
built from the tools' text against the ones built from arrays and from a callable, and cover.vm_offset, which is
host code.  The reference's own addr2line table is tests/golden/symbolizer_kats.json.

tests/cover_ingest_cases.py builds the families and restates the constants they sit on.  The CPU tests assert on
each family the property it relies on (a needle met at every offset of a step and across a tile boundary, more
kept lines in a tile than a store group holds, more tiles than waves, the line limit on both sides), so a case
that drifts off its edge fails without a GPU; they also pin the oracle to hand-written expectations.  The GPU
tests compare every output element by element; no tolerance anywhere."""
import ctypes
import os
import re

import numpy as np
import pytest

from tests import cover_ingest_cases as K
from tests import cover_ingest_oracle as OR
from tests.conftest import ROOT

U8, U32, U64, I64 = np.uint8, np.uint32, np.uint64, np.int64
FILL = 0xA5
_memo = {}


def memo(fn, *args):
    """a family's case and its oracle result, built once and shared by its CPU and GPU tests"""
    key = (fn.__name__,) + args
    if key not in _memo:
        _memo[key] = fn(*args)
    return _memo[key]


def sites_by_tile(text, call=K.CALL, func=K.FUNC):
    """kept objdump lines by the tile they start in"""
    out = [0] * K.ntiles(len(text))
    for s, ln in OR.scan_lines(text):
        if OR.objdump_pcs(ln, call, func):
            out[s // K.TILE] += 1
    return out


# ---- CPU ---------------------------------------------------------------------------------------
def test_restated_constants_are_the_kernel_file_s():
    src = open(os.path.join(ROOT, "syzkaller_amd", "csrc", "sg_cover_ingest.hip")).read()
    hdr = open(os.path.join(ROOT, "include", "syzsig.h")).read()
    assert re.search(r"kCiTileLog = (\d+);", src).group(1) == str(K.TILE.bit_length() - 1)
    assert "kCiMaxWaves = 1u << %d;" % (K.MAX_WAVES.bit_length() - 1) in src
    assert "std::min<uint64_t>((pl.ntiles + 3) & ~3ull, kCiMaxWaves)" in src   # nwaves
    assert "(a.ntiles + a.nwaves - 1) / a.nwaves" in src                       # a wave's share
    assert "(nkeep & 63) == 63" in src and K.GROUP == 64 and "cb += 256;" in src and K.STEP == 64
    assert "#define SG_INGEST_MAX_LINE %d\n" % K.MAX_LINE in hdr and OR.MAX_LINE == K.MAX_LINE
    assert "#define SG_INGEST_MAX_NEEDLE %d\n" % K.MAX_NEEDLE in hdr
    from syzkaller_amd import cover as C

    assert C.INGEST_MAX_LINE == K.MAX_LINE


def test_oracle_meets_the_written_expectations():
    for ln, want in K.objdump_rules():
        assert OR.objdump_pcs(ln) == ([] if want is None else [want]), ln
        assert OR.objdump_pcs(ln + b"\n") == OR.objdump_pcs(ln)
    for ln, want in K.nm_rules():
        got = OR.nm_symbols(b"\n" + ln)
        if want is None:
            assert got == [], ln
        else:
            addr, size, name = want
            assert got == [(addr, OR.go_int_size(size), 1 + len(ln.rstrip(b"\r")) - len(name), name)], ln
    # int(size+15)/16*16 as Go computes it
    assert [OR.go_int_size(x) for x in (0, 1, 16, 17, 0x59)] == [0, 16, 16, 32, 0x60]
    assert OR.go_int_size((1 << 64) - 1) == 0 and OR.go_int_size((1 << 64) - 15) == 0 and OR.go_int_size((1 << 64) - 16) == 0
    assert OR.go_int_size(1 << 63) == -(1 << 63) + 16 and OR.go_int_size((1 << 63) - 15) == -(1 << 63)
    assert OR.go_int_size((1 << 64) - 32) == -16
    text, want = memo(K.objdump_rules_text)
    assert OR.objdump_pcs(text) == want and len(want) == sum(pc is not None for _, pc in K.objdump_rules())
    # other needles: what newer binutils print
    assert OR.objdump_pcs(b"10:\tcall   20 <__sanitizer_cov_trace_pc>\n") == []
    assert OR.objdump_pcs(b"10:\tcall   20 <__sanitizer_cov_trace_pc>\n", b"call ") == [0x10]


def test_line_rule_cases():
    for kind, parse in (("objdump", OR.objdump_pcs), ("nm", OR.nm_symbols)):
        seen = {}
        for name, text in memo(K.line_rule_texts, kind):
            try:
                seen[name] = len(parse(text))
            except OR.TooLong as e:
                seen[name] = ("too long", e.pos)
        first = len(K.short_line(kind, 0)) + 1 + len(K.short_line(kind, 1)) + 1
        assert seen["empty"] == 0 and seen["newline_only"] == 0 and seen["no_trailing_newline"] == 2
        assert seen["crlf"] == 3 and seen["empty_lines"] == 2
        n = K.MAX_LINE - 1  # the longest line that passes is kept: its parse walks 64 tiles
        assert (seen["start_%d" % n], seen["middle_%d" % n], seen["end_nl_%d" % n], seen["end_%d" % n]) == (3, 5, 3, 3)
        n = K.MAX_LINE
        assert seen["start_%d" % n] == ("too long", 0) and seen["cr_%d" % n] == ("too long", first)
        assert seen["middle_%d" % n] == seen["end_nl_%d" % n] == seen["end_%d" % n] == ("too long", first)
        assert seen["two_long"] == ("too long", len(K.short_line(kind, 0)) + 1)


def test_objdump_family_conditions():
    text, want = memo(K.objdump_offsets)
    assert OR.objdump_pcs(text) == want == list(range(1, len(want) + 1))
    for needle in (K.CALL, K.FUNC):
        at, p = set(), text.find(needle)
        while p >= 0:
            at.add(p)
            p = text.find(needle, p + 1)
        assert {p % K.STEP for p in at} == set(range(K.STEP))
        cross = {K.TILE - p % K.TILE for p in at if p % K.TILE > K.TILE - 40} | {0 for p in at if p % K.TILE == 0}
        assert cross >= set(range(len(needle) + 2)), needle          # every split of the needle over a tile boundary
    text, want = memo(K.objdump_tile_edge)
    assert OR.objdump_pcs(text) == sorted(want)
    starts = [s for s, ln in OR.scan_lines(text) if OR.objdump_pcs(ln)]
    assert [s % K.TILE for s in starts[:4]] == [K.TILE - 1, 0, K.TILE - 1, 0]
    assert text[9 * K.TILE - 1] == 10 and text[11 * K.TILE - 1] == 13 and text[11 * K.TILE] == 10
    text, want = memo(K.objdump_order)
    got = [OR.objdump_pcs(ln)[0] for _, ln in OR.scan_lines(text) if OR.objdump_pcs(ln)]
    assert got != sorted(got) and len(set(got)) < len(got) and sorted(got) == want == OR.objdump_pcs(text)
    assert got[:350] == sorted(got[:350], reverse=True)
    text, want = memo(K.objdump_dense)
    assert OR.objdump_pcs(text, K.DENSE_CALL, K.DENSE_FUNC) == want and OR.objdump_pcs(text) == []
    prof = sites_by_tile(text, K.DENSE_CALL, K.DENSE_FUNC)
    assert len(prof) > 4 and min(prof[:-1]) > 3 * K.GROUP and max(prof) % K.GROUP != 0


def test_objdump_many_tiles_conditions():
    text, want = memo(K.objdump_many_tiles)
    tiles = K.ntiles(len(text))
    assert tiles > K.MAX_WAVES and K.nwaves(tiles) == K.MAX_WAVES and -(-tiles // K.MAX_WAVES) == 2
    assert len(text) < 10 << 20 and len(want) > 1000
    got = memo(OR.objdump_pcs, text)
    assert got == want


def test_nm_family_conditions():
    text = memo(K.nm_ties)
    syms = OR.nm_symbols(text)
    starts = [s[0] for s in syms]
    assert len(syms) == 900 and len(set(starts)) == 200 and starts != sorted(starts)
    ss, se, order = OR.nm_sorted(syms)
    assert ss == sorted(starts) and all(ss[j] < ss[j + 1] or order[j] < order[j + 1] for j in range(899))
    text = memo(K.nm_dense)
    per = [0] * K.ntiles(len(text))
    for s in OR.nm_symbols(text):
        per[(s[2] - len(b"x x t ")) // K.TILE] += 1
    assert len(OR.nm_symbols(text)) == 1200 and min(per[:-1]) > 2 * K.GROUP
    text = memo(K.nm_tile_edge)
    syms = OR.nm_symbols(text)
    assert len(syms) == 9 and max(len(s[3]) for s in syms) > 2 * K.TILE
    lines = [(s, ln) for s, ln in OR.scan_lines(text) if OR.nm_symbols(ln)]
    assert lines[0][0] % K.TILE == K.TILE - 1
    blanks = {(s + ln.index(b" ")) % K.TILE for s, ln in lines} | {(s + 33) % K.TILE for s, ln in lines}
    assert {0, K.TILE - 1} <= blanks and any((s + 34) % K.TILE == K.TILE - 1 for s, _ in lines)


def test_vm_offset():
    from syzkaller_amd import cover as C

    for text, want in K.vm_offset_cases():
        for fn in (OR.vm_offset, C.vm_offset):
            if want is None:
                with pytest.raises(ValueError):
                    fn(text)
            else:
                assert fn(text) == want, (fn.__module__, text[-60:])


def test_argument_checks_come_before_the_context():
    """Nothing below reaches the context: the handle is a block of zeros."""
    from syzkaller_amd import _lib
    from syzkaller_amd._lib import SG_EINVAL as E
    from syzkaller_amd._lib import lib

    vp = ctypes.c_void_p
    blk = np.zeros(1 << 13, U64)
    fake = blk.ctypes.data_as(vp)
    p8, p64, p32 = (lambda a: a.ctypes.data_as(_lib.P8)), (lambda a: a.ctypes.data_as(_lib.P64)), (lambda a: a.ctypes.data_as(_lib.P32))
    text = np.frombuffer(K.site(0x10), U8).copy()
    call, func = np.frombuffer(K.CALL, U8).copy(), np.frombuffer(K.FUNC, U8).copy()
    big = np.zeros(K.MAX_NEEDLE + 1, U8)
    pcs = np.zeros(4, U64)
    n, st, pos = ctypes.c_size_t(77), ctypes.c_uint32(77), ctypes.c_uint64(77)
    ref = ctypes.byref
    args = [fake, p8(text), text.size, p8(call), call.size, p8(func), func.size, p64(pcs), 4, ref(n), ref(st), ref(pos)]

    def bad(fn, a, i, v):
        b = list(a)
        b[i] = v
        assert getattr(lib, fn)(*b) == E, (fn, i)
        assert lib.sg_last_error()

    for i in (0, 1, 3, 5, 7, 9, 10, 11):                    # a NULL where something is needed
        bad("sg_objdump_pcs", args, i, None)
    for i in (4, 6):                                         # a needle of 0 and of 65 bytes
        bad("sg_objdump_pcs", args, i, 0)
        a = list(args)
        a[i - 1] = p8(big)
        bad("sg_objdump_pcs", a, i, K.MAX_NEEDLE + 1)
    bad("sg_objdump_pcs", args, 2, 1 << 33)
    assert b"2^33" in lib.sg_last_error()
    dev = [fake, fake, text.size, p8(call), call.size, p8(func), func.size, fake, 4, fake]
    for i in (0, 1, 3, 5, 7, 9):
        bad("sg_objdump_pcs_dev", dev, i, None)
    for i in (4, 6):
        bad("sg_objdump_pcs_dev", dev, i, 0)
        bad("sg_objdump_pcs_dev", dev, i, K.MAX_NEEDLE + 1)
    bad("sg_objdump_pcs_dev", dev, 2, 1 << 33)
    a64, i64 = np.zeros(4, U64), np.zeros(4, I64)
    u32 = np.zeros(4, U32)
    nm = [fake, p8(text), text.size, p64(a64), i64.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), p64(a64), p32(u32),
          p64(a64), p64(a64), p32(u32), 4, ref(n), ref(st), ref(pos)]
    for i in (0, 1, 11, 12, 13):
        bad("sg_nm_symbols", nm, i, None)
    bad("sg_nm_symbols", nm, 2, 1 << 33)
    nmd = [fake, fake, text.size] + [fake] * 7 + [4, fake]
    for i in (0, 1, 11):
        bad("sg_nm_symbols_dev", nmd, i, None)
    bad("sg_nm_symbols_dev", nmd, 2, 1 << 33)
    assert (n.value, st.value, pos.value) == (77, 77, 77) and not pcs.any()


def test_a2l_and_fused_argument_checks_come_before_the_context():
    from syzkaller_amd import _lib
    from syzkaller_amd._lib import SG_EINVAL as E
    from syzkaller_amd._lib import lib

    blk = np.zeros(1 << 13, U64)
    fake = blk.ctypes.data_as(ctypes.c_void_p)
    t = np.frombuffer(b"0x10\nf\n/a.c:1\n", U8).copy()
    a64, u32, i64, info = np.zeros(8, U64), np.zeros(8, U32), np.zeros(8, I64), np.full(8, 77, U64)
    p8, p64, p32 = t.ctypes.data_as(_lib.P8), a64.ctypes.data_as(_lib.P64), u32.ctypes.data_as(_lib.P32)
    pi = i64.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))
    good = [fake, p8, t.size, 1, p64, p64, p32, pi, p32, 4, p64, p32, p64, p32, 64, info.ctypes.data_as(_lib.P64)]
    for i, v in ((0, None), (1, None), (4, None), (5, None), (6, None), (7, None), (8, None), (10, None), (11, None),
                 (12, None), (13, None), (15, None), (14, 0), (14, 65), (3, (1 << 32) - 1), (2, 1 << 33)):
        a = list(good)
        a[i] = v
        assert lib.sg_addr2line_frames(*a) == E and lib.sg_last_error(), i
    out = ctypes.c_void_p(5)
    fused = [fake, p8, t.size, p64, 1, p8, t.size, 1, 64, p64, p32, p64, p32, 4, info.ctypes.data_as(_lib.P64),
             ctypes.byref(out)]
    for i, v in ((0, None), (1, None), (3, None), (5, None), (9, None), (10, None), (11, None), (12, None), (14, None),
                 (15, None), (8, 0), (8, 65), (7, (1 << 32) - 1), (2, 1 << 33), (6, 1 << 33)):
        a = list(fused)
        a[i] = v
        assert lib.sg_cover_table_from_text(*a) == E and lib.sg_last_error(), i
    assert (info == 77).all()


# ---- GPU ---------------------------------------------------------------------------------------
def _objdump(ctx, text, call=K.CALL, func=K.FUNC):
    from syzkaller_amd import cover as C

    return C.objdump_pcs(text, call, func, ctx=ctx).tolist()


def _check_nm(ctx, text):
    from syzkaller_amd import cover as C

    want = memo(OR.nm_symbols, text)
    got = C.nm_symbols(text, ctx=ctx)
    assert len(got) == len(want)
    assert got.addr.tolist() == [s[0] for s in want]
    assert got.size.tolist() == [s[1] for s in want] and got.size.dtype == I64
    assert got.name_pos.tolist() == [s[2] for s in want]
    assert got.name_len.tolist() == [len(s[3]) for s in want]
    assert [got.name(k) for k in range(len(want))] == [s[3] for s in want]
    ss, se, order = OR.nm_sorted(want)
    assert got.sym_start.tolist() == ss and got.sym_end.tolist() == se and got.order.tolist() == order
    return got


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["objdump", "nm"])
def test_gpu_line_rule(ctx, kind):
    from syzkaller_amd import cover as C

    for name, text in memo(K.line_rule_texts, kind):
        try:
            want = OR.objdump_pcs(text) if kind == "objdump" else None
            if kind == "nm":
                OR.nm_symbols(text)
        except OR.TooLong as e:
            with pytest.raises(C.LineTooLong) as got:
                (C.objdump_pcs if kind == "objdump" else C.nm_symbols)(text, ctx=ctx)
            assert got.value.pos == e.pos, name
            continue
        if kind == "objdump":
            assert _objdump(ctx, text) == want, name
        else:
            _check_nm(ctx, text)


@pytest.mark.gpu
def test_gpu_objdump_rules_and_places(ctx):
    text, want = memo(K.objdump_rules_text)
    assert _objdump(ctx, text) == want
    for ln, pc in K.objdump_rules():                       # each alone: a one-line text without its '\n'
        assert _objdump(ctx, ln) == ([] if pc is None else [pc]), ln
    assert _objdump(ctx, b"10:\tcall   20 <__sanitizer_cov_trace_pc>\n") == []
    assert _objdump(ctx, b"10:\tcall   20 <__sanitizer_cov_trace_pc>\n", b"call ") == [0x10]
    assert _objdump(ctx, b"1:ab\n2:a\n3:b\n4:ba\n", b"ab", b"b") == [1]        # the needles overlap
    assert _objdump(ctx, b"1:ab\r\n2:a\r\n", b"a", b"b\r") == []               # the dropped '\r' is not the line's
    for fam in (K.objdump_offsets, K.objdump_tile_edge, K.objdump_order):
        text, want = memo(fam)
        assert _objdump(ctx, text) == sorted(want), fam.__name__
    text, want = memo(K.objdump_dense)
    assert _objdump(ctx, text, K.DENSE_CALL, K.DENSE_FUNC) == want and _objdump(ctx, text) == []
    big = bytes(range(1, K.MAX_NEEDLE + 1)).replace(b"\n", b"N").replace(b":", b"C")
    assert _objdump(ctx, b"7f:" + big + b"\n" + b"80:" + big[:-1] + b"\n", big, big) == [0x7f]


@pytest.mark.gpu
def test_gpu_objdump_many_tiles(ctx):
    text, want = memo(K.objdump_many_tiles)
    assert _objdump(ctx, text) == want


@pytest.mark.gpu
def test_gpu_objdump_cap_and_device_form(ctx):
    import torch

    from syzkaller_amd import _lib
    from syzkaller_amd._lib import call

    text, want = memo(K.objdump_order)
    t = np.frombuffer(text, U8)
    nc, nf = np.frombuffer(K.CALL, U8), np.frombuffer(K.FUNC, U8)
    p8, p64 = (lambda a: a.ctypes.data_as(_lib.P8)), (lambda a: a.ctypes.data_as(_lib.P64))
    n, st, pos = ctypes.c_size_t(), ctypes.c_uint32(), ctypes.c_uint64()
    for cap in (0, 1, len(want) - 1):                          # too small: the count alone
        out = np.full(len(want), FILL, U64)
        call("sg_objdump_pcs", ctx.h, p8(t), t.size, p8(nc), nc.size, p8(nf), nf.size, p64(out) if cap else None, cap,
             ctypes.byref(n), ctypes.byref(st), ctypes.byref(pos))
        assert (n.value, st.value) == (len(want), 0) and (out == np.full(len(want), FILL, U64)).all()
    d_text = torch.from_numpy(t.copy()).to("cuda")
    for cap in (len(want), len(want) + 7, len(want) - 1):
        d_pcs = torch.full((8 * cap + 16,), FILL, dtype=torch.uint8, device="cuda")
        d_info = torch.full((24 + 16,), FILL, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        call("sg_objdump_pcs_dev", ctx.h, d_text.data_ptr(), t.size, p8(nc), nc.size, p8(nf), nf.size, d_pcs.data_ptr(),
             cap, d_info.data_ptr())
        ctx.sync()
        info, pcs = d_info.cpu().numpy(), d_pcs.cpu().numpy()
        assert info[:24].view(U64).tolist() == [len(want), 0, 0] and (info[24:] == FILL).all()
        if cap >= len(want):
            assert pcs[:8 * len(want)].view(U64).tolist() == want and (pcs[8 * len(want):] == FILL).all()
        else:
            assert (pcs == FILL).all()
    long_text = memo(K.line_rule_texts, "objdump")[-1][1]
    d_long = torch.from_numpy(np.frombuffer(long_text, U8).copy()).to("cuda")
    d_info = torch.zeros(3, dtype=torch.int64, device="cuda")
    call("sg_objdump_pcs_dev", ctx.h, d_long.data_ptr(), len(long_text), p8(nc), nc.size, p8(nf), nf.size, None, 0,
         d_info.data_ptr())
    ctx.sync()
    assert d_info.cpu().tolist() == [0, 1, len(K.short_line("objdump", 0)) + 1]


@pytest.mark.gpu
def test_gpu_nm(ctx):
    got = _check_nm(ctx, memo(K.nm_rules_text))
    assert len(got) == sum(w is not None for _, w in K.nm_rules())
    for ln, _ in K.nm_rules():
        _check_nm(ctx, ln)
    for fam in (K.nm_ties, K.nm_dense, K.nm_tile_edge):
        _check_nm(ctx, memo(fam))


@pytest.mark.gpu
def test_gpu_nm_cap_and_device_form(ctx):
    import torch

    from syzkaller_amd import _lib
    from syzkaller_amd._lib import call

    text = memo(K.nm_ties)
    want = memo(OR.nm_symbols, text)
    ss, se, order = OR.nm_sorted(want)
    k = len(want)
    t = np.frombuffer(text, U8)
    n, st, pos = ctypes.c_size_t(), ctypes.c_uint32(), ctypes.c_uint64()
    out = np.full(k, FILL, U64)
    call("sg_nm_symbols", ctx.h, t.ctypes.data_as(_lib.P8), t.size, out.ctypes.data_as(_lib.P64), None, None, None, None,
         None, None, k - 1, ctypes.byref(n), ctypes.byref(st), ctypes.byref(pos))
    assert (n.value, st.value) == (k, 0) and (out == np.full(k, FILL, U64)).all()
    # only two arrays wanted
    order_only = np.full(k, FILL, U32)
    call("sg_nm_symbols", ctx.h, t.ctypes.data_as(_lib.P8), t.size, out.ctypes.data_as(_lib.P64), None, None, None, None,
         None, order_only.ctypes.data_as(_lib.P32), k, ctypes.byref(n), ctypes.byref(st), ctypes.byref(pos))
    assert out.tolist() == [s[0] for s in want] and order_only.tolist() == order
    d_text = torch.from_numpy(t.copy()).to("cuda")
    sizes = (8, 8, 8, 4, 8, 8, 4)
    bufs = [torch.full((m * k + 16,), FILL, dtype=torch.uint8, device="cuda") for m in sizes]
    d_info = torch.zeros(3, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    call("sg_nm_symbols_dev", ctx.h, d_text.data_ptr(), t.size, *[b.data_ptr() for b in bufs], k, d_info.data_ptr())
    ctx.sync()
    assert d_info.cpu().tolist() == [k, 0, 0]
    outs = [b.cpu().numpy() for b in bufs]
    for o, m in zip(outs, sizes):
        assert (o[m * k:] == FILL).all()
    assert outs[0][:8 * k].view(U64).tolist() == [s[0] for s in want]
    assert outs[1][:8 * k].view(I64).tolist() == [s[1] for s in want]
    assert outs[2][:8 * k].view(U64).tolist() == [s[2] for s in want]
    assert outs[3][:4 * k].view(U32).tolist() == [len(s[3]) for s in want]
    assert outs[4][:8 * k].view(U64).tolist() == ss and outs[5][:8 * k].view(U64).tolist() == se
    assert outs[6][:4 * k].view(U32).tolist() == order


@pytest.mark.gpu
def test_gpu_ingest_feeds_cover_uncovered(ctx):
    """the two scans' outputs are what sg_cover_uncovered takes: the same answer as from the oracle's arrays"""
    from syzkaller_amd import cover as C

    nm_text = b"".join(b"%016x %016x %c f%d\n" % (0xffffffff81000000 + 256 * k, 200 + k % 50, b"tT"[k % 2], k)
                       for k in range(300))
    sites = [0xffffffff81000000 + 256 * (k // 3) + 32 * (k % 3) + 5 for k in range(900)]
    od_text = b"".join(K.other(k) + K.site(pc) for k, pc in enumerate(reversed(sites)))
    syms = C.nm_symbols(nm_text, ctx=ctx)
    pcs = C.objdump_pcs(od_text, ctx=ctx)
    assert pcs.tolist() == sorted(sites)
    cov = np.array([(pc + 5) & 0xffffffff for pc in sites[::7]], dtype=U32)
    got = C.cover_uncovered(cov, 0xffffffff, syms.sym_start, syms.sym_end, pcs, ctx=ctx)
    ss, se, _ = OR.nm_sorted(OR.nm_symbols(nm_text))
    want = C.cover_uncovered(cov, 0xffffffff, np.array(ss, U64), np.array(se, U64), np.array(sorted(sites), U64), ctx=ctx)
    assert got.size > 0 and np.array_equal(got, want)


# ---- addr2line -----------------------------------------------------------------------------------
def _a2l_want(text, nrec):
    try:
        return (0, 0, OR.addr2line_frames(text, nrec))
    except OR.A2LError as e:
        return (e.status, e.pos, None)


def _sym_kats():
    import json

    from tests.conftest import GOLDEN

    with open(os.path.join(GOLDEN, "symbolizer_kats.json")) as f:
        return json.load(f)["tests"]


SENTINEL = b"0xffffffffffffffff\n??\n??:0\n"


def test_a2l_oracle_reproduces_the_reference_s_table():
    kats = _sym_kats()
    assert len(kats) == 6
    for t in kats:                                                   # each alone, as symbolize(pcs[:1]) reads it
        recs = OR.addr2line_frames(t["resp"].encode() + SENTINEL, 1)
        assert [(pc, [(fn.decode(), fl.decode(), ln) for fn, fl, ln, _, _ in fr]) for pc, fr in recs] == \
            [(t["pc"], [(f["func"], f["file"], f["line"]) for f in t["frames"]])]
        assert all(f["pc"] == t["pc"] for f in t["frames"])
    text = b"".join(t["resp"].encode() for t in kats) + SENTINEL     # and all of them in one output
    for n in range(len(kats) + 1):
        recs = OR.addr2line_frames(text, n)
        assert [pc for pc, _ in recs] == [t["pc"] for t in kats[:n]]
        assert [len(fr) for _, fr in recs] == [len(t["frames"]) for t in kats[:n]]
    assert OR.parse_uint0(b"0x0000000000123124") == 0x123124 and OR.parse_uint0(b"017") == 15 and OR.parse_uint0(b"0") == 0
    assert OR.parse_uint0(b"0x") is None and OR.parse_uint0(b"08") is None and OR.parse_uint0(b"") is None
    assert OR.parse_uint0(b"1_000") == 1000 and OR.parse_uint0(b"1__0") is None and OR.parse_uint0(b"_1") is None
    assert OR.parse_uint0(b"0x_1f") == 0x1f and OR.parse_uint0(b"0b101") == 5 and OR.parse_uint0(b"0o17") == 15
    assert OR.parse_uint0(b"18446744073709551615") == (1 << 64) - 1 and OR.parse_uint0(b"18446744073709551616") is None
    assert OR.parse_uint0(b"0x1ffffffffffffffff") is None and OR.parse_uint0(b"+1") is None and OR.parse_uint0(b"1 ") is None


def test_a2l_parallel_reading_equals_the_sequential_one():
    """The kernels find the records without walking the text in order.  Their reading, restated (a2l_model), gives
    what the sequential restatement of symbolize / parse gives: status, position and every frame."""
    kinds = {}
    for seed in range(25):
        for text, nrec in K.a2l_random_texts(seed, 1000):
            want = _a2l_want(text, nrec)
            assert K.a2l_model(text, nrec, OR) == want, (text, nrec)
            kinds[want[0]] = kinds.get(want[0], 0) + 1
    assert set(kinds) == {0, 1, 2, 3, 4, 6} and kinds[0] > 5000 and min(kinds.values()) > 500
    seen = set()
    for name, text, nrec in memo(K.a2l_failure_cases):
        want = _a2l_want(text, nrec)
        assert K.a2l_model(text, nrec, OR) == want, name
        seen.add(want[0])
        if name.startswith("tile_") and want[0]:
            end = text.find(b"\n", want[1])
            assert want[1] < K.TILE <= (end if end >= 0 else len(text)), name                     # the failing line lies across the boundary
    assert seen == {0, 1, 2, 3, 4, 5, 6}
    tiles = {name: _a2l_want(text, nrec)[0] for name, text, nrec in memo(K.a2l_failure_cases) if name.startswith("tile_")}
    assert tiles == {"tile_no_colon": 3, "tile_bad_pc": 2, "tile_too_long": 5, "tile_no_file_line": 4, "tile_ok": 0}
    by = {name: _a2l_want(text, nrec) for name, text, nrec in memo(K.a2l_failure_cases)}
    for where in ("first", "last"):
        assert [by[k + where][0] for k in ("bad_pc_", "no_colon_", "odd_lines_", "too_long_", "long_ok_")] == [2, 3, 3, 5, 0]
    assert by["too_long_line0"][:2] == (5, 0) and by["long_ok_line0"][2][0][0] == 15
    assert [by[k % j][0] for j in (0, 1) for k in ("too_long_middle_%d", "long_ok_middle_%d")] == [5, 0, 5, 0]
    assert by["bad_pc_colon_first"][0] == 2 and by["bad_pc_colon_last"][0] == 0      # the last record just ends there
    for k in ("garbage_behind_last", "garbage_in_sentinel", "last_record_ends_at_colon_line", "nrec_0", "pc_octal",
              "pc_decimal", "shaped_file_line", "colon_in_file", "discriminator", "tile_ok"):
        assert by[k][0] == 0, k
    assert by["too_few"][:2] == (6, len(memo(K.a2l_failure_cases)[0][1])) and by["eof_after_function"][0] == 4
    assert by["pc_octal"][2][0][0] == 15 and by["pc_decimal"][2][0][0] == 12345 and by["pc_binary_underscore"][2][0][0] == 5
    assert by["colon_in_file"][2][0][1][0][1:3] == (b"C:/dir:x/y.c:12", 34)
    assert by["shaped_file_line"][2][0][1][0][1:3] == (b"0x10", 77) and by["discriminator"][2][0][1][0][2] == 588
    assert [f[:3] for f in by["dropped_frames"][2][0][1]] == [
        (b"k", b"/s/a.c", 12), (b"m", b"/s/a.c", (1 << 63) - 1), (b"n", b"/s/a.c", 5), (b"z", b"/s/f0.c", 5)]


def test_a2l_world_conditions():
    recs = memo(K.a2l_world)
    text = K.a2l_render(recs)
    got = OR.addr2line_frames(text, len(recs))
    assert [(pc, [f[:3] for f in fr]) for pc, fr in got] == [(pc, list(fr)) for pc, fr in recs]
    files, funcs = OR.intern(got)
    assert len(funcs) > 65536 and len(files) > 64
    nfr = [len(fr) for _, fr in recs]
    assert 0 in nfr and 1 in nfr and max(nfr) > 64
    fnv = lambda b: __import__("functools").reduce(lambda h, c: ((h ^ c) * 0x100000001b3) & OR.U64, b, 0xcbf29ce484222325)  # noqa: E731
    first = sorted(funcs, key=funcs.get)[:50]
    assert [fnv(x) for x in first] != sorted(fnv(x) for x in first)        # first occurrence is not hash order
    assert any(funcs[fn] < funcs[prev] for _, fr in got for (prev, *_), (fn, *_) in zip(fr, fr[1:]))  # names come back


def _check_a2l(ctx, text, nrec, bits=64):
    from syzkaller_amd import cover as C

    want = memo(_a2l_want, text, nrec)
    if want[0]:
        with pytest.raises(C.Addr2lineError) as e:
            C.addr2line_frames(text, nrec, hash_bits=bits, ctx=ctx)
        assert (e.value.status, e.value.pos) == want[:2]
        return None
    got = C.addr2line_frames(text, nrec, hash_bits=bits, ctx=ctx)
    recs = want[2]
    assert got.rec_pc.tolist() == [pc for pc, _ in recs]
    assert got.frame_off.tolist() == np.concatenate([[0], np.cumsum([len(fr) for _, fr in recs])]).tolist()
    files, funcs = OR.intern(recs)
    frames = [f for _, fr in recs for f in fr]
    assert got.frame_line.tolist() == [f[2] for f in frames] and got.frame_line.dtype == I64
    assert got.frame_file.tolist() == [files[f[1]] for f in frames]
    assert got.frame_func.tolist() == [funcs[f[0]] for f in frames]
    assert got.files() == sorted(files, key=files.get) and got.funcs() == sorted(funcs, key=funcs.get)
    first_file, first_func = {}, {}
    for fn, fl, _, fn_pos, fl_pos in frames:
        first_file.setdefault(fl, fl_pos)
        first_func.setdefault(fn, fn_pos)
    assert got.file_pos.tolist() == [first_file[x] for x in got.files()]       # the span of the first occurrence
    assert got.func_pos.tolist() == [first_func[x] for x in got.funcs()]
    return got


@pytest.mark.gpu
def test_gpu_a2l_reference_table_and_cases(ctx):
    kats = _sym_kats()
    for t in kats:
        _check_a2l(ctx, t["resp"].encode() + SENTINEL, 1)
    text = b"".join(t["resp"].encode() for t in kats) + SENTINEL
    for n in range(len(kats) + 2):
        _check_a2l(ctx, text, n)
    for name, text, nrec in memo(K.a2l_failure_cases):
        for bits in (64, 1):
            _check_a2l(ctx, text, nrec, bits)


@pytest.mark.gpu
def test_gpu_a2l_random_sequences(ctx):
    for text, nrec in K.a2l_random_texts(1, 400) + K.a2l_random_texts(2, 400):
        _check_a2l(ctx, text, nrec, 64 if nrec % 2 else 8)


@pytest.mark.gpu
def test_gpu_a2l_interning_at_every_hash_width(ctx):
    recs = memo(K.a2l_world)
    text = K.a2l_render(recs)
    rounds = {}
    for bits in (64, 8, 1):
        got = _check_a2l(ctx, text, len(recs), bits)
        rounds[bits] = got.rounds
    assert rounds[64] == 0 and rounds[8] == 2 and rounds[1] == 2       # a column each went round again


@pytest.mark.gpu
def test_gpu_a2l_cap_and_device_form(ctx):
    import torch

    from syzkaller_amd import _lib
    from syzkaller_amd._lib import call

    name, text, nrec = memo(K.a2l_failure_cases)[0]
    want = _a2l_want(text, nrec)[2]
    files, funcs = OR.intern(want)
    nfr = sum(len(fr) for _, fr in want)
    t = np.frombuffer(text, U8)
    d_text = torch.from_numpy(t.copy()).to("cuda")
    for cap in (nfr, nfr - 1):
        sizes = (8 * nrec, 8 * (nrec + 1), 4 * cap, 8 * cap, 4 * cap, 8 * cap, 4 * cap, 8 * cap, 4 * cap, 48)
        bufs = [torch.full((m + 16,), FILL, dtype=torch.uint8, device="cuda") for m in sizes]
        torch.cuda.synchronize()
        p = [b.data_ptr() for b in bufs]
        call("sg_addr2line_frames_dev", ctx.h, d_text.data_ptr(), t.size, nrec, p[0], p[1], p[2], p[3], p[4], cap, p[5],
             p[6], p[7], p[8], 64, p[9])
        ctx.sync()
        outs = [b.cpu().numpy() for b in bufs]
        for o, m in zip(outs, sizes):
            assert (o[m:] == FILL).all()
        info = outs[9][:48].view(U64).tolist()
        assert outs[0][:sizes[0]].view(U64).tolist() == [pc for pc, _ in want]
        assert int(outs[1][:sizes[1]].view(U64)[-1]) == nfr
        if cap >= nfr:
            assert info == [nfr, len(files), len(funcs), 0, 0, 0]
            assert outs[3][:8 * nfr].view(I64).tolist() == [f[2] for _, fr in want for f in fr]
            assert outs[2][:4 * nfr].view(U32).tolist() == [files[f[1]] for _, fr in want for f in fr]
        else:
            assert info == [nfr, 0, 0, 0, 0, 0] and all((outs[k] == FILL).all() for k in range(2, 9))
    blk = np.zeros(1 << 13, U64)
    fake = blk.ctypes.data_as(ctypes.c_void_p)
    E = _lib.SG_EINVAL
    good = [fake, fake, 10, 3, fake, fake, fake, fake, fake, 4, fake, fake, fake, fake, 64, fake]
    for i, v in ((0, None), (1, None), (4, None), (5, None), (6, None), (10, None), (15, None), (14, 0), (14, 65),
                 (3, (1 << 32) - 1), (2, 1 << 33)):
        a = list(good)
        a[i] = v
        assert _lib.lib.sg_addr2line_frames_dev(*a) == E, i


# ---- the table and the report from the tools' text -----------------------------------------------------
def _world_texts(w):
    nm = b"".join(b"%016x %016x %c sym_%d\n" % (s, e - s, b"tT"[k % 2], k)
                  for k, (s, e) in enumerate(zip(w.sym_start.tolist(), w.sym_end.tolist())))
    od = b"".join(K.other(k) + K.site(pc) for k, pc in enumerate(w.sites.tolist()))

    def addr2line(pcs):
        return K.a2l_render([(pc, [(fn.encode(), fl.encode(), ln) for fn, fl, ln in w.frames.get(int(pc), [])])
                             for pc in pcs])

    return nm, od, addr2line


@pytest.mark.gpu
def test_gpu_table_and_report_from_text(ctx):
    from syzkaller_amd import cover as C
    from syzkaller_amd._lib import SG_EINVAL, SyzSigError
    from tests import cover_lines_cases as LK

    for w in (LK.hand_world(), LK.frames_world(), LK.random_world(seed=3, nsym=300, helpers=40)):
        nm, od, addr2line = _world_texts(w)
        ss, se, _ = OR.nm_sorted(OR.nm_symbols(nm))
        sites = w.sites
        assert C.objdump_pcs(od, ctx=ctx).tolist() == sites.tolist()
        tab, off, ff, fl, fn, files, funcs = LK.intern(w, {int(pc): w.frames[int(pc)] for pc in sites.tolist()})
        t_ref = C.CoverTable(ss, se, sites, tab, off, ff, fl, fn, len(files), len(funcs), ctx=ctx)
        t_txt, got_files, got_funcs = C.CoverTable.from_text(nm, sites, addr2line(sites.tolist()), ctx=ctx)
        assert [x.decode() for x in got_files] == files and [x.decode() for x in got_funcs] == funcs
        assert t_txt.nslots == t_ref.nslots
        rng = np.random.default_rng(5)
        covers = [LK.cov_of(sites[rng.random(sites.size) < p]) for p in (0.05, 0.5, 1.0)] + [LK.cov_of(sites[:1])]
        srcs = [b"".join(b"line %d of %d <&>\n" % (k, f) for k in range(1, 80)) for f in range(len(files))]
        soff = np.concatenate([[0], np.cumsum([len(s) for s in srcs])]).astype(U64)
        src = C.SourceTable([1] * len(files), b"".join(srcs), soff, ctx=ctx)
        for cov in covers:
            a, b = C.cover_lines(t_txt, cov, LK.BASE), C.cover_lines(t_ref, cov, LK.BASE)
            assert all(np.array_equal(x, y) for x, y in zip(a, b))
            a, b = C.cover_pages(t_txt, src, cov, LK.BASE), C.cover_pages(t_ref, src, cov, LK.BASE)
            assert all(np.array_equal(np.asarray(x).copy(), np.asarray(y).copy()) for x, y in zip(a[:9], b[:9])) and a[9] == b[9]
        src.close()
        # the report: the same object state, file sets and pages as from the symbolize callable
        by_name = dict(zip(files, srcs))

        def read(name):                   # (a rebuild for missing PCs brings files the first table did not name)
            return by_name.get(name, srcs[0])

        r_ref = C.CoverReport(np.array(ss, U64), np.array(se, U64), sites, w.symbolize, ctx=ctx, read_file=read)
        r_txt = C.CoverReport.from_tools(nm, od, addr2line, read_file=read, ctx=ctx)
        assert r_txt.files == r_ref.files and r_txt.funcs == r_ref.funcs and r_txt.frames == r_ref.frames
        assert r_txt.names == r_ref.names and np.array_equal(r_txt.all_pcs, r_ref.all_pcs)
        assert np.array_equal(r_txt.sym_start, r_ref.sym_start) and np.array_equal(r_txt.sym_end, r_ref.sym_end)
        extra = [pc for pc in sorted(w.frames) if pc not in set(sites.tolist())][:2]
        for cov in covers[:2] + ([LK.cov_of(np.array(extra + sites[:3].tolist(), U64))] if extra else []):
            try:
                want = r_ref.file_set(cov, LK.BASE)
            except ValueError as e:
                with pytest.raises(ValueError, match=str(e)[:20]):
                    r_txt.file_set(cov, LK.BASE)
                continue
            assert r_txt.file_set(cov, LK.BASE) == want
            assert r_txt.pages(cov, LK.BASE) == r_ref.pages(cov, LK.BASE)
        def named(r):   # (a rebuild from text numbers the names again: compare by name)
            fi, fu = sorted(r.files, key=r.files.get), sorted(r.funcs, key=r.funcs.get)
            return {pc: [(fi[a], ln, fu[b]) for a, ln, b in fr] for pc, fr in r.frames.items()}

        assert named(r_txt) == named(r_ref)
        r_txt.close()
        r_ref.close()
        # what the table build rejects: duplicate or unsorted records; a call site without its record
        dup = np.concatenate([sites[:2], sites[1:]])
        with pytest.raises(SyzSigError) as e:
            C.CoverTable.from_text(nm, dup, addr2line(dup.tolist()), ctx=ctx)
        assert e.value.rc == SG_EINVAL
        rev = sites[::-1].copy()
        if rev.size > 1:
            with pytest.raises(SyzSigError) as e:
                C.CoverTable.from_text(nm, rev, addr2line(rev.tolist()), ctx=ctx)
            assert e.value.rc == SG_EINVAL
        with pytest.raises(SyzSigError, match="no record") as e:
            C.CoverTable.from_text(nm, sites, addr2line(sites[:-1].tolist() + [int(sites[-1]) + 1]), ctx=ctx)
        assert e.value.rc == SG_EINVAL
        first = next((fr[0] for pc in sites.tolist() for fr in [w.frames[int(pc)]] if fr), None)
        if first:                                  # a kept frame whose line does not fit the table's 32 bits
            big = addr2line(sites.tolist()).replace(b"\n%s:%d\n" % (first[1].encode(), first[2]),
                                                    b"\n%s:4294967296\n" % first[1].encode(), 1)
            assert b":4294967296\n" in big
            with pytest.raises(SyzSigError, match="2\\^32") as e:
                C.CoverTable.from_text(nm, sites, big, ctx=ctx)
            assert e.value.rc == SG_EINVAL
        # records beyond the call sites: the table of all of them
        allp = np.array(sorted(w.frames), U64)
        if allp.size > sites.size:
            tab, off, ff, fl, fn, files2, funcs2 = LK.intern(w)
            t2 = C.CoverTable(ss, se, sites, tab, off, ff, fl, fn, len(files2), len(funcs2), ctx=ctx)
            t3, f3, u3 = C.CoverTable.from_text(nm, sites, addr2line(allp.tolist()), nrec=allp.size, hash_bits=8, ctx=ctx)
            assert [x.decode() for x in f3] == files2 and [x.decode() for x in u3] == funcs2
            cov = LK.cov_of(allp)
            assert all(np.array_equal(x, y) for x, y in zip(C.cover_lines(t3, cov, LK.BASE), C.cover_lines(t2, cov, LK.BASE)))
            t2.close()
            t3.close()
        t_txt.close()
        t_ref.close()
