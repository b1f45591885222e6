"""Executor-exact comparisons: the flag_collect_comps branch of
handle_completion (executor/executor.h:379-387, :621-673) over raw
KCOV_TRACE_CMP buffers.  On the CPU the test oracle (tests/exec_comps_oracle.py)
against the fixture the reference's own compiled operator<, operator== and
write() produced (tests/golden/exec_comps_golden.npz); on the GPU sg_exec_comps
and sg_exec_comps_dev exact against both, on the fast shapes and on the general
path."""
import functools
import os

import numpy as np
import pytest

from oracle import ipc_oracle as I
from tests import exec_comps_cases as EC
from tests import exec_comps_oracle as X
from tests import hints_oracle as H
from tests.conftest import GOLDEN

M64 = (1 << 64) - 1
FILL64, FILL32 = 0xA5A5A5A5A5A5A5A5, 0xA5A5A5A5


@functools.lru_cache(maxsize=None)
def _golden():
    with np.load(os.path.join(GOLDEN, "exec_comps_golden.npz"), allow_pickle=False) as z:
        return {k: z[k] for k in z.files}


@functools.lru_cache(maxsize=None)
def _edges():
    return EC.edge_calls(np.random.default_rng(31))


# ---- CPU: the oracle against the reference's output ---------------------------
def test_golden_is_the_recorded_calls():
    g = _golden()
    recs, off = EC.to_arrays(EC.golden_calls())
    assert np.array_equal(g["recs"], recs) and np.array_equal(g["call_off"], off)
    lens = np.diff(off.astype(np.int64))
    assert lens.size == 39 and lens.max() == 16383 and (lens == 0).any()
    # the full buffer is mostly repeats: 16,383 records of 500 distinct triples
    assert int(g["comp_off"][-1] - g["comp_off"][-2]) == 500


def test_oracle_reproduces_the_reference():
    g = _golden()
    comp_off, comps, word_off, words = X.batch(g["recs"], g["call_off"])
    assert np.array_equal(comp_off, g["comp_off"]) and np.array_equal(comps, g["comps"])
    assert np.array_equal(word_off, g["word_off"]) and np.array_equal(words, g["words"])
    assert comps.dtype == g["comps"].dtype and words.dtype == g["words"].dtype


def test_oracle_edge_semantics():
    # sorted as unsigned 64-bit triples; the extension comes after sort and unique
    t, w = X.call_comps([(4, 0x100000005, 1, 0), (4, 0x5, 1, 0)])
    assert t == [(4, 5, 1), (4, 5, 1)] and w == [4, 5, 1, 4, 5, 1]
    t, w = X.call_comps([((1 << 32) + 1, 3, 4, 0), (7, M64, M64, 0), (1, 3, 4, 9)])
    assert [x[0] for x in t] == [1, 7, (1 << 32) + 1] and w == [1, 3, 4, 7] + [0xFFFFFFFF] * 4 + [1, 3, 4]
    # the writer's widths: size 8 takes four operand words, the others two (executor.h:646-656)
    t, w = X.call_comps([(6, (7 << 32) | 1, 1 << 63, 0), (0, 0x80, 0x7F, 0), (2, 0x8000, 0x7FFF, 0), (4, 1 << 31, 1, 0)])
    assert t == [(0, M64 - 0x7F, 0x7F), (2, M64 - 0x7FFF, 0x7FFF), (4, M64 - 0x7FFFFFFF, 1), (6, (7 << 32) | 1, 1 << 63)]
    assert w == [0, 0xFFFFFF80, 0x7F, 2, 0xFFFF8000, 0x7FFF, 4, 0x80000000, 1, 6, 1, 7, 0, 0x80000000]
    assert w[9:] == I.write_call(0, 0, 0, 0, [], [], [(6, (7 << 32) | 1, 1 << 63)], "writer")[7:]
    # equal (type, arg1, arg2), different pc: one entry
    assert X.call_comps([(2, 5, 6, pc) for pc in range(9)])[0] == [(2, 5, 6)]


# ---- GPU ----------------------------------------------------------------------
def _dev(ctx, recs, off, words=True, comps_cap=None, words_cap=None):
    """sg_exec_comps_dev through torch buffers; payloads prefilled."""
    import torch

    from syzkaller_amd._lib import call

    recs = np.ascontiguousarray(np.asarray(recs, np.uint64).reshape(-1, 4))
    off = np.ascontiguousarray(np.asarray(off, np.uint64))
    ncalls, nrecs = off.size - 1, int(off[-1])
    d = "cuda"
    t_recs = torch.from_numpy(recs.view(np.int64).copy()).to(d)
    t_off = torch.from_numpy(off.view(np.int64).copy()).to(d)
    ccap = nrecs if comps_cap is None else comps_cap
    wcap = 5 * nrecs if words_cap is None else words_cap
    comp_off = torch.full((ncalls + 1,), -1, dtype=torch.int64, device=d)
    word_off = torch.full((ncalls + 1,), -1, dtype=torch.int64, device=d)
    comps = torch.from_numpy(np.full(3 * max(ccap, 1), FILL64, np.uint64).view(np.int64)).to(d)
    wbuf = torch.from_numpy(np.full(max(wcap, 1), FILL32, np.uint32).view(np.int32)).to(d)
    torch.cuda.synchronize()
    call("sg_exec_comps_dev", ctx.h, t_recs.data_ptr(), t_off.data_ptr(), ncalls, nrecs, comp_off.data_ptr(),
         comps.data_ptr(), ccap, word_off.data_ptr() if words else None, wbuf.data_ptr() if words else None,
         wcap if words else 0)
    ctx.sync()
    return (comp_off.cpu().numpy().view(np.uint64), comps.cpu().numpy().view(np.uint64).reshape(-1, 3),
            word_off.cpu().numpy().view(np.uint64), wbuf.cpu().numpy().view(np.uint32))


def _same(got, exp):
    comp_off, comps, word_off, words = got
    assert np.array_equal(comp_off, exp[0]) and np.array_equal(word_off, exp[2])
    assert np.array_equal(comps, exp[1])
    assert np.array_equal(words, exp[3])


def _check(ctx, ctx_option, recs, off, exp, general_auto, dev=True):
    """Host and device form on both paths against exp; general_auto: the calls
    the auto path must send down the general path."""
    from syzkaller_amd import hints as G

    ncalls = len(off) - 1
    for path, general in ((-1, general_auto), (0, ncalls if int(off[-1]) else 0)):
        ctx_option(ctx, "exec_comps_path", path)
        _same(G.exec_comps(recs, off, ctx=ctx), exp)
        assert ctx.counter("exec_comps_general") == general, path
        if dev:
            comp_off, comps, word_off, words = _dev(ctx, recs, off)
            assert ctx.counter("exec_comps_general") == general, path
            _same((comp_off, comps[: int(comp_off[-1])], word_off, words[: int(word_off[-1])]), exp)
            assert (comps[int(comp_off[-1]):] == FILL64).all() and (words[int(word_off[-1]):] == FILL32).all()


def _check_calls(ctx, ctx_option, calls, general_auto=0, dev=True):
    recs, off = EC.to_arrays(calls)
    exp = X.batch(recs, off)
    _check(ctx, ctx_option, recs, off, exp, general_auto, dev)
    return exp


@pytest.mark.gpu
def test_golden_on_the_gpu(ctx, ctx_option):
    g = _golden()
    exp = (g["comp_off"], g["comps"], g["word_off"], g["words"])
    _check(ctx, ctx_option, g["recs"], g["call_off"], exp, 0)  # 500 distinct of 16,383: the fast shape


@pytest.mark.gpu
def test_edge_cases_and_lengths(ctx, ctx_option):
    from syzkaller_amd import hints as G

    e = _edges()
    assert ctx.counter("exec_comps_fast_cap") == G.EXEC_COMPS_FAST_CAP
    # every named case in one batch, then each length alone (a batch of one call)
    exp = _check_calls(ctx, ctx_option, list(e.values()))
    names = list(e)
    ncomp = dict(zip(names, np.diff(exp[0].astype(np.int64)).tolist()))
    assert ncomp["empty"] == 0 and ncomp["two_equal"] == 1 and ncomp["pcs"] == 2 and ncomp["equal_300"] == 1
    assert ncomp["distinct_300"] == 300 and ncomp["above_width"] == 8 and ncomp["sizes"] == 48
    rng = np.random.default_rng(32)
    p = EC.pool(rng, 40)
    # (256 and 2,048 records are the edges between the three workgroup shapes)
    for n in (0, 1, 2, 63, 64, 65, 255, 256, 257, 2047, 2048, 2049):
        _check_calls(ctx, ctx_option, [EC.draw(rng, p, n)], dev=n in (0, 1, 256, 257, 2048, 2049))
        _check_calls(ctx, ctx_option, [EC.distinct(rng, n)], dev=False)
    # no calls at all; calls but no records
    _check_calls(ctx, ctx_option, [])
    _check_calls(ctx, ctx_option, [[], [], []])


@pytest.mark.gpu
def test_many_short_calls(ctx, ctx_option):
    rng = np.random.default_rng(33)
    p = EC.pool(rng, 50)
    calls = [EC.draw(rng, p, int(n)) for n in rng.integers(0, 41, size=3000)]
    exp = _check_calls(ctx, ctx_option, calls)
    assert 0 < int(exp[0][-1]) < sum(len(c) for c in calls)  # repeats were removed


@pytest.mark.gpu
@pytest.mark.parametrize("delta", [-1, 0, 1])
def test_fast_shape_capacity(ctx, ctx_option, delta):
    from syzkaller_amd import hints as G

    rng = np.random.default_rng(34 + delta)
    n = G.EXEC_COMPS_FAST_CAP + delta
    calls = [EC.distinct(rng, 5), EC.distinct(rng, n), EC.distinct(rng, 300)]
    exp = _check_calls(ctx, ctx_option, calls, general_auto=1 if delta > 0 else 0)
    assert np.diff(exp[0].astype(np.int64)).tolist() == [5, n, 300]


@pytest.mark.gpu
def test_full_buffers(ctx, ctx_option):
    rng = np.random.default_rng(35)
    p = EC.pool(rng, 30)
    # 16,383 records (kCoverSize 64 Ki words): all distinct between short calls, then all equal
    calls = [EC.draw(rng, p, 20), EC.distinct(rng, 16383), EC.draw(rng, p, 700), [],
             [(5, 1 << 63, M64, EC.PC0 + 4 * i) for i in range(16383)], EC.distinct(rng, 9000, types=3)]
    exp = _check_calls(ctx, ctx_option, calls, general_auto=2)
    n = np.diff(exp[0].astype(np.int64)).tolist()
    assert n[1] == 16383 and n[4] == 1 and n[5] == 9000 and n[3] == 0


@pytest.mark.gpu
def test_workspace_growth_between_the_two_paths(ctx):  # (ctx: the session's context exists before any other, as for every GPU test here)
    """Three calls on one fresh context, on the auto path: the edge cases (the
    workspace takes its first 64 MiB); a batch whose first pass fits in those
    and whose general path does not; the edge cases again.  The second call's
    first pass has run when the workspace grows and drops its contents: the
    call has to run it again, with its pointers bound to the new block.

    The bytes, from exec_comps() and ec_general_bytes() (regions rounded up to
    256 B).  First pass: 24 B per record (tmp) and 17 B per call, plus the
    scan's few KiB.  General path over ng records: gidx, gcall, rlo, rhi
    (4 x 4 B), the five tables (5 x 8 B), v, ka, kb (3 x 8 B), pos (8 B), flags
    (4 B) = 92 B per record; 8 B per call; the sort's 256 counters of 12 B per
    tile of 8,192 keys; the scans; 4 KiB.  With calls of 65,535 distinct
    records (all on the general path: 65,535 > 4,096) that is, first pass /
    both:
      8 calls, 524,280 records: 12,585,216 / 61,025,792 B  (fits 67,108,864)
      9 calls, 589,815 records: 14,158,080 / 68,653,056 B  (does not)
    so 9 calls is the smallest such batch."""
    from syzkaller_amd import cover as C
    from syzkaller_amd import hints as G

    rng = np.random.default_rng(37)
    ncalls, per = 9, 65535
    # EC.distinct's records, drawn as arrays: the multiplier is odd, so arg1 alone tells the records of a call apart
    i = np.arange(per, dtype=np.uint64)
    big = np.empty((ncalls, per, 4), np.uint64)
    for c in range(ncalls):
        big[c, :, 0] = i % np.uint64(8)
        big[c, :, 1] = rng.permutation(per).astype(np.uint64) * np.uint64(0x9E3779B97F4A7C15)
        big[c, :, 2] = rng.integers(0, 1 << 62, size=per, dtype=np.uint64)
        big[c, :, 3] = np.uint64(EC.PC0) + np.uint64(4) * i
    big, big_off = big.reshape(-1, 4), np.arange(ncalls + 1, dtype=np.uint64) * np.uint64(per)
    small, small_off = EC.to_arrays(list(_edges().values()))
    e_small, e_big = X.batch(small, small_off), X.batch(big, big_off)
    assert np.diff(e_big[0].astype(np.int64)).tolist() == [per] * ncalls
    c = C.Context()
    try:
        _same(G.exec_comps(small, small_off, ctx=c), e_small)
        assert c.counter("workspace_bytes") == 64 << 20 and c.counter("exec_comps_general") == 0
        _same(G.exec_comps(big, big_off, ctx=c), e_big)
        assert c.counter("exec_comps_general") == ncalls and c.counter("workspace_bytes") > 64 << 20
        _same(G.exec_comps(small, small_off, ctx=c), e_small)
    finally:
        c.close()


@pytest.mark.gpu
def test_capacity_convention_and_arguments(ctx, ctx_option):
    import torch

    from syzkaller_amd import _lib
    from syzkaller_amd.cover import _p32, _p64

    lib, h, E = _lib.lib, ctx.h, _lib.SG_EINVAL
    e = _edges()
    recs, off = EC.to_arrays([e["sizes"], e["above_width"], [], e["pool_65"]])
    recs = np.ascontiguousarray(recs.reshape(-1))
    e_co, e_c, e_wo, e_w = X.batch(recs, off)
    ncalls, nc, nw = off.size - 1, int(e_co[-1]), int(e_wo[-1])
    assert nc > 1 and nw > 1
    for path in (-1, 0):
        ctx_option(ctx, "exec_comps_path", path)
        co, wo = np.zeros(ncalls + 1, np.uint64), np.zeros(ncalls + 1, np.uint64)
        comps, words = np.full((nc, 3), FILL64, np.uint64), np.full(nw, FILL32, np.uint32)
        # one short: the offsets are filled, that payload untouched (each payload by its own cap)
        assert lib.sg_exec_comps(h, _p64(recs), _p64(off), ncalls, _p64(co), _p64(comps), nc - 1, _p64(wo), _p32(words),
                                 nw - 1) == 0
        assert np.array_equal(co, e_co) and np.array_equal(wo, e_wo)
        assert (comps == FILL64).all() and (words == FILL32).all()
        assert lib.sg_exec_comps(h, _p64(recs), _p64(off), ncalls, _p64(co), _p64(comps), nc, _p64(wo), _p32(words),
                                 nw - 1) == 0
        assert np.array_equal(comps, e_c) and (words == FILL32).all()
        assert lib.sg_exec_comps(h, _p64(recs), _p64(off), ncalls, _p64(co), _p64(comps), nc, _p64(wo), _p32(words),
                                 nw) == 0
        assert np.array_equal(words, e_w)
        # the device form, one short
        d = _dev(ctx, recs, off, comps_cap=nc - 1, words_cap=nw - 1)
        assert np.array_equal(d[0], e_co) and np.array_equal(d[2], e_wo)
        assert (d[1] == FILL64).all() and (d[3] == FILL32).all()
        # word_off == NULL: the triples alone
        co[:] = 0
        comps[:] = FILL64
        assert lib.sg_exec_comps(h, _p64(recs), _p64(off), ncalls, _p64(co), _p64(comps), nc, None, None, 0) == 0
        assert np.array_equal(co, e_co) and np.array_equal(comps, e_c)
        d = _dev(ctx, recs, off, words=False)
        assert np.array_equal(d[0], e_co) and np.array_equal(d[1][:nc], e_c)
        assert (d[2] == M64).all() and (d[3] == FILL32).all()  # never touched
        # the offsets alone
        co[:] = 0
        assert lib.sg_exec_comps(h, _p64(recs), _p64(off), ncalls, _p64(co), None, 0, None, None, 0) == 0
        assert np.array_equal(co, e_co)
    from syzkaller_amd import hints as G

    got = G.exec_comps(recs, off, ctx=ctx, words=False)
    assert got[2] is None and got[3] is None and np.array_equal(got[1], e_c)
    # a NULL where a pointer is required; offsets that do not start at 0 or go down
    co, wo = np.zeros(ncalls + 1, np.uint64), np.zeros(ncalls + 1, np.uint64)
    comps, words = np.zeros((nc, 3), np.uint64), np.zeros(nw, np.uint32)
    a = (_p64(recs), _p64(off), ncalls, _p64(co), _p64(comps), nc, _p64(wo), _p32(words), nw)

    def but(i, v):
        return a[:i] + (v,) + a[i + 1:]

    assert lib.sg_exec_comps(None, *a) == E
    for i in (0, 1, 3, 4, 7):
        assert lib.sg_exec_comps(h, *but(i, None)) == E, i
    bad = off.copy()
    bad[0] = 1
    assert lib.sg_exec_comps(h, *but(1, _p64(bad))) == E
    bad = off.copy()
    bad[1], bad[2] = bad[2], bad[1] - 1
    assert lib.sg_exec_comps(h, *but(1, _p64(bad))) == E
    t = torch.zeros(64, dtype=torch.int64, device="cuda")
    p = t.data_ptr()
    dev = lib.sg_exec_comps_dev
    assert dev(None, p, p, 1, 1, p, p, 1, p, p, 5) == E
    assert dev(h, None, p, 1, 1, p, p, 1, p, p, 5) == E
    assert dev(h, p, None, 1, 1, p, p, 1, p, p, 5) == E
    assert dev(h, p, p, 1, 1, None, p, 1, p, p, 5) == E
    assert dev(h, p, p, 1, 1, p, None, 1, p, p, 5) == E
    assert dev(h, p, p, 1, 1, p, p, 1, p, None, 5) == E
    assert dev(h, p, p, 1, 1 << 32, p, p, 1, p, p, 5) == E  # nrecs < 2^32
    assert dev(h, p, p, 1 << 31, 1, p, p, 1, p, p, 5) == E  # ncalls < 2^31
    from syzkaller_amd._lib import SyzSigError

    for bad in (1, -2):
        with pytest.raises(SyzSigError):
            ctx.set_option("exec_comps_path", bad)


def _regions(calls_per_prog, comp_counts, word_lists):
    """Output regions as executor.h:369-427 writes them in comps mode: per call
    the seven header words (no signal, no cover) and its comparison words."""
    out, out_off, call_off, nums, r = [], [0], [0], [], 0
    for k in calls_per_prog:
        out.append(k)
        for ci in range(k):
            out += I.write_call(ci, 100 + ci, 0, 0, [], [], [])[:6] + [comp_counts[r]] + word_lists[r]
            nums.append(100 + ci)
            r += 1
        out_off.append(len(out))
        call_off.append(r)
    return (np.array(out, np.uint64).astype(np.uint32), np.array(out_off, np.uint64), np.array(call_off, np.uint64),
            np.array(nums, np.uint32))


@pytest.mark.gpu
def test_composition_with_the_reader(ctx):
    """The words as the comparison part of output regions: sg_ipc_comps on them
    equals the reader's oracle, statuses included, whatever the widths (the
    reader misreads the writer's layout, as it does the executor's)."""
    from syzkaller_amd import hints as G

    rng = np.random.default_rng(36)
    e = _edges()
    p = EC.pool(rng, 40)
    three = [r for r in EC.draw(rng, p, 400) if (r[0] & 6) != 6]
    # a program of one call with one size-8 comparison is the layout the reader walks through: it takes the type
    # and two of the four operand words, and ignores what trails its last record
    calls = [three[:50], [], e["sizes"], [(6, (9 << 32) | 5, 77, EC.PC0)], three[50:90], e["above_width"], e["extremes"],
             e["big_type"], EC.draw(rng, p, 200), [], [r for r in e["sizes"] if (r[0] & 6) == 6], [(7, 3, 4, EC.PC0)] * 3,
             [(0, 1, 2, EC.PC0), (0, 1, 3, EC.PC0), (0, 2, 1, EC.PC0)]]  # every word a legal type: the reader runs out
    recs, off = EC.to_arrays(calls)
    comp_off, comps, word_off, words = G.exec_comps(recs, off, ctx=ctx)
    _same((comp_off, comps, word_off, words), X.batch(recs, off))
    counts = np.diff(comp_off.astype(np.int64)).tolist()
    lists = [words[int(word_off[c]):int(word_off[c + 1])].tolist() for c in range(len(calls))]
    out, oo, co, nums = _regions([2, 1, 1, 2, 1, 1, 1, 1, 1, 1, 1], counts, lists)
    status, pairs, po = G.ipc_comps(out, oo, co, nums)
    e_status, e_lists = H.comps_batch(out, oo, co, nums)
    assert status.tolist() == e_status
    assert np.diff(po.astype(np.int64)).tolist() == [len(x) for x in e_lists]
    assert pairs.tolist() == [list(kv) for x in e_lists for kv in x]
    # both outcomes occur: regions the reader walks through, and regions it rejects
    assert {I.OK, I.COMPS_SHORT, I.COMPS_TYPE} <= set(e_status) and sum(len(x) for x in e_lists) > 0
