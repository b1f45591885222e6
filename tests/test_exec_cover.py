"""Executor cover: the flag_collect_cover branch of handle_completion
(executor/executor.h:402-415) over raw KCOV buffers.  On the CPU the boundary
(header, binding, exports, argument checks) and the test oracle
(tests/exec_cover_oracle.py) on hand-written cases; on the GPU sg_exec_cover and
sg_exec_cover_dev exact against the oracle, on the fast shapes and on the
general path."""
import os
import re
import subprocess

import numpy as np
import pytest

from tests import exec_cover_oracle as X
from tests.conftest import ROOT

M64 = (1 << 64) - 1
FILL32 = 0xA5A5A5A5
TEXT = 0xFFFFFFFF81000000  # where kernel text lies: the high word of a real PC is all ones


# ---- CPU: the boundary ---------------------------------------------------------
def _header():
    return open(os.path.join(ROOT, "include", "syzsig.h")).read()


def test_header_declares_exec_cover():
    src = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    for name in ("sg_exec_cover", "sg_exec_cover_dev"):
        assert re.search(r"\bint %s\s*\(" % name, src), name
    from syzkaller_amd import cover as C

    m = re.search(r"#define SG_EXEC_COVER_FAST_CAP (\d+)", src)
    assert m and int(m.group(1)) == C.EXEC_COVER_FAST_CAP
    # a table of twice the capacity in u64 keys fits the 160 KiB of LDS
    assert 2 * C.EXEC_COVER_FAST_CAP * 8 <= 160 * 1024 < 4 * C.EXEC_COVER_FAST_CAP * 8
    # the header says where the truncation happens, and cites the reference's own remark
    assert ":411-412" in _header()


def test_binding_and_library_export_exec_cover():
    from syzkaller_amd import _lib
    from syzkaller_amd import cover as C

    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r" T (sg_[a-z0-9_]+)$", out, flags=re.M))
    for name in ("sg_exec_cover", "sg_exec_cover_dev"):
        assert name in _lib.SIGNATURES and name in exported, name
    assert callable(C.exec_cover)


def test_null_context_is_einval():
    from syzkaller_amd import _lib
    from syzkaller_amd.cover import _p32, _p64

    pcs, off = np.array([TEXT, TEXT + 16], np.uint64), np.array([0, 2], np.uint64)
    cvo, cov = np.zeros(2, np.uint64), np.zeros(2, np.uint32)
    assert _lib.lib.sg_exec_cover(None, _p64(pcs), _p64(off), 1, 1, _p64(cvo), _p32(cov), 2) == _lib.SG_EINVAL
    assert _lib.lib.sg_exec_cover_dev(None, None, None, 1, 2, 1, None, None, 2) == _lib.SG_EINVAL


# ---- CPU: the oracle on hand-written cases ---------------------------------------
def test_oracle_edge_semantics():
    # sorted as unsigned 64-bit, one of every run of equals, truncated last (:408-414)
    assert X.call_cover([TEXT + 32, TEXT + 16, TEXT + 32, TEXT + 16, TEXT]).tolist() == \
        [0x81000000, 0x81000010, 0x81000020]
    # the truncation comes after the unique: two entries, in u64 order
    assert X.call_cover([0x2_0000_0010, 0x1_0000_0010]).tolist() == [0x10, 0x10]
    # ... so the u32 list need not be ascending
    assert X.call_cover([0x2_0000_0005, 0x1_0000_0010, 0x2_0000_0005]).tolist() == [0x10, 0x05]
    # unsigned order: 2^63 and 2^64 - 1 sort after every positive int64
    assert X.call_cover([M64, 1 << 63, 0, (1 << 63) - 1]).tolist() == [0, 0xFFFFFFFF, 0, 0xFFFFFFFF]
    # without flag_dedup_cover: every PC, in trace order (:413-414)
    assert X.call_cover([TEXT + 32, TEXT, TEXT + 32, 0x1_0000_0007], dedup=False).tolist() == \
        [0x81000020, 0x81000000, 0x81000020, 7]
    assert X.call_cover([]).size == 0 and X.call_cover([], dedup=False).size == 0
    cov, off = X.batch(*X.to_arrays([[5, 5, 4], [], [1 << 40]]))
    assert cov.tolist() == [4, 5, 0] and off.tolist() == [0, 2, 2, 3] and cov.dtype == np.uint32
    cov, off = X.batch(*X.to_arrays([]))
    assert cov.size == 0 and off.tolist() == [0]


# ---- GPU -----------------------------------------------------------------------
def draw(rng, n, nvals):
    """n PCs of a pool of nvals kernel-text PCs: repeats, as loops give."""
    pool = TEXT + 16 * rng.choice(1 << 20, size=max(nvals, 1), replace=False).astype(np.uint64)
    return pool[rng.integers(0, max(nvals, 1), size=n)]


def distinct(rng, n):
    """n distinct PCs, any u64, in random order."""
    v = np.unique(rng.integers(0, 1 << 63, size=n + 64, dtype=np.uint64) * np.uint64(2) + np.uint64(1))
    assert v.size >= n
    return rng.permutation(v)[:n]


def _dev(ctx, pcs, off, dedup=1, cap=None):
    """sg_exec_cover_dev through torch buffers; the payload prefilled."""
    import torch

    from syzkaller_amd._lib import call

    pcs = np.ascontiguousarray(np.asarray(pcs, np.uint64).reshape(-1))
    off = np.ascontiguousarray(np.asarray(off, np.uint64))
    ncalls, npcs = off.size - 1, int(off[-1])
    d = "cuda"
    t_pcs = torch.from_numpy(np.concatenate([pcs, np.zeros(1, np.uint64)]).view(np.int64).copy()).to(d)
    t_off = torch.from_numpy(off.view(np.int64).copy()).to(d)
    cap = npcs if cap is None else cap
    cov_off = torch.full((ncalls + 1,), -1, dtype=torch.int64, device=d)
    cov = torch.from_numpy(np.full(max(cap, 1) + 8, FILL32, np.uint32).view(np.int32)).to(d)
    torch.cuda.synchronize()
    call("sg_exec_cover_dev", ctx.h, t_pcs.data_ptr(), t_off.data_ptr(), ncalls, npcs, dedup, cov_off.data_ptr(),
         cov.data_ptr(), cap)
    ctx.sync()
    return cov.cpu().numpy().view(np.uint32), cov_off.cpu().numpy().view(np.uint64)


def _check(ctx, ctx_option, calls, general_auto=0, dev=True):
    """Host and device form on both paths against the oracle; general_auto: the
    calls the auto path must send down the general path."""
    from syzkaller_amd import cover as C

    pcs, off = X.to_arrays(calls)
    e_cov, e_off = X.batch(pcs, off)
    ncalls, n = len(calls), int(e_off[-1])
    for path, general in ((-1, general_auto), (0, ncalls if pcs.size else 0)):
        ctx_option(ctx, "exec_cover_path", path)
        cov, cvo = C.exec_cover(pcs, off, ctx=ctx)
        assert np.array_equal(cvo, e_off) and np.array_equal(cov, e_cov), path
        assert cov.dtype == np.uint32 and ctx.counter("exec_cover_general") == general, path
        if dev:
            cov, cvo = _dev(ctx, pcs, off)
            assert ctx.counter("exec_cover_general") == general, path
            assert np.array_equal(cvo, e_off) and np.array_equal(cov[:n], e_cov), path
            assert (cov[n:] == FILL32).all(), path  # untouched past the written length
    return e_cov, e_off


@pytest.mark.gpu
def test_lengths_and_shape_edges(ctx, ctx_option):
    from syzkaller_amd import cover as C

    assert ctx.counter("exec_cover_fast_cap") == C.EXEC_COVER_FAST_CAP == 8192
    rng = np.random.default_rng(41)
    # (256 and 2,048 PCs are the edges between the three workgroup shapes)
    lens = (0, 1, 2, 63, 64, 65, 255, 256, 257, 2047, 2048, 2049)
    for n in lens:
        on_dev = n in (0, 1, 65, 256, 257, 2048, 2049)
        _check(ctx, ctx_option, [draw(rng, n, 40)], dev=on_dev)
        _check(ctx, ctx_option, [distinct(rng, n)], dev=on_dev)
    # all of them in one batch, both kinds
    _, e_off = _check(ctx, ctx_option, [draw(rng, n, 40) for n in lens] + [distinct(rng, n) for n in lens])
    assert np.diff(e_off.astype(np.int64)).tolist()[len(lens):] == list(lens)
    # no calls at all; calls but no PCs
    _check(ctx, ctx_option, [])
    _check(ctx, ctx_option, [[], [], []])


@pytest.mark.gpu
@pytest.mark.parametrize("delta", [-1, 0, 1])
def test_fast_shape_capacity(ctx, ctx_option, delta):
    from syzkaller_amd import cover as C

    rng = np.random.default_rng(42 + delta)
    n = C.EXEC_COVER_FAST_CAP + delta
    # the n distinct PCs twice over, shuffled: the call is flagged by its distinct PCs, not by its length
    big = rng.permutation(np.concatenate([distinct(rng, n)] * 2))
    _, e_off = _check(ctx, ctx_option, [distinct(rng, 5), big, draw(rng, 300, 30)], general_auto=1 if delta > 0 else 0)
    assert np.diff(e_off.astype(np.int64)).tolist()[:2] == [5, n]
    # the marker's own value counts as a distinct PC of the capacity
    withm = rng.permutation(np.concatenate([distinct(rng, n - 1), [M64, M64]]).astype(np.uint64))
    _, e_off = _check(ctx, ctx_option, [withm], general_auto=1 if delta > 0 else 0, dev=False)
    assert int(e_off[-1]) == n


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["distinct", "equal", "loops"])
def test_full_buffers(ctx, ctx_option, kind):
    # 65,535 PCs: a full KCOV buffer (kCoverSize 64 Ki words, one of them the count), between short calls
    rng = np.random.default_rng(43)
    full = {"distinct": lambda: distinct(rng, 65535), "equal": lambda: np.full(65535, TEXT + 0x1230, np.uint64),
            "loops": lambda: draw(rng, 65535, 520)}[kind]()
    _, e_off = _check(ctx, ctx_option, [draw(rng, 20, 8), full, draw(rng, 700, 90), [], distinct(rng, 3)],
                      general_auto=1 if kind == "distinct" else 0)
    got = int(e_off[2] - e_off[1])
    assert {"distinct": got == 65535, "equal": got == 1, "loops": 500 < got <= 520}[kind]


@pytest.mark.gpu
def test_many_short_calls(ctx, ctx_option):
    rng = np.random.default_rng(44)
    calls = [draw(rng, int(n), 12) for n in rng.integers(0, 41, size=3000)]
    _, e_off = _check(ctx, ctx_option, calls)
    assert 0 < int(e_off[-1]) < sum(len(c) for c in calls)  # repeats were removed


@pytest.mark.gpu
def test_wide_pcs_and_special_values(ctx, ctx_option):
    rng = np.random.default_rng(45)
    # PCs that differ only above bit 31: separate entries, in u64 order; the u32 list repeats and goes down
    low = rng.integers(0, 1 << 32, size=50, dtype=np.uint64)
    wide = rng.permutation(np.concatenate([low + (np.uint64(h) << np.uint64(32)) for h in (0, 1, 2, 0xFFFFFFFF)] * 3))
    e_cov, e_off = _check(ctx, ctx_option, [wide, [0x2_0000_0010, 0x1_0000_0010], [0x2_0000_0005, 0x1_0000_0010]])
    assert int(e_off[1]) == 200 and (np.diff(e_cov[:200].astype(np.int64)) < 0).any()
    assert e_cov[200:].tolist() == [0x10, 0x10, 0x10, 0x05]
    # 0, 2^63, 2^64 - 1 (the table's empty marker): each alone, repeated, and with its neighbours
    calls = []
    for v in (0, 1 << 63, M64):
        nb = [(v - 1) & M64, v, (v + 1) & M64]
        calls += [[v], [v] * 70, nb, nb[::-1] * 3, list(rng.permutation(np.array(nb * 100, np.uint64)))]
    calls.append([0, 1 << 63, M64, M64 - 1, 1, (1 << 63) - 1, (1 << 63) + 1] * 40)
    calls.append(np.concatenate([distinct(rng, 3000), np.full(9, M64, np.uint64)]))  # the marker on the large shape
    _check(ctx, ctx_option, calls)


@pytest.mark.gpu
def test_without_dedup(ctx, ctx_option):
    from syzkaller_amd import cover as C

    rng = np.random.default_rng(46)
    calls = [draw(rng, 300, 20), [], [0x2_0000_0010, M64, 0, 0x2_0000_0010], distinct(rng, 2500), draw(rng, 1, 1)]
    pcs, off = X.to_arrays(calls)
    e_cov, e_off = X.batch(pcs, off, dedup=False)
    assert np.array_equal(e_off, off) and e_cov.size == pcs.size
    for path in (-1, 0):  # (the option plays no part)
        ctx_option(ctx, "exec_cover_path", path)
        cov, cvo = C.exec_cover(pcs, off, dedup=False, ctx=ctx)
        assert np.array_equal(cvo, off) and np.array_equal(cov, e_cov)
        assert ctx.counter("exec_cover_general") == 0
        cov, cvo = _dev(ctx, pcs, off, dedup=0)
        assert np.array_equal(cvo, off) and np.array_equal(cov[: pcs.size], e_cov) and (cov[pcs.size:] == FILL32).all()
    cov, cvo = _dev(ctx, pcs, off, dedup=0, cap=pcs.size - 1)  # one short: the offsets alone
    assert np.array_equal(cvo, off) and (cov == FILL32).all()
    cov, cvo = C.exec_cover([], [0, 0, 0], dedup=False, ctx=ctx)
    assert cov.size == 0 and cvo.tolist() == [0, 0, 0]


@pytest.mark.gpu
def test_staging_buffer_growth():
    """Three calls on one fresh context: a few hundred PCs, a batch whose
    staging (8 B per PC in, 4 B out) is past the buffer's first 16 MiB, the
    first batch again.  A region laid out past the reserved total would
    corrupt the second call, a pointer bound before the buffer moved the third."""
    from syzkaller_amd import cover as C

    rng = np.random.default_rng(48)
    small = X.to_arrays([draw(rng, 200, 30), [], distinct(rng, 90)])
    big = X.to_arrays([draw(rng, 55000, 400) for _ in range(40)])
    assert big[0].size * 12 > 16 << 20
    c = C.Context()
    try:
        got = []
        for pcs, off in (small, big, small):
            e_cov, e_off = X.batch(pcs, off)
            cov, cvo = C.exec_cover(pcs, off, ctx=c)
            assert np.array_equal(cvo, e_off) and np.array_equal(cov, e_cov), pcs.size
            e_cov, e_off = X.batch(pcs, off, dedup=False)
            raw, rwo = C.exec_cover(pcs, off, dedup=False, ctx=c)
            assert np.array_equal(rwo, e_off) and np.array_equal(raw, e_cov), pcs.size
            got.append((cov.copy(), cvo.copy(), raw.copy(), rwo.copy()))
        assert all(np.array_equal(a, b) for a, b in zip(got[0], got[2]))
    finally:
        c.close()


@pytest.mark.gpu
def test_workspace_growth_between_the_two_paths(ctx):  # (ctx: the session's context exists before any other, as for every GPU test here)
    """Three calls on one fresh context, on the auto path: a few hundred PCs
    (the workspace takes its first 64 MiB); a batch whose first pass fits in
    those and whose general path does not; the first batch again.  The second
    call's first pass has run when the workspace grows and drops its contents:
    the call has to run it again, with its pointers bound to the new block.

    The bytes, from exec_cover() and xc_general_bytes() (regions rounded up to
    256 B).  First pass: 4 B per PC (tmp) and 13 B per call, plus the scan's
    few KiB.  General path over ng PCs: gidx, gcall, rank (3 x 4 B), U (8 B),
    v, ka, kb (3 x 8 B), pos (8 B), flags (4 B) = 56 B per PC; 8 B per call;
    the sort's 256 counters of 12 B per tile of 8,192 keys; the scans; 4 KiB.
    With calls of 65,535 distinct PCs (a full KCOV buffer, all on the general
    path: 65,535 > 8,192) that is, first pass / both:
      16 calls, 1,048,560 PCs: 4,196,352 / 63,321,344 B  (fits 67,108,864)
      17 calls, 1,114,095 PCs: 4,458,496 / 67,278,592 B  (does not)
    so 17 calls is the smallest such batch."""
    from syzkaller_amd import cover as C

    rng = np.random.default_rng(49)
    ncalls, per = 17, 65535
    small = X.to_arrays([draw(rng, 200, 30), [], distinct(rng, 90)])
    big = (distinct(rng, ncalls * per), np.arange(ncalls + 1, dtype=np.uint64) * np.uint64(per))
    e_small, e_big = X.batch(*small), X.batch(*big)
    assert int(e_big[1][-1]) == ncalls * per
    c = C.Context()
    try:
        cov, cvo = C.exec_cover(*small, ctx=c)
        assert np.array_equal(cvo, e_small[1]) and np.array_equal(cov, e_small[0])
        assert c.counter("workspace_bytes") == 64 << 20 and c.counter("exec_cover_general") == 0
        cov, cvo = C.exec_cover(*big, ctx=c)
        assert np.array_equal(cvo, e_big[1]) and np.array_equal(cov, e_big[0])
        assert c.counter("exec_cover_general") == ncalls and c.counter("workspace_bytes") > 64 << 20
        cov, cvo = C.exec_cover(*small, ctx=c)
        assert np.array_equal(cvo, e_small[1]) and np.array_equal(cov, e_small[0])
    finally:
        c.close()


@pytest.mark.gpu
def test_capacity_convention_and_arguments(ctx, ctx_option):
    import torch

    from syzkaller_amd import _lib
    from syzkaller_amd.cover import _p32, _p64

    lib, h, E = _lib.lib, ctx.h, _lib.SG_EINVAL
    rng = np.random.default_rng(47)
    pcs, off = X.to_arrays([draw(rng, 90, 11), [], draw(rng, 400, 60), distinct(rng, 2100)])
    e_cov, e_off = X.batch(pcs, off)
    ncalls, n = off.size - 1, int(e_off[-1])
    assert 1 < n < pcs.size
    for path in (-1, 0):
        ctx_option(ctx, "exec_cover_path", path)
        cvo, cov = np.zeros(ncalls + 1, np.uint64), np.full(n, FILL32, np.uint32)
        # one short: the offsets are filled, the payload untouched
        assert lib.sg_exec_cover(h, _p64(pcs), _p64(off), ncalls, 1, _p64(cvo), _p32(cov), n - 1) == 0
        assert np.array_equal(cvo, e_off) and (cov == FILL32).all()
        assert lib.sg_exec_cover(h, _p64(pcs), _p64(off), ncalls, 1, _p64(cvo), _p32(cov), n) == 0
        assert np.array_equal(cov, e_cov)
        d_cov, d_off = _dev(ctx, pcs, off, cap=n - 1)
        assert np.array_equal(d_off, e_off) and (d_cov == FILL32).all()
        d_cov, d_off = _dev(ctx, pcs, off, cap=n)
        assert np.array_equal(d_cov[:n], e_cov) and (d_cov[n:] == FILL32).all()
        # the offsets alone
        cvo[:] = 0
        assert lib.sg_exec_cover(h, _p64(pcs), _p64(off), ncalls, 1, _p64(cvo), None, 0) == 0
        assert np.array_equal(cvo, e_off)
    # a NULL where a pointer is required; offsets that do not start at 0 or go down; dedup above 1
    cvo, cov = np.zeros(ncalls + 1, np.uint64), np.zeros(n, np.uint32)
    a = (_p64(pcs), _p64(off), ncalls, 1, _p64(cvo), _p32(cov), n)

    def but(i, v):
        return a[:i] + (v,) + a[i + 1:]

    assert lib.sg_exec_cover(None, *a) == E
    for i in (0, 1, 4, 5):
        assert lib.sg_exec_cover(h, *but(i, None)) == E, i
    assert lib.sg_exec_cover(h, *but(3, 2)) == E and lib.sg_exec_cover(h, *but(3, -1)) == E
    bad = off.copy()
    bad[0] = 1
    assert lib.sg_exec_cover(h, *but(1, _p64(bad))) == E
    bad = off.copy()
    bad[2], bad[3] = bad[3], bad[2] - 1
    assert lib.sg_exec_cover(h, *but(1, _p64(bad))) == E
    t = torch.zeros(64, dtype=torch.int64, device="cuda")
    p = t.data_ptr()
    dev = lib.sg_exec_cover_dev
    assert dev(None, p, p, 1, 1, 1, p, p, 1) == E
    assert dev(h, None, p, 1, 1, 1, p, p, 1) == E
    assert dev(h, p, None, 1, 1, 1, p, p, 1) == E
    assert dev(h, p, p, 1, 1, 1, None, p, 1) == E
    assert dev(h, p, p, 1, 1, 1, p, None, 1) == E
    assert dev(h, p, p, 1, 1, 2, p, p, 1) == E        # dedup is 0 or 1
    assert dev(h, p, p, 1, 1 << 32, 1, p, p, 1) == E  # npcs < 2^32
    assert dev(h, p, p, 1 << 31, 1, 1, p, p, 1) == E  # ncalls < 2^31
    from syzkaller_amd._lib import SyzSigError

    for bad in (1, -2):
        with pytest.raises(SyzSigError):
            ctx.set_option("exec_cover_path", bad)
