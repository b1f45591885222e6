"""Call priorities (prog/prio.go:27-36, :133-229; syz-manager/manager.go:816-837):
sg_prio_table_*, sg_call_prios*.  On the CPU the boundary, every rejected
argument, the no-device result, the test oracle (tests/call_prios_oracle.py:
its literal and its closed form agree, and give the worked example's matrices)
and the conditions the cases must hold, among them that the parity corpus
tells a fused multiply-add from the reference's two roundings.  On the GPU
counts, dynamic, prios and run bit-exact against the oracle."""
import functools
import os
import re
import subprocess

import numpy as np
import pytest

from tests import call_prios_cases as K
from tests import call_prios_checks as CK
from tests import call_prios_oracle as OR
from tests.conftest import ROOT

U8, U32, U64, I32, F32 = np.uint8, np.uint32, np.uint64, np.int32, np.float32
NO_CALL = K.NO_CALL
NAMES = ("sg_prio_table_create", "sg_prio_table_destroy", "sg_prio_table_clear", "sg_prio_table_add",
         "sg_prio_table_add_dev", "sg_prio_table_counts", "sg_call_prios", "sg_call_prios_dev",
         "sg_call_prios_from_progs")
FILLF, FILLI = F32(-7.5), -123456789


_has_gpu, _bits, _same, _to_dev = CK.has_gpu, CK.bits, CK.same, CK.to_dev  # (shared with the edge file)


# ---- CPU: the boundary ---------------------------------------------------------
def test_header_binding_and_library():
    import syzkaller_amd
    from syzkaller_amd import _lib
    from syzkaller_amd import prio as P

    text = open(os.path.join(ROOT, "include", "syzsig.h")).read()
    for cite in ("syz-manager/manager.go:816-837", "syz-manager/html.go:196-224", "prog/prio.go:27-36",
                 "prog/prio.go:138-151", "prog/prio.go:158-192", "prog/prio.go:203-229", "prog/prio.go:106-116"):
        assert cite in text, cite
    assert "no NaN can arise" in text and "Removing programs is left out" in text
    assert re.search(r"#define SG_NO_CALL 0xffffffffu\b", text) and re.search(r"#define SG_PRIO_MAX_CALLS 8192\b", text)
    src = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r" T (sg_[a-z0-9_]+)$", out, flags=re.M))
    for name in NAMES:
        assert re.search(r"\b(int|void) %s\s*\(" % name, src), name
        assert name in _lib.SIGNATURES and name in exported, name
    for name in ("PrioTable", "CalculatePriorities", "BuildChoiceTable", "ChoiceTable"):
        assert callable(getattr(P, name)) and getattr(syzkaller_amd, name) is getattr(P, name)
    assert P.NO_CALL == NO_CALL and P.MAX_CALLS == 8192
    # the unit turns contraction off in its source and leaves the Makefile's flags alone
    unit = open(os.path.join(ROOT, "syzkaller_amd", "csrc", "sg_call_prios.hip")).read()
    assert "#pragma clang fp contract(off)" in unit and "__fdividef" not in unit.split("#include", 1)[1]
    assert "contract" not in open(os.path.join(ROOT, "syzkaller_amd", "Makefile")).read()


def _example():
    from syzkaller_amd.cover import _p8, _p32, _p64
    from syzkaller_amd.prio import _pf

    ids, off = K.csr(K.EX_PROGS)
    st, en = K.EX_STATIC.copy(), K.EX_ENABLED.copy()
    return ids, off, st, en, _p32(ids), _p64(off), _pf(st), _p8(en)


def test_invalid_arguments_are_einval():
    """Every check the calls make before they touch the context: a context, or a table, that is only a readable
    block of memory is enough (a zeroed table has ncalls == 0, so any id is out of range)."""
    from syzkaller_amd import _lib
    from syzkaller_amd.cover import _p32, _p64
    from syzkaller_amd.prio import _pf, _pi

    lib, E = _lib.lib, _lib.SG_EINVAL
    ids, off, st, en, pids, poff, pst, pen = _example()
    block = np.zeros(1 << 16, U8)
    fake = block.ctypes.data_as(_lib.c_void_p)  # never used: each case below returns first
    out = _lib.c_void_p()
    ref = _lib.ctypes.byref(out)
    assert lib.sg_prio_table_create(None, 4, 3, pst, pen, ref) == E
    assert lib.sg_prio_table_create(fake, 4, 3, None, pen, ref) == E
    assert lib.sg_prio_table_create(fake, 4, 3, pst, pen, None) == E
    assert lib.sg_prio_table_create(fake, 0, NO_CALL, pst, pen, ref) == E
    assert lib.sg_prio_table_create(fake, 8193, NO_CALL, pst, pen, ref) == E
    assert lib.sg_prio_table_create(fake, 4, 4, pst, pen, ref) == E            # mmap_id == ncalls
    assert lib.sg_prio_table_create(fake, 4, 0xFFFFFFFE, pst, pen, ref) == E
    for bad in (np.nan, np.inf, -np.inf, -0.001, 1.0001):
        s = st.copy()
        s[3, 3] = bad
        assert lib.sg_prio_table_create(fake, 4, 3, _pf(s), pen, ref) == E, bad
        assert lib.sg_last_error()
    assert not out.value

    dyn, pr, run = np.zeros(16, F32), np.zeros(16, F32), np.zeros(16, I32)
    outs = (_pf(dyn), _pf(pr), _pi(run))
    for fn, tail in ((lib.sg_prio_table_add, ()), (lib.sg_call_prios_from_progs, outs)):
        assert fn(None, pids, poff, 4, *tail) == E
        assert fn(fake, pids, None, 4, *tail) == E
        assert fn(fake, None, poff, 4, *tail) == E
        o = off.copy()
        o[0] = 1
        assert fn(fake, pids, _p64(o), 4, *tail) == E                           # prog_off[0] != 0
        o = off.copy()
        o[2] = 1
        assert fn(fake, pids, _p64(o), 4, *tail) == E                           # decreasing
        o = np.array([0, 1 << 32], U64)
        assert fn(fake, pids, _p64(o), 1, *tail) == E                           # 2^32 ids
        assert fn(fake, pids, poff, 4, *tail) == E                              # an id >= ncalls (0 here)
    assert np.all(dyn == 0) and np.all(run == 0)
    assert lib.sg_prio_table_add_dev(None, fake, fake, 1, 1) == E
    assert lib.sg_prio_table_add_dev(fake, fake, None, 1, 1) == E
    assert lib.sg_prio_table_add_dev(fake, None, fake, 1, 1) == E
    assert lib.sg_prio_table_add_dev(fake, fake, fake, 1, 1 << 32) == E
    assert lib.sg_prio_table_clear(None) == E
    assert lib.sg_prio_table_counts(None, _p64(np.zeros(16, U64))) == E
    assert lib.sg_prio_table_counts(fake, None) == E
    assert lib.sg_call_prios(None, *outs) == E and lib.sg_call_prios_dev(None, None, None, None) == E
    lib.sg_prio_table_destroy(None)


@pytest.mark.skipif(_has_gpu(), reason="checks the no-GPU failure path")
def test_no_device_is_enodev():
    """Valid arguments and no device: the first thing the call asks of the context fails."""
    from syzkaller_amd import _lib

    ids, off, st, en, pids, poff, pst, pen = _example()
    block = np.zeros(1 << 16, U8)  # a zeroed sg_ctx: device 0, an unlocked mutex
    out = _lib.c_void_p()
    rc = _lib.lib.sg_prio_table_create(block.ctypes.data_as(_lib.c_void_p), 4, 3, pst, pen, _lib.ctypes.byref(out))
    assert rc == _lib.SG_ENODEV and not out.value


# ---- CPU: the oracle ---------------------------------------------------------------
def test_oracle_worked_example():
    ids, off = K.csr(K.EX_PROGS)
    cells = OR.literal_cells(K.EX_PROGS, K.EX_NCALLS, K.EX_MMAP)
    assert np.array_equal(cells, K.EX_COUNTS.astype(F32))
    cnt, dyn, pr, run = OR.everything(ids, off, K.EX_NCALLS, K.EX_MMAP, K.EX_STATIC, K.EX_ENABLED)
    assert np.array_equal(cnt, K.EX_COUNTS)
    assert np.array_equal(_bits(dyn), K.EX_DYNAMIC_BITS)
    assert np.array_equal(_bits(OR.literal_normalize(cells)), K.EX_DYNAMIC_BITS)
    assert np.array_equal(run, K.EX_RUN)
    lit = OR.literal_run(pr, K.EX_ENABLED)
    assert lit[2] is None and [lit[i] for i in (0, 1, 3)] == [K.EX_RUN[i].tolist() for i in (0, 1, 3)]


@functools.lru_cache(maxsize=None)
def _expected(name):
    """(ids, off, ncalls, mmap_id, static, enabled, (counts, dynamic, prios, run)), computed once and shared."""
    if name == "example":
        progs, nc, mm, st, en = K.EX_PROGS, K.EX_NCALLS, K.EX_MMAP, K.EX_STATIC, K.EX_ENABLED
    elif name == "corpus12":
        progs, nc, mm, st, en = K.corpus12()
    else:
        nc = int(name)
        progs, nc, mm, st, en = K.random_case(nc, 1000 + nc, nprogs=1500 if nc == 257 else 60)
    ids, off = K.csr(progs)
    exp = OR.everything(ids, off, nc, mm, st, en)
    for a in (ids, off, st, en) + exp:
        a.setflags(write=False)
    return ids, off, nc, mm, st, en, exp


def test_oracle_literal_and_closed_forms_agree():
    for name in ("example", "corpus12", "1", "63"):
        ids, off, nc, mm, st, en, (cnt, dyn, pr, run) = _expected(name)
        cells = OR.literal_cells(OR.programs(ids, off), nc, mm)
        assert np.array_equal(cells, OR.cells(cnt)), name
        assert np.array_equal(_bits(OR.literal_normalize(cells)), _bits(dyn)), name
        lit = OR.literal_run(pr, en)
        for i in range(nc):
            assert (lit[i] is None and not en[i] and not run[i].any()) or lit[i] == run[i].tolist(), (name, i)
    # the sticking add, on a cell alone: 2^24 + 1 == 2^24 in float32
    assert F32(F32(1 << 24) + F32(1)) == F32(1 << 24) and F32(F32((1 << 24) - 1) + F32(1)) == F32(1 << 24)
    assert OR.cells(np.array([[K.SAT_N * K.SAT_N]], U64))[0, 0] == F32(1 << 24)


def test_generator_conditions():
    ids, off, nc, mm, st, en, (cnt, dyn, pr, run) = _expected("corpus12")
    progs = OR.programs(ids, off)
    assert len(progs) == 40 and min(len(p) for p in progs) >= 1 and max(len(p) for p in progs) <= 9
    assert any(len(set(p.tolist())) < len(p) for p in progs)                   # a repeated id
    assert not cnt[11].any() and not cnt[mm].any() and (dyn[11] == 1).all()    # all-zero rows
    assert not en[5] and not run[5].any() and (run[:, 5] == run[:, 4]).all()   # a disabled row and column
    assert K.SAT_N * K.SAT_N == 16785409 > 1 << 24                              # a cell above 2^24
    ids2, off2 = K.csr([K.SAT_PROG])
    c2 = OR.counts(ids2, off2, 2, NO_CALL)
    assert c2[0, 1] == c2[1, 0] == 16785409 and len(K.SAT_PROG) > 8192
    # the random cases: an empty program, an mmap-only one, programs at and past the band path's length
    for name in map(str, K.SIZES):
        ids, off, nc, mm, st, en, exp = _expected(name)
        lens = np.diff(off.astype(np.int64))
        assert 0 in lens and K.SHORT_LEN in lens and K.SHORT_LEN + 1 in lens and 300 in lens, name
        assert any(len(p) and (p == mm).all() for p in OR.programs(ids, off)), name
        assert nc == 1 or (en == 0).any(), name
    assert int(_expected("257")[1][-1]) > 2 * 4096                             # more than one part of the id stream
    assert (K.BAND_EDGE - 1) ** 2 <= K.BAND_CELLS < K.BAND_EDGE ** 2


def test_parity_corpus_tells_contraction():
    """A build that fused q * 0.9 + 0.1 would differ from the oracle on the 12-call corpus, so the GPU parity
    test cannot hide contraction."""
    ids, off, nc, mm, st, en, (cnt, dyn, pr, run) = _expected("corpus12")
    fused = OR.normalize_fused(OR.cells(cnt))
    ndiff = int((_bits(fused) != _bits(dyn)).sum())
    print("cells of the 12-call corpus that a fused multiply-add changes:", ndiff, "of", dyn.size)
    assert ndiff > 0


# ---- GPU ----------------------------------------------------------------------------------
def _table(ctx, name):
    from syzkaller_amd.prio import PrioTable

    ids, off, nc, mm, st, en, exp = _expected(name)
    return PrioTable(st, mm, en, ctx=ctx), ids, off, exp


@pytest.mark.gpu
@pytest.mark.parametrize("name", ("example", "corpus12") + tuple(map(str, K.SIZES)))
def test_bit_exact(ctx, name):
    assert ctx.counter("prio_band_cells") == K.BAND_CELLS and ctx.counter("prio_short_len") == K.SHORT_LEN
    t, ids, off, exp = _table(ctx, name)
    t.add(csr=(ids, off))
    assert np.array_equal(t.counts(), exp[0]), name
    _same(t.prios(), exp, name)
    assert np.array_equal(t.counts(), exp[0])            # the finish leaves the counts alone
    _same(t.from_progs(csr=(ids, off)), exp, name)           # clear + add + finish: nothing doubles
    assert np.array_equal(t.counts(), exp[0])
    t.close()


@pytest.mark.gpu
def test_worked_example_written_out(ctx):
    from syzkaller_amd.prio import CalculatePriorities, PrioTable

    t = PrioTable(K.EX_STATIC, K.EX_MMAP, K.EX_ENABLED, ctx=ctx)
    dyn, pr, run = t.from_progs(K.EX_PROGS)
    assert np.array_equal(t.counts(), K.EX_COUNTS)
    assert np.array_equal(_bits(dyn), K.EX_DYNAMIC_BITS) and np.array_equal(run, K.EX_RUN)
    assert np.array_equal(_bits(CalculatePriorities(K.EX_PROGS, K.EX_STATIC, K.EX_MMAP, ctx=ctx)), _bits(pr))
    t.close()


@pytest.mark.gpu
def test_empty_corpus_empty_programs_and_mmap(ctx):
    from syzkaller_amd.prio import PrioTable

    rng = np.random.default_rng(5)
    st = rng.integers(0, 1001, size=(6, 6)).astype(F32) / F32(1000)
    for mm in (2, NO_CALL):
        t = PrioTable(st, mm, ctx=ctx)
        for progs in ([], [[]], [[], [], []], [[4]], [[2, 2, 2]], [[], [2, 2], [1], [], [0, 2, 1, 2]]):
            ids, off = K.csr(progs)
            exp = OR.everything(ids, off, 6, mm, st, None)
            _same(t.from_progs(progs), exp, (mm, progs))
            assert np.array_equal(t.counts(), exp[0]), (mm, progs)
        t.close()


@pytest.mark.gpu
def test_saturation_and_a_program_longer_than_any_buffer(ctx):
    from syzkaller_amd.prio import PrioTable

    st = np.array([[0.5, 0.75, 1], [1, 0.25, 0.5], [0.125, 1, 1]], F32)
    t = PrioTable(st, NO_CALL, ctx=ctx)
    progs = [K.SAT_PROG, [0, 1, 2], [2, 1]]
    ids, off = K.csr(progs)
    exp = OR.everything(ids, off, 3, NO_CALL, st, None)
    assert exp[0][0, 1] == exp[0][1, 0] == 16785409 + 1 and OR.cells(exp[0])[0, 1] == F32(1 << 24)
    got = t.from_progs(progs)
    assert np.array_equal(t.counts(), exp[0])            # exact, not saturated
    _same(got, exp, "saturation")                        # dynamic from the saturated cell
    # the same count from short programs alone (the band path, every part of the id stream adding into one
    # cell): 16392 programs of 32 * 32 pairs are 16,785,408, and one pair more
    t.clear()
    short = [[0] * 32 + [1] * 32] * 16392
    t.add(short + [[0, 1]])
    c = t.counts()
    assert c[0, 1] == c[1, 0] == 16785409 and c.sum() == 2 * 16785409
    t.close()


@pytest.mark.gpu
def test_two_adds_clear_and_from_progs(ctx):
    t, ids, off, exp = _table(ctx, "65")
    progs = OR.programs(ids, off)
    h = len(progs) // 2
    t.add(progs[:h])
    t.add(progs[h:])
    assert np.array_equal(t.counts(), exp[0])
    _same(t.prios(), exp, "two adds")
    t.add(progs)                                          # accumulates
    assert np.array_equal(t.counts(), 2 * exp[0])
    t.clear()
    assert not t.counts().any()
    d, p, r = t.prios()
    assert (d == 1).all()                                 # every row all zero
    t.add(csr=(ids, off))
    three = t.prios()
    one = t.from_progs(csr=(ids, off))
    for a, b in zip(three, one):
        assert np.array_equal(a.view(U32), b.view(U32))
    t.close()


@pytest.mark.gpu
def test_device_form_skips_bad_ids(ctx):
    import torch

    from syzkaller_amd._lib import call

    t, ids, off, exp = _table(ctx, "corpus12")
    nc = 12
    # out-of-range ids put into the programs (one in a long program): skipped, the rest as before
    progs = [p.tolist() for p in OR.programs(ids, off)]
    progs[0] = [nc] + progs[0]
    progs[5] = progs[5] + [0xFFFFFFFF, 4000000000]
    progs.append([nc + 1] * 3 + [1] * 70)                 # a long program: 3 bad ids, and only call 1
    bids, boff = K.csr(progs)
    d_ids, d_off = _to_dev(bids), _to_dev(boff)
    n = nc * nc
    d_dyn = torch.full((n + 16,), float(FILLF), dtype=torch.float32, device="cuda")
    d_pr = torch.full((n + 16,), float(FILLF), dtype=torch.float32, device="cuda")
    d_run = torch.full((n + 16,), FILLI, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    before = ctx.counter("prio_bad_ids")
    call("sg_prio_table_add_dev", t.h, d_ids.data_ptr(), d_off.data_ptr(), len(progs), bids.size)
    call("sg_call_prios_dev", t.h, d_dyn.data_ptr(), d_pr.data_ptr(), d_run.data_ptr())
    ctx.sync()
    assert ctx.counter("prio_bad_ids") == before + 6
    assert np.array_equal(t.counts(), exp[0])
    dyn, pr, run = d_dyn.cpu().numpy(), d_pr.cpu().numpy(), d_run.cpu().numpy()
    _same((dyn[:n].reshape(nc, nc), pr[:n].reshape(nc, nc), run[:n].reshape(nc, nc)), exp, "device form")
    assert (dyn[n:] == FILLF).all() and (pr[n:] == FILLF).all() and (run[n:] == FILLI).all()
    # ranges are clamped to nids: offsets that run past the ids count only the ids that are there
    t.clear()
    call("sg_prio_table_add_dev", t.h, d_ids.data_ptr(), _to_dev(np.array([0, 1000], U64)).data_ptr(), 1, 3)
    ctx.sync()
    first = OR.counts(bids[:3], np.array([0, 3], U64), nc + 1, 3)[:nc, :nc]  # (the bad id dropped with its row)
    assert np.array_equal(t.counts(), first)
    t.close()


@pytest.mark.gpu
def test_null_outputs_and_tails(ctx):
    from syzkaller_amd import _lib
    from syzkaller_amd.cover import _p32, _p64
    from syzkaller_amd.prio import _pf, _pi

    t, ids, off, exp = _table(ctx, "63")
    n = 63 * 63
    t.add(csr=(ids, off))
    for mask in (0b111, 0b110, 0b101, 0b011, 0b001, 0b010, 0b100, 0b000):
        for fused in (False, True):
            dyn, pr = np.full(n + 16, FILLF, F32), np.full(n + 16, FILLF, F32)
            run = np.full(n + 16, FILLI, I32)
            ptrs = [_pf(dyn) if mask & 1 else None, _pf(pr) if mask & 2 else None, _pi(run) if mask & 4 else None]
            if fused:
                _lib.call("sg_call_prios_from_progs", t.h, _p32(ids), _p64(off), off.size - 1, *ptrs)
            else:
                _lib.call("sg_call_prios", t.h, *ptrs)
            for k, (buf, e, fill) in enumerate(((dyn, exp[1], FILLF), (pr, exp[2], FILLF), (run, exp[3], FILLI))):
                assert (buf[n:] == fill).all(), (mask, k)
                if mask >> k & 1:
                    assert np.array_equal(buf[:n].view(U32), np.ascontiguousarray(e).reshape(-1).view(U32)), (mask, k)
                else:
                    assert (buf[:n] == fill).all(), (mask, k)
            assert np.array_equal(t.counts(), exp[0])
    t.close()


@pytest.mark.gpu
def test_choice_table_and_choose(ctx):
    from syzkaller_amd.prio import BuildChoiceTable, ChoiceTable

    t, ids, off, exp = _table(ctx, "corpus12")
    ids, off, nc, mm, st, en, _ = _expected("corpus12")
    t.add(csr=(ids, off))
    ct = BuildChoiceTable(t)
    assert isinstance(ct, ChoiceTable) and ct.run[5] is None
    lit = OR.literal_run(exp[2], en)
    for i in range(nc):
        assert (lit[i] is None and ct.run[i] is None) or ct.run[i].tolist() == lit[i], i
    # from a matrix, with column 0 disabled as well: SearchInts(run, 0) is 0, the one draw that lands on a
    # disabled column (run[j] == run[j - 1] keeps every later one from being found)
    en2 = en.copy()
    en2[0] = 0
    ct2 = BuildChoiceTable(exp[2], en2, ctx=ctx)
    ct3 = BuildChoiceTable(exp[2], ctx=ctx)              # every call enabled
    lit2, full = OR.literal_run(exp[2], en2), OR.literal_run(exp[2], np.ones(nc, U8))
    for i in range(nc):
        assert (lit2[i] is None and ct2.run[i] is None) or ct2.run[i].tolist() == lit2[i], i
        assert ct3.run[i].tolist() == full[i], i
    draws = [0, 7, 123456, 99, 31337, 2, 0, 4242, 65535, 1, 5000, 777, 88, 3, 600, 12, 999999]
    for call_id in (-1, 0, 1, 5, 7, 11):
        for k in range(8):
            seq = draws[k:] + draws
            gi, wi = K.draws_from(seq), K.draws_from(seq)
            got, want = ct2.Choose(gi, call_id), OR.choose(lit2, en2, wi, call_id)
            assert got == want and gi.used == wi.used and en2[got], (call_id, k)
            if k == 0:  # the first draw is 0: retried on an enabled row, taken as an index on a disabled one
                assert gi.used == (2 if en2[call_id] and call_id >= 0 else 1), call_id
    t.close()


@pytest.mark.gpu
def test_minimize_unchanged_around_a_table(ctx, kats):
    from syzkaller_amd import cover as C

    def kat():
        for case in kats["TestMinimize"]["cases"]:
            assert C.Minimize([np.array(c, np.uint32) for c in case["inp"]], ctx=ctx) == case["out"]

    kat()
    t, ids, off, exp = _table(ctx, "64")
    _same(t.from_progs(csr=(ids, off)), exp, "64")
    kat()
    t.close()
    kat()
