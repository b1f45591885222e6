"""Hint seeds: raw KCOV_TRACE_CMP buffers and argument values to shrinkExpand's
replacers (syz-fuzzer/fuzzer.go:627-643, pkg/ipc/ipc_linux.go:266-304,
prog/hints.go:50-177).  On the CPU the oracle chain (tests/hint_seed_oracle.py)
against the reference's own tables, turned into raw records, and the boundary;
on the GPU sg_comps_pairs and sg_hints_from_kcov, host and device forms, exact
against that chain and against the three separate calls."""
import ctypes
import functools
import os

import numpy as np
import pytest

from tests import exec_comps_cases as EC
from tests import exec_comps_oracle as X
from tests import hint_seed_oracle as O
from tests import hints_cases as HC
from tests import hints_oracle as H
from tests.conftest import GOLDEN

M64 = (1 << 64) - 1
FILL64 = 0xA5A5A5A5A5A5A5A5
NAMES = ("sg_comps_pairs", "sg_comps_pairs_dev", "sg_hints_from_kcov", "sg_hints_from_kcov_dev")
PC = EC.PC0


def _u64(x):
    return np.ascontiguousarray(np.asarray(x, dtype=np.uint64).reshape(-1))


def _off(lens):
    return np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)


# ---- the reference's tables as raw records --------------------------------------
@functools.lru_cache(maxsize=None)
def _kat_seeds():
    """The 17 tables of hints_kats.json as hint seeds: (name, records, arg,
    res).  A CompMap entry key: {v...} becomes records (type 7, arg1 = v,
    arg2 = key, a random pc), each repeated 1 to 3 times, the list shuffled."""
    rng = np.random.default_rng(41)
    t = HC.load_kats()["tests"]
    seeds = []
    for name in ("TestHintsCheckConstArg", "TestHintsCheckDataArg", "TestHintsShrinkExpand"):
        for c in t[name]:
            recs = []
            for key, vs in c["comps"]:
                for v in vs:
                    for _ in range(int(rng.integers(1, 4))):
                        recs.append((7, int(v, 0), int(key, 0), PC + 4 * int(rng.integers(0, 1 << 12))))
            recs = [recs[i] for i in rng.permutation(len(recs))]
            if name == "TestHintsCheckDataArg":
                arg, res = bytes.fromhex(c["in"]), {bytes.fromhex(x) for x in c["res"]}
            else:
                arg, res = int(c["in"], 0), {int(x, 0) for x in c["res"]}
            seeds.append((name + ": " + c["name"], recs, arg, res))
    return seeds


def _slots(arg):
    """An argument's value slots (hints.go:95-118)."""
    if isinstance(arg, bytes):
        return [H.slice_to_uint64(arg[i:]) for i in range(min(len(arg), H.MAX_DATA_LENGTH))]
    return [arg]


def _results(arg, reps):
    """What checkConstArg / checkDataArg make of the slots' replacers."""
    if not isinstance(arg, bytes):
        return set(reps[0])
    res = set()
    for i, slot in enumerate(reps):
        k = min(8, len(arg) - i)
        for rep in slot:
            res.add(arg[:i] + rep.to_bytes(8, "little")[:k] + arg[i + k:])
    return res


# ---- CPU ------------------------------------------------------------------------
def test_kats_through_raw_records():
    seeds = _kat_seeds()
    assert len(seeds) == 3 + 5 + 9
    recs, off = EC.to_arrays([s[1] for s in seeds])
    slots = [_slots(s[2]) for s in seeds]
    voff = _off([len(x) for x in slots])
    status, _, reps = O.batch(recs, off, [v for x in slots for v in x], voff)
    assert status == [O.OK] * len(seeds)
    for c, (name, _, arg, res) in enumerate(seeds):
        assert _results(arg, reps[int(voff[c]):int(voff[c + 1])]) == res, name


def test_pair_rule_edges():
    # operands equal only after the extension stay distinct triples and yield nothing
    t, _ = X.call_comps([(0, 0x180, 0x80, PC), (0, 0x80, 0x180, PC), (0, 0x80, 0x7F, PC)])
    assert len(t) == 3
    st, pairs = O.pairs_of(t)
    assert st == O.OK and pairs == [(0x7F, M64 - 0x7F), (M64 - 0x7F, 0x7F)]
    assert t[0] == (0, M64 - 0x7F, 0x7F)  # sorted raw: (0x80, 0x7f) first
    assert O.pairs_of(t[1:]) == (O.OK, []) and O.pairs_of(t[:1]) == (O.OK, pairs)
    # the extension is applied to any triples: raw ones give the same
    assert O.pairs_of([(0, 0x80, 0x7F)]) == (O.OK, pairs)
    # a const comparison yields one pair, (op2, op1)
    assert O.pairs_of([(1, 5, 6)]) == (O.OK, [(6, 5)])
    assert O.pairs_of([(6, 5, 6)]) == (O.OK, [(6, 5), (5, 6)])
    # a type above 7 anywhere: the reader returns before it assigns Comps
    for bad in (8, (1 << 32) + 1):
        for where in (0, 1, 2):
            trip = [(6, 5, 6), (2, 1, 2)]
            trip.insert(where, (bad, 3, 4))
            assert O.pairs_of(trip) == (O.COMPS_TYPE, [])
    status, lists, reps = O.batch(*EC.to_arrays([[(6, 5, 6, PC)], [(8, 5, 6, PC)], [((1 << 32) + 1, 5, 6, PC)]]),
                                  [5, 5, 5], [0, 1, 2, 3])
    assert status == [O.OK, O.COMPS_TYPE, O.COMPS_TYPE] and lists == [[(6, 5), (5, 6)], [], []]
    assert reps == [[6], [], []]


def test_boundary():
    from syzkaller_amd import _lib
    from tests.test_abi import declared

    names = declared()
    for n in NAMES:
        assert n in names and n in _lib.SIGNATURES, n
        getattr(ctypes.CDLL(_lib.LIB_PATH), n)
    lib, E = _lib.lib, _lib.SG_EINVAL
    one = np.zeros(4, np.uint64)
    p = one.ctypes.data_as(_lib.P64)
    st = np.zeros(1, np.int32).ctypes.data_as(ctypes.POINTER(ctypes.c_int32))
    assert lib.sg_comps_pairs(None, p, p, 1, st, p, p, 1) == E
    assert lib.sg_comps_pairs_dev(None, p, p, 1, 0, st, p, p, 1) == E
    assert lib.sg_hints_from_kcov(None, p, p, 1, p, p, st, p, p, 1) == E
    assert lib.sg_hints_from_kcov_dev(None, p, p, 1, 0, p, p, 0, st, p, p, 1) == E


# ---- GPU ------------------------------------------------------------------------
def _to_dev(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64).copy()).to("cuda")


def _filled(n, value=FILL64):
    return _to_dev(np.full(max(n, 1), value, np.uint64))


def _dev_pairs(ctx, comp_off, comps, cap=None):
    """sg_comps_pairs_dev through torch buffers; outputs prefilled."""
    import torch

    from syzkaller_amd._lib import call

    co, c = _u64(comp_off), _u64(comps)
    ncalls, ncomps = co.size - 1, int(co[-1])
    cap = 2 * ncomps if cap is None else cap
    t_co, t_c = _to_dev(co), _to_dev(c)
    status = torch.full((max(ncalls, 1),), -1, dtype=torch.int32, device="cuda")
    po, pairs = _filled(ncalls + 1, M64), _filled(2 * max(cap, 1))
    torch.cuda.synchronize()
    call("sg_comps_pairs_dev", ctx.h, t_co.data_ptr(), t_c.data_ptr(), ncalls, ncomps, status.data_ptr(), po.data_ptr(),
         pairs.data_ptr(), cap)
    ctx.sync()
    return (status.cpu().numpy()[:ncalls], pairs.cpu().numpy().view(np.uint64).reshape(-1, 2),
            po.cpu().numpy().view(np.uint64))


def _dev_fused(ctx, recs, off, vals, voff, cap=None):
    """sg_hints_from_kcov_dev through torch buffers; outputs prefilled."""
    import torch

    from syzkaller_amd._lib import call

    r, co, v, vo = _u64(recs), _u64(off), _u64(vals), _u64(voff)
    ncalls, nrecs, nvals = co.size - 1, int(co[-1]), v.size
    cap = max(1024, 8 * nvals) if cap is None else cap
    t_r, t_co, t_v, t_vo = _to_dev(r), _to_dev(co), _to_dev(v), _to_dev(vo)
    status = torch.full((max(ncalls, 1),), -1, dtype=torch.int32, device="cuda")
    ro, reps = _filled(nvals + 1, M64), _filled(cap)
    torch.cuda.synchronize()
    call("sg_hints_from_kcov_dev", ctx.h, t_r.data_ptr(), t_co.data_ptr(), ncalls, nrecs, t_vo.data_ptr(), t_v.data_ptr(),
         nvals, status.data_ptr(), ro.data_ptr(), reps.data_ptr(), cap)
    ctx.sync()
    return status.cpu().numpy()[:ncalls], reps.cpu().numpy().view(np.uint64), ro.cpu().numpy().view(np.uint64)


def _expect(recs, off, vals, voff):
    status, lists, reps = O.batch(recs, off, vals, voff)
    return np.array(status, np.int32), O.pairs_arrays(lists), O.reps_arrays(reps)


def _check(ctx, ctx_option, recs, off, vals, voff, general_auto=None, paths=(-1, 0), triples=None):
    """The fused call (host and device form), the three-call chain, and
    sg_comps_pairs (host and device form) fed `triples` (the oracle's unless
    given), all equal to the oracle.  general_auto: the calls the auto path
    must send down the general path.  Returns the oracle's result."""
    from syzkaller_amd import hints as G

    recs, off, vals, voff = _u64(recs).reshape(-1, 4), _u64(off), _u64(vals), _u64(voff)
    ncalls, nrecs = off.size - 1, int(off[-1])
    e_st, (e_pairs, e_po), (e_reps, e_ro) = exp = _expect(recs, off, vals, voff)
    e_co, e_comps = triples if triples is not None else X.batch(recs, off)[:2]
    nr = int(e_ro[-1])

    def same_reps(got):
        st, reps, ro = got
        assert np.array_equal(st, e_st) and st.dtype == np.int32
        assert np.array_equal(ro, e_ro) and np.array_equal(reps[:nr], e_reps)

    for path in paths:
        ctx_option(ctx, "exec_comps_path", path)
        general = None if general_auto is None else (general_auto if path < 0 else (ncalls if nrecs else 0))
        # 1. the fused call
        same_reps(G.hints_from_kcov(recs, off, vals, voff, ctx=ctx))
        cands = ctx.counter("hints_candidates")
        assert general is None or ctx.counter("exec_comps_general") == general, path
        st, reps, ro = _dev_fused(ctx, recs, off, vals, voff, cap=nr + 7)
        same_reps((st, reps, ro))
        assert (reps[nr:] == FILL64).all()
        assert ctx.counter("hints_candidates") == cands
        assert general is None or ctx.counter("exec_comps_general") == general, path
        # 2. the three calls
        co, comps, _, _ = G.exec_comps(recs, off, ctx=ctx, words=False)
        assert np.array_equal(co, e_co) and np.array_equal(comps, e_comps)
        st, pairs, po = G.comps_pairs(co, comps, ctx=ctx)
        assert np.array_equal(st, e_st) and np.array_equal(po, e_po) and np.array_equal(pairs, e_pairs)
        reps, ro = G.shrink_expand_batch(pairs, po, vals, voff, ctx=ctx)
        same_reps((st, reps, ro))
        assert ctx.counter("hints_candidates") == cands
    # 3. the pairs alone, from the given triples
    st, pairs, po = G.comps_pairs(e_co, e_comps, ctx=ctx)
    assert np.array_equal(st, e_st) and np.array_equal(po, e_po) and np.array_equal(pairs, e_pairs)
    st, pairs, po = _dev_pairs(ctx, e_co, e_comps)
    npairs = int(e_po[-1])
    assert np.array_equal(st, e_st) and np.array_equal(po, e_po) and np.array_equal(pairs[:npairs], e_pairs)
    assert (pairs[npairs:] == FILL64).all()
    return exp


def _vals_meeting(rng, call, n):
    """n values for a call: mostly second operands of its records, as write()
    leaves them (the keys of its (op2, op1) pairs), some of them inside a
    wider value (the shrink matches), some unrelated."""
    out = []
    for _ in range(n):
        if not call or rng.integers(0, 5) == 0:
            out.append(int(rng.integers(0, 1 << 64, dtype=np.uint64)))
            continue
        op2 = X.write(call[int(rng.integers(0, len(call)))])[2]
        out.append(op2 if rng.integers(0, 3) else (op2 & 0xFF) | 0x1200)
    return out


def _with_vals(rng, calls, slots):
    vals = [_vals_meeting(rng, c, n) for c, n in zip(calls, slots)]
    recs, off = EC.to_arrays(calls)
    return recs, off, [v for x in vals for v in x], _off([len(x) for x in vals])


@pytest.mark.gpu
def test_three_routes_on_the_golden_triples(ctx, ctx_option):
    """The recorded output of the reference's own operator<, operator== and
    write() into sg_comps_pairs; its records through the fused call."""
    with np.load(os.path.join(GOLDEN, "exec_comps_golden.npz"), allow_pickle=False) as z:
        g = {k: z[k] for k in z.files}
    rng = np.random.default_rng(42)
    rows = g["recs"].tolist()
    calls = [[tuple(r) for r in rows[int(a):int(b)]] for a, b in zip(g["call_off"][:-1], g["call_off"][1:])]
    recs, off, vals, voff = _with_vals(rng, calls, [int(n) for n in rng.integers(0, 9, size=len(calls))])
    assert np.array_equal(recs, g["recs"])
    e_st, _, (_, e_ro) = _check(ctx, ctx_option, recs, off, vals, voff, general_auto=0,
                                triples=(g["comp_off"], g["comps"]))
    assert O.COMPS_TYPE in e_st.tolist() and O.OK in e_st.tolist() and int(e_ro[-1]) > 0


@pytest.mark.gpu
def test_kats_end_to_end(ctx):
    from syzkaller_amd import hints as G

    seeds = _kat_seeds()
    for name, recs, arg, res in seeds:
        assert G.HintSeed([(np.array(recs, np.uint64).reshape(-1, 4), [arg])], ctx=ctx) == [[res]], name
    got = G.HintSeed([(np.array(recs, np.uint64).reshape(-1, 4), [arg]) for _, recs, arg, _ in seeds], ctx=ctx)
    assert got == [[res] for _, _, _, res in seeds]
    # several arguments of both kinds in one call; a call without arguments; an empty data argument
    _, recs, _, _ = seeds[1]  # 0xabcd: {2, 3}
    r = np.array(recs, np.uint64).reshape(-1, 4)
    got = G.HintSeed([(r, [0xabcd, b"\xcd\xab", 7, b""]), (r, []), (np.zeros((0, 4), np.uint64), [0xabcd])], ctx=ctx)
    assert got == [[{2, 3}, {b"\x02\x00", b"\x03\x00"}, set(), set()], [], [set()]]
    assert G.HintSeed([], ctx=ctx) == []


@functools.lru_cache(maxsize=None)
def _random_batch():
    rng = np.random.default_rng(43)
    p = HC.pool(rng)
    calls, vals, k = [], [], 0
    for n in rng.integers(0, 41, size=3000):
        call = [c + (PC + 4 * int(rng.integers(0, 1 << 12)),) for c in HC.comparisons(rng, p, int(n))]
        if call:
            k += 1
            if k % 97 == 0:
                call[0] = (int(rng.integers(8, 17)),) + call[0][1:]
        calls.append(call)
        vals.append([p[int(rng.integers(0, len(p)))] for _ in range(int(rng.integers(0, 13)))])
    recs, off = EC.to_arrays(calls)
    return recs, off, _u64([v for x in vals for v in x]), _off([len(x) for x in vals])


@pytest.mark.gpu
def test_random_batch(ctx, ctx_option):
    recs, off, vals, voff = _random_batch()
    e_st, (_, e_po), (_, e_ro) = _check(ctx, ctx_option, recs, off, vals, voff, general_auto=0)
    # the case is not vacuous
    with_reps = int((np.diff(e_ro.astype(np.int64)) > 0).sum())
    assert 10 * with_reps >= vals.size > 0
    assert (e_st == O.COMPS_TYPE).sum() >= 1 and (e_st == O.OK).sum() >= 2900
    bad = np.flatnonzero(e_st == O.COMPS_TYPE)
    assert (e_po[bad] == e_po[bad + 1]).all()


@pytest.mark.gpu
def test_shape_edges_inside_the_fused_call(ctx, ctx_option):
    from syzkaller_amd import hints as G

    rng = np.random.default_rng(44)
    p = EC.pool(rng, 40)
    # either side of exec_comps' three workgroup shapes and of the 64 triples of a wave step
    calls = [EC.draw(rng, p, n) for n in (0, 1, 63, 64, 65, 256, 257, 2047, 2048, 2049)]
    calls.append(EC.draw(rng, EC.pool(rng, 500), 16383))           # a full buffer over 500 triples
    calls.append(EC.distinct(rng, G.EXEC_COMPS_FAST_CAP + 1))      # leaves the fast shape
    # either side of the join's two workgroup shapes and of its tile
    slots = [5, 0, 63, 64, 65, 513, 0, 64, 65, 3, 513, 63]
    recs, off, vals, voff = _with_vals(rng, calls, slots)
    _, (_, e_po), (_, e_ro) = _check(ctx, ctx_option, recs, off, vals, voff, general_auto=1)
    assert int(e_ro[-1]) > 0 and np.diff(e_po.astype(np.int64)).max() > 2 * 64
    # each length alone, with a few values
    for call in calls[:10]:
        _check(ctx, ctx_option, *_with_vals(rng, [call], [4]), general_auto=0)
    # no calls; calls but no values; values but no records
    _check(ctx, ctx_option, np.zeros((0, 4), np.uint64), [0], [], [0], general_auto=0)
    recs, off = EC.to_arrays(calls[:6])
    _check(ctx, ctx_option, recs, off, [], [0] * 7, general_auto=0)
    _check(ctx, ctx_option, np.zeros((0, 4), np.uint64), [0, 0, 0], [1, 2, 3], [0, 1, 3], general_auto=0)
    # every comparison has equal operands (some only once extended): no pairs, no replacers
    eq = [[(int(t), x, x, PC) for t, x in zip(rng.integers(0, 8, size=n), rng.integers(0, 1 << 62, size=n))]
          for n in (3, 70, 300)]
    eq.append([(0, 0x180, 0x80, PC), (2, 0x18000, 0x8000, PC), (4, 0x100000005, 5, PC)])
    recs, off = EC.to_arrays(eq)
    vals = [c[i % len(c)][1] for c in eq for i in range(6)]
    _, (_, e_po), (_, e_ro) = _check(ctx, ctx_option, recs, off, vals, _off([6] * len(eq)), general_auto=0)
    assert int(e_po[-1]) == 0 and not e_ro.any()


@pytest.mark.gpu
def test_semantics(ctx, ctx_option):
    from syzkaller_amd import hints as G

    def seed(*calls):
        return G.HintSeed([(np.array(r, np.uint64).reshape(-1, 4), args) for r, args in calls], ctx=ctx)

    # the shrink-to-8 match against the sign-extended operand
    assert seed(([(0, 0x80, 0x7E, PC)], [0x1280])) == [[{0x127E}]]
    # a const comparison keeps (op2, op1) alone
    assert seed(([(1, 0x7E, 0x80, PC)], [0x1280])) == [[{0x127E}]]
    assert seed(([(1, 0x80, 0x7E, PC)], [0x1280])) == [[set()]]
    # a bad-typed call between two good ones
    good = [(0, 0x80, 0x7E, PC), (6, 0xdeadbeef, 0xcafebabe, PC)]
    alone = seed((good, [0x1280, 0xcafebabe]))
    assert alone == [[{0x127E}, {0xdeadbeef}]]
    for bad in (8, (1 << 32) + 1, M64):
        got = seed((good, [0x1280, 0xcafebabe]), (good + [(bad, 1, 2, PC)], [0x1280, 0xcafebabe]),
                   (good, [0x1280, 0xcafebabe]))
        assert got == [alone[0], [set(), set()], alone[0]]
    recs, off = EC.to_arrays([good, [(9, 1, 2, PC)] + good, good])
    e_st, _, _ = _check(ctx, ctx_option, recs, off, [0x1280] * 3, [0, 1, 2, 3], general_auto=0)
    assert e_st.tolist() == [O.OK, O.COMPS_TYPE, O.OK]
    # operands that differ only above the width: two triples, one distinct pair set
    recs, off = EC.to_arrays([[(4, 0x100000005, 1, PC), (4, 0x5, 1, PC)]])
    _, (e_pairs, e_po), (e_reps, _) = _check(ctx, ctx_option, recs, off, [1], [0, 1], general_auto=0)
    assert int(e_po[-1]) == 4 and {tuple(x) for x in e_pairs.tolist()} == {(1, 5), (5, 1)} and e_reps.tolist() == [5]


@pytest.mark.gpu
def test_conventions(ctx):
    import torch

    from syzkaller_amd import _lib
    from syzkaller_amd import hints as G
    from syzkaller_amd.cover import _p64

    lib, h, E = _lib.lib, ctx.h, _lib.SG_EINVAL
    rng = np.random.default_rng(45)
    p = EC.pool(rng, 40)
    calls = [EC.draw(rng, p, 70), [], [(8, 1, 2, PC)], EC.draw(rng, p, 300)]
    recs, off, vals, voff = _with_vals(rng, calls, [9, 2, 3, 70])
    recs, vals = _u64(recs), _u64(vals)
    e_st, (e_pairs, e_po), (e_reps, e_ro) = _expect(recs, off, vals, voff)
    e_co, e_comps = X.batch(recs, off)[:2]
    e_comps = _u64(e_comps)
    ncalls, npairs, nr = off.size - 1, int(e_po[-1]), int(e_ro[-1])
    assert npairs > 1 and nr > 1

    def pi32(a):
        return a.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))

    # -- sg_comps_pairs: cap one short, then exact; pairs == NULL with cap == 0
    st, po = np.full(ncalls, -1, np.int32), np.zeros(ncalls + 1, np.uint64)
    pairs = np.full((npairs, 2), FILL64, np.uint64)
    a = (_p64(e_co), _p64(e_comps), ncalls, pi32(st), _p64(po), _p64(pairs), npairs)
    assert lib.sg_comps_pairs(h, *a[:6], npairs - 1) == 0
    assert np.array_equal(po, e_po) and np.array_equal(st, e_st) and (pairs == FILL64).all()
    assert lib.sg_comps_pairs(h, *a) == 0 and np.array_equal(pairs, e_pairs)
    po[:] = 0
    assert lib.sg_comps_pairs(h, *a[:5], None, 0) == 0 and np.array_equal(po, e_po)
    d_st, d_pairs, d_po = _dev_pairs(ctx, e_co, e_comps, cap=npairs - 1)
    assert np.array_equal(d_po, e_po) and np.array_equal(d_st, e_st) and (d_pairs == FILL64).all()

    def but(args, i, v):
        return args[:i] + (v,) + args[i + 1:]

    assert lib.sg_comps_pairs(None, *a) == E
    for i in (0, 1, 3, 4, 5):
        assert lib.sg_comps_pairs(h, *but(a, i, None)) == E, i
    bad = e_co.copy()
    bad[0] = 1
    assert lib.sg_comps_pairs(h, *but(a, 0, _p64(bad))) == E
    bad = e_co.copy()
    bad[1], bad[2] = bad[2] + 1, bad[1]
    assert lib.sg_comps_pairs(h, *but(a, 0, _p64(bad))) == E
    big = np.array([0, 1 << 31], np.uint64)
    assert lib.sg_comps_pairs(h, _p64(big), _p64(e_comps), 1, pi32(st), _p64(po), _p64(pairs), npairs) == E
    assert lib.sg_comps_pairs(h, _p64(e_co), _p64(e_comps), 1 << 31, pi32(st), _p64(po), _p64(pairs), npairs) == E
    t = torch.zeros(64, dtype=torch.int64, device="cuda")
    q = t.data_ptr()
    dev = lib.sg_comps_pairs_dev
    assert dev(h, q, q, 1, 0, q, q, None, 0) == 0  # the offsets alone
    assert dev(None, q, q, 1, 1, q, q, q, 2) == E
    assert dev(h, None, q, 1, 1, q, q, q, 2) == E
    assert dev(h, q, None, 1, 1, q, q, q, 2) == E
    assert dev(h, q, q, 1, 1, None, q, q, 2) == E
    assert dev(h, q, q, 1, 1, q, None, q, 2) == E
    assert dev(h, q, q, 1, 1, q, q, None, 2) == E
    assert dev(h, q, q, 1, 1 << 31, q, q, q, 2) == E
    assert dev(h, q, q, 1 << 31, 1, q, q, q, 2) == E
    ctx.sync()

    # -- sg_hints_from_kcov: cap one short, then exact; the wrapper's second call; reps == NULL with cap == 0
    st, ro = np.full(ncalls, -1, np.int32), np.zeros(vals.size + 1, np.uint64)
    reps = np.full(nr, FILL64, np.uint64)
    a = (_p64(recs), _p64(off), ncalls, _p64(voff), _p64(vals), pi32(st), _p64(ro), _p64(reps), nr)
    assert lib.sg_hints_from_kcov(h, *a[:8], nr - 1) == 0
    assert np.array_equal(ro, e_ro) and np.array_equal(st, e_st) and (reps == FILL64).all()
    assert lib.sg_hints_from_kcov(h, *a) == 0 and np.array_equal(reps, e_reps)
    ro[:] = 0
    assert lib.sg_hints_from_kcov(h, *a[:7], None, 0) == 0 and np.array_equal(ro, e_ro)
    d_st, d_reps, d_ro = _dev_fused(ctx, recs, off, vals, voff, cap=nr - 1)
    assert np.array_equal(d_ro, e_ro) and np.array_equal(d_st, e_st) and (d_reps == FILL64).all()
    g_st, g_reps, g_ro = G.hints_from_kcov(recs, off, vals, voff, ctx=ctx, cap=1)
    assert np.array_equal(g_st, e_st) and np.array_equal(g_reps, e_reps) and np.array_equal(g_ro, e_ro)
    assert lib.sg_hints_from_kcov(None, *a) == E
    for i in (0, 1, 3, 4, 5, 6, 7):
        assert lib.sg_hints_from_kcov(h, *but(a, i, None)) == E, i
    for i, o in ((1, off), (3, voff)):
        bad = o.copy()
        bad[0] = 1
        assert lib.sg_hints_from_kcov(h, *but(a, i, _p64(bad))) == E
        bad = o.copy()
        bad[1], bad[2] = bad[2] + 1, bad[1]
        assert lib.sg_hints_from_kcov(h, *but(a, i, _p64(bad))) == E
    big = np.array([0, 1 << 31], np.uint64)
    assert lib.sg_hints_from_kcov(h, _p64(recs), _p64(big), 1, _p64(voff), _p64(vals), pi32(st), _p64(ro), _p64(reps),
                                  nr) == E
    big = np.array([0, 1 << 32], np.uint64)
    assert lib.sg_hints_from_kcov(h, _p64(recs), _p64(off), 1, _p64(big), _p64(vals), pi32(st), _p64(ro), _p64(reps),
                                  nr) == E
    assert lib.sg_hints_from_kcov(h, *but(a, 2, 1 << 31)) == E
    dev = lib.sg_hints_from_kcov_dev
    ok = (q, q, 1, 1, q, q, 1, q, q, q, 4)
    assert dev(None, *ok) == E
    for i in (0, 1, 4, 5, 7, 8, 9):
        assert dev(h, *but(ok, i, None)) == E, i
    assert dev(h, *but(ok, 3, 1 << 31)) == E   # records
    assert dev(h, *but(ok, 2, 1 << 31)) == E   # calls
    assert dev(h, *but(ok, 6, 1 << 32)) == E   # value slots
    ctx.sync()
