"""Comparison hints: the executor's comparisons into CompMaps
(pkg/ipc/ipc_linux.go:257-304) and shrinkExpand / checkConstArg / checkDataArg
(prog/hints.go:95-177).  On the CPU the test oracle (tests/hints_oracle.py)
against the reference's own tables and against ipc_oracle's statuses; on the
GPU sg_ipc_comps and sg_hints_replacers exact against that oracle."""
import ctypes
import functools

import numpy as np
import pytest

from oracle import ipc_oracle as I
from tests import hints_cases as HC
from tests import hints_oracle as H
from tests import ipc_cases as K

M64 = (1 << 64) - 1


@functools.lru_cache(maxsize=None)
def _kats():
    return HC.load_kats()


def _cmap(comps):
    return {int(k, 0): {int(v, 0) for v in vs} for k, vs in comps}


def _const_cases():
    t = _kats()["tests"]
    return [(name, c) for name in ("TestHintsCheckConstArg", "TestHintsShrinkExpand") for c in t[name]]


# ---- CPU: the oracle itself --------------------------------------------------
def test_golden_holds_every_reference_table():
    k = _kats()
    assert [len(k["tests"][n]) for n in ("TestHintsCheckConstArg", "TestHintsCheckDataArg", "TestHintsShrinkExpand")] \
        == [3, 5, 9]
    assert [int(x, 0) for x in k["special_ints"]] == H.SPECIAL_INTS and len(H.SPECIAL_INTS) == 33


def test_oracle_reproduces_the_kats():
    for name, c in _const_cases():
        fn = H.check_const_arg if name == "TestHintsCheckConstArg" else H.shrink_expand
        assert fn(int(c["in"], 0), _cmap(c["comps"])) == {int(x, 0) for x in c["res"]}, c["name"]
    for c in _kats()["tests"]["TestHintsCheckDataArg"]:
        got = H.check_data_arg(bytes.fromhex(c["in"]), _cmap(c["comps"]))
        assert got == {bytes.fromhex(x) for x in c["res"]}, c["name"]


def test_oracle_statuses_equal_the_ipc_oracle():
    out, oo, co, nums = K.batch(3, nprog=240, kinds=K.FAULTS)
    for cn in (nums, None):
        status, _ = H.comps_batch(out, oo, co, cn)
        assert status == I.parse_batch(out, oo, co, cn)[2]
    assert set(status) >= {I.COMPS_SHORT, I.COMPS_TYPE, I.OK}


def test_oracle_reader_order_and_widths():
    # type 6: two words; type 0: four words, both directions; type 1: const, one direction; equal operands: nothing
    comps = [(6, 5, 9), (0, (7 << 32) | 1, 3), (1, 10, 11), (4, 8, 8)]
    st, got = H.read_comps([1] + I.write_call(0, 0, 0, 0, [1], [2], comps, "reader"), 1)
    assert st == I.OK
    assert got[0] == [(9, 5), (5, 9), (3, (7 << 32) | 1), ((7 << 32) | 1, 3), (11, 10)]


# ---- GPU ---------------------------------------------------------------------
def _check_comps(out, oo, co, nums, against_parse=True):
    from syzkaller_amd import cover as C
    from syzkaller_amd import hints as G

    status, pairs, po = G.ipc_comps(out, oo, co, nums)
    e_status, e_lists = H.comps_batch(out, oo, co, nums)
    assert status.tolist() == e_status
    assert np.diff(po.astype(np.int64)).tolist() == [len(x) for x in e_lists]
    assert pairs.tolist() == [list(kv) for x in e_lists for kv in x]
    if against_parse:  # the wave walk against the one-thread walk
        assert status.tolist() == C.ipc_parse(out, oo, co, nums, cover=False)[2].tolist()
    return e_status, e_lists


@pytest.mark.gpu
@pytest.mark.parametrize("seed", [1, 2, 3])
def test_ipc_comps_vs_oracle(ctx, seed):
    out, oo, co, nums = K.batch(seed, 300)
    _check_comps(out, oo, co, nums)


@pytest.mark.gpu
def test_ipc_comps_every_error_path(ctx):
    out, oo, co, nums = K.batch(7, nprog=240, kinds=K.FAULTS)
    st, _ = _check_comps(out, oo, co, nums)
    assert set(st) == set(range(10))
    _check_comps(out, oo, co, None)


NCALLS = 12


def _region_program(rng, p, n, types, tail=True, damage=None, lead=0):
    """One program of NCALLS calls: call 3 with 3 + lead signal words, cover
    and n comparisons, then (tail) call 11 whose header words are all above 7.
    damage = (kind, j) plants an error at comparison j."""
    comps = HC.comparisons(rng, p, n, types)
    # operand words in 0..7 and above 7; equal operands; const and non-const
    for j in range(0, n, 7):
        comps[j] = (comps[j][0], int(rng.integers(0, 8)), int(rng.integers(0, 8)) | (int(rng.integers(0, 8)) << 32))
    w = I.write_call(3, 103, 0, 0, [11, 12, 13] + [14] * lead, [0x81000010, 0x81000020], comps, "reader")
    starts, pos = [], 7 + 3 + lead + 2
    for typ, _, _ in comps:
        starts.append(pos)
        pos += 1 + (2 if (typ & 6) == 6 else 4)
    ncmd = 1
    if damage:
        kind, j = damage
        if kind == "type":
            w[starts[j]] = 8 + int(rng.integers(0, 1000))
        elif kind == "cut_type":  # the region ends right after a type word
            w, tail = w[: starts[j] + 1], False
        elif kind == "cut_operand":
            w, tail = w[: starts[j] + 2], False
        elif kind == "one_more":  # ncomps one more than is present
            w[6] = n + 1
    if tail:
        w += I.write_call(11, 111, 14, 9, list(range(100, 109)), list(range(200, 209)),
                          HC.comparisons(rng, p, 9, types), "reader")
        ncmd = 2
    return [ncmd] + w, NCALLS, np.arange(100, 100 + NCALLS, dtype=np.uint32)


@functools.lru_cache(maxsize=None)
def _edge_batches():
    rng = np.random.default_rng(5)
    p = HC.pool(rng)
    three, five, alt = [6, 7], [0, 1, 2, 3, 4, 5], [6, 0, 7, 1, 2, 6]
    programs = []
    for ni, n in enumerate((0, 1, 63, 64, 65, 255, 256, 257, 5000)):
        for ti, types in enumerate((three, five, alt, None)):
            # the region starts 0..3 words later from one program to the next: with the
            # widths this puts type words at every offset of a lane's 4 words and of a step
            programs.append(_region_program(rng, p, n, types, lead=(ni + ti) % 4))
    faults = []
    n = 130
    for types in (alt, three, five):
        for j in (0, 1, 63, 64, 65, n - 1):
            faults.append(_region_program(rng, p, n, types, damage=("type", j), lead=j % 4))
            faults.append(_region_program(rng, p, n, types, damage=("cut_type", j), lead=(j + 1) % 4))
            faults.append(_region_program(rng, p, n, types, damage=("cut_operand", j), lead=(j + 2) % 4))
        faults.append(_region_program(rng, p, n, types, tail=False, damage=("one_more", 0)))
        faults.append(_region_program(rng, p, n, types, tail=True, damage=("one_more", 0)))
    return HC.assemble(programs), HC.assemble(faults)


@pytest.mark.gpu
def test_ipc_comps_region_edges(ctx):
    good, bad = _edge_batches()
    st, lists = _check_comps(*good)
    assert st == [I.OK] * len(st)
    assert max(len(x) for x in lists) > 5000  # the long record, both directions
    st, lists = _check_comps(*bad)
    assert {I.COMPS_TYPE, I.COMPS_SHORT} <= set(st) and I.OK not in set(st)
    assert all(len(x) == 0 for x in lists)
    # an empty batch; programs with no calls (an empty region, and ncmd = 0)
    z = np.zeros(1, np.uint64)
    _check_comps(np.zeros(0, np.uint32), z, z, None)
    _check_comps(np.array([0], np.uint32), np.array([0, 0, 1, 1], np.uint64), np.zeros(4, np.uint64), None)


@pytest.mark.gpu
def test_kats_on_the_gpu(ctx):
    from syzkaller_amd import hints as G

    for name, c in _const_cases():
        fn = G.CheckConstArg if name == "TestHintsCheckConstArg" else G.ShrinkExpand
        assert fn(int(c["in"], 0), _cmap(c["comps"])) == {int(x, 0) for x in c["res"]}, c["name"]
    for c in _kats()["tests"]["TestHintsCheckDataArg"]:
        got = G.CheckDataArg(bytes.fromhex(c["in"]), _cmap(c["comps"]))
        assert got == {bytes.fromhex(x) for x in c["res"]}, c["name"]
    # the special ints (prog/rand.go:59-67) are never the replaced bits
    special = {0xabcd: set(H.SPECIAL_INTS) | {0x2}}
    assert G.ShrinkExpand(0xabcd, special) == H.shrink_expand(0xabcd, special) == {0x2}
    # ... and their neighbours are: 2^k - 1, 2^k, 2^k + 1 and the values next to them, for every k
    near = {(1 << k) + d for k in range(64) for d in range(-3, 4) if 0 <= (1 << k) + d <= M64} - {0xabcd}
    kept = near - set(H.SPECIAL_INTS)
    assert G.ShrinkExpand(0xabcd, {0xabcd: near}) == H.shrink_expand(0xabcd, {0xabcd: near}) == kept
    assert G.comp_maps([[1, 2], [1, 3], [4, 1]], [0, 2, 2, 3]) == [{1: {2, 3}}, {}, {4: {1}}]


def _check_reps(pair_lists, vals, val_off):
    """shrink_expand_batch against the oracle; returns (replacers, matches,
    largest slot), the oracle's figures for the case."""
    from syzkaller_amd import hints as G

    pairs, po = HC.pairs_csr(pair_lists)
    reps, ro = G.shrink_expand_batch(pairs, po, vals, val_off)
    e_reps, matches = HC.expected_replacers(pair_lists, vals, val_off)
    assert np.diff(ro.astype(np.int64)).tolist() == [len(x) for x in e_reps]
    assert reps.tolist() == [x for s in e_reps for x in s]
    return sum(len(x) for x in e_reps), matches, max([len(x) for x in e_reps] + [0])


@functools.lru_cache(maxsize=None)
def _pool_batch(seed):
    out, oo, co, nums, vals, vo = HC.batch(seed)
    status, lists = H.comps_batch(out, oo, co, nums)
    assert status == [I.OK] * len(status)
    return (out, oo, co, nums, vals, vo), lists


@pytest.mark.gpu
@pytest.mark.parametrize("seed", [1, 2, 3])
def test_shrink_expand_batch_vs_oracle(ctx, seed):
    (_, _, _, _, vals, vo), lists = _pool_batch(seed)
    nreps, matches, largest = _check_reps(lists, vals, vo)
    # the case is not trivial: replacers exist, deduplication is exercised, a slot holds several
    assert nreps > 0 and matches > nreps and largest >= 2
    nv = np.diff(vo.astype(np.int64))
    np_ = np.array([len(x) for x in lists])
    assert ((nv == 0) & (np_ > 0)).any() and ((nv > 0) & (np_ == 0)).any()  # records with no values / no pairs


@pytest.mark.gpu
def test_shrink_expand_batch_shapes(ctx):
    rng = np.random.default_rng(9)
    p = HC.pool(rng)
    # 1,300 slots, half of them equal: several tiles, long runs of equal keys
    added = [(p[int(rng.integers(0, len(p)))], p[int(rng.integers(0, len(p)))]) for _ in range(4000)]
    vals = [0x1234567890abcdef] * 650 + [p[int(rng.integers(0, len(p)))] for _ in range(650)]
    vals = [vals[i] for i in rng.permutation(1300)]
    nreps, matches, largest = _check_reps([added], np.array(vals, np.uint64), np.array([0, 1300], np.uint64))
    assert nreps > 0 and matches > nreps and largest >= 2
    # records of 63, 64, 65 and 513 slots: either side of the join's two workgroup shapes and of a tile
    sizes = [63, 64, 65, 513]
    lists = [[(p[int(rng.integers(0, len(p)))], p[int(rng.integers(0, len(p)))]) for _ in range(300)] for _ in sizes]
    vals = np.array([p[int(rng.integers(0, len(p)))] for _ in range(sum(sizes))], np.uint64)
    nreps, _, _ = _check_reps(lists, vals, np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint64))
    assert nreps > 0
    # one slot against 3,000 distinct (0, x) pairs, next to an untouched record
    xs = sorted({int(x) for x in rng.integers(1, 1 << 64, size=3000, dtype=np.uint64)} | {1, 31, 4096, 1 << 32})
    added = [(0, x) for x in xs] + [(0, xs[5])] * 3
    nreps, matches, largest = _check_reps([[], added, [(1, 2)]], np.array([7, 0, 5], np.uint64),
                                          np.array([0, 1, 2, 3], np.uint64))
    assert largest == len(xs) - 4 == nreps and largest >= 2990
    # v = all ones: the mutants 0xff, 0xffff, 0xffffffff and v itself (the sign extensions coincide with it)
    added = [(M64, M64 - 1), (M64, 0xfffffffffffffeff), (0xFF, 0xfe), (0xFFFF, 0x1234), (0xFFFFFFFF, 0x12345678),
             (0xFF, 0x1234), (M64, 5), (M64, 1)]
    nreps, _, _ = _check_reps([added], np.array([M64], np.uint64), np.array([0, 1], np.uint64))
    assert nreps >= 5
    # two sizes give the same replacer; and a sign-extended operand gives v back
    added = [(0x34, 0xab), (0x1234, 0x12ab), (0x34, M64 - 0xcb)]
    nreps, matches, _ = _check_reps([added], np.array([0x1234], np.uint64), np.array([0, 1], np.uint64))
    assert (nreps, matches) == (2, 3)
    # no records; records but no values; values but no pairs anywhere
    e = np.zeros(1, np.uint64)
    _check_reps([], np.zeros(0, np.uint64), e)
    _check_reps([[(1, 2)], []], np.zeros(0, np.uint64), np.zeros(3, np.uint64))
    _check_reps([[], []], np.array([1, 2, 3], np.uint64), np.array([0, 1, 3], np.uint64))


@pytest.mark.gpu
def test_workspace_growth_between_count_and_sort(ctx):  # (ctx: the session's context exists before any other, as for every GPU test here)
    """Three calls on one fresh context: a small batch (the workspace takes its
    first 64 MiB); one whose count pass fits in those and whose candidates do
    not; the small batch again.  The second call's counts are in the workspace
    when it grows and drops its contents: the call has to count again.

    The bytes, from hints_replacers() (regions rounded up to 256 B).  Count
    pass: one record, 2,304 B.  Then per candidate cslot (4 B), crep, ka, kb
    (3 x 8 B), flags (4 B), pos (8 B), U (8 B) and, for the host form with a
    capacity of at least the candidates, its replacer (8 B) = 56 B; 4 B per
    value slot; the sort's 256 counters of 12 B per tile of 8,192 keys; the
    scans.  One record of 2,048 pairs (v, x_j), x_j distinct, and value slots
    all holding v: every pair matches every slot at the full width alone, 2,048
    candidates per slot.
      581 slots, 1,189,888 candidates: 67,097,344 B  (fits 67,108,864)
      582 slots, 1,191,936 candidates: 67,212,032 B  (does not)
    The expected lists are the oracle's for one slot, once per slot:
    HC.expected_replacers gives slot i H.shrink_expand(vals[i], the record's
    CompMap), which reads no other slot."""
    from syzkaller_amd import cover as C
    from syzkaller_amd import hints as G

    rng = np.random.default_rng(10)
    v, npairs, nslots = 0x1234567890abcdef, 2048, 582
    xs = sorted({int(x) for x in rng.integers(1 << 40, 1 << 64, size=npairs + 64, dtype=np.uint64)} - {v})[:npairs]
    added = [(v, xs[int(j)]) for j in rng.permutation(npairs)]
    (one,), matches = HC.expected_replacers([added], [v], [0, 1])
    assert len(one) == matches == npairs
    pairs, po = HC.pairs_csr([added])
    vals, vo = np.full(nslots, v, np.uint64), np.array([0, nslots], np.uint64)
    (_, _, _, _, s_vals, s_vo), s_lists = _pool_batch(1)
    s_pairs, s_po = HC.pairs_csr(s_lists)
    s_exp, _ = HC.expected_replacers(s_lists, s_vals, s_vo)
    c = C.Context()
    try:
        def small():
            reps, ro = G.shrink_expand_batch(s_pairs, s_po, s_vals, s_vo, ctx=c)
            assert np.diff(ro.astype(np.int64)).tolist() == [len(x) for x in s_exp]
            assert reps.tolist() == [x for s in s_exp for x in s]

        small()
        assert c.counter("workspace_bytes") == 64 << 20
        reps, ro = G.shrink_expand_batch(pairs, po, vals, vo, ctx=c, cap=nslots * npairs)
        assert np.array_equal(ro, np.arange(nslots + 1, dtype=np.uint64) * np.uint64(npairs))
        assert np.array_equal(reps.reshape(nslots, npairs), np.tile(np.array(one, np.uint64), (nslots, 1)))
        assert c.counter("hints_candidates") == nslots * npairs and c.counter("workspace_bytes") > 64 << 20
        small()
    finally:
        c.close()


@pytest.mark.gpu
def test_end_to_end_regions_to_replacers(ctx):
    from syzkaller_amd import hints as G

    (out, oo, co, nums, vals, vo), lists = _pool_batch(4)
    status, pairs, po = G.ipc_comps(out, oo, co, nums)
    assert (status == 0).all()
    reps, ro = G.shrink_expand_batch(pairs, po, vals, vo)
    e_reps, _ = HC.expected_replacers(lists, vals, vo)
    assert sum(len(x) for x in e_reps) > 0
    for i, e in enumerate(e_reps):  # per call and per value
        assert reps[int(ro[i]):int(ro[i + 1])].tolist() == e, i
    # the maps the Go side would build from the pairs
    assert G.comp_maps(pairs, po) == [H.comp_map(x) for x in lists]


@pytest.mark.gpu
def test_capacity_and_argument_checks(ctx):
    from syzkaller_amd import _lib
    from syzkaller_amd import hints as G
    from syzkaller_amd.cover import _p32, _p64

    (out, oo, co, nums, vals, vo), lists = _pool_batch(4)
    lib, h = _lib.lib, ctx.h
    nprog, nrec = oo.size - 1, int(co[-1])
    _, e_pairs, e_po = G.ipc_comps(out, oo, co, nums)
    total = int(e_po[-1])
    assert total > 1
    status = np.empty(nprog, np.int32)
    pst = status.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))
    po = np.zeros(nrec + 1, np.uint64)
    pairs = np.full((total, 2), 0xA5A5A5A5A5A5A5A5, np.uint64)
    # cap too small: the offsets are filled, the pairs untouched
    assert lib.sg_ipc_comps(h, _p32(out), _p64(oo), _p64(co), _p32(nums), nprog, pst, _p64(po), _p64(pairs),
                            total - 1) == 0
    assert np.array_equal(po, e_po) and (pairs == 0xA5A5A5A5A5A5A5A5).all()
    assert lib.sg_ipc_comps(h, _p32(out), _p64(oo), _p64(co), _p32(nums), nprog, pst, _p64(po), _p64(pairs), total) == 0
    assert np.array_equal(pairs, e_pairs)
    e_reps, e_ro = G.shrink_expand_batch(e_pairs, e_po, vals, vo)
    nr = int(e_ro[-1])
    assert nr > 1
    ro = np.zeros(vals.size + 1, np.uint64)
    reps = np.full(nr, 0xA5A5A5A5A5A5A5A5, np.uint64)
    flat = np.ascontiguousarray(e_pairs)
    assert lib.sg_hints_replacers(h, _p64(e_po), _p64(flat), nrec, _p64(vo), _p64(vals), _p64(ro), _p64(reps),
                                  nr - 1) == 0
    assert np.array_equal(ro, e_ro) and (reps == 0xA5A5A5A5A5A5A5A5).all()
    assert lib.sg_hints_replacers(h, _p64(e_po), _p64(flat), nrec, _p64(vo), _p64(vals), _p64(ro), _p64(reps), nr) == 0
    assert np.array_equal(reps, e_reps)
    # a NULL where a pointer is required
    E = _lib.SG_EINVAL
    assert lib.sg_ipc_comps(h, _p32(out), None, _p64(co), _p32(nums), nprog, pst, _p64(po), _p64(pairs), total) == E
    assert lib.sg_ipc_comps(h, _p32(out), _p64(oo), _p64(co), _p32(nums), nprog, pst, None, _p64(pairs), total) == E
    assert lib.sg_ipc_comps(h, _p32(out), _p64(oo), _p64(co), _p32(nums), nprog, None, _p64(po), _p64(pairs), total) == E
    assert lib.sg_ipc_comps(h, _p32(out), _p64(oo), _p64(co), _p32(nums), nprog, pst, _p64(po), None, total) == E
    assert lib.sg_ipc_comps(None, _p32(out), _p64(oo), _p64(co), _p32(nums), nprog, pst, _p64(po), _p64(pairs), total) == E
    assert lib.sg_hints_replacers(h, None, _p64(flat), nrec, _p64(vo), _p64(vals), _p64(ro), _p64(reps), nr) == E
    assert lib.sg_hints_replacers(h, _p64(e_po), None, nrec, _p64(vo), _p64(vals), _p64(ro), _p64(reps), nr) == E
    assert lib.sg_hints_replacers(h, _p64(e_po), _p64(flat), nrec, _p64(vo), None, _p64(ro), _p64(reps), nr) == E
    assert lib.sg_hints_replacers(h, _p64(e_po), _p64(flat), nrec, _p64(vo), _p64(vals), None, _p64(reps), nr) == E
    assert lib.sg_hints_replacers(h, _p64(e_po), _p64(flat), nrec, _p64(vo), _p64(vals), _p64(ro), None, nr) == E
    assert lib.sg_ipc_comps_dev(h, None, None, None, None, 1, 1, None, None, None, 0) == E
    assert lib.sg_hints_replacers_dev(h, None, None, 1, None, None, 1, None, None, 0) == E
