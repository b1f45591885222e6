"""The pkg/cover slice algebra (sg_merge.hip) at the edges of its paths: the
generic merge with many pairs, k_diff_small, k_merge_small's gap and tile
forms, HasDifference's two kernels and the big Canonicalize path.

tests/merge_cases.py builds each case on one constant of the kernels and
states what it claims: the path every pair takes (the context counters
"merge_pairs_*" / "canon_*" of the last call), the insertion points, run
counts, pass counts and parities.  The CPU tests below check those claims from
the restated routing rule, check the C oracle against a plain numpy statement
of pkg/cover/cover.go:28-117, and run a positional model of the kernel file's
element rule: the model equals the oracle on every case, and with each of the
named mistakes it differs from the oracle on at least one case of its family,
which is how the cases are shown to discriminate; a second model follows the
generic path's addressing over a whole batch (the pair search over the offsets,
the prefix differences at the pair starts) with mistakes of its own.  The GPU
tests run every case
through merge_batch, the single-pair calls, HasDifference (both forms) and
Canonicalize (both forms), bit-exact against the oracle with the result lengths
and the whole canonicalized slice, and with every counter as claimed.

A case of more than 100 pairs runs the model on every eighth pair and on every
pair of more than 100 values (the oracle and the library see all of them)."""
import numpy as np
import pytest

from oracle import pyoracle as O
from tests import merge_cases as M
from tests import refmodel as R

CASES = M.merge_cases()
IDS = [c.name for c in CASES]
SINGLES = [c for c in CASES if len(c.pairs) <= 16]
HD = M.hd_cases()
CANON = M.canon_cases()
SENT = M.SENT
FAMILY_OF_PATH = {"generic": "generic", "diff_small": "diff_small", "gap": "gap", "tile": "tile"}
MERGE_CTRS = ("merge_pairs_generic", "merge_pairs_diff_small", "merge_pairs_gap", "merge_pairs_tile")
CANON_CTRS = ("canon_wave_lists", "canon_block_lists", "canon_big_segments", "canon_merge_passes")

_exp = {}


def expected(case):
    """the oracle's result of every pair under every op, computed once"""
    if case.name not in _exp:
        e = {op: [O.foreach(op, a, b) for a, b in case.pairs] for op in M.OPS}
        for lst in e.values():
            for x in lst:
                x.setflags(write=False)
        _exp[case.name] = e
    return _exp[case.name]


def numpy_foreach(op, a, b):
    """pkg/cover/cover.go:42-102 by value counts, in plain numpy"""
    va, ca = np.unique(a, return_counts=True)
    vb, cb = np.unique(b, return_counts=True)
    v = np.union1d(va, vb)
    x, y = np.zeros(v.size, np.int64), np.zeros(v.size, np.int64)
    x[np.searchsorted(v, va)] = ca
    y[np.searchsorted(v, vb)] = cb
    k = {M.DIFF: np.maximum(x - y, 0), M.SYMDIFF: np.abs(x - y), M.UNION: np.maximum(x, y),
         M.INTER: np.minimum(x, y)}[op]
    k[v == SENT] = 0
    return np.repeat(v, k).astype(np.uint32)


def numpy_has_difference(a, b):
    """cover.go:106-117: some value more often in a than in b (no value is special)"""
    return numpy_foreach_raw_diff(a, b) > 0


def numpy_foreach_raw_diff(a, b):
    va, ca = np.unique(a, return_counts=True)
    vb, cb = np.unique(b, return_counts=True)
    y = np.zeros(va.size, np.int64)
    at = np.searchsorted(vb, va)
    hit = (at < vb.size) & (vb[np.minimum(at, max(vb.size - 1, 0))] == va) if vb.size else np.zeros(va.size, bool)
    y[hit] = cb[at[hit]]
    return int(np.maximum(ca - y, 0).sum())


def model_pairs(case):
    n = len(case.pairs)
    return [k for k in range(n) if n <= 100 or k % 8 == 0 or case.pairs[k][0].size + case.pairs[k][1].size > 100]


# ---- CPU: the restatement and the claims -----------------------------------------
def test_routing_restatement():
    r = M.route
    for op in (M.UNION, M.SYMDIFF):
        assert r(op, [4096, 9000, 0], [9000, 4096, 0]) == (0, 0, 1, 2)
        assert r(op, [4096, 4097, 0], [9000, 4097, 0]) == (3, 0, 0, 0)
        assert r(op, [1, 1], [32, 31]) == (0, 0, 1, 1)
        # 32-bit indices in the small kernels: a pair of 2^32 values goes generic
        assert r(op, [1, 5], [(1 << 32) - 2, 5]) == (0, 0, 1, 1)
        assert r(op, [1, 5], [(1 << 32) - 1, 5]) == (2, 0, 0, 0)
    for op in (M.DIFF, M.INTER):
        assert r(op, [4096, 0], [1 << 20, 7]) == (0, 2, 0, 0)
        assert r(op, [4097, 0], [1, 7]) == (2, 0, 0, 0)
        assert r(op, [3, 3], [(1 << 32) - 4, 1]) == (0, 2, 0, 0)
        assert r(op, [3, 3], [(1 << 32) - 3, 1]) == (2, 0, 0, 0)
    assert M.is_gap(0, 0) and M.is_gap(0, 1) and M.is_gap(4096, 131072) and not M.is_gap(4096, 131071)
    assert [M.canon_passes(n) for n in (4096, 4097, 8192, 8193, 16384, 16385, 32768, 32769)] == [0, 1, 1, 2, 2, 3, 3, 4]
    assert M.canon_route([0, 1, 1024, 1025, 4096]) == (2, 2, 0, 0)
    assert M.canon_route([0, 1, 4097, 1025, 9000]) == (0, 0, 2, 2)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_case_claims(case):
    al, bl = case.lens()
    for k, ((a, b), kind, fits) in enumerate(zip(case.pairs, case.kinds, case.fits)):
        ns, nl = min(a.size, b.size), max(a.size, b.size)
        assert kind == ("big" if ns > M.KMS else "gap" if M.is_gap(ns, nl) else "tile"), k
        assert fits == ("a" if a.size <= M.KMS else "") + ("b" if b.size <= M.KMS else ""), k
        for op in M.OPS:
            assert case.claim_pair(op, k) == M.route(op, [a.size], [b.size])
    for op in M.OPS:
        assert case.claim(op) == M.route(op, al, bl), M.OPNAME[op]
    # the layout the batch call gets holds exactly the pairs
    A, ab, aln, B, bb, bln = case.batch()
    for k, (a, b) in enumerate(case.pairs):
        assert np.array_equal(A[int(ab[k]):int(ab[k] + aln[k])], a)
        assert np.array_equal(B[int(bb[k]):int(bb[k] + bln[k])], b)
    fam = case.family
    if fam in ("tile", "gap"):  # every pair of the family's cases is on the family's path
        assert set(case.kinds) == {fam}
    if fam == "diff_small":
        # k_diff_small whenever every first list is a small one (the swapped cases: only where both lists fit)
        assert (case.claim(M.DIFF)[1] > 0) == all(a.size <= M.KMS for a, _ in case.pairs)
        assert case.claim(M.DIFF)[1] > 0 or case.name.endswith("_sw")
    if fam == "generic":
        assert all(case.claim(op)[0] == len(case.pairs) > 1 for op in M.OPS)
    nt, base = case.notes, case.name.replace("_sw", "")
    SL = [(a, b) if a.size <= b.size else (b, a) for a, b in case.pairs]
    if base == "route_min4096":
        assert min(min(a.size, b.size) for a, b in case.pairs if max(a.size, b.size) > M.KMS) == M.KMS
        assert case.claim(M.UNION) == (0, 0, 6, 6)
        assert any(L.size == 32 * S.size > 0 for S, L in SL) and any(L.size == 32 * S.size - 1 for S, L in SL)
        assert {L.size for S, L in SL if S.size == 0} == {0, 1, 300}
    if base == "route_min4097":
        assert case.claim(M.UNION) == (13, 0, 0, 0) and (4097, 4097) in zip(al, bl)
    if base == "route_a4096" and not case.name.endswith("_sw"):
        assert max(al) == M.KMS and case.claim(M.DIFF) == case.claim(M.INTER) == (0, 6, 0, 0)
    if base == "route_a4097" and not case.name.endswith("_sw"):
        assert max(al) == M.KMS + 1 and case.claim(M.DIFF) == (7, 0, 0, 0) and case.claim(M.UNION)[0] == 0
    if base == "tile_nl_edges":
        assert [L.size for _, L in SL] == [8191, 8192, 8193, 16384, 16385]
        assert all(S.size == L.size // 32 + 1 for S, L in SL)
    if "ins" in nt:
        for S, L in SL:
            ins = set(np.searchsorted(L, S, "left").tolist()) | set(np.searchsorted(L, S, "right").tolist())
            assert {0, 8191, 8192, L.size} <= ins
            # ... and 8192 as the upper bound of a value L holds (the insertion point of cov1's copy)
            assert 8192 in np.searchsorted(L, S, "right")[np.searchsorted(L, S, "left") == 8191]
        assert sorted(L.size % M.MTILE == 0 for _, L in SL) == [False, False, True, True]
    if "run" in nt and fam == "tile":
        start, run = nt["run"]
        for (S, L), cnt in zip(SL, (1, run - 1, run, run + 1)):
            x = L[start]
            assert start < M.MTILE < start + run
            assert np.array_equal(np.flatnonzero(L == x), np.arange(start, start + run))
            assert int((S == x).sum()) == cnt
    if "dense" in nt:
        for (S, L), want in zip(SL, nt["dense"]):
            depth = [int(np.searchsorted(S, L[min(w + 63, L.size - 1)], "right") - np.searchsorted(S, L[w], "left"))
                     for w in range(0, L.size, 64)]
            assert max(depth) == want and depth[1] == want and sorted(depth)[-2] <= 2
    if base == "tile_ballot_steps":
        assert [S.size for S, _ in SL] == [63, 63, 64, 64, 65, 65, 4096, 4096]
        assert all(S[-1] < L[0] for S, L in SL[0::2]) and all(S[0] > L[-1] for S, L in SL[1::2])
    if base == "tile_s4096_equal":
        assert [int((L == S[0]).sum()) for S, L in SL] == [100, 4096, 5000] and all(np.all(S == S[0]) for S, _ in SL)
    if "sent_tail" in nt:
        s0, n = nt["sent_tail"]
        L = SL[0][1]
        assert L.size == n and np.array_equal(np.flatnonzero(L == SENT), np.arange(s0, n)) and s0 < M.MTILE < n
        assert all(np.all(S == SENT) for S, _ in SL[1:])
    if fam == "gap" and "runs" in nt:
        runs = nt["runs"] if isinstance(nt["runs"], tuple) else (nt["runs"],) * len(SL)
        assert [np.unique(S).size for S, _ in SL] == list(runs)
    if base == "gap_4096_runs":
        assert SL[0][0].size == 4096 and SL[0][1].size == 131072
    if base == "gap_4096_equal":
        assert [int((L == S[0]).sum()) for S, L in SL] == [4095, 4096, 4097] and all(L.size == 131072 for _, L in SL)
    if base == "gap_counts":
        S, L = SL[0]
        sign = {int(np.sign(int((S == v).sum()) - int((L == v).sum()))) for v in np.unique(S)}
        assert sign == {-1, 0, 1}
        assert SL[1][1][0] == SL[1][0][0] and SL[2][1][-1] == SL[2][0][-1]  # the first / the last gap empty
    if "gaps" in nt:
        for q, (S, L) in enumerate(SL):
            ub, lb = np.searchsorted(L, S, "right"), np.searchsorted(L, S, "left")
            gaps = [int(lb[0])] + [int(lb[j + 1] - ub[j]) for j in range(S.size - 1)] + [int(L.size - ub[-1])]
            assert tuple(gaps[1:-1]) == nt["gaps"] and gaps[0] == q % 2 and gaps[-1] == 0
    if base == "gap_sentinels":
        assert SL[0][0][0] > SL[0][1][-1] and np.all(SL[1][1] == SENT) and SENT in SL[2][0] and SENT in SL[2][1]
    if base == "diff_sizes":
        assert sorted(set(zip(*CASES[IDS.index(base)].lens()))) == sorted(
            (x, y) for x in (0, 1, 4095, 4096) for y in (0, 1, 100000))
    if "tail" in nt and not case.name.endswith("_sw"):
        for (a, b), r in zip(case.pairs, nt["tail"]):
            assert a.size == M.KMS and np.all(a == a[0]) and int((b == a[0]).sum()) == r
            assert r == 0 or np.array_equal(np.flatnonzero(b == a[0]), np.arange(b.size - r, b.size))
            assert b[b.size - r - 1] < a[0]  # q = lower_bound + t reaches nb for copy t == r
    if "a_off" in nt:
        sw = case.name.endswith("_sw")
        assert np.cumsum(bl if sw else al).tolist() == nt["a_off"]
        assert np.cumsum(al if sw else bl).tolist() == nt["b_off"]
        for offs in (nt["a_off"], nt["b_off"]):
            mods = {(o % 4096, o % 256) for o in offs}
            assert {(0, 0), (1, 1), (4095, 255)} <= mods and {0, 1, 255} <= {m for _, m in mods}
            assert len(offs) == 41 and len(set(offs)) < len(offs)  # (repeated offsets: empty sides)
    if base == "gen_empties":
        e = [a.size + b.size == 0 for a, b in case.pairs]
        assert e[0] and e[-1] and any(e[k] and e[k + 1] for k in range(1, len(e) - 2))
        assert any(a.size == 0 < b.size for a, b in case.pairs) and any(b.size == 0 < a.size for a, b in case.pairs)
    if "total_mod" in nt:
        assert sum(al) == sum(bl) == 2 * M.TILE + nt["total_mod"]
    if base == "gen_run5000":
        big, oth = (1, 0) if case.name.endswith("_sw") else (0, 1)
        assert [int((p[oth] == 1234).sum()) for p in case.pairs] == [0, 4999, 5000, 5001]
        assert all(int((p[big] == 1234).sum()) == 5000 for p in case.pairs)
        at = np.flatnonzero(case.pairs[0][big] == 1234)
        assert at[0] // M.CHUNK < at[-1] // M.CHUNK - 18
    if base == "gen_shared":
        A, ab, aln, B, bb, bln = case.layout
        for beg, ln in ((ab, aln), (bb, bln)):
            beg, ln = beg.astype(np.int64), ln.astype(np.int64)
            shared = len({(x, y) for x, y in zip(beg.tolist(), ln.tolist())}) < beg.size
            overlap = any(beg[i] < beg[j] + ln[j] and beg[j] < beg[i] + ln[i] and ln[i] and ln[j]
                          for i in range(beg.size) for j in range(i))
            assert shared or (overlap and np.any(np.diff(beg) < 0))
    if "npair" in nt:
        assert len(case.pairs) == nt["npair"] and sum(1 for a, b in case.pairs if a.size + b.size > 6) == 1
        assert {(min(a.size, 4), min(b.size, 4)) for a, b in case.pairs} == {(x, y) for x in range(5) for y in range(5)
                                                                           if (x == 4) == (y == 4)}


def test_cases_hold_the_extreme_values():
    vals = np.concatenate([x for c in CASES for p in c.pairs for x in p])
    assert 0 in vals and M.TOP in vals and SENT in vals


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_oracle_against_plain_statements(case):
    e = expected(case)
    for op in M.OPS:
        for k, (a, b) in enumerate(case.pairs):
            assert np.array_equal(e[op][k], numpy_foreach(op, a, b)), (M.OPNAME[op], k)
            if a.size + b.size <= 400 and (len(case.pairs) <= 100 or k % 8 == 0):
                assert e[op][k].tolist() == R.foreach_counts(op, a.tolist(), b.tolist()), (M.OPNAME[op], k)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_model_equals_oracle(case):
    e = expected(case)
    al, bl = case.lens()
    for op in M.OPS:
        for k in model_pairs(case):
            a, b = case.pairs[k]
            # as the batch routes it, and as the pair routes on its own
            for path in {M.pair_path(op, al, bl, k), M.pair_path(op, [a.size], [b.size], 0)}:
                assert M.same(M.model(op, a, b, path), e[op][k]), (M.OPNAME[op], k, path)


@pytest.mark.parametrize("mistake", sorted(M.MISTAKES), ids=sorted(M.MISTAKES))
def test_mistaken_model_is_caught(mistake):
    """each named mistake, made on each path it belongs to, gives a result
    that differs from the oracle on some case of that path's family"""
    for path in M.MISTAKES[mistake][0]:
        caught = None
        for case in CASES:
            if case.family != FAMILY_OF_PATH[path]:
                continue
            al, bl = case.lens()
            for op in M.OPS:
                for k in model_pairs(case):
                    a, b = case.pairs[k]
                    if path not in (M.pair_path(op, al, bl, k), M.pair_path(op, [a.size], [b.size], 0)):
                        continue
                    if not M.same(M.model(op, a, b, path, mistake), expected(case)[op][k]):
                        caught = (case.name, M.OPNAME[op], k)
                        break
                if caught:
                    break
            if caught:
                break
        print(f"{mistake} on the {path} path: caught by {caught}")
        assert caught is not None, (mistake, path, M.MISTAKES[mistake][1])


GENERIC = [c for c in CASES if c.family == "generic"]


def _batch_same(case, op, mistake=None):
    got = M.model_generic_batch(op, case.batch(), mistake)
    return got is not None and all(M.same(g, w) for g, w in zip(got, expected(case)[op]))


@pytest.mark.parametrize("case", GENERIC, ids=[c.name for c in GENERIC])
def test_generic_batch_model_equals_oracle(case):
    """the generic path's addressing over the whole batch (pair search over the
    offsets, prefix differences at the pair starts, the prefix past the last
    chunk, cov1 without masks under Difference / Intersection)"""
    for op in M.OPS:
        assert _batch_same(case, op), M.OPNAME[op]


@pytest.mark.parametrize("mistake", sorted(M.BATCH_MISTAKES))
def test_mistaken_batch_model_is_caught(mistake):
    caught = [(c.name, M.OPNAME[op]) for c in GENERIC for op in M.OPS if not _batch_same(c, op, mistake)]
    print(f"{mistake}: caught by {sorted({n for n, _ in caught})}")
    assert caught, M.BATCH_MISTAKES[mistake]
    names, every_op = {n for n, _ in caught}, lambda n: all((n, M.OPNAME[op]) in caught for op in M.OPS)  # noqa: E731
    if mistake == "prefix_end_zero":  # only a total that is a multiple of 4096 reaches that branch
        assert every_op("gen_total_m0") and every_op("gen_total_m0_sw")
        assert not names & {"gen_total_m1", "gen_total_m1_sw"}
    if mistake == "seg_first_repeat":  # needs an empty side before a non-empty one
        assert {"gen_empties", "gen_offsets", "gen_3000_tiny"} <= names and every_op("gen_offsets")
        assert not names & {"gen_run5000", "gen_shared", "gen_total_m0", "gen_total_m1"}  # (no empty sides there)
    if mistake == "no_pair_base":
        assert names == {c.name for c in GENERIC}


def _caught(mistake, path, name, k):
    """whether the mistaken model differs from the oracle on pair k of the case under some op"""
    case = CASES[IDS.index(name)]
    a, b = case.pairs[k]
    ops = [op for op in M.OPS if M.pair_path(op, [a.size], [b.size], 0) == path]
    assert ops, (name, k, path)
    return any(not M.same(M.model(op, a, b, path, mistake), expected(case)[op][k]) for op in ops)


@pytest.mark.parametrize("sw", ("", "_sw"))
def test_edges_sit_on_their_constants(sw):
    """the pairs either side of a constant: the mistake shows on the one and
    not on the other (k_diff_small's cases only with a the small list)"""
    # the dense fallback: 16 values in a window are read whole, 17 are not
    assert [_caught("dense_cap16", "tile", "tile_dense_16_17" + sw, k) for k in (0, 1)] == [False, True]
    # the post-loop branch: nl = 16384, 16385, 8192, 12000
    assert [_caught("lost_at_nl", "tile", "tile_ins_points" + sw, k) for k in range(4)] == [True, False, True, False]
    # S's count 1, run - 1, run, run + 1 of the run that crosses a tile end: from run on, no copy of L's is kept
    assert [_caught("t_from_tile", "tile", "tile_run_cross" + sw, k) for k in range(4)] == [True, True, False, False]
    assert not any(_caught("t_from_tile", "tile", "tile_nl_edges" + sw, k) for k in range(5))
    assert _caught("drops_cl", "gap", "gap_counts" + sw, 0)
    assert [_caught("no_sentinel_clamp", "gap", "gap_sentinels" + sw, k) for k in range(4)] == [False, True, True, True]
    if not sw:  # a run of r copies at b's end: copy t == r has q == nb, and a holds it iff r < 4096
        assert [_caught("q_eq_nb_match", "diff_small", "diff_4096_equal_tail", k) for k in range(5)] == \
            [True, True, True, False, False]


@pytest.mark.parametrize("case", HD, ids=[c.name for c in HD])
def test_has_difference_claims(case):
    for (a, b), want, at in zip(case.pairs, case.expect, case.at):
        assert O.has_difference(a, b) == want == numpy_has_difference(a, b)
        if at is not None:  # the sole element b lacks
            assert numpy_foreach_raw_diff(a, b) == 1 and not O.has_difference(np.delete(a, at), b)
    if case.name.startswith("hd_single"):
        (a, _), = case.pairs
        assert a.size == M.HD_GRID + 1  # the grid's second round holds one element
    if case.name == "hd_batch_positions":
        assert case.at == [0, M.HD_BLOCK - 1, M.HD_BLOCK, case.pairs[0][0].size - 1, None]
    if case.name == "hd_batch_one_differs":
        assert sum(case.expect) == 1


@pytest.mark.parametrize("case", CANON, ids=[c.name for c in CANON])
def test_canonicalize_claims(case):
    lens = np.diff(case.off.astype(np.int64)).tolist()
    assert case.claim == M.canon_route(lens)
    for s in case.segs:
        want, n = M.canon_expected(s)
        got, gn = O.canonicalize(s)
        assert gn == n and np.array_equal(got, want)
        if s.size <= 300:
            assert got[:gn].tolist() == R.canonicalize(s.tolist())
    if case.name == "canon_runs_mixed":
        assert sorted(x for x in lens if x >= M.TILE - 1) == case.notes["lens"] == sorted(
            M.TILE * m + d for m in M.CANON_M for d in M.CANON_D)
        big = [(int(case.off[k]), x) for k, x in enumerate(lens) if x > M.TILE]
        assert all(s % 64 for s, _ in big) and lens[0] > 0
        assert [x for _, x in big] != sorted(x for _, x in big)  # (shuffled)
        assert {M.canon_passes(x) for _, x in big} == {1, 2, 3, 4}  # every pass count, so both buffer parities
        for k, s in enumerate(case.segs):  # equal keys across every run boundary
            runs = [set(s[q:q + M.TILE].tolist()) for q in range(0, s.size, M.TILE)]
            assert all(runs[r] & runs[r + 1] for r in range(len(runs) - 1)), k
    if case.name == "canon_8193_sentinels":
        assert M.canon_expected(case.segs[0])[1] == 0
    if case.name == "canon_one_value":
        assert [M.canon_expected(s)[1] for s in case.segs] == [1, 1, 1]
    if case.name == "canon_full_range":
        s = case.segs[1]
        assert s.min() == 0 and M.TOP in s and SENT in s and np.unique(s >> 28).size == 16


# ---- GPU ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def C(ctx):
    from syzkaller_amd import cover

    return cover


def merge_counters(ctx):
    return tuple(ctx.counter(n) for n in MERGE_CTRS)


def canon_counters(ctx):
    return tuple(ctx.counter(n) for n in CANON_CTRS)


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_gpu_merge_batch(C, ctx, case):
    e = expected(case)
    layout = case.batch()
    for op in M.OPS:
        outs = C.merge_batch(op, *layout, ctx=ctx)
        assert merge_counters(ctx) == case.claim(op), M.OPNAME[op]
        for k, want in enumerate(e[op]):
            assert outs[k].size == want.size and np.array_equal(outs[k], want), (M.OPNAME[op], k)


@pytest.mark.gpu
@pytest.mark.parametrize("case", SINGLES, ids=[c.name for c in SINGLES])
def test_gpu_merge_single(C, ctx, case):
    e = expected(case)
    fn = {M.DIFF: C.Difference, M.SYMDIFF: C.SymmetricDifference, M.UNION: C.Union, M.INTER: C.Intersection}
    for op in M.OPS:
        for k, (a, b) in enumerate(case.pairs):
            got = fn[op](a, b, ctx=ctx)
            if a.size + b.size:  # (two empty lists never reach the device)
                assert merge_counters(ctx) == case.claim_pair(op, k), (M.OPNAME[op], k)
            assert got.size == e[op][k].size and np.array_equal(got, e[op][k]), (M.OPNAME[op], k)


@pytest.mark.gpu
@pytest.mark.parametrize("case", HD, ids=[c.name for c in HD])
def test_gpu_has_difference(C, ctx, case):
    a = np.concatenate([x for x, _ in case.pairs])
    b = np.concatenate([y for _, y in case.pairs])
    al = np.array([x.size for x, _ in case.pairs], np.uint64)
    bl = np.array([y.size for _, y in case.pairs], np.uint64)
    ab = np.concatenate([[0], np.cumsum(al)[:-1]]).astype(np.uint64)
    bb = np.concatenate([[0], np.cumsum(bl)[:-1]]).astype(np.uint64)
    assert C.has_difference_batch(a, ab, al, b, bb, bl, ctx=ctx).tolist() == case.expect
    if case.single:
        for (x, y), want in zip(case.pairs, case.expect):
            assert C.HasDifference(x, y, ctx=ctx) == want


@pytest.mark.gpu
@pytest.mark.parametrize("case", CANON, ids=[c.name for c in CANON])
def test_gpu_canonicalize(C, ctx, case):
    vals = case.vals.copy()
    lens = C.canonicalize_batch(vals, case.off, ctx=ctx)
    assert canon_counters(ctx) == case.claim
    for k, s in enumerate(case.segs):
        want, n = M.canon_expected(s)
        assert int(lens[k]) == n, k
        assert np.array_equal(vals[int(case.off[k]):int(case.off[k + 1])], want), k  # the stale tail included
    for k, s in enumerate(case.segs):
        if s.size == 0 or (s.size < M.TILE - 1 and k % 5):
            continue
        buf = s.copy()
        got = C.Canonicalize(buf, ctx=ctx)
        want, n = M.canon_expected(s)
        assert canon_counters(ctx) == M.canon_route([s.size]), k
        assert got.size == n and np.array_equal(buf, want), k
