"""triageInput's batched signal math (syz-fuzzer/fuzzer.go:526-532, :567,
:584-587): the oracle composition against line-by-line Python (CPU), and the
product's sg_triage_newsig / sg_triage_intersect / sg_triage_subset against the
oracle (GPU).  Bit-exact."""
import numpy as np
import pytest

from oracle import pyoracle as O
from tests import refmodel as R

SENT = 0xFFFFFFFF


def _inputs(rng, n, hi, maxlen, sent_frac=0.02):
    lists = []
    for k in range(n):
        L = int(rng.integers(0, maxlen)) if k % 7 else 0
        v = rng.integers(0, hi, size=L).astype(np.uint32)
        v[rng.random(L) < sent_frac] = SENT
        if L and k % 5 == 0:
            v[rng.integers(0, L, size=L // 3)] = v[rng.integers(0, L, size=L // 3)]  # duplicates
        lists.append(v)
    return lists


def _csr(lists):
    return O._csr(lists)


def _reexec(rng, new_lists, hi, keep):
    """A re-execution's raw signal: most of new_k (flaky coverage drops some), plus other values."""
    out = []
    for a in new_lists:
        kept = a[rng.random(a.size) < keep]
        extra = rng.integers(0, hi, size=int(rng.integers(0, 300))).astype(np.uint32)
        r = np.concatenate([kept, extra, kept[: kept.size // 2]])
        rng.shuffle(r)
        out.append(r.astype(np.uint32))
    return out


def test_oracle_composition_vs_python():
    rng = np.random.default_rng(31)
    corpus = set(int(x) for x in rng.integers(0, 3000, size=2000))
    oc = O.OSet(np.array(sorted(corpus), np.uint32))
    lists = _inputs(rng, 60, 4000, 200)
    vals, off = _csr(lists)
    nv, no = O.triage_newsig(oc, vals, off)
    for k, s in enumerate(lists):
        diff = [int(x) for x in s if int(x) not in corpus]  # cover.go:169-176
        exp = R.canonicalize(diff)
        assert list(nv[int(no[k]):int(no[k + 1])]) == exp
    news = [nv[int(no[k]):int(no[k + 1])] for k in range(len(lists))]
    rs = _reexec(rng, news, 4000, 0.9)
    rv, ro = _csr(rs)
    iv, io = O.triage_intersect(nv, no, rv, ro)
    ok = O.triage_subset(nv, no, rv, ro)
    for k in range(len(lists)):
        exp = R.foreach_loop(3, list(news[k]), R.canonicalize([int(x) for x in rs[k]]))
        assert list(iv[int(io[k]):int(io[k + 1])]) == exp
        assert ok[k] == (len(exp) == news[k].size)


@pytest.mark.gpu
def test_triage_newsig_vs_oracle(ctx):
    from syzkaller_amd import cover as C

    rng = np.random.default_rng(32)
    m0 = rng.integers(0, 1 << 20, size=200000).astype(np.uint32)
    cs, oc = C.SignalSet(ctx), O.OSet(m0)
    C.SignalAdd(cs, m0)
    for trial, (n, maxlen) in enumerate([(1, 10), (300, 3000), (40, 40000), (500, 5)]):
        lists = _inputs(rng, n, 1 << 21, maxlen)
        vals, off = _csr(lists)
        gv, go = C.triage_newsig(cs, vals, off)
        ev, eo = O.triage_newsig(oc, vals, off)
        assert np.array_equal(go, eo), trial
        assert np.array_equal(gv, ev), trial
    # the corpus is only read
    assert np.array_equal(cs.export(), oc.export())
    # nothing new: every new_k empty
    gv, go = C.triage_newsig(cs, m0[:1000], np.array([0, 400, 1000], np.uint64))
    assert gv.size == 0 and list(go) == [0, 0, 0]


@pytest.mark.gpu
def test_triage_intersect_and_subset_vs_oracle(ctx):
    from syzkaller_amd import cover as C

    rng = np.random.default_rng(33)
    for trial, (n, maxlen, keep) in enumerate([(200, 300, 0.9), (50, 20000, 0.999), (100, 50, 1.0), (7, 9000, 0.5)]):
        lists = _inputs(rng, n, 1 << 22, maxlen, sent_frac=0.0 if trial == 2 else 0.02)
        canon = []
        for v in lists:
            a, m = O.canonicalize(v)
            canon.append(a[:m])
        if trial == 3:  # sorted inputs with duplicate runs (multiset Intersection keeps one copy)
            canon = [np.sort(np.concatenate([a, a[: a.size // 2]])).astype(np.uint32) for a in canon]
        nv, no = _csr(canon)
        rs = _reexec(rng, canon, 1 << 22, keep)
        rv, ro = _csr(rs)
        gv, go = C.triage_intersect(nv, no, rv, ro, ctx=ctx)
        ev, eo = O.triage_intersect(nv, no, rv, ro)
        assert np.array_equal(go, eo), trial
        assert np.array_equal(gv, ev), trial
        gok = C.triage_subset(nv, no, rv, ro, ctx=ctx)
        eok = O.triage_subset(nv, no, rv, ro)
        assert np.array_equal(gok, eok), trial
        if trial == 2:
            assert gok.all()  # every element re-executed: the predicate holds
    # empty new lists: Intersection(nil, x) is empty and the predicate holds
    z = np.zeros(4, np.uint64)
    rv = np.arange(30, dtype=np.uint32)
    ro = np.array([0, 10, 10, 30], np.uint64)
    gv, go = C.triage_intersect(np.zeros(0, np.uint32), z, rv, ro, ctx=ctx)
    assert gv.size == 0 and not go.any()
    assert C.triage_subset(np.zeros(0, np.uint32), z, rv, ro, ctx=ctx).all()


# ---- the LDS chunks of Intersection (counter "tinput_chunk") ---------------------------
def _ascending(L, seed):
    """L distinct ascending values: a canonical new list."""
    return (7 + np.cumsum(np.random.default_rng(seed).integers(1, 5, size=L))).astype(np.uint32)


def _edge_batch(C, pick, seed):
    """New lists of C - 1, C, C + 1, 2C and 2C + 1 values with short lists between them; r_k = pick(new_k, rng)."""
    rng = np.random.default_rng(seed)
    news, rs = [], []
    for i, L in enumerate((C - 1, 3, C, 0, C + 1, 300, 2 * C, 1, 2 * C + 1)):
        a = _ascending(L, seed + i)
        news.append(a)
        rs.append(np.asarray(pick(a, rng), dtype=np.uint32))
    return news, rs


def _both(ctx, news, rs, tag):
    """sg_triage_intersect and sg_triage_subset against the oracle; returns the kept lists."""
    from syzkaller_amd import cover as C

    nv, no = _csr(news)
    rv, ro = _csr(rs)
    gv, go = C.triage_intersect(nv, no, rv, ro, ctx=ctx)
    ev, eo = O.triage_intersect(nv, no, rv, ro)
    assert np.array_equal(go, eo), tag
    assert np.array_equal(gv, ev), tag
    gok = C.triage_subset(nv, no, rv, ro, ctx=ctx)
    assert np.array_equal(gok, O.triage_subset(nv, no, rv, ro)), tag
    return [gv[int(go[k]):int(go[k + 1])] for k in range(len(news))], gok


def _shuffled_twice(a, rng):
    r = np.concatenate([a, a[: a.size // 3]])
    rng.shuffle(r)
    return r


@pytest.mark.gpu
@pytest.mark.parametrize("what", ("everything", "nothing", "chunk 1 only", "chunk ends", "unsorted with duplicates"))
def test_intersect_and_subset_at_the_chunk_edges(ctx, what):
    C = ctx.counter("tinput_chunk")
    assert C == 8192
    ends = lambda a: a[[j for j in (C - 1, C, 2 * C - 1, 2 * C) if j < a.size]]  # noqa: E731
    pick = {"everything": lambda a, rng: rng.permutation(a),
            "nothing": lambda a, rng: np.setdiff1d(a + 1, a),   # next to the values, never equal
            "chunk 1 only": lambda a, rng: a[C:2 * C],
            "chunk ends": lambda a, rng: ends(a),
            "unsorted with duplicates": lambda a, rng: _shuffled_twice(a[rng.random(a.size) < 0.7], rng)}[what]
    news, rs = _edge_batch(C, pick, 40)
    kept, ok = _both(ctx, news, rs, what)
    for a, r, k, o in zip(news, rs, kept, ok):
        assert o == (k.size == a.size)  # canonical lists: the predicate is "everything was kept"
        if what == "everything":
            assert np.array_equal(k, a) and o
        elif what == "nothing":
            assert k.size == 0 and o == (a.size == 0)
        elif what == "chunk 1 only":
            assert np.array_equal(k, a[C:2 * C])
        elif what == "chunk ends":
            assert np.array_equal(k, ends(a))


@pytest.mark.gpu
def test_intersect_runs_of_equal_values_across_the_chunk_edges(ctx):
    C = ctx.counter("tinput_chunk")
    base = _ascending(2 * C + 40, 41)
    x, y, top = int(base[C - 2]), int(base[2 * C - 2]), 0xFFFFFFFF
    one = base.copy()
    one[C - 2:C + 3] = x                      # one value over indices C - 2 .. C + 2
    two = one.copy()
    two[2 * C - 2:2 * C + 3] = y              # ... and another over the second edge
    three = base.copy()
    three[2 * C - 2:2 * C + 3] = y            # the second run alone: chunk 0 is all distinct
    assert (np.diff(two.astype(np.int64)) >= 0).all() and (two == x).sum() == 5 and (two == y).sum() == 5
    last = np.concatenate([base[:C], [top]]).astype(np.uint32)  # 0xFFFFFFFF as the last value, the first of chunk 1
    lasts = np.concatenate([base[:C - 1], [top]]).astype(np.uint32)  # ... the last of chunk 0
    cases = [("present", one, np.array([x], np.uint32), [x]),
             ("absent", one, np.setdiff1d(base, [x]), None),
             ("both present, everything kept", two, two[::-1].copy(), None),
             ("chunk 0, then y", two, np.concatenate([two[:C], [y]]).astype(np.uint32), np.unique(two[:C]).tolist() + [y]),
             # chunk 0 is kept whole: the value before chunk 1 has been written in place by the time it is read
             ("chunk 0 whole, then y", three, np.concatenate([three[:C], [y]]).astype(np.uint32), three[:C].tolist() + [y]),
             ("chunks 0 and 1 of r, the second run", three, three[:2 * C][::-1].copy(), np.unique(three[:2 * C]).tolist()),
             ("the second run, everything kept", three, three, np.unique(three).tolist()),
             ("only y", two, np.array([y, y], np.uint32), [y]),
             ("both absent", two, np.setdiff1d(base, [x, y]), None),
             ("sentinel first of chunk 1", last, last, None),
             ("sentinel last of chunk 0", lasts, lasts[::-1].copy(), None),
             ("sentinel alone in r", last, np.array([top], np.uint32), [])]
    kept, ok = _both(ctx, [c[1] for c in cases], [c[2] for c in cases], "runs")
    for (name, a, r, want), k, o in zip(cases, kept, ok):
        if want is not None:
            assert k.tolist() == want, name
        assert (k == x).sum() == int(x in r and x in a) and (k == y).sum() == int(y in r and y in a), name  # one copy or none
        assert top not in k and (np.diff(k.astype(np.int64)) > 0).all(), name
    byname = {c[0]: k for c, k in zip(cases, kept)}
    assert byname["both present, everything kept"].tolist() == np.unique(two).tolist()
    assert byname["sentinel first of chunk 1"].tolist() == base[:C].tolist()
    assert byname["sentinel last of chunk 0"].tolist() == base[:C - 1].tolist()
    assert not ok.any()  # no list is kept whole: each has repeats or the sentinel
