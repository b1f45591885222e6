"""sg_triage_runs_from_kcov at the edges of its routes: the cover fold (copy, LDS
sort, by ranks, single-lane foreach) around triage_runs_sort_cap and its
padding, over 2 to 8 lists, with repeats, sentinel tails and exactly full
slots; the run loop at nruns 2, 4 and 8; newSignal across tinput_chunk.

The cases are tests/triage_runs_cases.py's.  On the CPU every case's (m, total,
ascending, sentinel-first, cap) is derived from the oracle's per-run (Signal,
Cover) and must give the route and the edge the case is built for; on the GPU
the host and the device forms are bit-exact against tests/triage_runs_oracle.py
on both exec_cover paths, and the five route counters equal the CPU-derived
expectation after every call."""
import numpy as np
import pytest

from tests import triage_runs_cases as K
from tests import triage_runs_oracle as TR
from tests.test_triage_runs import _check

ALL_ROUTES = ("threshold", "three_lists", "five_lists", "eight_lists", "full_slots")  # batches that take all four


# ---- CPU: the generators hold what they promise -------------------------------------
@pytest.mark.parametrize("name", K.BATCHES)
def test_cases_have_their_shape(name):
    _, cases, exp, shapes = K.batch(name)
    assert len(cases) == len(shapes) == exp[0].size
    for k, (c, sh) in enumerate(zip(cases, shapes)):
        assert sh.status == exp[0][k], c.name
        assert K.route_of(sh) == c.route, (c.name, sh[:7])
        if c.m is not None:
            assert sh.m == c.m, (c.name, sh[:7])
        if c.total is not None:
            assert sh.total == c.total, (c.name, sh[:7])
        if c.pred is not None:
            assert c.pred(sh), (c.name, sh[:7])
        assert sh.total <= sh.cap, c.name
        # the oracle's inputCover is as long as the shape says a copy is, and never longer than the lists
        n_cov = int(exp[4][k + 1] - exp[4][k])
        assert n_cov == sh.total if sh.m == 1 else n_cov <= sh.total, c.name


def test_batches_reach_every_route():
    for name in ALL_ROUTES:
        want = K.counters(K.batch(name)[3])
        assert all(want["triage_runs_" + r] >= 1 for r in K.ROUTES) and want["triage_runs_wide"] >= 1, (name, want)


def test_threshold_sits_on_the_sort_cap_and_its_padding():
    shapes = {c.name: sh for c, sh in zip(*K.batch("threshold")[1::2])}
    cap = K.SORT_CAP
    assert [shapes["total=%d" % t].total for t in (cap - 1, cap, cap + 1)] == [cap - 1, cap, cap + 1]
    assert [K.route_of(shapes["total=%d" % t]) for t in (cap - 1, cap, cap + 1)] == ["sorted", "sorted", "ranked"]
    for t in (cap // 2, cap // 2 + 1, 2, 3):
        assert shapes["total=%d" % t].total == t and K.route_of(shapes["total=%d" % t]) == "sorted"
    assert max(len(x) for x in shapes["long+short"].lists) > cap  # one list alone past the cap


def test_full_slots_are_full_and_alternate():
    _, cases, _, shapes = K.batch("full_slots")
    assert [K.route_of(sh) for sh in shapes] == ["ranked", "foreach", "copied", "sorted", "ranked", "foreach"]
    assert all(sh.total == sh.cap for sh in shapes)
    assert [sh.m for sh in shapes] == [2, 2, 1, 2, 2, 2]  # one Union in a foreach: its result is in the second buffer


def test_run_loop_counts_the_runs_it_should():
    for n in (2, 4, 8):
        _, cases, exp, shapes = K.batch("run_loop%d" % n)
        assert all(len(c.cand[2]) == n for c in cases)
        assert set(exp[0].tolist()) == {TR.OK, TR.NO_NEW, TR.NOT_EXECUTED, TR.FLAKY}
        assert shapes[0].counted == tuple(range(n))  # at 8 runs: the state word's bit 31


def test_chunk_cases_sit_on_the_chunk():
    pcs, sig, short, _ = K._long_trace()
    assert pcs.size == sig.size == 20000 == np.unique(sig).size  # 20,000 distinct signals, one per PC
    C = K.CHUNK
    batches = K.chunk_batches()
    got = {}
    for b, (_, cases, extra) in enumerate(batches):
        exp = K.batch("chunk%d" % b)[2]
        for k, (c, (new1, want)) in enumerate(zip(cases, extra)):
            kept = exp[1][int(exp[2][k]):int(exp[2][k + 1])]
            got[c.name] = (c.cand[0].size, new1, kept)
            assert sum(x.size for r in c.cand[2] for x in r) < 50000, c.name
    assert sorted(v[0] for v in got.values()) == [C - 1, C, C + 1, 2 * C + 1, 2 * C + 1]
    n, new1, kept = got["K=2C+1, chunk 0 empties"]
    assert new1.size > C + 300 and kept.size >= 293 and np.searchsorted(new1, kept[0]) == C  # the smallest at rank C
    n, new1, kept = got["K=2C+1, last of chunk 0 and first of chunk 1"]
    assert np.searchsorted(new1, kept).tolist() == [C - 1, C]
    assert got["K=C, nothing kept"][2].size == 0
    for name in ("K=C-1", "K=C+1"):
        n, new1, kept = got[name]
        assert 0 < kept.size < 100 and kept[-1] == new1[-1] and C - 400 < new1.size < n


def test_signal_lengths():
    corpus, cases, exp, shapes = K.batch("signal_lengths")
    assert [c.cand[0].size for c in cases] == [255, 256, 257, 513]
    for k, c in enumerate(cases):
        v = c.cand[0]
        assert (v == K.S).sum() == 3 and np.unique(v).size < v.size - 2  # sentinels and duplicates
        new = exp[1][int(exp[2][k]):int(exp[2][k + 1])]
        assert 0 < new.size < v.size // 2 + 2 and not np.isin(new, corpus).any()


# ---- GPU ---------------------------------------------------------------------------
def _run(ctx, ctx_option, name):
    assert ctx.counter("triage_runs_sort_cap") == K.SORT_CAP and ctx.counter("tinput_chunk") == K.CHUNK
    corpus, cases, exp, shapes = K.batch(name)
    want = K.counters(shapes)
    _check(ctx, ctx_option, corpus, [c.cand for c in cases], exp, wide=want["triage_runs_wide"], counters=want)
    return want


@pytest.mark.gpu
def test_constants_are_the_ones_the_cases_are_built_for(ctx):
    assert ctx.counter("triage_runs_sort_cap") == K.SORT_CAP
    assert ctx.counter("tinput_chunk") == K.CHUNK


@pytest.mark.gpu
@pytest.mark.parametrize("name", ALL_ROUTES)
def test_cover_fold(ctx, ctx_option, name):
    want = _run(ctx, ctx_option, name)
    assert all(want["triage_runs_" + r] >= 1 for r in K.ROUTES), want  # all four routes ran, and were counted


@pytest.mark.gpu
@pytest.mark.parametrize("nruns", (2, 4, 8))
def test_run_loop(ctx, ctx_option, nruns):
    _run(ctx, ctx_option, "run_loop%d" % nruns)


@pytest.mark.gpu
@pytest.mark.parametrize("part", (0, 1))
def test_new_signal_across_the_chunk(ctx, ctx_option, part):
    _run(ctx, ctx_option, "chunk%d" % part)


@pytest.mark.gpu
def test_signal_lengths_around_the_diff_rounds(ctx, ctx_option):
    _run(ctx, ctx_option, "signal_lengths")
