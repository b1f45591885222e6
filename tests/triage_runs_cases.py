"""TEST INFRASTRUCTURE ONLY: the edge cases of sg_triage_runs_from_kcov.

Seeded generators of (signal, call, runs, minimized) candidates whose per-run
Cover is fully controlled, each with the route of k_tr_cover it is built for
(copy, LDS sort, by ranks, the single-lane foreach) and the edge it sits on;
and shape(), which derives a candidate's (m, total, ascending, sentinel-first,
cap) and with them its route from the oracle's per-run (Signal, Cover) alone,
so that a generator that drifts fails on the CPU (tests/test_triage_runs_edges.py).

A controlled run is one call: a fixed head of 64 distinct PCs with high word 0
(low words 16..1024, in one fixed order), then the payload, element i being
(i + 1) << 32 | low_i.  The executor's u64 sort keeps the payload in its given
order behind the head, so the Cover is 16, 32, .. 1024, low_0, low_1, ...: any
non-decreasing lows >= 1024 give an ascending list with arbitrary repeats,
0xFFFFFFFF lows at the end a sentinel tail, a decreasing step a wide list.  The
head gives every run the same first edges: inp.signal, the first 40 of run 0,
survives every run.
"""
import collections
import functools

import numpy as np

from oracle import pyoracle as O
from tests import triage_runs_oracle as TR

U32, U64 = np.uint32, np.uint64
S = 0xFFFFFFFF
TEXT = 0xFFFFFFFF81000000
SORT_CAP = 8192   # ctx.counter("triage_runs_sort_cap"): the cases are built for this value
CHUNK = 8192      # ctx.counter("tinput_chunk")
TB = 256          # threads of k_tr_cover / k_tr_round: a list is walked in rounds of as many elements
NHEAD = 64
HEAD = (16 * (1 + np.random.default_rng(60).permutation(NHEAD))).astype(U64)
ROUTES = ("copied", "sorted", "ranked", "foreach")

Case = collections.namedtuple("Case", "name cand route m total pred")
Shape = collections.namedtuple("Shape", "status counted m total ascending sent_first cap lists")


def call_of(lows, head=HEAD):
    """One call's KCOV buffer: head, then lows behind rising high words."""
    lows = np.asarray(lows, dtype=U64).reshape(-1)
    payload = ((np.arange(lows.size, dtype=U64) + U64(1)) << U64(32)) | lows
    return payload if head is None else np.concatenate([head, payload])


def asc(rng, n, span=None, lo=2048):
    """n non-decreasing lows of [lo, lo + span): repeats, and overlap between lists of one pool."""
    span = max(2 * n, 4) if span is None else span
    return np.sort(rng.integers(lo, lo + span, size=n)).astype(U64)


def sig_of(run, call=0):
    info = TR.run_info(run, call)
    return info[0] if info is not None else TR.EMPTY


def fold(lists, head=HEAD, nsig=40, minimized=False, extra_runs=()):
    """A candidate of one-call runs, run q's payload lists[q]; extra_runs are appended as they are."""
    runs = [[call_of(x, head)] for x in lists] + list(extra_runs)
    return (sig_of(runs[0])[:nsig].copy(), 0, runs, minimized)


def split(total, m):
    """m list lengths (head included) that sum to total, no two alike when total allows."""
    base = total // m
    lens = [base + (q - m // 2) * 3 for q in range(m)]
    lens[-1] += total - sum(lens)
    assert sum(lens) == total and min(lens) > NHEAD
    return lens


# ---- the shape of a candidate, from the oracle's per-run (Signal, Cover) ---------
def shape(corpus, cand):
    """fuzzer.go:526-575 followed for which Covers fold; never the product."""
    signal, call, runs, minimized = cand
    cap = sum(int(np.asarray(c).size) for r in runs for c in r)
    infos = [TR.run_info(r, call) for r in runs]
    new = O.signal_diff(corpus, signal)
    lists, counted, status = [], [], TR.OK
    if len(new) == 0:
        status = TR.NO_NEW
    elif minimized:
        for i, info in enumerate(infos):
            if info is not None and len(info[1]):
                lists, counted = [info[1]], [i]
                break
    else:
        a, n = O.canonicalize(new)
        new, skipped = a[:n], False
        for i, info in enumerate(infos):
            if info is None or len(info[0]) == 0:
                if skipped:
                    status = TR.NOT_EXECUTED
                    break
                skipped = True
                continue
            c, k = O.canonicalize(info[0])
            new = O.foreach(O.INTER, new, c[:k])
            if len(new) == 0:
                status = TR.FLAKY
                break
            counted.append(i)
            if len(info[1]):  # an empty Cover changes neither a copy nor a Union
                lists.append(info[1])
    if status != TR.OK:
        lists, counted = [], []
    return Shape(status, tuple(counted), len(lists), sum(len(x) for x in lists),
                 all(bool((x[1:] >= x[:-1]).all()) for x in lists), any(int(x[0]) == S for x in lists), cap, lists)


def route_of(sh, sort_cap=SORT_CAP):
    """k_tr_cover's choice, restated from its header."""
    if sh.status != TR.OK or sh.m == 0:
        return None
    if sh.m == 1:
        return "copied"
    if not sh.ascending or sh.sent_first or sh.total > sh.cap:
        return "foreach"
    return "ranked" if sh.total > sort_cap else "sorted"


def counters(shapes):
    """The five device counters a call over these candidates leaves."""
    out = {"triage_runs_" + r: 0 for r in ROUTES}
    out["triage_runs_wide"] = sum(1 for sh in shapes if sh.status == TR.OK and sh.m >= 1 and not sh.ascending)
    for sh in shapes:
        r = route_of(sh)
        if r is not None:
            out["triage_runs_" + r] += 1
    return out


def _case(name, cand, route, m=None, total=None, pred=None):
    return Case(name, cand, route, m, total, pred)


def _full(sh):
    return sh.total == sh.cap


# ---- cover fold ------------------------------------------------------------------
def _sized(rng, name, route, total, m, **kw):
    lens = split(total, m)
    span = max(total // 2, 4)  # one pool for the m lists: about half of a list's values are in another one too
    return _case(name, fold([asc(rng, n - NHEAD, span) for n in lens], **kw), route, m, total, _full)


def _wide(rng, n0, others, **kw):
    """A list with decreasing steps (a shuffled payload), then ascending ones."""
    w = asc(rng, n0 - NHEAD, n0)
    rng.shuffle(w)
    return fold([w] + [asc(rng, n - NHEAD, n0) for n in others], **kw)


def _tails(rng, sizes, tails):
    return [np.concatenate([asc(rng, n - NHEAD - t, 2 * n), np.full(t, S, U64)]) for n, t in zip(sizes, tails)]


def threshold():
    """nruns = 2: total around triage_runs_sort_cap and around its power-of-two padding."""
    rng = np.random.default_rng(61)
    c = [_sized(rng, "total=%d" % t, r, t, 2) for t, r in
         ((SORT_CAP - 1, "sorted"), (SORT_CAP, "sorted"), (SORT_CAP + 1, "ranked"), (SORT_CAP // 2, "sorted"),
          (SORT_CAP // 2 + 1, "sorted"), (10001, "ranked"))]
    five = np.array([5], U64)
    c.append(_case("total=2", fold([five, five], head=None), "sorted", 2, 2, _full))
    c.append(_case("total=3", fold([five, np.array([5, 9], U64)], head=None), "sorted", 2, 3, _full))
    # a list past exec_cover's fast shape beside a short one
    c.append(_case("long+short", fold([asc(rng, 9000), asc(rng, 200, 18000)]), "ranked", 2, 9264 + 64, _full))
    # m = 1 keeps the sentinel tail, the Unions beside it drop theirs
    t1, t3 = _tails(rng, (300, 500), (1, 3))
    keeps = lambda sh: int(sh.lists[0][-1]) == S  # noqa: E731
    c.append(_case("copy keeps S (skipped run)", fold([t3], extra_runs=[[]]), "copied", 1, 500, keeps))
    c.append(_case("union drops S", fold([t1, t3]), "sorted", 2, 800, lambda sh: all(int(x[-1]) == S for x in sh.lists)))
    c.append(_case("copy keeps S (minimized)", fold([t1, t3], minimized=True), "copied", 1, 300, keeps))
    big = _tails(rng, (5000, 4500), (3, 1))
    c.append(_case("ranked union drops S", fold(big), "ranked", 2, 9500, lambda sh: all(int(x[-1]) == S for x in sh.lists)))
    c.append(_case("wide, one Union", _wide(rng, 700, (400,)), "foreach", 2, 1100, _full))
    return np.zeros(0, U32), c


def three_lists():
    """nruns = 3: sentinel tails on both routes, the rank route's last-element branches, foreach at size."""
    rng = np.random.default_rng(62)
    c = [_sized(rng, "m=3 sorted", "sorted", SORT_CAP, 3), _sized(rng, "m=3 ranked", "ranked", 10000, 3)]
    tails = lambda sh: [int((x == S).sum()) for x in sh.lists] == [0, 1, 3]  # noqa: E731
    c.append(_case("tails 0/1/3 sorted", fold(_tails(rng, (900, 1000, 1100), (0, 1, 3))), "sorted", 3, 3000, tails))
    c.append(_case("tails 0/1/3 ranked", fold(_tails(rng, (3300, 3000, 3100), (0, 1, 3))), "ranked", 3, 9400, tails))
    # a ranked list of 12 x 256 values that ends in a sentinel: its last element is not written
    a, b, d = _tails(rng, (3000, 12 * TB, 3500), (0, 1, 2))
    c.append(_case("ranked, 256 | len, last S", fold([a, b, d]), "ranked", 3, 3000 + 12 * TB + 3500,
                   lambda sh: len(sh.lists[1]) % TB == 0 and int(sh.lists[1][-1]) == S))
    # ... that ends in a duplicate the first list owns at the same count
    top = np.array([0xFFFFFFF0, 0xFFFFFFF0], U64)
    a = np.concatenate([asc(rng, 3000 - NHEAD - 2, 6000), top])
    b = np.concatenate([asc(rng, 12 * TB - NHEAD - 2, 6000), top])
    c.append(_case("ranked, 256 | len, last owned", fold([a, b, asc(rng, 3500 - NHEAD, 6000)]), "ranked", 3,
                   3000 + 12 * TB + 3500,
                   lambda sh: len(sh.lists[1]) % TB == 0 and sh.lists[1][-2:].tolist() == sh.lists[0][-2:].tolist()))
    # foreach: a wide list of about 3,000 values with two ascending ones (two Unions: the result in the first buffer)
    c.append(_case("wide 3000, two Unions", _wide(rng, 3000, (2500, 2000)), "foreach", 3, 7500, _full))
    # ... one Union (a skipped run): the result in the second buffer
    w = _wide(rng, 1500, (1200,), extra_runs=[[]])
    c.append(_case("wide, skipped run, one Union", w, "foreach", 2, 2700, _full))
    # a first list of sentinels only.  Its Signal is S and v = S ^ hash(S); the real lists end in two S lows and so
    # hold v too.  Union drops the first list's values, the later lists come out right
    v = np.array([S ^ O.exec_hash(S)], U32)
    only = lambda n: [call_of(np.full(n, S, U64), None)]  # noqa: E731
    real = lambda n: [call_of(np.concatenate([asc(rng, n - NHEAD - 2, 3000), [S, S]]))]  # noqa: E731
    c.append(_case("S-only first", (v, 0, [only(3), real(900), real(700)], False), "foreach", 3, 1603,
                   lambda sh: sh.sent_first and sh.ascending))
    # ... twice: the Union of the two is empty, so the third Cover is copied, tail and all (the n == 0 rule)
    c.append(_case("S-only twice, then a copy", (v, 0, [only(3), only(2), real(800)], False), "foreach", 3, 805,
                   lambda sh: sh.sent_first and sh.ascending))
    c.append(_case("copy", fold([asc(rng, 300), asc(rng, 900), asc(rng, 100)], minimized=True), "copied", 1, 364))
    return np.zeros(0, U32), c


def _counts(rng, n, pool, x, counts, extra=None):
    """Five payloads of about n values of one pool, the value x at counts[q] in list q."""
    out = []
    for q, k in enumerate(counts):
        base = asc(rng, n, pool)
        base = base[base != x]
        parts = [base, np.full(k, x, U64)]
        if extra is not None:
            parts.append(extra(q))
        out.append(np.sort(np.concatenate(parts)))
    return out


def five_lists():
    """nruns = 5: repeats at different counts per list, on both routes."""
    rng = np.random.default_rng(63)
    c = [_sized(rng, "m=5 sorted", "sorted", SORT_CAP, 5), _sized(rng, "m=5 ranked", "ranked", 10000, 5)]
    x, top = 3000, 0xFFFFFFFE

    def cnt(sh):
        return [int((l == x).sum()) for l in sh.lists] == [1, 3, 2, 0, 3]

    for route, n in (("sorted", 400), ("ranked", 2400)):
        # the largest value below the sentinel, repeated at other counts; sentinels behind it in two lists
        ends = lambda q: np.concatenate([np.full((2, 0, 1, 3, 1)[q], top, U64), np.full(q % 3, S, U64)])  # noqa: E731
        ls = _counts(rng, n, 2 * n, x, (1, 3, 2, 0, 3), ends)
        c.append(_case("counts 1/3/2/0/3 " + route, fold(ls), route, 5, None,
                       lambda sh: cnt(sh) and [int((l == top).sum()) for l in sh.lists] == [2, 0, 1, 3, 1]))
        # one value 1,000 times; a run of equal values across index 256 of its list (head included)
        thousand = np.full(1000, 2500, U64)
        cross = asc(rng, n, 2 * n)
        cross[TB - NHEAD - 10:TB - NHEAD + 10] = cross[TB - NHEAD - 10]
        ls = [asc(rng, n, 2 * n), thousand, cross, np.concatenate([np.full(40, 2500, U64), asc(rng, n, 2 * n, lo=2500)]),
              asc(rng, n, 2 * n)]
        c.append(_case("1000 of one value, a run over 256, " + route, fold(ls), route, 5, None,
                       lambda sh: int((sh.lists[1] == 2500).sum()) == 1000
                       and len(set(sh.lists[2][TB - 10:TB + 10].tolist())) == 1 and _full(sh)))
        # the smallest value repeated, at other counts per list: no head, every run starts with low 5
        ls = [np.concatenate([np.full(k, 5, U64), asc(rng, n, 2 * n)]) for k in (2, 3, 1, 4, 2)]
        c.append(_case("smallest repeated, " + route, fold(ls, head=None), route, 5, None,
                       lambda sh: [int((l == 5).sum()) for l in sh.lists] == [2, 3, 1, 4, 2] and _full(sh)))
    c.append(_case("copy", fold([asc(rng, 50)] * 5, minimized=True), "copied", 1, 114))
    c.append(_case("wide, four Unions", _wide(rng, 500, (300, 400, 200, 100)), "foreach", 5, 1500, _full))
    return np.zeros(0, U32), c


def eight_lists():
    """nruns = 8 (kTrMaxRuns), every run counted: bit 31 of the state word."""
    rng = np.random.default_rng(64)
    c = [_sized(rng, "m=8 sorted", "sorted", SORT_CAP, 8), _sized(rng, "m=8 ranked", "ranked", 10000, 8)]
    for route, n in (("sorted", SORT_CAP // 8), ("ranked", 1300)):
        p = n - NHEAD
        one = asc(rng, p)
        c.append(_case("identical, " + route, fold([one] * 8), route, 8, 8 * n, _full))
        lo = 2048 + 3 * p * np.arange(8)
        c.append(_case("disjoint, " + route, fold([asc(rng, p, 2 * p, lo=int(lo[q])) for q in range(8)]), route, 8, 8 * n,
                       lambda sh: all(int(a[-1]) < int(b[NHEAD]) for a, b in zip(sh.lists, sh.lists[1:]))))
        every = 2048 + np.arange(8 * p, dtype=U64)
        c.append(_case("interleaved, " + route, fold([every[q::8] for q in range(8)]), route, 8, 8 * n, _full))
    c.append(_case("copy", fold([asc(rng, 70)] * 8, minimized=True), "copied", 1, 134))
    c.append(_case("wide, seven Unions", _wide(rng, 300, (200,) * 7), "foreach", 8, 1700, _full))
    return np.zeros(0, U32), c


def full_slots():
    """nruns = 2, every PC of a candidate distinct within its call and one call per execution: total == cap, every
    slot of the two buffers exactly full, another route in the next slot."""
    rng = np.random.default_rng(65)
    uniq = lambda n: np.sort(rng.choice(1 << 20, size=n - NHEAD, replace=False) + 2048).astype(U64)  # noqa: E731

    def wide(n0, n1):
        w = uniq(n0)
        rng.shuffle(w)
        return fold([w, uniq(n1)])

    c = [_case("ranked", fold([uniq(4500), uniq(4000)]), "ranked", 2, 8500, _full),
         _case("foreach", wide(900, 1100), "foreach", 2, 2000, _full),
         _case("copy", fold([uniq(1500)], minimized=True, extra_runs=[[]]), "copied", 1, 1500, _full),
         _case("sorted", fold([uniq(4096), uniq(4096)]), "sorted", 2, SORT_CAP, _full),
         _case("ranked again", fold([uniq(8000), uniq(300)]), "ranked", 2, 8300, _full),
         _case("foreach again", wide(256, 512), "foreach", 2, 768, _full)]
    return np.zeros(0, U32), c


# ---- the run loop ----------------------------------------------------------------
def run_loop(nruns):
    """inp.call = 1 of two-call executions, run i's Cover of its own length; every exit of the loop at the first
    and the last runs."""
    rng = np.random.default_rng(66 + nruns)
    N = nruns
    junk = TEXT + 16 * rng.choice(1 << 12, size=5, replace=False).astype(U64)
    T = [call_of(asc(rng, 40 + 13 * i, 400)) for i in range(N)]
    big = call_of(asc(rng, 200, 400))
    R = [[junk, t] for t in T]
    D = [junk, TEXT + 16 * ((1 << 13) + rng.choice(1 << 12, size=80, replace=False).astype(U64))]  # other edges altogether
    absent, never, empty = [junk], [], [junk, np.zeros(0, U64)]
    nosig = [big, big]  # the call's edges are its program's earlier call's: a Cover, the largest, and no Signal
    sig = sig_of(R[0], 1)[:40].copy()
    corpus = sig[:5].copy()
    last = N - 1

    def runs(**at):
        return [at.get("r%d" % i, R[i]) for i in range(N)]

    def st(status, counted=None):
        return lambda sh: sh.status == status and (counted is None or sh.counted == tuple(counted))

    allr = list(range(N))
    folded = lambda m: "copied" if m == 1 else "sorted"  # noqa: E731
    c = [_case("every run counted", (sig, 1, R, False), folded(N), N, None, st(TR.OK, allr)),
         _case("not executed at the last run only", (sig, 1, runs(**{"r%d" % last: absent}), False), folded(N - 1), N - 1,
               None, st(TR.OK, allr[:-1])),
         _case("not executed at run 0 only", (sig, 1, runs(r0=never), False), folded(N - 1), N - 1, None, st(TR.OK, allr[1:])),
         _case("not executed at the first and the last run", (sig, 1, runs(**{"r0": never, "r%d" % last: absent}), False),
               None, None, None, st(TR.NOT_EXECUTED)),
         _case("not executed at the last two runs", (sig, 1, runs(**{"r%d" % (last - 1): empty, "r%d" % last: never}), False),
               None, None, None, st(TR.NOT_EXECUTED)),
         _case("flaky first at the last run", (sig, 1, runs(**{"r%d" % last: D}), False), None, None, None, st(TR.FLAKY)),
         _case("flaky at run 0", (sig, 1, runs(r0=D), False), None, None, None, st(TR.FLAKY)),
         _case("minimized, the cover at run 0", (sig, 1, R, True), "copied", 1, T[0].size, st(TR.OK, [0])),
         _case("minimized, the first cover at the last run",
               (sig, 1, [absent, empty, never, absent, empty, never, absent][:last] + [R[last]], True), "copied", 1,
               T[last].size, st(TR.OK, [last])),
         _case("minimized, no cover anywhere", (sig, 1, [absent, empty, never, absent, empty, never, absent, empty][:N], True),
               None, 0, 0, st(TR.OK, [])),
         _case("nothing new", (corpus, 1, R, False), None, None, None, st(TR.NO_NEW)),
         _case("nothing new, minimized", (corpus[:3], 1, R, True), None, None, None, st(TR.NO_NEW)),
         # the run without Signal has the largest Cover, and it does not fold
         _case("the skipped run has the largest cover", (sig, 1, runs(**{"r%d" % (N // 2): nosig}), False), folded(N - 1),
               N - 1, sum(t.size for i, t in enumerate(T) if i != N // 2),
               lambda sh: sh.counted == tuple(i for i in allr if i != N // 2)
               and TR.run_info(nosig, 1)[1].size == big.size > max(t.size for t in T) and TR.run_info(nosig, 1)[0].size == 0),
         _case("every run counted, again", (sig, 1, R, False), folded(N), N, None, st(TR.OK, allr))]
    return corpus, c


# ---- newSignal across tinput_chunk -----------------------------------------------
@functools.lru_cache(maxsize=None)
def _long_trace():
    """20,000 distinct kernel-text PCs, their 20,000 signals, and the trace with about 1 % of its PCs removed."""
    rng = np.random.default_rng(70)
    pcs = TEXT + 16 * rng.choice(1 << 20, size=20000, replace=False).astype(U64)
    sig = sig_of([pcs])
    gone = np.zeros(pcs.size, bool)
    gone[rng.choice(np.arange(1, pcs.size), size=200, replace=False)] = True
    short = pcs[~gone]
    return pcs, sig, short, O.canonicalize(sig_of([short]))


def _chunk_case(name, K, pick):
    """inp.signal: the K smallest signals of the trace.  Run 1 drops the edges beside the removed PCs; run 2 holds
    the consecutive pairs (pc[j - 1], pc[j]) of the signals pick(new after run 1) names, and so those signals and junk."""
    pcs, sig, short, (c1, n1) = _long_trace()
    inp = np.sort(sig)[:K]
    new1 = O.foreach(O.INTER, inp, c1[:n1])
    at = {int(s): j for j, s in enumerate(sig)}
    lost = np.setdiff1d(inp, new1)
    want = pick(new1, lost)
    js = np.array([at[int(s)] for s in want if at[int(s)] > 0], dtype=np.int64)
    pairs = np.stack([pcs[js - 1], pcs[js]], axis=1).reshape(-1)
    return name, (inp, 0, [[pcs], [short], [pairs]], False), new1, want


def chunk_batches():
    """Two batches (nruns = 3) of candidates over one 20,000-PC trace; their covers are ranked."""
    C = CHUNK
    specs = [("K=2C+1, chunk 0 empties", 2 * C + 1, lambda new, lost: np.concatenate([new[C:C + 290], new[-3:]])),
             ("K=C-1", C - 1, lambda new, lost: np.concatenate([new[:3], new[1000:1040], new[-1:]])),
             ("K=2C+1, last of chunk 0 and first of chunk 1", 2 * C + 1, lambda new, lost: new[C - 1:C + 1]),
             ("K=C, nothing kept", C, lambda new, lost: lost[:50]),
             ("K=C+1", C + 1, lambda new, lost: np.concatenate([new[:1], new[TB - 1:TB + 1], new[-2:]]))]
    made = [_chunk_case(*s) for s in specs]
    out = []
    for part in (made[:2], made[2:]):
        cases = []
        for name, cand, new1, want in part:
            flaky = "nothing" in name
            cases.append(_case(name, cand, None if flaky else "ranked", None if flaky else 3, None,
                               (lambda sh: sh.status == TR.FLAKY) if flaky else (lambda sh: sh.status == TR.OK)))
        out.append((np.zeros(0, U32), cases, [(new1, want) for _, _, new1, want in part]))
    return out


# ---- inp.signal lengths ------------------------------------------------------------
def signal_lengths():
    """nruns = 2: inp.signal of 255, 256, 257 and 513 values (k_tin_diff's rounds of 256) with duplicates and
    sentinels, against a corpus that holds every second signal."""
    rng = np.random.default_rng(71)
    trace = TEXT + 16 * rng.choice(1 << 16, size=700, replace=False).astype(U64)
    sig = sig_of([trace])
    corpus = sig[::2].copy()
    cases = []
    for L in (255, 256, 257, 513):
        v = sig[:L].copy()
        v[[7, L - 1, L // 3]] = S                  # sentinels, one as the last value
        v[[3, L - 2, min(TB, L - 3)]] = v[[1, 1, 9]]   # duplicates, one at index 256 where there is one
        cases.append(_case("len=%d" % L, (v, 0, [[trace], [trace]], False), "sorted", 2, 1400,
                           lambda sh, L=L: sh.status == TR.OK))
    return corpus, cases


@functools.lru_cache(maxsize=None)
def batch(name):
    """(corpus values, cases, the oracle's result, the cases' shapes) of a named batch."""
    if name.startswith("run_loop"):
        corpus, cases = run_loop(int(name[8:]))
    elif name.startswith("chunk"):
        corpus, cases, _ = chunk_batches()[int(name[5:])]
    else:
        corpus, cases = globals()[name]()
    oc = O.OSet(corpus)
    cands = [c.cand for c in cases]
    return corpus, cases, TR.batch(oc, cands), [shape(oc, x) for x in cands]


BATCHES = ("threshold", "three_lists", "five_lists", "eight_lists", "full_slots", "run_loop2", "run_loop4", "run_loop8",
           "chunk0", "chunk1", "signal_lengths")
