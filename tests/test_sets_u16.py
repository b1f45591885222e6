"""The late pass 2 of a split bucket launch (option flag_skip_u16; sg_part.h
P2Late, sg_partition.hip k_p2_scatter16, sg_bucket.hip k_bucket_sets<true>,
k_late_bounds, buckets_one).  The slices of the bucket list's first window are
scattered before the first bucket launch, in 4-byte entries; the other slices
after the flag summary -- in 2-byte entries, the 16-bit signal alone, when
every record of the launch is flagged, else in 4-byte entries as ever.

What can go wrong: the window's slice boundary (a chunk scattered twice or
never, a bucket read in the other width); the device's decision (the 2-byte
form although a record is unflagged: its flag stays 0); a 2-byte run that
starts or ends at an odd position or away from a multiple of 8 (a neighbour's
entry taken, an own entry dropped); the one-entry second chunk; 2-byte entries
written over 4-byte entries that are still to be read (the rest of the
boundary slice); the group that a 2-byte entry no longer carries.  So every
case is bit-exact for the flags and both exported sets against
oracle/pyoracle.py (syz-fuzzer/fuzzer.go:645-693) and against the same call
with flag_skip_u16 0, and the counters flag_skip_used, flag_skip_all_flagged
and flag_skip_u16 are pinned to what the batch predicts: the first window is
the first nl >> k of the batch's nl distinct buckets, a signal's first owner
does not depend on other signals, so the flags after the first launch are the
oracle's over the entries of those buckets (tests/test_all_flagged.py), and a
launch is all-flagged iff they are all set.  Each case also asserts, on the
CPU, the structure it is named after."""
import numpy as np
import pytest

from oracle import pyoracle as O
from tests.test_flag_skip import GROUP, R, bsig

pytestmark = pytest.mark.gpu

K = 3  # flag_skip_split: the first launch takes the first 1 / 8 of the bucket list
PT = 16384  # kPT: entries per pass-2 chunk


@pytest.fixture(scope="module")
def C(ctx):
    from syzkaller_amd import cover

    return cover


def bucket_of(s):
    s = np.asarray(s).astype(np.uint32)
    return (((s >> 16) & 255) << 8) | ((s >> 8) & 255)


def bkt(d, f):
    return (d << 8) | f


def arrays(recs):
    lens = np.array([len(r) for r in recs], np.int64)
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    vals = np.concatenate([np.asarray(r, np.uint32) for r in recs]) if lens.sum() else np.empty(0, np.uint32)
    return vals.astype(np.uint32), off


def oset(values):
    values = np.asarray(values, np.uint32)
    return O.OSet(values if values.size else None)


def predict(vals, off, m0, k, mlr=None, newset=True):
    """The oracle's flags and sets, and per launch (record slice with
    entries) whether the first window leaves every record flagged."""
    nrec = off.size - 1
    mlr = mlr or nrec
    om, on = oset(m0), (O.OSet() if newset else None)
    flags, allf = np.zeros(nrec, np.uint8), []
    for r0 in range(0, nrec, mlr):
        r1 = min(r0 + mlr, nrec)
        v = vals[int(off[r0]): int(off[r1])]
        o = (off[r0: r1 + 1] - off[r0]).astype(np.uint64)
        if v.size == 0:
            continue
        bk = bucket_of(v)
        lst = np.unique(bk)
        in_a = np.isin(bk, lst[: lst.size >> k])
        rec = np.repeat(np.arange(r1 - r0), np.diff(o).astype(np.int64))
        off_a = np.concatenate([[0], np.cumsum(np.bincount(rec[in_a], minlength=r1 - r0))]).astype(np.uint64)
        after_a = O.triage_flags_only(oset(om.export()), None, v[in_a], off_a)
        allf.append(bool(after_a.all()))
        flags[r0:r1] = O.triage_flags_only(om, on, v, o)
    return flags, om, on, allf


def late_slice(vals, k):
    """D: the slice after the first window's last bucket (0: the window is empty)."""
    lst = np.unique(bucket_of(vals))
    na = lst.size >> k
    return (int(lst[na - 1]) >> 8) + 1 if na else 0


def positions(vals):
    """Every distinct bucket's [lo, hi) in the pass-2 output of a one-group
    batch: runs laid out [b1][slice]."""
    bk = bucket_of(vals)
    key = ((bk & 255).astype(np.int64) << 8) | (bk >> 8)
    ks, cnt = np.unique(key, return_counts=True)
    hi = np.cumsum(cnt)
    return {int(((x & 255) << 8) | (x >> 8)): (int(h - c), int(h)) for x, c, h in zip(ks, cnt, hi)}


def run(C, ctx, ctx_option, recs, want_allf, m0=(), k=K, mlr=None, newset=True, want_flags=None):
    """The batch with flag_skip 1 and flag_skip_u16 0 and -1 (on with the
    split) on fresh sets: both equal the oracle and each other, and the
    counters rise by what the batch predicts.  want_allf: the all-flagged
    answer per launch that the case is built for."""
    vals, off = arrays(recs)
    m0 = np.asarray(m0, np.uint32)
    exp, om, on, allf = predict(vals, off, m0, k, mlr, newset)
    assert allf == list(want_allf), allf  # the construction itself
    if want_flags is not None:
        assert np.array_equal(exp, want_flags)
    ctx_option(ctx, "m0_filter", 0)  # the partitioned path
    ctx_option(ctx, "flag_skip_split", k)
    ctx_option(ctx, "flag_skip", 1)
    if mlr:
        ctx_option(ctx, "max_launch_records", mlr)
    got = {}
    for u16 in (0, -1):
        ctx_option(ctx, "flag_skip_u16", u16)
        c0 = [ctx.counter(n) for n in ("flag_skip_used", "flag_skip_all_flagged", "flag_skip_u16")]
        ms, ns = C.SignalSet(ctx), (C.SignalSet(ctx) if newset else None)
        if m0.size:
            C.SignalAdd(ms, m0)
        f, _, _ = C.triage_batch(ms, ns, vals, off, want_diff=False, ctx=ctx)
        got[u16] = (f, ms.export(), ns.export() if newset else None)
        if newset:
            ns.close()
        ms.close()
        d = [ctx.counter(n) - c for n, c in zip(("flag_skip_used", "flag_skip_all_flagged", "flag_skip_u16"), c0)]
        print("flag_skip_u16", u16, "launches", len(allf), "counters", d)
        assert np.array_equal(f, exp), (u16, np.flatnonzero(f != exp)[:10])
        assert np.array_equal(got[u16][1], om.export()), u16
        if newset:
            assert np.array_equal(got[u16][2], on.export()), u16
        assert d == [len(allf), sum(allf), sum(allf) if u16 else 0], (u16, d, allf)
    assert np.array_equal(got[0][0], got[-1][0]) and np.array_equal(got[0][1], got[-1][1])
    if newset:
        assert np.array_equal(got[0][2], got[-1][2])
    return vals, off, on


def buckets(nA, rng, d_last=9):
    """nA first-window buckets in slices 0 .. d_last (bucket 0 and one in slice
    d_last among them) and 7 nA others: a few in the rest of slice d_last (read
    in 4-byte entries either way), the others in later slices, bucket 65535
    among them."""
    last = bkt(d_last, 100)
    a = np.sort(rng.permutation(np.arange(1, last))[: nA - 2])
    A = np.concatenate([[0], a, [last]]).astype(np.int64)
    nB = 7 * nA
    rest = min(3, nB - 1)
    b1 = np.sort(rng.permutation(np.arange(last + 1, bkt(d_last, 255) + 1))[:rest])
    b2 = np.sort(rng.permutation(np.arange(bkt(d_last + 1, 0), 65535))[: nB - rest - 1])
    B = np.concatenate([b1, b2, [65535]]).astype(np.int64)
    assert np.unique(np.concatenate([A, B])).size == 8 * nA and A.max() < B.min()
    return A, B


def batch(nrec, A, B, rng):
    """Record r owns one signal of its own in first-window bucket A[r mod nA]
    and one in B[r mod nB]; the buckets of B that no record reaches so get an
    entry of record 0, 1, ..."""
    nA, nB = len(A), len(B)
    lo = rng.permutation(65536)
    assert -(-nrec // nA) + -(-nrec // nB) + 1 < 65536
    r = np.arange(nrec)
    recs = np.stack([bsig(A[r % nA], lo[r // nA]), bsig(B[r % nB], lo[65535 - r // nB])], axis=1).tolist()
    for j in range(nrec, nB):
        recs[(j - nrec) % nrec].append(int(bsig(B[j], lo[65535])))
    if nrec < nA:  # (the first window's other buckets: non-empty too)
        for j in range(nrec, nA):
            recs[(j - nrec) % nrec].append(int(bsig(A[j], lo[0])))
    return recs


# ---- 1. record-count edges --------------------------------------------------------------------
@pytest.mark.parametrize("nrec", [1, R - 1, R, R + 1])
def test_record_count_edges(C, ctx, ctx_option, nrec):
    """All records flagged by the first window; R + 1 has a partial last summary block."""
    rng = np.random.default_rng(7100 + nrec)
    A, B = buckets(4, rng)
    recs = batch(nrec, A, B, rng)
    vals, _, _ = run(C, ctx, ctx_option, recs, [True], want_flags=np.ones(nrec, np.uint8))
    assert vals.size < 3 * (R + 1) and late_slice(vals, K) == 10


# ---- 2. run alignment -------------------------------------------------------------------------
def test_run_alignment(C, ctx, ctx_option):
    """2-byte buckets starting at every position mod 8 with 1, 7, 8 and 9
    entries each, empty buckets between them, and bucket 65535 ending at the
    buffer's last entry."""
    rng = np.random.default_rng(7200)
    nrec = 600
    A, B = buckets(60, rng)
    recs = batch(nrec, A, B, rng)
    want_len = rng.choice([1, 7, 8, 9], size=len(B))
    vals0, _ = arrays(recs)
    have = np.bincount(bucket_of(vals0), minlength=65536)
    for b, w in zip(B, want_len):
        more = int(w) - int(have[b])
        if more > 0:  # distinct signals of the bucket, to records in turn
            for i, s in enumerate(bsig(b, 1000 + np.arange(more))):
                recs[(int(b) + i) % nrec].append(int(s))
    vals, _ = arrays(recs)
    pos, D = positions(vals), late_slice(vals, K)
    assert D == 10
    seen = {(lo % 8, hi - lo) for b, (lo, hi) in pos.items() if (b >> 8) >= D}
    assert {(m, n) for m in range(8) for n in (1, 7, 8, 9)} <= seen, sorted(seen)
    assert pos[65535][1] == vals.size  # the last bucket ends the buffer
    assert len(pos) < 65536 // 8  # (most buckets are empty)
    run(C, ctx, ctx_option, recs, [True], want_flags=np.ones(nrec, np.uint8))


# ---- 3. chunk edges ---------------------------------------------------------------------------
@pytest.mark.parametrize("n", [PT - 1, PT, PT + 1])
def test_chunk_edges(C, ctx, ctx_option, n):
    """Slice 200 holds exactly n entries of one record group: a chunk one short
    of full, a full one (the unpredicated path), and a full one with a
    one-entry second chunk."""
    rng = np.random.default_rng(7300 + n)
    nrec, nA = 2048, 32
    A = np.sort(rng.permutation(bkt(10, 0))[:nA]).astype(np.int64)
    B = bkt(200, np.sort(rng.permutation(256)[: 7 * nA])).astype(np.int64)
    lo = rng.permutation(65536)
    recs = [[int(bsig(A[r % nA], lo[r // nA]))] for r in range(nrec)]
    b = np.concatenate([B, B[rng.integers(0, B.size, n - B.size)]])  # every bucket of B non-empty
    s = bsig(b, rng.integers(0, 65536, n))
    for i, x in enumerate(s):
        recs[i % nrec].append(int(x))
    vals, _ = arrays(recs)
    assert int(((vals >> 16) & 255 == 200).sum()) == n and late_slice(vals, K) <= 10
    run(C, ctx, ctx_option, recs, [True], want_flags=np.ones(nrec, np.uint8))


# ---- 4. the window boundary -------------------------------------------------------------------
def test_slices_31_and_32(C, ctx, ctx_option):
    """Entries only in slices 31 and 32: two buckets of slice 31 are the first
    window, fourteen of slice 32 the 2-byte window."""
    rng = np.random.default_rng(7400)
    A = np.array([bkt(31, 0), bkt(31, 255)])
    B = bkt(32, np.sort(rng.permutation(256)[:14]))
    recs = batch(300, A, B, rng)
    vals, _, _ = run(C, ctx, ctx_option, recs, [True])
    assert late_slice(vals, K) == 32 and set(np.unique((vals >> 16) & 255)) == {31, 32}


def test_first_window_empty(C, ctx, ctx_option):
    """Five non-empty buckets: 5 >> 3 = 0, nothing is flagged before the
    summary, and the 4-byte form scatters every chunk after it."""
    rng = np.random.default_rng(7410)
    bs = np.array([bkt(0, 0), bkt(31, 7), bkt(32, 7), bkt(200, 9), 65535])
    recs = [[int(bsig(bs[r % 5], r))] for r in range(R + 100)]
    vals, _, _ = run(C, ctx, ctx_option, recs, [False], want_flags=np.ones(R + 100, np.uint8))
    assert late_slice(vals, K) == 0


def test_late_window_empty(C, ctx, ctx_option):
    """Every bucket in slice 7: the slices after the first window hold nothing,
    and the rest of the boundary slice is read in 4-byte entries."""
    rng = np.random.default_rng(7420)
    f = np.sort(rng.permutation(256)[:16])
    recs = batch(500, bkt(7, f[:2]), bkt(7, f[2:]), rng)
    vals, _, _ = run(C, ctx, ctx_option, recs, [True])
    assert late_slice(vals, K) == 8 and set(np.unique((vals >> 16) & 255)) == {7}


# ---- 5. fallback: one record that the first window cannot flag --------------------------------
def test_record_without_entries(C, ctx, ctx_option):
    rng = np.random.default_rng(7500)
    A, B = buckets(8, rng)
    recs = batch(R + 50, A, B, rng)
    recs.insert(R - 1, [])
    want = np.ones(R + 51, np.uint8)
    want[R - 1] = 0
    run(C, ctx, ctx_option, recs, [False], want_flags=want)


def test_record_all_in_max(C, ctx, ctx_option):
    rng = np.random.default_rng(7510)
    A, B = buckets(8, rng)
    recs = batch(R + 50, A, B, rng)
    m0 = np.array(recs[R], np.uint32)
    want = np.ones(R + 50, np.uint8)
    want[R] = 0
    run(C, ctx, ctx_option, recs, [False], m0=m0, want_flags=want)


# ---- 6. duplicates and known bits -------------------------------------------------------------
def test_one_signal_many_times(C, ctx, ctx_option):
    """A 2-byte bucket whose 777 entries are all one signal."""
    rng = np.random.default_rng(7600)
    A, B = buckets(8, rng)
    recs = batch(800, A, B, rng)
    b = int(B[len(B) // 2])
    recs = [[x for x in r if bucket_of(x) != b] for r in recs]
    s = int(bsig(b, 0xABCD))
    for r in range(777):
        recs[r].append(s)
    vals, _, on = run(C, ctx, ctx_option, recs, [True])
    assert late_slice(vals, K) <= b >> 8
    assert np.array_equal(np.unique(vals[bucket_of(vals) == b]), [s]) and s in on.export()


def test_bucket_all_in_max(C, ctx, ctx_option):
    """A 2-byte bucket whose entries are all in maxSignal already: none of its
    words is written, and newSignal gets nothing of it."""
    rng = np.random.default_rng(7610)
    A, B = buckets(8, rng)
    recs = batch(800, A, B, rng)
    b = int(B[len(B) // 2])
    recs = [[x for x in r if bucket_of(x) != b] for r in recs]
    known = bsig(b, rng.permutation(65536)[:300])
    for i, s in enumerate(np.concatenate([known, known[:100]])):
        recs[i % 800].append(int(s))
    vals, _, on = run(C, ctx, ctx_option, recs, [True], m0=known)
    assert late_slice(vals, K) <= b >> 8
    assert not (bucket_of(on.export()) == b).any()


# ---- 7. two record groups ---------------------------------------------------------------------
def test_two_groups(C, ctx, ctx_option):
    """More than 65,536 records: the 2-byte entries carry no group, the set
    update needs none."""
    rng = np.random.default_rng(7700)
    nrec = GROUP + 300
    A, B = buckets(64, rng)
    recs = batch(nrec, A, B, rng)
    shared = int(bsig(int(B[10]), 4242))  # one signal in records of both groups
    for r in (5, GROUP - 1, GROUP, nrec - 1):
        recs[r].append(shared)
    run(C, ctx, ctx_option, recs, [True], want_flags=np.ones(nrec, np.uint8))


# ---- 8. record slices: the decision is each launch's own --------------------------------------
def test_record_slices(C, ctx, ctx_option):
    """max_launch_records 3000 over 6000 records: the first launch is
    all-flagged, a record of the second owns nothing in its first window."""
    rng = np.random.default_rng(7800)
    A, B = buckets(8, rng)
    recs = batch(6000, A, B, rng)
    recs[4000] = recs[4000][1:]  # its first-window signal dropped
    run(C, ctx, ctx_option, recs, [True, False], mlr=3000, want_flags=np.ones(6000, np.uint8))


# ---- 9. no newSignal set ----------------------------------------------------------------------
def test_without_newsig(C, ctx, ctx_option):
    rng = np.random.default_rng(7900)
    A, B = buckets(8, rng)
    run(C, ctx, ctx_option, batch(R + 7, A, B, rng), [True], newset=False)


# ---- 10. the option ---------------------------------------------------------------------------
def test_option_forces_the_split(C, ctx, ctx_option):
    """flag_skip_u16 1 splits a launch that flag_skip 0 would not: -1, 0, 1 are
    its values, anything else is refused."""
    from syzkaller_amd._lib import SG_EINVAL, SyzSigError

    rng = np.random.default_rng(7950)
    A, B = buckets(8, rng)
    vals, off = arrays(batch(R + 7, A, B, rng))
    exp, om, on, allf = predict(vals, off, np.empty(0, np.uint32), K)
    assert allf == [True]
    for bad in (-2, 2):
        with pytest.raises(SyzSigError) as e:
            ctx.set_option("flag_skip_u16", bad)
        assert e.value.rc == SG_EINVAL
    ctx_option(ctx, "m0_filter", 0)
    ctx_option(ctx, "flag_skip_split", K)
    ctx_option(ctx, "flag_skip", 0)
    ctx_option(ctx, "flag_skip_u16", 1)
    assert ctx.get_option("flag_skip_u16") == 1
    c0 = [ctx.counter(n) for n in ("flag_skip_used", "flag_skip_u16")]
    ms, ns = C.SignalSet(ctx), C.SignalSet(ctx)
    f, _, _ = C.triage_batch(ms, ns, vals, off, want_diff=False, ctx=ctx)
    assert np.array_equal(f, exp)
    assert np.array_equal(ms.export(), om.export()) and np.array_equal(ns.export(), on.export())
    ns.close()
    ms.close()
    assert [ctx.counter(n) - c for n, c in zip(("flag_skip_used", "flag_skip_u16"), c0)] == [1, 1]
