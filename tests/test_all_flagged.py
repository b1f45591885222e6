"""The map-free second phase of a split bucket launch (sg_bucket.hip
k_bucket_sets, buckets_one; counter flag_skip_all_flagged).  When the summary
between the two launches finds every record of the launch flagged, the rest of
the bucket list needs only its set update: each bucket's entries that are not
in maxSignal ORed into maxSignal and newSignal, without the owner map.  The
decision is the device's: the summary's full-block count against the launch's
ceil(nrec / 4096) blocks.  One record short of that and the regular second
launch runs unchanged.

What can go wrong: a launch taken as all-flagged although a record is not
(that record's flag stays 0 where the oracle has 1); a set update that loses,
invents or misplaces a bit (first and last word of a slice, a word shared with
maxSignal, an entry outside the bucket's range); the window of the list; both
forms of the second phase running, or neither.  So every case is bit-exact
against oracle/pyoracle.py (syz-fuzzer/fuzzer.go:645-693) for the flags, the
maxSignal export and the newSignal export, with flag_skip 0 and 1 and m0_filter
0, and pins flag_skip_all_flagged.

The batches are tests/test_flag_skip.py's: record r owns one signal in phase-A
bucket r mod nA and one in phase-B bucket r mod nB."""
import ctypes

import numpy as np
import pytest

from oracle import pyoracle as O
from tests.test_flag_skip import GROUP, N2G, R, Batch, _traces, bsig, nblocks

pytestmark = pytest.mark.gpu

ALLF = "flag_skip_all_flagged"


@pytest.fixture(scope="module")
def C(ctx):
    from syzkaller_amd import cover

    return cover


def run(C, ctx, ctx_option, bt, allf, full=None, used=1, flags=None, newset=True):
    """The batch with flag_skip 0 and 1 on fresh sets: both equal the oracle.
    The forced-on run split `used` launches, `allf` of them ran their second
    phase map-free, and its last one found `full` blocks."""
    vals, off = bt.arrays()
    om, on = O.OSet(bt.m0 if bt.m0.size else None), (O.OSet() if newset else None)
    exp = O.triage_flags_only(om, on, vals, off)
    if flags is not None:
        assert np.array_equal(exp, flags)  # the construction itself
    ctx_option(ctx, "m0_filter", 0)
    ctx_option(ctx, "flag_skip_split", bt.k)
    for fs in (0, 1):
        ctx_option(ctx, "flag_skip", fs)
        u0, a0 = ctx.counter("flag_skip_used"), ctx.counter(ALLF)
        ms, ns = C.SignalSet(ctx), (C.SignalSet(ctx) if newset else None)
        if bt.m0.size:
            C.SignalAdd(ms, bt.m0)
        got, _, _ = C.triage_batch(ms, ns, vals, off, want_diff=False, ctx=ctx)
        assert np.array_equal(got, exp), (fs, np.flatnonzero(got != exp)[:10])
        assert np.array_equal(ms.export(), om.export()), fs
        if newset:
            assert np.array_equal(ns.export(), on.export()), fs
            ns.close()
        ms.close()
        du, da = ctx.counter("flag_skip_used") - u0, ctx.counter(ALLF) - a0
        assert (du, da) == ((used, allf) if fs else (0, 0)), (fs, du, da)
        if fs and full is not None:
            assert ctx.counter("flag_skip_full_blocks") == full
    return exp


def bucket_of(s):
    s = np.asarray(s).astype(np.uint32)
    return (((s >> 16) & 255) << 8) | ((s >> 8) & 255)


def add_extra(bt, rec, sigs):
    e = np.asarray(sigs, np.uint32).ravel()
    bt.extra[rec] = np.concatenate([bt.extra[rec], e]) if rec in bt.extra else e


def edge_contents(bt):
    """Into the phase-B buckets of an all-flagged batch: the window's first
    bucket and bucket 65535 with their signal numbers 0 and 65535 (first and
    last slice word, bits 0 and 31); candidates in words that maxSignal holds
    other bits of; entries that hit maxSignal; one signal in records of both
    groups."""
    first, last = int(bt.bB[0]), int(bt.bB[-1])
    assert last == 65535 and first > int(bt.bA[-1])
    for i, b in enumerate((first, last)):
        add_extra(bt, 10 + i, bsig(b, [0, 65535]))
        add_extra(bt, GROUP + 10 + i, bsig(b, [65535, 0, 31, 32]))
    # words 100 and 2047 of the first bucket, word 0 of the last: some bits in maxSignal, others candidates
    inmax = np.concatenate([bsig(first, [3200 + 5, 3200 + 31, 65535 - 7]), bsig(last, [1, 30])])
    bt.m0 = np.concatenate([bt.m0, inmax])
    add_extra(bt, 20, bsig(first, [3200 + 4, 3200 + 6, 3200 + 30, 65535 - 6]))
    add_extra(bt, N2G - 1, bsig(last, [2, 29]))
    # entries that hit maxSignal, beside candidates of the same record
    add_extra(bt, 21, inmax)
    add_extra(bt, GROUP + 21, inmax[::-1])
    # one signal held by several records of both groups
    shared = bsig(int(bt.bB[len(bt.bB) // 2]), [12345])
    for r in (7, R - 1, R, GROUP - 1, GROUP, GROUP + R + 1, N2G - 1):
        add_extra(bt, r, shared)


# ---- 1. every record flagged by the first launch: the map-free second phase ------------
@pytest.mark.parametrize("newset", [True, False])
@pytest.mark.parametrize("k", [1, 3])
def test_all_flagged(C, ctx, ctx_option, k, newset):
    bt = Batch(np.random.default_rng(9100 + k), N2G, k)
    edge_contents(bt)
    run(C, ctx, ctx_option, bt, allf=1, full=nblocks(N2G), flags=np.ones(N2G, np.uint8), newset=newset)
    assert nblocks(N2G) == 33


# ---- 2. a phase-B bucket past the 8192-slot map: nothing to spill without a map --------
def test_all_flagged_large_bucket(C, ctx, ctx_option):
    """The last bucket of the list holds 20000 distinct candidates, owned by
    records that the first launch flags: the launch is all-flagged, and the
    map-free kernel takes the bucket whole (the regular second launch would
    leave it to k_bucket_direct, tests/test_flag_skip.py)."""
    rng = np.random.default_rng(9500)
    bt = Batch(rng, N2G, 1)
    last = int(bt.bB[-1])
    cand = bsig(last, rng.permutation(65536)[:20000])
    owners = np.sort(rng.permutation(N2G)[:400])
    for r, e in zip(owners, np.array_split(cand, owners.size)):
        add_extra(bt, int(r), e)
    vals, _ = bt.arrays()
    assert np.unique(vals[bucket_of(vals) == last]).size >= 20000
    # (No counter tells of spilled buckets, so "nothing left to the direct kernel" is not asserted: k_bucket_sets
    # never writes the spill list, and the counter below says that it, not the regular second launch, ran.)
    run(C, ctx, ctx_option, bt, allf=1, full=nblocks(N2G), flags=np.ones(N2G, np.uint8))


# ---- 3. one record short: the regular second launch ---------------------------------------
EDGES = [0, N2G - 1, GROUP - 1, GROUP, 5 * R]  # record 0, the partial last block's last, group and block edges


@pytest.mark.parametrize("rec", EDGES)
def test_one_record_short(C, ctx, ctx_option, rec):
    """A single record owns only a phase-B signal: the launch is not
    all-flagged, and the regular second launch stores its flag."""
    bt = Batch(np.random.default_rng(9200 + rec), N2G, 1)
    bt.only_b([rec])
    run(C, ctx, ctx_option, bt, allf=0, full=nblocks(N2G) - 1, flags=np.ones(N2G, np.uint8))


@pytest.mark.parametrize("rec", EDGES[1:])  # (record 0 has no earlier record)
def test_one_record_never_flagged(C, ctx, ctx_option, rec):
    """A single record whose only candidate the record before it, flagged by
    the first launch, also holds: its flag stays 0, and the launch is not
    all-flagged."""
    bt = Batch(np.random.default_rng(9250 + rec), N2G, 1)
    bt.dup_b([rec])
    want = np.ones(N2G, np.uint8)
    want[rec] = 0
    run(C, ctx, ctx_option, bt, allf=0, full=nblocks(N2G) - 1, flags=want)


# ---- 4. a record whose entries are all in maxSignal ---------------------------------------
def test_record_all_in_max(C, ctx, ctx_option):
    """It can never be flagged, so the launch is never all-flagged."""
    bt = Batch(np.random.default_rng(9300), N2G, 3)
    bt.in_max([GROUP + R - 1])
    want = np.ones(N2G, np.uint8)
    want[GROUP + R - 1] = 0
    run(C, ctx, ctx_option, bt, allf=0, full=nblocks(N2G) - 1, flags=want)


# ---- 5. record slices: the decision is each launch's own --------------------------------------
def test_record_slices(C, ctx, ctx_option):
    """max_launch_records 5000 over 10300 records: three launches.  A record
    of the middle slice is unflagged after its first launch; the other two
    slices run map-free."""
    n = 10300
    bt = Batch(np.random.default_rng(9600), n, 1, per_bucket=2600)
    bt.only_b([7000])
    ctx_option(ctx, "max_launch_records", 5000)
    run(C, ctx, ctx_option, bt, allf=2, full=1, used=3, flags=np.ones(n, np.uint8))


# ---- 6. one non-empty bucket: the first window is empty ---------------------------------------
class OneBucket:
    """nrec records with one signal each, all of one bucket: the list has one
    entry, so the first launch's window (1 >> k entries) is empty."""

    def __init__(self, nrec, bucket, k=1):
        self.k, self.m0 = k, np.empty(0, np.uint32)
        self.vals = bsig(bucket, np.random.default_rng(9700).permutation(65536)[:nrec])
        self.off = np.arange(nrec + 1, dtype=np.uint64)

    def arrays(self):
        return self.vals, self.off


def test_one_bucket_in_the_batch(C, ctx, ctx_option):
    n = R + 100
    run(C, ctx, ctx_option, OneBucket(n, 0x1234), allf=0, full=0, flags=np.ones(n, np.uint8))


# ---- 7. the raw-trace entry and the two-stream pipeline ---------------------------------------
def expect_all_flagged(batches, k):
    """Per batch of (vals, off), triaged in turn from empty sets: is its split
    launch all-flagged?  Reasoned from the batch alone: phase A is the first
    nl >> k of its nl distinct buckets in ascending order, a signal's first
    owner does not depend on other signals, so the flags after phase A are the
    oracle's over the entries of those buckets against the running maxSignal.
    Also returns the oracle's flags of the whole batches and its final sets."""
    om, on = O.OSet(), O.OSet()
    allf, flags = [], []
    for vals, off in batches:
        bk = bucket_of(vals)
        lst = np.unique(bk)
        in_a = np.isin(bk, lst[: lst.size >> k])
        rec = np.repeat(np.arange(off.size - 1), np.diff(off).astype(np.int64))
        off_a = np.concatenate([[0], np.cumsum(np.bincount(rec[in_a], minlength=off.size - 1))]).astype(np.uint64)
        after_a = O.triage_flags_only(O.OSet(om.export()), None, vals[in_a], off_a)
        allf.append(bool(after_a.all()))
        flags.append(O.triage_flags_only(om, on, vals, off))
    return allf, flags, om, on


def test_trace_entry_and_pipeline(C, ctx, ctx_option):
    """sg_triage_traces_dev and syzkaller_amd/pipeline.py over three Zipf
    trace batches and the first of them again (nothing new: no record is
    flagged), with flag_skip 0 and 1: flags and sets equal the oracle's over
    the executor signal batch by batch, and the forced-on run's counter rises
    by the number of batches that expect_all_flagged finds all-flagged, on
    both entries."""
    import torch

    from syzkaller_amd._lib import call
    from syzkaller_amd.pipeline import PipelinedTriage

    k = 3
    ctx_option(ctx, "m0_filter", 0)
    ctx_option(ctx, "flag_skip_split", k)
    batches = [_traces(ctx, 96, 16, 256, 160 + i) for i in range(3)]
    batches.append(batches[0])
    sigs, host = [], []
    for t, co, po in batches:
        n, ncalls = t.numel(), co.numel() - 1
        s = torch.empty(n, dtype=torch.int32, device="cuda")
        so = torch.empty(ncalls + 1, dtype=torch.int64, device="cuda")
        call("sg_exec_signal_dev", ctx.h, t.data_ptr(), co.data_ptr(), po.data_ptr(), po.numel() - 1, ncalls, n,
             s.data_ptr(), so.data_ptr())
        torch.cuda.synchronize()
        sigs.append((s[: int(so[-1].item())].clone(), so))
        host.append((sigs[-1][0].cpu().numpy().view(np.uint32), so.cpu().numpy().astype(np.uint64)))
    allf, eflags, om, on = expect_all_flagged(host, k)
    print("all-flagged batches expected:", allf)
    assert 0 < sum(allf) < len(allf)  # both forms of the second phase are reached
    for fs in (0, 1):
        ctx_option(ctx, "flag_skip", fs)
        a0 = ctx.counter(ALLF)
        ms, ns = C.SignalSet(ctx), C.SignalSet(ctx)
        tf = []
        for t, co, _ in batches:
            f = torch.zeros(co.numel() - 1, dtype=torch.uint8, device="cuda")
            call("sg_triage_traces_dev", ctx.h, ms.h, ns.h, t.data_ptr(), co.data_ptr(), t.numel(), co.numel() - 1,
                 f.data_ptr())
            tf.append(f)
        torch.cuda.synchronize()
        a1 = ctx.counter(ALLF)
        out = [f.cpu().numpy() for f in tf] + [ms.export(), ns.export()]
        ns.close()
        ms.close()
        ms, ns = C.SignalSet(ctx), C.SignalSet(ctx)
        pt = PipelinedTriage(ctx)
        pf = []
        for v, o in sigs:
            f = torch.full((o.numel() - 1,), 7, dtype=torch.uint8, device="cuda")
            pt.submit(ms, ns, v, o, v.numel(), o.numel() - 1, f)
            pf.append(f)
        pt.close()
        torch.cuda.synchronize()
        a2 = ctx.counter(ALLF)
        out += [f.cpu().numpy() for f in pf] + [ms.export(), ns.export()]
        ns.close()
        ms.close()
        nb = len(batches)
        for part in (out[: nb + 2], out[nb + 2:]):
            for got, want in zip(part[:nb], eflags):
                assert np.array_equal(got, want), fs
            assert np.array_equal(part[nb], om.export()) and np.array_equal(part[nb + 1], on.export()), fs
        want = sum(allf) if fs else 0
        assert (a1 - a0, a2 - a1) == (want, want), (fs, a1 - a0, a2 - a1, allf)


def test_pipeline_all_flagged_with_prefix_words(C, ctx, ctx_option):
    """The kept-partition form with a prefix bitmap (sg_prefix_end_dev: the
    test is against maxSignal | prefix, and a word that gains bits gets the
    prefix's bits too): an all-flagged batch, its phase-B buckets holding
    prefix signals.  Flags and newSignal equal the oracle's against the union;
    maxSignal is the forced-off path's, word for word."""
    import torch

    from syzkaller_amd._lib import call, lib

    bt = Batch(np.random.default_rng(9800), 2 * R + 77, 2)
    first = int(bt.bB[0])
    pre = np.concatenate([bsig(first, [0, 40, 65535]), bsig(65535, [64, 65])])
    add_extra(bt, 3, pre)                                   # entries that hit the prefix
    add_extra(bt, R + 3, bsig(first, [1, 41, 65534]))       # candidates in the prefix's words
    vals, off = bt.arrays()
    n = bt.nrec
    om, on = O.OSet(pre), O.OSet()
    exp = O.triage_flags_only(om, on, vals, off)
    assert exp.all()
    ctx_option(ctx, "m0_filter", 0)
    ctx_option(ctx, "flag_skip_split", bt.k)
    d_vals = torch.from_numpy(vals.view(np.int32)).cuda()
    d_off = torch.from_numpy(off.astype(np.int64)).cuda()
    got = {}
    for fs in (0, 1):
        ctx_option(ctx, "flag_skip", fs)
        a0 = ctx.counter(ALLF)
        ms, ns, ps = C.SignalSet(ctx), C.SignalSet(ctx), C.SignalSet(ctx)
        C.SignalAdd(ps, pre)
        words = torch.zeros(1 << 27, dtype=torch.int32, device="cuda")
        w = ctypes.c_void_p()
        call("sg_set_wrap_dev", ctx.h, ctypes.c_void_p(words.data_ptr()), ctypes.byref(w))
        call("sg_set_copy", w, ps.h)
        f = torch.zeros(n, dtype=torch.uint8, device="cuda")
        call("sg_prefix_begin_form_dev", ctx.h, 0, 2, None, None, d_vals.data_ptr(), d_off.data_ptr(), vals.size, n, None)
        call("sg_prefix_end_dev", ctx.h, 0, ms.h, ctypes.c_void_p(words.data_ptr()), ns.h, f.data_ptr())
        ctx.sync()
        torch.cuda.synchronize()
        assert ctx.counter(ALLF) - a0 == fs
        assert np.array_equal(f.cpu().numpy(), exp)
        assert np.array_equal(ns.export(), on.export())
        got[fs] = ms.export()
        lib.sg_set_destroy(w)
        for s in (ps, ns, ms):
            s.close()
    assert np.array_equal(got[0], got[1])
    # between maxSignal's new signal and that with the prefix (include/syzsig.h)
    assert np.isin(on.export(), got[1]).all() and np.isin(got[1], om.export()).all()
