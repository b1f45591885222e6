"""The flags path's bucket stage in two launches (sg_bucket.hip buckets_one,
k_flag_summary, k_bucket<.., kSkip>, option flag_skip): the first launch takes
the first 1 / 2^k of the list of non-empty buckets (ascending bucket number
b2 << 8 | b1) and stores every record flag; the summary then holds one bit per
block of 4096 consecutive records of the launch, set iff every existing record
of the block is flagged; the second launch takes the rest of the list and
leaves out the flag stores of records in such blocks.

A store skipped wrongly leaves a flag 0 that the oracle has at 1, so every case
is bit-exact against oracle/pyoracle.py (syz-fuzzer/fuzzer.go:645-693) for the
flags, the maxSignal export and the newSignal export, with flag_skip 0 and 1,
and the counter flag_skip_full_blocks is pinned to its exact value: a block
taken as full although one of its records is not flagged yet (an off-by-one at
a block, group or batch edge, a partial last block) shows there first.

The batches are built per bucket: record r owns one signal of its own in
phase-A bucket r mod nA and one in phase-B bucket r mod nB, so after the first
launch every record is flagged except those a case takes out."""
import numpy as np
import pytest

from oracle import pyoracle as O

pytestmark = pytest.mark.gpu

R = 4096                      # kFsRecs: records per summary bit
GROUP = 1 << 16               # kGroupRecs
N2G = 2 * GROUP + 300         # two full groups and a partial block: 33 blocks
PER_BUCKET = 2048             # distinct candidates per bucket: a quarter of the 8192-slot LDS map


@pytest.fixture(scope="module")
def C(ctx):
    from syzkaller_amd import cover

    return cover


def sig(d, pos):
    """The signal of slice d (its byte b2) at the 24-bit slice position
    pos = b1 << 16 | b3 << 8 | b0 (as tests/test_m0_filter_edges.py)."""
    pos, d = np.asarray(pos).astype(np.uint64), np.asarray(d).astype(np.uint64)
    return ((((pos >> np.uint64(8)) & np.uint64(255)) << np.uint64(24)) | (d << np.uint64(16))
            | ((pos >> np.uint64(16)) << np.uint64(8)) | (pos & np.uint64(255))).astype(np.uint32)


def bsig(bucket, lo):
    """Signal number lo (16 bits) of bucket b2 << 8 | b1."""
    bucket, lo = np.asarray(bucket).astype(np.uint64), np.asarray(lo).astype(np.uint64)
    s = sig(bucket >> np.uint64(8), ((bucket & np.uint64(255)) << np.uint64(16)) | lo)
    assert np.all(((((s >> 16) & 255) << 8) | ((s >> 8) & 255)) == bucket.astype(np.uint32))
    return s


class Batch:
    """nrec records over nA phase-A and nB phase-B buckets (k: the split;
    nA = (nA + nB) >> k): a_sig[r] / b_sig[r] are record r's own signals."""

    def __init__(self, rng, nrec, k, per_bucket=PER_BUCKET):
        self.nrec, self.k = nrec, k
        nA = -(-nrec // per_bucket)
        nl = nA << k
        self.nl = nl
        nB = nl - nA
        b = np.sort(rng.permutation(65536 - 2)[: nl - 2] + 1)
        b = np.concatenate([[0], b, [65535]])  # the first and the last bucket too
        assert np.unique(b).size == nl and (nl >> k) == nA
        self.bA, self.bB = b[:nA], b[nA:]
        r = np.arange(nrec)
        lo = rng.permutation(65536)
        self.a_sig = bsig(self.bA[r % nA], lo[r // nA])
        self.b_sig = bsig(self.bB[r % nB], lo[65535 - r // nB])
        self.has_a = np.ones(nrec, bool)
        self.b_of = self.b_sig.copy()
        self.extra = {}  # record -> more entries
        self.m0 = np.empty(0, np.uint32)

    def only_b(self, recs):
        self.has_a[np.asarray(recs)] = False

    def in_max(self, recs):
        """Both entries of these records are in maxSignal."""
        recs = np.asarray(recs)
        self.m0 = np.concatenate([self.m0, self.a_sig[recs], self.b_sig[recs]])

    def dup_b(self, recs):
        """These records hold only the phase-B signal of the record before."""
        recs = np.asarray(recs)
        self.has_a[recs] = False
        self.b_of[recs] = self.b_sig[recs - 1]

    def arrays(self):
        lens = 1 + self.has_a.astype(np.int64)
        for r, e in self.extra.items():
            lens[r] += len(e)
        off = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
        vals = np.empty(int(off[-1]), np.uint32)
        o = off[:-1].astype(np.int64)
        vals[o] = self.b_of  # the phase-B entry first: order inside a record is free
        vals[o[self.has_a] + 1] = self.a_sig[self.has_a]
        for r, e in self.extra.items():
            vals[o[r] + 1 + int(self.has_a[r]): o[r] + lens[r]] = e
        return vals, off


def nblocks(n):
    return -(-n // R)


def run(C, ctx, ctx_option, bt, full=None, used=1, flags=None, diff=False):
    """The batch with flag_skip 0 and 1 on fresh sets: both equal the oracle;
    the forced-on run split `used` launches and its last one found `full` blocks."""
    vals, off = bt.arrays()
    om, on = O.OSet(bt.m0 if bt.m0.size else None), O.OSet()
    exp = O.triage_flags_only(om, on, vals, off)
    if flags is not None:
        assert np.array_equal(exp, flags)  # the construction itself
    ctx_option(ctx, "m0_filter", 0)  # the partitioned path (the M0 filter would finish these small batches itself)
    ctx_option(ctx, "flag_skip_split", bt.k)
    for fs in (0, 1):
        ctx_option(ctx, "flag_skip", fs)
        u0 = ctx.counter("flag_skip_used")
        ms, ns = C.SignalSet(ctx), C.SignalSet(ctx)
        if bt.m0.size:
            C.SignalAdd(ms, bt.m0)
        got, _, _ = C.triage_batch(ms, ns, vals, off, want_diff=diff, ctx=ctx)
        assert np.array_equal(got, exp), (fs, np.flatnonzero(got != exp)[:10])
        assert np.array_equal(ms.export(), om.export()) and np.array_equal(ns.export(), on.export())
        ns.close()
        ms.close()
        du = ctx.counter("flag_skip_used") - u0
        assert du == (used if fs else 0), (fs, du)
        if fs and full is not None:
            assert ctx.counter("flag_skip_full_blocks") == full
    return exp


# ---- 1. every record flagged by the first launch ----------------------------------
@pytest.mark.parametrize("k", [1, 3])
def test_all_blocks_full(C, ctx, ctx_option, k):
    """Every record owns a signal in a phase-A and one in a phase-B bucket:
    all 33 blocks, the partial last one included, are full after phase A."""
    bt = Batch(np.random.default_rng(9100 + k), N2G, k)
    run(C, ctx, ctx_option, bt, full=nblocks(N2G), flags=np.ones(N2G, np.uint8))
    assert nblocks(N2G) == 33


# ---- 2. records that only the second launch flags -----------------------------------
def test_phase_b_only_records_at_edges(C, ctx, ctx_option):
    """The first and the last record of a block, the last record of a group
    and the last record of the batch own only a phase-B signal: their four
    blocks are not full, and the second launch must store their flags."""
    bt = Batch(np.random.default_rng(9200), N2G, 1)
    bt.only_b([3 * R, 5 * R + R - 1, GROUP - 1, N2G - 1])
    run(C, ctx, ctx_option, bt, full=nblocks(N2G) - 4, flags=np.ones(N2G, np.uint8))


# ---- 3. / 4. records that stay unflagged inside saturated blocks ----------------------
def test_unflagged_records_in_saturated_blocks(C, ctx, ctx_option):
    """Records whose entries are all in maxSignal, and records whose only
    candidate (a phase-B signal) an earlier record owns: flags 0, their blocks
    not full, every other block full."""
    bt = Batch(np.random.default_rng(9300), N2G, 1)
    inmax = [100, 7 * R, GROUP + R - 1]          # blocks 0, 7, 16
    dup = [2 * R + 17, GROUP - 1, N2G - 1]       # blocks 2, 15, 32
    bt.in_max(inmax)
    bt.dup_b(dup)
    want = np.ones(N2G, np.uint8)
    want[inmax + dup] = 0
    run(C, ctx, ctx_option, bt, full=nblocks(N2G) - 6, flags=want)


# ---- 5. a phase-B bucket past the LDS map: the direct-table kernel --------------------
def test_spilled_phase_b_bucket(C, ctx, ctx_option):
    """The last bucket of the list holds 20000 distinct candidates (more than
    the 8192-slot map: it is redone by k_bucket_direct, as in
    tests/test_gpu_parity.py), owned by records of full blocks and by records
    that own nothing else (their blocks are not full: the direct kernel must
    store their flags)."""
    rng = np.random.default_rng(9500)
    bt = Batch(rng, N2G, 1)
    last = int(bt.bB[-1])
    used = np.unique(bt.b_sig[(bt.b_sig >> 16 & 255) << 8 | (bt.b_sig >> 8 & 255) == last])
    cand = bsig(last, rng.permutation(65536)[:21000])
    cand = cand[~np.isin(cand, used)][:20000]
    lonely = [R, 4 * R - 1, GROUP - 1, GROUP + 5, N2G - 1]   # blocks 1, 3, 15, 16, 32
    bt.only_b(lonely)
    for i, r in enumerate(lonely):
        bt.b_of[r] = cand[i]
    rest = cand[len(lonely):]
    owners = np.sort(rng.permutation(N2G)[:400])
    owners = owners[~np.isin(owners, lonely)]
    for r, e in zip(owners, np.array_split(rest, owners.size)):
        bt.extra[int(r)] = e
    run(C, ctx, ctx_option, bt, full=nblocks(N2G) - 5, flags=np.ones(N2G, np.uint8))


# ---- 6. record slices ---------------------------------------------------------------
@pytest.mark.parametrize("mlr", [1000, 5000])
def test_record_slices(C, ctx, ctx_option, mlr):
    """max_launch_records 1000 and 5000 (a slice of one block and a partial
    one): every slice is a launch of its own, its blocks counted from its first
    record.  Records that only the second launch flags sit at slice-relative
    block edges; the last slice (300 records) is full."""
    n = 10300
    bt = Batch(np.random.default_rng(9600 + mlr), n, 1, per_bucket=2600)
    bt.only_b([R - 1, R, 4999, 5000, 5000 + R - 1, 5000 + R, 9999])
    ctx_option(ctx, "max_launch_records", mlr)
    assert n % mlr == 300
    run(C, ctx, ctx_option, bt, full=1, used=-(-n // mlr), flags=np.ones(n, np.uint8))


def test_record_slices_last_not_full(C, ctx, ctx_option):
    n = 10300
    bt = Batch(np.random.default_rng(9650), n, 1, per_bucket=2600)
    bt.only_b([10000, n - 1])
    ctx_option(ctx, "max_launch_records", 5000)
    run(C, ctx, ctx_option, bt, full=0, used=3, flags=np.ones(n, np.uint8))


# ---- 7. the auto regime ---------------------------------------------------------------
def test_auto_sequence(C):
    """A fresh context on auto: its first slice does not split; the slice
    after a fully queued one does; the slice after a low-novelty one does not.
    (m0_filter 0: the queued count then runs for flag_skip alone.)"""
    c = C.Context(0)
    try:
        assert c.get_option("flag_skip") == -1
        c.set_option("m0_filter", 0)
        rng = np.random.default_rng(9700)
        x, y = Batch(rng, 3 * R + 5, 3), Batch(rng, 3 * R + 5, 3)
        ms, ns = C.SignalSet(c), C.SignalSet(c)
        om, on = O.OSet(), O.OSet()
        used = []
        for bt in (x, y, y, y, x):
            vals, off = bt.arrays()
            got, _, _ = C.triage_batch(ms, ns, vals, off, want_diff=False, ctx=c)
            assert np.array_equal(got, O.triage_flags_only(om, on, vals, off))
            c.sync()
            used.append(c.counter("flag_skip_used"))
        # x fresh: first slice | y fresh after a queued one: split | y again (nothing new) after a
        # queued one: split | y after a low-novelty one: not | x (nothing new) after a low-novelty one: not
        assert used == [0, 1, 2, 2, 2], used
        assert np.array_equal(ms.export(), om.export()) and np.array_equal(ns.export(), on.export())
        ns.close()
        ms.close()
    finally:
        c.close()


# ---- 8. the raw-trace entry and the two-stream pipeline -----------------------------------
def _traces(ctx, nprog, calls, pcs, seed):
    import torch

    from syzkaller_amd._lib import call

    n = nprog * calls * pcs
    trace = torch.empty(n, dtype=torch.int32, device="cuda")
    call("sg_gen_zipf_traces_dev", ctx.h, 0x5A17C0DE, seed, 1.1, 1 << 20, 0, nprog, calls, pcs, trace.data_ptr())
    call_off = torch.arange(0, n + 1, pcs, dtype=torch.int64, device="cuda")
    prog_off = torch.arange(0, nprog * calls + 1, calls, dtype=torch.int64, device="cuda")
    return trace, call_off, prog_off


def test_trace_entry_and_pipeline(C, ctx, ctx_option):
    """sg_triage_traces_dev and syzkaller_amd/pipeline.py with flag_skip 1:
    flags and sets equal the forced-off path's, batch by batch."""
    import torch

    from syzkaller_amd._lib import call
    from syzkaller_amd.pipeline import PipelinedTriage

    ctx_option(ctx, "m0_filter", 0)
    ctx_option(ctx, "flag_skip_split", 3)
    batches = [_traces(ctx, 96, 16, 256, 60 + i) for i in range(3)]
    sigs = []
    for t, co, po in batches:
        n, ncalls = t.numel(), co.numel() - 1
        s = torch.empty(n, dtype=torch.int32, device="cuda")
        so = torch.empty(ncalls + 1, dtype=torch.int64, device="cuda")
        call("sg_exec_signal_dev", ctx.h, t.data_ptr(), co.data_ptr(), po.data_ptr(), po.numel() - 1, ncalls, n,
             s.data_ptr(), so.data_ptr())
        torch.cuda.synchronize()
        sigs.append((s[: int(so[-1].item())].clone(), so))
    res = {}
    for fs in (0, 1):
        ctx_option(ctx, "flag_skip", fs)
        u0 = ctx.counter("flag_skip_used")
        # raw traces
        ms, ns = C.SignalSet(ctx), C.SignalSet(ctx)
        tf = []
        for t, co, _ in batches:
            f = torch.zeros(co.numel() - 1, dtype=torch.uint8, device="cuda")
            call("sg_triage_traces_dev", ctx.h, ms.h, ns.h, t.data_ptr(), co.data_ptr(), t.numel(), co.numel() - 1,
                 f.data_ptr())
            tf.append(f)
        torch.cuda.synchronize()
        u1 = ctx.counter("flag_skip_used")
        out = [f.cpu().numpy() for f in tf] + [ms.export(), ns.export()]
        ns.close()
        ms.close()
        # the pipeline over the same batches' signal
        ms, ns = C.SignalSet(ctx), C.SignalSet(ctx)
        pt = PipelinedTriage(ctx)
        pf = []
        for v, o in sigs:
            f = torch.full((o.numel() - 1,), 7, dtype=torch.uint8, device="cuda")
            pt.submit(ms, ns, v, o, v.numel(), o.numel() - 1, f)
            pf.append(f)
        pt.close()
        torch.cuda.synchronize()
        u2 = ctx.counter("flag_skip_used")
        out += [f.cpu().numpy() for f in pf] + [ms.export(), ns.export()]
        ns.close()
        ms.close()
        assert (u1 - u0, u2 - u1) == ((3, 3) if fs else (0, 0))
        res[fs] = out
    assert len(res[0]) == len(res[1])
    for a, b in zip(res[0], res[1]):
        assert np.array_equal(a, b)
    assert 0 < sum(int(f.sum()) for f in res[0][:3])


# ---- 9. the ordered outputs -----------------------------------------------------------
def test_ordered_outputs_same_flags(C, ctx, ctx_option):
    """The call with diff buffers (the emitting bucket kernels, never split)
    returns the flags of the flags path with flag_skip 1."""
    bt = Batch(np.random.default_rng(9900), 2 * R + 77, 2)
    bt.only_b([0, R - 1, 2 * R + 76])
    bt.dup_b([R + 1])
    bt.in_max([5])
    vals, off = bt.arrays()
    ctx_option(ctx, "m0_filter", 0)
    ctx_option(ctx, "flag_skip_split", bt.k)
    ctx_option(ctx, "flag_skip", 1)
    got = []
    for diff in (False, True):
        u0 = ctx.counter("flag_skip_used")
        ms, ns = C.SignalSet(ctx), C.SignalSet(ctx)
        C.SignalAdd(ms, bt.m0)
        om, on = O.OSet(bt.m0), O.OSet()
        f, dv, do = C.triage_batch(ms, ns, vals, off, want_diff=diff, ctx=ctx)
        ef, ev, eo = O.triage_batch(om, on, vals, off)
        assert np.array_equal(f, ef)
        if diff:
            assert np.array_equal(dv, ev) and np.array_equal(do, eo)
        assert np.array_equal(ms.export(), om.export()) and np.array_equal(ns.export(), on.export())
        assert ctx.counter("flag_skip_used") - u0 == (0 if diff else 1)
        got.append(f)
        ns.close()
        ms.close()
    assert np.array_equal(got[0], got[1]) and got[0][R + 1] == 0 and got[0][5] == 0 and got[0].sum() == got[0].size - 2
