"""The ordered-output sweep (sg_triage.hip owned_outputs: k_own_pipe,
k_own_wave, k_own_big) at its set, chunk and probe-chain edges.

tests/owned_cases.py builds each batch on one edge and states what it claims:
the signals every record owns, the chain of full buckets its keys make in the
LDS set, and how many records the call leaves to k_own_big (the context
counter "owned_big_records").  The CPU tests below check those claims from the
restated hash and predicates and from the oracle's lists alone; the GPU tests
run every case through sg_triage_batch (host form), sg_triage_batch_dev with
diff buffers at element shifts 0..3 (16-B aligned and not) and sg_merge_poll,
bit-exact against oracle/pyoracle.py (syz-fuzzer/fuzzer.go:645-693,
syz-manager/manager.go:949-956) in the flags, the offsets, the values and both
sets, with the counter equal to its prediction; the cases with a slice_at run
again cut into record slices, the owning record the first of a slice."""
import numpy as np
import pytest

from oracle import pyoracle as O
from tests import owned_cases as W
from tests import refmodel as R

CASES = W.all_cases()
IDS = [c.name for c in CASES]
CHAINS = [c for c in CASES if c.chainf]
SLICED = [c for c in CASES if c.slice_at is not None]
SENT = W.SENT

_facts, _exp = {}, {}


def facts(case):
    if case.name not in _facts:
        _facts[case.name] = W.facts(case)
    return _facts[case.name]


def expected(case):
    """the oracle's results of the case, computed once: the triage form's
    flags, diff CSR and both sets, the Poll form's CSR and set"""
    if case.name not in _exp:
        om, on = O.OSet(case.m0), O.OSet()
        ef, ev, eo = O.triage_batch(om, on, case.vals, case.off)
        pm = O.OSet(case.m0)
        pv, po = O.merge_poll(pm, case.vals, case.off)
        _exp[case.name] = {"f": ef, "v": ev, "o": eo, "m": om.export(), "n": on.export(), "pv": pv, "po": po,
                           "pm": pm.export()}
        for a in _exp[case.name].values():
            a.setflags(write=False)
    return _exp[case.name]


# ---- CPU: the restatement and the claims ---------------------------------------
def test_hash_inverse_and_bucket_counts():
    assert (W.MULT * W.INV) & W.M32 == 1
    for bb in (4, 6, 9, 12, 14):
        for home in (0, 1, (1 << bb) - 1):
            vs = W.chain(bb, home, 7, range(3, 10))
            assert len(set(vs)) == 7 and all(W.own_home(v, bb) == home for v in vs)
            # fewer bits: the home's high bits
            assert all(W.own_home(v, 4) == home >> (bb - 4) for v in vs)
    assert [W.own_bits(n) for n in (1, 16, 17, 32, 33, 256, 257, 512, 513, 4095, 4096)] == \
        [4, 4, 5, 5, 6, 8, 9, 9, 10, 12, 12]
    # the empty marker's own home (it is never stored)
    assert W.own_home(SENT, 4) == ((-W.MULT) & W.M32) >> 28


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_case_claims(case):
    f = facts(case)
    assert f["owned_triage"] == case.owned and f["owned_poll"] == case.owned
    assert f["big_triage"] == case.big_triage and f["big_poll"] == case.big_poll
    off, nvals = case.off.astype(np.int64), int(case.vals.size)
    nt = case.notes
    if "span" in nt:  # every owning record starts at 0, 1 or 255 (mod 256) and spans exactly that
        assert sorted({int(off[r]) % 256 for r in case.owned}) == [0, 1, 255]
        assert {f["span"][r] for r in case.owned} == {nt["span"]}
        assert sorted({n for n in case.owned.values()}) == list(W.OWNED_EDGES)
        assert all((int(off[r + 1]) - 1) // 256 < nvals // 256 for r in case.owned)
        # a record's first and last entries are owned: a sweep that stopped a chunk short, or
        # masked its ends one element short, would lose an entry of its list
        dv, do = expected(case)["v"], expected(case)["o"]
        for r in case.owned:
            seg = case.vals[off[r]:off[r + 1]]
            d = dv[int(do[r]):int(do[r + 1])]
            assert d[-1] == seg[-1] and (case.owned[r] == 1 or d[0] == seg[0])
    if "end_mod" in nt:
        last = off.size - 2
        assert nvals % 256 == nt["end_mod"] and last in case.owned and f["span"][last] <= 5
        assert ((int(off[last + 1]) - 1) // 256 < nvals // 256) == (nt["end_mod"] == 0)
    if "nrec" in nt:
        assert off.size - 1 == nt["nrec"]
    if "np" in nt:
        assert f["np"] == nt["np"]
    if "pieces" in nt:
        (r, n), = case.owned.items()
        assert -(-n // W.PIECE) == nt["pieces"]
        seg = case.vals[off[r]:off[r + 1]]
        for v in np.unique(O.triage_batch(O.OSet(case.m0), None, case.vals, case.off)[1]):
            at = np.flatnonzero(seg == v)
            assert at.size == 2 and at[1] - at[0] >= 256  # twice, in different chunks
        assert (SENT in seg) == case.name.endswith("_ff")
    if "pairs" in nt:
        r = nt["rec"]
        seg = case.vals[off[r]:off[r + 1]]
        assert off[r] % 256 == 0
        for j in range(nt["pairs"]):
            assert seg[256 * j + 255] == seg[256 * j + 256] and int(seg[256 * j + 255]) not in set(case.m0.tolist())
    if "steps" in nt:
        (r, n), = case.owned.items()
        seg = case.vals[off[r]:off[r + 1]]
        s1, s2 = nt["steps"]
        assert s1 == 5 * 256 and s2 == 5 * 16 * 256 and off[r] % 256 == 0 and n > W.WAVE_CAP
        assert np.array_equal(seg[:n], seg[s1:s1 + n]) and np.array_equal(seg[:n], seg[s2:s2 + n])
    if case.name.startswith("poll_ff"):
        (r, n), = case.owned.items()
        seg = case.vals[off[r]:off[r + 1]]
        assert off[r] % 256 == 0 and np.array_equal(np.flatnonzero(seg == SENT), [254, 255, 256])
    if case.name.startswith("groups"):
        assert tuple(sorted(case.owned)) == W.GROUP_OWNERS and set(case.owned.values()) == {1}
        s = {r: int(case.vals[off[r] + 1]) for r in case.owned}
        for r in (0, 65535, 65537):
            assert abs(s[r] - s[r + 65536]) == 1  # neighbours: one partition bucket
    if case.slice_at is not None:  # the sliced rerun: the second slice starts at an owning record, off a 16-B boundary
        r = case.slice_at
        assert 0 < r < off.size - 1 and r in case.owned and off[r] != 0 and off[r] % 4 != 0


@pytest.mark.parametrize("case", CHAINS, ids=[c.name for c in CHAINS])
def test_chain_claims(case):
    cf = case.chainf
    bb, H, rec, full = cf["bb"], cf["home"], cf["rec"], cf["full_run"]
    nb = 1 << bb
    e = expected(case)
    own = np.unique(e["v"][int(e["o"][rec]):int(e["o"][rec + 1])]).tolist()
    assert W.own_bits(len(own)) == bb and H == nb - 1 and full >= 3
    assert set(cf["chain"]) | set(cf["mid"]) <= set(own)
    assert all(W.own_home(v, bb) == H for v in cf["chain"] + cf["miss_home"])
    assert all(W.own_home(v, bb) == 0 for v in cf["mid"] + cf["miss_mid"])
    # the misses: members of m0, or owned by record 0; all of them in the record
    m0, seg = set(case.m0.tolist()), set(case.vals[int(case.off[rec]):int(case.off[rec + 1])].tolist())
    own0 = set(e["v"][int(e["o"][0]):int(e["o"][1])].tolist())
    misses = cf["miss_home"] + cf["miss_mid"] + cf["half"]
    assert all((v in m0) != (v in own0) for v in misses) and any(v in own0 for v in cf["miss_home"])
    assert set(misses) <= seg and not set(misses) & set(own)
    counts = None
    for order in (own, own[::-1], cf["mid"] + [v for v in own if v not in cf["mid"]]):
        s = W.OwnedSet(bb)
        for v in order:
            s.insert(v)
        # the buckets' fill does not depend on the order of the inserts
        assert counts is None or s.counts() == counts
        counts = s.counts()
        run = [(H + j) & (nb - 1) for j in range(full + 1)]
        assert all(counts[b] == 4 for b in run[:-1]) and counts[run[-1]] < 4 and counts[(H - 1) & (nb - 1)] < 4
        for v in cf["miss_home"]:  # the whole chain, through the wrap to bucket 0
            hit, reads, seen = s.probe(v)
            assert not hit and reads == cf["miss_reads"] and seen == run
        for v in cf["miss_mid"]:
            hit, reads, seen = s.probe(v)
            assert not hit and reads == cf["miss_mid_reads"] and seen == run[1:]
        for v in cf["half"]:  # stops at once on a bucket that is neither empty nor full
            hit, reads, seen = s.probe(v)
            assert not hit and reads == 1 and 0 < counts[seen[0]] < 4
        hits = [s.probe(v) for v in own]
        assert all(h[0] for h in hits)
        # some key is found only in the third bucket of its walk or later, past the wrap
        assert max(h[1] for h in hits) >= 3 and any(h[1] >= 3 and h[2][0] == H for h in hits)
        # the record's diff list is the sweep over this set; a lookup that gave
        # up after its second bucket would lose entries of it: the case tells
        seq = case.vals[int(case.off[rec]):int(case.off[rec + 1])].tolist()
        want = e["v"][int(e["o"][rec]):int(e["o"][rec + 1])].tolist()
        assert [v for v in seq if s.probe(v)[0]] == want
        assert [v for v in seq if s.probe(v)[0] and s.probe(v)[1] <= 2] != want


def test_routing_both_outcomes():
    """every clause of the flags-and-diff predicate, and the Poll one, true and
    false over the cases; the edges on both sides with the other clauses true"""
    seen = {k: set() for k in ("owns", "cap", "span", "whole", "poll")}
    edge = set()
    for case in CASES:
        off, nvals = case.off.astype(np.int64), int(case.vals.size)
        if len(case.owned) < off.size - 1:
            seen["owns"].add(False)
        for r, n in case.owned.items():
            c0, c1 = int(off[r]) // 256, (int(off[r + 1]) - 1) // 256
            cl = (n <= 512, c1 - c0 < 5, c1 < nvals // 256)
            seen["owns"].add(True)
            seen["cap"].add(cl[0])
            seen["span"].add(cl[1])
            seen["whole"].add(cl[2])
            seen["poll"].add(W.wave_poll(n))
            assert W.wave_triage(n, c0, c1, nvals) == all(cl)
            if cl[1] and cl[2] and n in (511, 512, 513):
                edge.add(("cap", n))
            if cl[0] and cl[2] and c1 - c0 in (3, 4, 5):
                edge.add(("span", c1 - c0 + 1))
            if cl[0] and cl[1] and r == off.size - 2:
                edge.add(("end", nvals % 256))
    assert all(v == {True, False} for v in seen.values()), seen
    assert edge >= {("cap", 511), ("cap", 512), ("cap", 513), ("span", 4), ("span", 5), ("span", 6), ("end", 0),
                    ("end", 1), ("end", 255)}


@pytest.mark.parametrize("case", [c for c in CASES if c.small], ids=[c.name for c in CASES if c.small])
def test_oracle_lists_vs_python_loops(case):
    e = expected(case)
    off = case.off.astype(np.int64)
    recs = [case.vals[off[r]:off[r + 1]].tolist() for r in range(off.size - 1)]
    ms, ns = set(case.m0.tolist()), set()
    flags, diffs = R.triage(ms, ns, recs)
    assert flags == e["f"].tolist()
    assert [len(d) for d in diffs] == np.diff(e["o"].astype(np.int64)).tolist()
    assert [x for d in diffs for x in d] == e["v"].tolist()
    assert sorted(ms) == e["m"].tolist() and sorted(ns) == e["n"].tolist()
    pm = set(case.m0.tolist())
    news = R.merge_poll(pm, recs)
    assert [len(d) for d in news] == np.diff(e["po"].astype(np.int64)).tolist()
    assert [x for d in news for x in d] == e["pv"].tolist() and sorted(pm) == e["pm"].tolist()


# ---- GPU ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def C(ctx):
    from syzkaller_amd import cover

    return cover


@pytest.fixture(scope="module")
def sets(C, ctx):
    ms, ns = C.SignalSet(ctx), C.SignalSet(ctx)
    yield ms, ns
    ns.close()
    ms.close()


def _start(C, sets, case):
    ms, ns = sets
    ms.clear()
    ns.clear()
    C.SignalAdd(ms, case.m0)
    return ms, ns


def _host_form(C, ctx, sets, case):
    e = expected(case)
    ms, ns = _start(C, sets, case)
    f, dv, do = C.triage_batch(ms, ns, case.vals, case.off, ctx=ctx)
    assert np.array_equal(f, e["f"])
    assert np.array_equal(do, e["o"]) and np.array_equal(dv, e["v"])
    assert np.array_equal(ms.export(), e["m"]) and np.array_equal(ns.export(), e["n"])
    assert ctx.counter("owned_big_records") == case.big_triage


def _dev_form(C, ctx, sets, case, shift):
    import torch
    from syzkaller_amd._lib import call

    e = expected(case)
    ms, ns = _start(C, sets, case)
    n, nrec = int(case.vals.size), case.off.size - 1
    fill = 0x5A5A5A5A
    buf = torch.zeros(n + 8, dtype=torch.int32, device="cuda")
    buf[shift:shift + n] = torch.from_numpy(case.vals.view(np.int32)).cuda()
    dvals = buf[shift:shift + n]
    assert (dvals.data_ptr() % 16 != 0) == (shift != 0)
    doff = torch.from_numpy(case.off.view(np.int64)).cuda()
    # outputs prefilled: what the call leaves unwritten shows
    flags = torch.full((nrec,), 0xEE, dtype=torch.uint8, device="cuda")
    dv = torch.full((n + 8,), fill, dtype=torch.int32, device="cuda")
    do = torch.full((nrec + 1,), -1, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()  # the library queues on its own stream
    call("sg_triage_batch_dev", ctx.h, ms.h, ns.h, dvals.data_ptr(), doff.data_ptr(), n, nrec, flags.data_ptr(),
         dv.data_ptr(), do.data_ptr())
    big = ctx.counter("owned_big_records")  # (waits for the stream)
    assert np.array_equal(flags.cpu().numpy(), e["f"])
    assert np.array_equal(do.cpu().numpy().view(np.uint64), e["o"])
    got = dv.cpu().numpy().view(np.uint32)
    nd = int(e["o"][-1])
    assert np.array_equal(got[:nd], e["v"]) and (got[nd:] == fill).all()
    assert np.array_equal(ms.export(), e["m"]) and np.array_equal(ns.export(), e["n"])
    assert big == case.big_triage


def _poll_form(C, ctx, sets, case):
    e = expected(case)
    ms, _ = _start(C, sets, case)
    pv, po = C.merge_poll(ms, case.vals, case.off, ctx=ctx)
    assert np.array_equal(po, e["po"]) and np.array_equal(pv, e["pv"])
    assert np.array_equal(ms.export(), e["pm"])
    assert ctx.counter("owned_big_records") == case.big_poll


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_host_form(C, ctx, sets, case):
    _host_form(C, ctx, sets, case)


@pytest.mark.gpu
@pytest.mark.parametrize("shift", (0, 1, 2, 3))
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_dev_form(C, ctx, sets, case, shift):
    _dev_form(C, ctx, sets, case, shift)


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_poll_form(C, ctx, sets, case):
    _poll_form(C, ctx, sets, case)


@pytest.mark.gpu
@pytest.mark.parametrize("case", SLICED, ids=[c.name for c in SLICED])
def test_record_slices(C, ctx, ctx_option, sets, case):
    """cut every slice_at records: the owning record is the first record of
    the second slice, at an element offset that is no multiple of 4; the
    counter is the sum over the slices"""
    ctx_option(ctx, "max_launch_records", case.slice_at)
    assert ctx.counter("max_launch_records") == case.slice_at
    _host_form(C, ctx, sets, case)
    _dev_form(C, ctx, sets, case, 0)
    _dev_form(C, ctx, sets, case, 3)
    _poll_form(C, ctx, sets, case)


@pytest.mark.gpu
def test_counter_is_the_last_calls(C, ctx, sets):
    """the counter is zeroed by every ordered-output call, one without signal
    entries included; an unknown name is still refused"""
    from syzkaller_amd._lib import SG_EINVAL, SyzSigError

    big = next(c for c in CASES if c.name == "route_span6_min")
    _host_form(C, ctx, sets, big)
    assert ctx.counter("owned_big_records") == 24
    ms, ns = sets
    off = np.zeros(4, np.uint64)
    f, dv, do = C.triage_batch(ms, ns, np.zeros(0, np.uint32), off, ctx=ctx)
    assert not f.any() and dv.size == 0 and not do.any()
    assert ctx.counter("owned_big_records") == 0
    _poll_form(C, ctx, sets, big)
    pv, po = C.merge_poll(ms, np.zeros(0, np.uint32), off, ctx=ctx)
    assert pv.size == 0 and not po.any() and ctx.counter("owned_big_records") == 0
    with pytest.raises(SyzSigError) as e:
        ctx.counter("owned_big_record")
    assert e.value.rc == SG_EINVAL
