"""The M0 filter (sg_m0filter.hip k_m0_index / k_m0_filter / k_m0_tail_*,
m0_filter(), m0f_try()) at its capacity edges, across the partition's
geometries and through every caller that reaches it.

An entry that the LDS index fails to prove is re-checked by the tail against
the bitmap, so a broken overflow-block read, spill lookup or part mask still
gives the oracle's flags and sets: it only produces more survivors.  The
constructions here therefore pin the counter m0_filter_survivors to its exact
value as well -- the number of entries outside maxSignal, plus the members that
the index's capacities leave unproven by design -- and the branch taken ("used":
the filter's tail produced the results; "fallback": the survivors overflowed
and pass 2 with the bucket stage ran).  Everything is bit-exact against
oracle/pyoracle.py (syz-fuzzer/fuzzer.go:645-693, syz-manager/manager.go:907-912):
flags, maxSignal export, newSignal export."""
import numpy as np
import pytest

from oracle import pyoracle as O

pytestmark = pytest.mark.gpu

SENT = 0xFFFFFFFF

# The kernel's constants (syzkaller_amd/csrc/sg_m0filter.hip; the last two sg_part.h).
K_REM_BITS = 11          # kFRemBits    positions per filter bucket: 2^11 (2^(11-k) with 2^k index parts)
K_BUCKETS = 8192         # kFBuckets    buckets per index part
K_OV_USABLE = 1984 - 1   # kFOvBlocks - 1   overflow blocks per index part (block 0 is the dummy)
K_SPILL = 512            # kFSpill      spill list per index part
K_PARTS = 8              # kFParts (SG_FPARTS)   filter workgroups per slice, 8 >> k per index part
K_WG_CAP = 2048          # kFWgCap      survivors per filter workgroup
K_SURV_CAP = 1 << 20     # kFSurvCap    survivors per launch
K_HDR = 8                # fields of a bucket header (k_m0_index: 7 values and the block link past 8 values)
K_BLK = 8                # values of an overflow block
K_TILE = 16384           # kPT (SG_PT)  entries per pass-1 tile
K_GROUP = 1 << 16        # kGroupRecs   records per group


@pytest.fixture(scope="module")
def C(ctx):
    from syzkaller_amd import cover

    _check_model()
    return cover


# ---- positions ---------------------------------------------------------------
def sig(d, pos):
    """The signal of slice d (its byte b2) at the 24-bit slice position
    pos = b1 << 16 | b3 << 8 | b0."""
    pos, d = np.asarray(pos).astype(np.uint64), np.asarray(d).astype(np.uint64)
    return ((((pos >> np.uint64(8)) & np.uint64(255)) << np.uint64(24)) | (d << np.uint64(16))
            | ((pos >> np.uint64(16)) << np.uint64(8)) | (pos & np.uint64(255))).astype(np.uint32)


def slice_pos(s):
    """(slice, position) of signals: the inverse of sig()."""
    s = np.asarray(s).astype(np.uint64)
    d = (s >> np.uint64(16)) & np.uint64(255)
    pos = (((s >> np.uint64(8)) & np.uint64(255)) << np.uint64(16)) | ((s >> np.uint64(24)) << np.uint64(8)) \
        | (s & np.uint64(255))
    return d, pos


def bucket_pos(k, part, j, v):
    """Position v of bucket j of index part `part`, the index in 2^k parts:
    the part is pos >> (24-k), the bucket (pos >> (11-k)) & 8191."""
    return (np.asarray(part).astype(np.uint64) << np.uint64(24 - k)) \
        | (np.asarray(j).astype(np.uint64) << np.uint64(K_REM_BITS - k)) | np.asarray(v).astype(np.uint64)


def index_spill(m0, k):
    """CPU model of k_m0_index over maxSignal m0 with 2^k parts per slice:
    {slice << k | part: values in its spill list's queue}.  A bucket of n <= 8
    values sits in its header; past 8, 7 in the header and 8 in an overflow
    block while blocks last (1983 per part), the rest spilled: n - 15 with a
    block, n - 7 without.  Which buckets get the blocks depends on the order
    of the atomics, so past the pool the wanting buckets must be equally
    large for the total to be determined."""
    d, pos = slice_pos(m0)
    b = ((d << np.uint64(24)) | pos) >> np.uint64(K_REM_BITS - k)
    ub, n = np.unique(b, return_counts=True)
    part = ub >> np.uint64(13)
    out = {}
    for p in np.unique(part[n > K_HDR]):
        nn = n[(part == p) & (n > K_HDR)].astype(np.int64)
        if nn.size <= K_OV_USABLE:
            sp = np.maximum(nn - (K_HDR - 1 + K_BLK), 0).sum()
        else:
            assert (nn == nn[0]).all()
            n0 = int(nn[0])
            sp = K_OV_USABLE * max(n0 - (K_HDR - 1 + K_BLK), 0) + (nn.size - K_OV_USABLE) * (n0 - (K_HDR - 1))
        out[int(p)] = int(sp)
    return out


def unproven(spill):
    """Members the index cannot prove: the spilled values past the list."""
    return sum(max(0, s - K_SPILL) for s in spill.values())


def _check_model():
    """The mirrored numbers the constructions below rest on, checked on the
    CPU once before the first GPU run (fixture C)."""
    assert K_BUCKETS == 1 << (24 - K_REM_BITS) and K_WG_CAP == 4 * K_SURV_CAP // (256 * K_PARTS)
    rng = np.random.default_rng(7000)
    s = rng.integers(0, 1 << 32, size=1000, dtype=np.uint64).astype(np.uint32)
    d, pos = slice_pos(s)
    assert np.array_equal(sig(d, pos), s) and np.array_equal(d, (s >> 16) & 255)
    for k in (0, 1, 2):
        p = bucket_pos(k, (1 << k) - 1, K_BUCKETS - 1, (1 << (K_REM_BITS - k)) - 1)
        assert int(p) == (1 << 24) - 1
        p = bucket_pos(k, 1 if k else 0, 5, 3)
        assert int(p) >> (24 - k) == (1 if k else 0) and (int(p) >> (K_REM_BITS - k)) & (K_BUCKETS - 1) == 5
        nv = 1 << (K_REM_BITS - k)
        # (b): 9-member buckets past the pool spill 2 values each; (c): 16-member ones 1 each; (d): a full bucket
        for nb, occ, want in ((1983, 9, 0), (1984, 9, 2), (2100, 9, 234), (2283, 9, 600), (512, 16, 512),
                              (513, 16, 513), (1, nv, nv - 15)):
            m = sig(3, bucket_pos(k, 0, np.repeat(np.arange(nb), occ), np.tile(np.arange(occ), nb)))
            assert index_spill(m, k).get(3 << k, 0) == want
        assert [max(0, nv - 15 - K_SPILL) for nv in (2048, 1024, 512)] == [1521, 497, 0]
        # (e): the shares of a slice run of L entries among the part's workgroups
        g = K_PARTS >> k
        assert max(_shares(g * K_WG_CAP, g)) == K_WG_CAP and max(_shares(g * K_WG_CAP + 1, g)) == K_WG_CAP + 1


def _shares(n, g):
    """k_m0_filter's split of a slice run of n entries among g workgroups."""
    return [n * (x + 1) // g - n * x // g for x in range(g)]


# ---- batches -------------------------------------------------------------------
def _records(rng, entries, nrec):
    """The entries shuffled over nrec records of mixed length, some empty."""
    vals = np.asarray(entries, np.uint32)[rng.permutation(len(entries))]
    cuts = rng.integers(0, vals.size + 1, size=nrec - 1)
    cuts[rng.integers(0, nrec - 1, size=nrec // 6)] = cuts[rng.integers(0, nrec - 1, size=nrec // 6)]
    off = np.concatenate([[0], np.sort(cuts), [vals.size]]).astype(np.uint64)
    assert (np.diff(off.astype(np.int64)) == 0).any()
    return vals, off


def _other(rng, n, avoid):
    """Ordinary members outside the slices under test, none of their buckets
    past its header (so the index proves every one of them)."""
    s = np.unique(rng.integers(0, 1 << 32, size=n, dtype=np.uint64).astype(np.uint32))
    s = s[~np.isin((s >> 16) & 255, avoid)]
    d, pos = slice_pos(s)
    assert np.unique(((d << np.uint64(24)) | pos) >> np.uint64(K_REM_BITS), return_counts=True)[1].max() <= K_HDR
    return s


def _fresh(rng, n, members, avoid=()):
    """n distinct signals outside `members` and outside the slices `avoid`."""
    s = np.unique(rng.integers(0, 1 << 32, size=2 * n + 16, dtype=np.uint64).astype(np.uint32))
    s = s[~np.isin(s, members) & ~np.isin((s >> 16) & 255, list(avoid))]
    assert s.size >= n
    return s[rng.permutation(s.size)[:n]]


def _neighbours(rng, n, members):
    """n distinct non-members at pos +- 1 of members, in the members' slices
    (all there are, around a full bucket)."""
    d, pos = slice_pos(members)
    cd = np.concatenate([d, d])
    cp = np.concatenate([pos.astype(np.int64) - 1, pos.astype(np.int64) + 1])
    ok = (cp >= 0) & (cp < (1 << 24))
    c = np.unique(sig(cd[ok], cp[ok]))
    c = c[~np.isin(c, members)]
    assert c.size >= min(n, 2)
    return c[rng.permutation(c.size)[:n]]


def _run(C, ctx, m0, vals, off, expect, survivors=None, newset=True):
    """One batch through sg_triage_batch (flags only) on fresh sets against
    the oracle, the branch taken, and the survivor count."""
    u0, f0 = ctx.counter("m0_filter_used"), ctx.counter("m0_filter_fallback")
    ms, ns = C.SignalSet(ctx), C.SignalSet(ctx) if newset else None
    if len(m0):
        C.SignalAdd(ms, m0)
    got, _, _ = C.triage_batch(ms, ns, vals, off, want_diff=False, ctx=ctx)
    du, df = ctx.counter("m0_filter_used") - u0, ctx.counter("m0_filter_fallback") - f0
    sv = ctx.counter("m0_filter_survivors")
    om, on = O.OSet(m0 if len(m0) else None), O.OSet() if newset else None
    exp = O.triage_flags_only(om, on, vals, off)
    assert np.array_equal(got, exp)
    assert np.array_equal(ms.export(), om.export())
    if newset:
        assert np.array_equal(ns.export(), on.export())
        ns.close()
    ms.close()
    _branch(expect, du, df)
    if survivors is not None:
        assert sv == survivors, (sv, survivors)
    return exp


def _branch(expect, du, df):
    if expect == "used":
        assert du == 1 and df == 0, (du, df)
    elif expect == "fallback":
        assert df == 1 and du == 0, (du, df)


def _bucket_members(rng, k, d, part, js, occ):
    """occ members at random positions in each bucket js of (d, part)."""
    nv = 1 << (K_REM_BITS - k)
    v = np.argsort(rng.random((len(js), nv)), axis=1)[:, :occ]
    return sig(d, bucket_pos(k, part, np.repeat(np.asarray(js), occ), v.reshape(-1)))


def _one_part_case(C, ctx, rng, k, d, part, nb, occ, hits):
    """nb buckets of occ members in one index part, every member hit `hits`
    times, q non-members (neighbours of members, v = 0 of other buckets of
    the part, and fresh ones of other slices): "used", survivors = q + hits x (members past the index's
    capacity).  Returns the part's spill total."""
    members = _bucket_members(rng, k, d, part, rng.permutation(K_BUCKETS)[:nb], occ)
    assert np.unique(members).size == nb * occ
    other = _other(rng, 30_000, [d])
    m0 = np.concatenate([members, other])
    spill = index_spill(m0, k)
    assert set(spill) <= {(d << k) | part}
    near = _neighbours(rng, 150, members)
    same = np.unique(sig(d, bucket_pos(k, part, rng.integers(0, K_BUCKETS, size=60), 0)))  # of the part's other buckets
    same = same[~np.isin(same, members)]
    non = np.concatenate([near, near[:40], same, _fresh(rng, 150, m0, [d])])
    # (all the slice's survivors fit one workgroup's region wherever they fall)
    assert near.size + 40 + same.size + hits * unproven(spill) <= K_WG_CAP
    entries = np.concatenate([np.repeat(members, hits), non, other[rng.integers(0, other.size, size=10_000)]])
    vals, off = _records(rng, entries, 2500)
    _run(C, ctx, m0, vals, off, "used", survivors=non.size + hits * unproven(spill))
    return spill.get((d << k) | part, 0)


# ---- a. bucket occupancy edges ---------------------------------------------------
@pytest.mark.parametrize("k", [0, 1, 2])
def test_bucket_occupancy_edges(C, ctx, ctx_option, k):
    """In three slices and every index part of them: buckets of exactly 1, 7,
    8 (the header full), 9 (the first overflow value), 15 (the block full) and
    16 members (the first spilled value), among them a part's first and last
    bucket and a bucket's first and last position, and 60 more 16-member
    buckets per part (the spill list in use, far from full).  Every member is
    hit three times: none may survive.  The survivors are exactly the
    non-member entries: neighbours (pos +- 1) of members, v = 0 of empty
    buckets, some repeated."""
    ctx_option(ctx, "m0_filter", 1)
    ctx_option(ctx, "m0_filter_halves", k)
    rng = np.random.default_rng(7100 + k)
    nv = 1 << (K_REM_BITS - k)
    slices = [0, 77, 255]
    occs = [1, 7, 8, 9, 15, 16] * 2 + [16] * 60
    mem, empty = [], []
    for d in slices:
        for part in range(1 << k):
            js = 1 + rng.permutation(K_BUCKETS - 2)[: len(occs) + 8]
            js[0], js[1] = 0, K_BUCKETS - 1
            for i, (j, n) in enumerate(zip(js, occs)):
                if i < 6:  # with the bucket's first and last position
                    v = np.concatenate([[0], [nv - 1][: n - 1], 1 + rng.permutation(nv - 2)[: max(n - 2, 0)]])
                elif n == 1:
                    v = np.array([nv - 1])
                else:
                    v = rng.permutation(nv)[:n]
                assert np.unique(v).size == n
                mem.append(sig(d, bucket_pos(k, part, j, v)))
            empty.append(sig(d, bucket_pos(k, part, js[len(occs):], 0)))
    members = np.concatenate(mem)
    assert np.unique(members).size == members.size == len(slices) * (1 << k) * sum(occs)
    other = _other(rng, 50_000, slices)
    m0 = np.concatenate([members, other])
    spill = index_spill(m0, k)
    assert sorted(spill) == sorted((d << k) | p for d in slices for p in range(1 << k))
    assert set(spill.values()) == {62} and unproven(spill) == 0
    near, empty = _neighbours(rng, 600, members), np.concatenate(empty)
    assert not np.isin(empty, m0).any()
    non = np.concatenate([near, near[:100], empty])
    assert non.size < K_WG_CAP
    entries = np.concatenate([np.repeat(members, 3), non, other[rng.integers(0, other.size, size=20_000)]])
    vals, off = _records(rng, entries, 3000)
    exp = _run(C, ctx, m0, vals, off, "used", survivors=non.size)
    assert 0 < exp.sum() <= near.size + empty.size


# ---- b. overflow pool full ---------------------------------------------------------
@pytest.mark.parametrize("k", [0, 1, 2])
def test_overflow_pool_full(C, ctx, ctx_option, k):
    """9-member buckets in one index part: 1983 fill the pool exactly, every
    bucket past it keeps 7 values and spills 2 (1984: 2, 2100: 234 -- the list
    holds them); 1983 + 300 spill 600 against 512, so 88 members -- which ones
    is the atomics' order -- are unproven and their 3 hits each survive."""
    ctx_option(ctx, "m0_filter", 1)
    ctx_option(ctx, "m0_filter_halves", k)
    rng = np.random.default_rng(7200 + k)
    got = [_one_part_case(C, ctx, rng, k, 41, (1 << k) - 1, nb, 9, 3)
           for nb in (K_OV_USABLE, K_OV_USABLE + 1, 2100, K_OV_USABLE + 300)]
    assert got == [0, 2, 234, 600]


# ---- c. spill list 512 / 513 ----------------------------------------------------------
@pytest.mark.parametrize("k", [0, 1, 2])
def test_spill_list_full(C, ctx, ctx_option, k):
    """16-member buckets in one index part spill one value each: 512 fill the
    list (no member survives), the 513th bucket's value is past it (3 hits
    survive)."""
    ctx_option(ctx, "m0_filter", 1)
    ctx_option(ctx, "m0_filter_halves", k)
    rng = np.random.default_rng(7300 + k)
    got = [_one_part_case(C, ctx, rng, k, 200, 0, nb, 16, 3) for nb in (K_SPILL, K_SPILL + 1)]
    assert got == [512, 513]


# ---- d. a full bucket -----------------------------------------------------------------
@pytest.mark.parametrize("k", [0, 1, 2])
def test_full_bucket(C, ctx, ctx_option, k):
    """Every position of one bucket a member, each hit once: 15 proven by the
    header and its block, 512 by the spill list, the rest (1521, 497, 0) only
    by the tail's bitmap test -- nothing but the q non-members is new."""
    ctx_option(ctx, "m0_filter", 1)
    ctx_option(ctx, "m0_filter_halves", k)
    rng = np.random.default_rng(7400 + k)
    nv = 1 << (K_REM_BITS - k)
    sp = _one_part_case(C, ctx, rng, k, 128, (1 << k) // 2, 1, nv, 1)
    assert sp == nv - 15 and max(0, sp - K_SPILL) == [1521, 497, 0][k]


# ---- e. region edge ----------------------------------------------------------------------
@pytest.mark.parametrize("k", [0, 1, 2])
def test_region_edge(C, ctx, ctx_option, k):
    """maxSignal without a member in slice 9; the batch holds L entries of it,
    all in position part 0 (values repeated across records: first owners),
    among hits of other slices.  L = (8 >> k) x 2048 fills the region of every
    workgroup of that part exactly: "used"; one more: "fallback"."""
    ctx_option(ctx, "m0_filter", 1)
    ctx_option(ctx, "m0_filter_halves", k)
    rng = np.random.default_rng(7500 + k)
    d, g = 9, K_PARTS >> k
    other = _other(rng, 50_000, [d])
    for n, expect in ((g * K_WG_CAP, "used"), (g * K_WG_CAP + 1, "fallback")):
        pool = rng.integers(0, 1 << (24 - k), size=n // 3)
        hot = sig(d, pool[rng.integers(0, pool.size, size=n)])
        vals, off = _records(rng, np.concatenate([hot, other[rng.integers(0, other.size, size=30_000)]]), 2500)
        assert int((((vals >> 16) & 255) == d).sum()) == n
        assert max(_shares(n, g)) == (K_WG_CAP if expect == "used" else K_WG_CAP + 1)
        exp = _run(C, ctx, other, vals, off, expect, survivors=n if expect == "used" else None)
        assert exp.sum() > 100


# ---- f. launch cap and tail at load --------------------------------------------------------
@pytest.mark.parametrize("variant", ["contended", "distinct"])
def test_launch_cap_and_tail_load(C, ctx, ctx_option, variant):
    """An empty maxSignal and exactly 2^20 entries: every one survives, the
    launch cap is met, not passed ("used"); one more: "fallback".  contended:
    values drawn from 300K (atomicMin among a signal's owners); distinct: 2^20
    different signals, the tail's 2^21-slot table at load 0.5."""
    ctx_option(ctx, "m0_filter", 1)
    ctx_option(ctx, "m0_filter_halves", 0)
    rng = np.random.default_rng(7600)
    none = np.zeros(0, np.uint32)
    for n, expect in ((K_SURV_CAP, "used"), (K_SURV_CAP + 1, "fallback")):
        if variant == "contended":
            pool = np.unique(rng.integers(0, 1 << 32, size=300_000, dtype=np.uint64).astype(np.uint32))
            entries = pool[rng.integers(0, pool.size, size=n)]
        else:  # (an odd multiplier: a bijection of the 32-bit values)
            entries = (rng.permutation(n).astype(np.uint64) * np.uint64(0x9E3779B1)) & np.uint64(SENT)
            entries = entries.astype(np.uint32)
            assert np.unique(entries).size == n
        vals, off = _records(rng, entries, 30_000)
        per = np.bincount((vals >> 16) & 255, minlength=256)
        assert (-(-per // K_PARTS)).max() <= K_WG_CAP  # no region overflows: only the total decides
        _run(C, ctx, none, vals, off, expect, survivors=n if expect == "used" else None)


# ---- g. tiny runs ---------------------------------------------------------------------------
def test_tiny_runs(C, ctx, ctx_option):
    """Batches of a few entries (most filter workgroups without any), signals
    0 and 0xFFFFFFFF, values packed into one bucket or spread by the
    golden-ratio multiply; then 1..9 entries of one slice, the index in 1, 2
    and 4 parts."""
    ctx_option(ctx, "m0_filter", 1)
    ctx_option(ctx, "m0_filter_halves", 0)
    rng = np.random.default_rng(7700)
    ms, ns = C.SignalSet(ctx), C.SignalSet(ctx)

    def run(m0, vals, off):
        ms.clear()
        ns.clear()
        if m0.size:
            C.SignalAdd(ms, m0)
        u0, f0 = ctx.counter("m0_filter_used"), ctx.counter("m0_filter_fallback")
        got, _, _ = C.triage_batch(ms, ns, vals, off, want_diff=False, ctx=ctx)
        du, df = ctx.counter("m0_filter_used") - u0, ctx.counter("m0_filter_fallback") - f0
        om, on = O.OSet(m0 if m0.size else None), O.OSet()
        assert np.array_equal(got, O.triage_flags_only(om, on, vals, off))
        assert np.array_equal(ms.export(), om.export()) and np.array_equal(ns.export(), on.export())
        if vals.size:  # (at most 50 members, all in the header, block and spill list of their buckets)
            assert (du, df) == (1, 0)
            assert ctx.counter("m0_filter_survivors") == int((~np.isin(vals, m0)).sum())
        else:
            assert (du, df) == (0, 0)

    for it in range(60):
        nrec = int(rng.integers(0, 40))
        recs = [[int(x) for x in rng.integers(0, 80, size=rng.integers(0, 14))] for _ in range(nrec)]
        if it % 4 == 0 and nrec:
            recs[0] += [0, SENT, SENT]
        m0 = sorted(set(int(x) for x in rng.integers(0, 80, size=rng.integers(0, 50))))
        if it % 3 == 0:  # spread over the slices
            recs = [[(x * 0x9E3779B1) & SENT for x in r] for r in recs]
            m0 = sorted(set((x * 0x9E3779B1) & SENT for x in m0))
        vals = np.array([x for r in recs for x in r], dtype=np.uint32)
        off = np.concatenate([[0], np.cumsum([len(r) for r in recs])]).astype(np.uint64)
        run(np.array(m0, np.uint32), vals, off)
    for k in (0, 1, 2):
        ctx.set_option("m0_filter_halves", k)
        for n in range(1, 10):
            vals = sig(int(rng.integers(0, 256)), rng.integers(0, 1 << 24, size=n))
            vals[n // 2:] = vals[rng.integers(0, n, size=n - n // 2)]  # (repeats)
            cuts = np.sort(rng.integers(0, n + 1, size=int(rng.integers(0, 4))))
            off = np.concatenate([[0], cuts, [n]]).astype(np.uint64)
            run(np.unique(vals[: n // 3]), vals, off)
    ms.close()
    ns.close()


# ---- h. geometry for the tail's record lookup -------------------------------------------------
def test_tail_record_lookup_geometry(C, ctx, ctx_option):
    """The tail finds a survivor's record from its pass-1 tile (a search over
    the slice's run starts) and the 8-bit record in the tile.  Low-novelty
    batches ("used") whose new signals sit where that lookup can go wrong: in
    the last tile of a record spanning three, behind tiles cut by the
    256-record cap in a second record group, around runs of >= 256 empty
    records, and repeated in the last record of group 0 and the first of
    group 1 (the earlier record owns it)."""
    ctx_option(ctx, "m0_filter", 1)
    ctx_option(ctx, "m0_filter_halves", 0)
    rng = np.random.default_rng(7800)
    m0 = np.unique(rng.integers(0, 1 << 32, size=200_000, dtype=np.uint64).astype(np.uint32))
    new = _fresh(rng, 16, m0)

    def batch(lens, novelty):
        off = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
        vals = m0[rng.integers(0, m0.size, size=int(off[-1]))]
        f = rng.random(vals.size) < novelty
        vals[f] = rng.integers(0, 1 << 32, size=int(f.sum()), dtype=np.uint64).astype(np.uint32)
        return vals, off.astype(np.int64)

    # a record of 40K entries from tile 0 into tile 2, its only new signal the last entry
    vals, off = batch(np.concatenate([rng.integers(0, 30, size=200), [40_000], rng.integers(0, 30, size=200)]), 0.0)
    assert (off[200] // K_TILE, (off[201] - 1) // K_TILE) == (0, 2)
    vals[off[201] - 1] = new[0]
    exp = _run(C, ctx, m0, vals, off.astype(np.uint64), "used", survivors=1)
    assert exp.sum() == 1 and exp[200] == 1
    # 70,000 records of 0..3 entries: two record groups, every tile cut by the
    # record cap; a new signal in the last record of group 0 and the first of group 1
    lens = rng.integers(0, 4, size=70_000)
    lens[K_GROUP - 1: K_GROUP + 1] = 2
    vals, off = batch(lens, 1e-3)
    vals[off[K_GROUP - 1]: off[K_GROUP + 1]] = [new[1], m0[0], m0[1], new[1]]
    exp = _run(C, ctx, m0, vals, off.astype(np.uint64), "used")
    assert exp[K_GROUP - 1] == 1 and exp[K_GROUP] == 0 and 20 < exp.sum() < 1000
    # runs of 300 and 700 empty records around one record, then more: each
    # non-empty record ends in a new signal of its own and nothing else is new
    lens = np.concatenate([np.zeros(300, np.int64), [9000], np.zeros(700, np.int64), [20_000], np.zeros(64, np.int64),
                           [3], np.zeros(130, np.int64), [5]])
    vals, off = batch(lens, 0.0)
    owners = np.flatnonzero(lens)
    vals[off[owners + 1] - 1] = new[2: 2 + owners.size]
    exp = _run(C, ctx, m0, vals, off.astype(np.uint64), "used", survivors=owners.size)
    assert np.array_equal(np.flatnonzero(exp), owners)


# ---- i. callers -----------------------------------------------------------------------------------
def _counters(ctx):
    return ctx.counter("m0_filter_used"), ctx.counter("m0_filter_fallback")


def test_accept_batch_through_filter(C, ctx, ctx_option):
    """sg_accept_batch (manager.go:907-912) runs the flags path without a
    newSignal set and adds the accepted inputs' coverage afterwards: a
    low-novelty batch of 3000 inputs through the filter's tail, and a fresh
    one crowding one slice past its regions (pass 2 from a plane-less pass 1)."""
    ctx_option(ctx, "m0_filter", 1)
    ctx_option(ctx, "m0_filter_halves", 0)
    rng = np.random.default_rng(7900)
    pool = np.unique(rng.integers(0, 1 << 32, size=100_000, dtype=np.uint64).astype(np.uint32))
    n = 3000
    for kind, expect in (("low", "used"), ("fresh", "fallback")):
        cs, cc = C.SignalSet(ctx), C.SignalSet(ctx)
        oc, ov = O.OSet(), O.OSet()
        if kind == "low":
            C.SignalAdd(cs, pool)
            oc.add(pool)
            sigs = [np.unique(pool[rng.integers(0, pool.size, size=int(rng.integers(0, 40)))]) for _ in range(n)]
            for i in rng.integers(0, n, size=60):
                sigs[i] = np.unique(np.concatenate([sigs[i], _fresh(rng, 1, pool)]))
        else:  # slice 0 only: ~30K survivors for its 8 regions of 2048
            sigs = [np.unique((rng.integers(0, 1 << 16, size=int(rng.integers(5, 16)))
                               | (rng.integers(0, 256, size=1) << 24)).astype(np.uint32)) for _ in range(n)]
            for i in rng.integers(1, n, size=300):  # (inputs without anything new: an earlier input's signal)
                sigs[i] = sigs[i - 1]
            assert sum(len(s) for s in sigs) > K_PARTS * K_WG_CAP + 5000
        covs = [np.unique(rng.integers(0, 1 << 30, size=int(rng.integers(0, 30))).astype(np.uint32)) for _ in range(n)]
        sv, so = C.to_csr(sigs)
        cv, co = C.to_csr(covs)
        u0, f0 = _counters(ctx)
        acc = C.accept_batch(cs, cc, sv, so, cv, co, ctx=ctx)
        u1, f1 = _counters(ctx)
        eacc = O.accept_batch(oc, ov, sv, so, cv, co)
        assert np.array_equal(acc, eacc)
        assert 0 < eacc.sum() < n
        assert np.array_equal(cs.export(), oc.export())
        assert np.array_equal(cc.export(), ov.export())
        _branch(expect, u1 - u0, f1 - f0)
        cs.close()
        cc.close()


def test_triage_traces_fallback(C, ctx, ctx_option):
    """sg_triage_traces with the filter forced on a fresh trace batch of more
    than 2^20 new edges: the survivors overflow, the digit plane is made from
    the pass-1 entries (k_top_plane) and pass 2 runs on a trace pass 1."""
    ctx_option(ctx, "m0_filter", 1)
    ctx_option(ctx, "m0_filter_halves", 0)
    rng = np.random.default_rng(7901)
    ncalls = 6000
    call_off = np.concatenate([[0], np.cumsum(rng.integers(160, 210, size=ncalls))]).astype(np.uint64)
    pcs = rng.integers(0, 1 << 32, size=int(call_off[-1]), dtype=np.uint64).astype(np.uint32)
    pcs[rng.integers(0, pcs.size, size=pcs.size // 50)] = pcs[rng.integers(0, pcs.size, size=pcs.size // 50)]
    es, eo = O.exec_signal(pcs, call_off, np.arange(ncalls + 1, dtype=np.uint64))
    assert K_SURV_CAP + 20_000 < np.unique(es).size and pcs.size < 1_150_000
    om, on = O.OSet(), O.OSet()
    exp = O.triage_flags_only(om, on, es, eo)
    ms, ns = C.SignalSet(ctx), C.SignalSet(ctx)
    u0, f0 = _counters(ctx)
    got = C.triage_traces(ms, ns, pcs, call_off, ctx=ctx)
    u1, f1 = _counters(ctx)
    assert np.array_equal(got, exp)
    assert np.array_equal(ms.export(), om.export()) and np.array_equal(ns.export(), on.export())
    _branch("fallback", u1 - u0, f1 - f0)
    ms.close()
    ns.close()


def test_triage_traces_queued_through_filter(C, ctx, ctx_option):
    """sg_triage_traces_queued with the filter forced, low novelty: the flags,
    both sets and the queued calls' executor-exact lists."""
    ctx_option(ctx, "m0_filter", 1)
    ctx_option(ctx, "m0_filter_halves", 0)
    rng = np.random.default_rng(7902)
    ncalls = 600
    lens = rng.integers(0, 300, size=ncalls)
    lens[rng.integers(0, ncalls, size=80)] = 0
    call_off = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    prog_off = np.unique(np.concatenate([[0, ncalls], rng.integers(0, ncalls, size=70)])).astype(np.uint64)
    prog_off = np.sort(np.concatenate([prog_off, prog_off[5:6]]))  # (an empty program)
    p = (0x81000000 + 16 * (np.minimum(rng.zipf(1.1, size=int(call_off[-1])), 1 << 14) - 1)).astype(np.uint32)
    es, eo = O.exec_signal(p, call_off, prog_off)
    m0 = np.unique(es[: int(eo[ncalls * 9 // 10])])
    om, on = O.OSet(m0), O.OSet()
    ef = O.triage_flags_only(om, on, es, eo)
    assert 0 < ef.sum() < ncalls // 4
    ms, ns = C.SignalSet(ctx), C.SignalSet(ctx)
    C.SignalAdd(ms, m0)
    u0, f0 = _counters(ctx)
    flags, vals, off = C.triage_traces_queued(ms, ns, p, call_off, prog_off, ctx=ctx)
    u1, f1 = _counters(ctx)
    assert np.array_equal(flags, ef)
    for c in range(ncalls):
        want = es[int(eo[c]):int(eo[c + 1])] if ef[c] else np.zeros(0, np.uint32)
        assert np.array_equal(vals[int(off[c]):int(off[c + 1])], want), c
    assert np.array_equal(ms.export(), om.export()) and np.array_equal(ns.export(), on.export())
    _branch("used", u1 - u0, f1 - f0)
    ms.close()
    ns.close()


def test_triage_batch_without_newsignal(C, ctx, ctx_option):
    """newsig = NULL through the filter's tail (k_m0_tail_flush without a
    newSignal bitmap)."""
    ctx_option(ctx, "m0_filter", 1)
    ctx_option(ctx, "m0_filter_halves", 0)
    rng = np.random.default_rng(7903)
    m0 = np.unique(rng.integers(0, 1 << 32, size=100_000, dtype=np.uint64).astype(np.uint32))
    non = _fresh(rng, 500, m0)
    entries = np.concatenate([m0[rng.integers(0, m0.size, size=80_000)], non, non[:200], [0, SENT]]).astype(np.uint32)
    vals, off = _records(rng, entries, 4000)
    exp = _run(C, ctx, m0, vals, off, "used", survivors=non.size + 200 + 2 - int(np.isin([0, SENT], m0).sum()),
               newset=False)
    assert 0 < exp.sum() <= 502


# ---- j. shared auto state ---------------------------------------------------------------------------
def test_shared_auto_state_across_callers(C):
    """The auto regime's state (last slice filtered or partitioned, its queued
    fraction, the back-off) lives on the context and is shared by every
    caller of the flags path.  One fresh context left in auto, the callers
    interleaved in a fixed order: whichever regime each call runs in, every
    result and every set equals the oracle's."""
    ctx = C.Context(0)
    try:
        assert ctx.get_option("m0_filter") == -1
        rng = np.random.default_rng(8000)
        ms, ns, cs, cc = (C.SignalSet(ctx) for _ in range(4))
        om, on, oc, ov = O.OSet(), O.OSet(), O.OSet(), O.OSet()
        pool = np.unique(rng.integers(0, 1 << 32, size=150_000, dtype=np.uint64).astype(np.uint32))
        C.SignalAdd(ms, pool)
        om.add(pool)
        C.SignalAdd(cs, pool[::2])
        oc.add(pool[::2])
        sums = {}

        def fuzz(novelty, nrec, maxlen):
            lens = rng.integers(0, maxlen, size=nrec)
            off = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
            vals = pool[rng.integers(0, pool.size, size=int(off[-1]))]
            f = rng.random(vals.size) < novelty
            vals[f] = rng.integers(0, 1 << 32, size=int(f.sum()), dtype=np.uint64).astype(np.uint32)
            got, _, _ = C.triage_batch(ms, ns, vals, off, want_diff=False, ctx=ctx)
            exp = O.triage_flags_only(om, on, vals, off)
            assert np.array_equal(got, exp)
            return exp

        def low():
            return fuzz(1e-3, 8000, 40)

        def fresh():
            return fuzz(1.0, 8000, 40)

        def burst():  # ~1.1M new signals: past the launch cap whenever the filter is tried
            return fuzz(1.0, 30_000, 75)

        def accept():
            sigs = [np.unique(pool[rng.integers(0, pool.size, size=int(rng.integers(0, 30)))]) for _ in range(1500)]
            for i in rng.integers(0, 1500, size=40):
                sigs[i] = np.unique(np.concatenate([sigs[i], rng.integers(0, 1 << 32, size=2, dtype=np.uint64)
                                                    .astype(np.uint32)]))
            covs = [np.unique(rng.integers(0, 1 << 30, size=int(rng.integers(0, 20))).astype(np.uint32))
                    for _ in range(1500)]
            sv, so = C.to_csr(sigs)
            cv, co = C.to_csr(covs)
            acc = C.accept_batch(cs, cc, sv, so, cv, co, ctx=ctx)
            eacc = O.accept_batch(oc, ov, sv, so, cv, co)
            assert np.array_equal(acc, eacc)
            return eacc

        def traces():
            ncalls = 1500
            call_off = np.concatenate([[0], np.cumsum(rng.integers(0, 120, size=ncalls))]).astype(np.uint64)
            p = (0x81000000 + 16 * (np.minimum(rng.zipf(1.1, size=int(call_off[-1])), 1 << 14) - 1)).astype(np.uint32)
            es, eo = O.exec_signal(p, call_off, np.arange(ncalls + 1, dtype=np.uint64))
            got = C.triage_traces(ms, ns, p, call_off, ctx=ctx)
            exp = O.triage_flags_only(om, on, es, eo)
            assert np.array_equal(got, exp)
            return exp

        steps = [low, accept, fresh, traces, low, burst, accept, low, traces, fresh, accept, low, low]
        for i, step in enumerate(steps):
            res = step()
            sums.setdefault(step.__name__, []).append(int(res.sum()))
            assert np.array_equal(ms.export(), om.export()), (i, step.__name__)
            assert np.array_equal(ns.export(), on.export()), (i, step.__name__)
            assert np.array_equal(cs.export(), oc.export()), (i, step.__name__)
            assert np.array_equal(cc.export(), ov.export()), (i, step.__name__)
        # the inputs were what they were meant to be
        assert all(0 < s < 800 for s in sums["low"]) and all(s > 6000 for s in sums["fresh"])
        assert sums["burst"][0] > 25_000 and all(s > 0 for s in sums["accept"]) and sums["traces"][0] > 0
        for s in (ms, ns, cs, cc):
            s.close()
    finally:
        ctx.close()
