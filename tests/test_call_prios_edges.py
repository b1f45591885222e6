"""The call-priority kernels (sg_call_prios.hip) at their own constants: the 13/7/6/6-bit entry, the 40,960-cell
row band and its edges, the parts of the id stream, the 64-place wave window, the long path's 256-block stride
with LDS reused, the 2^24 saturation behind a 64-bit count, the finish's four-wave reductions and its
256-column scan with a carry.

tests/call_prios_cases.py builds each family (deterministic) and restates the launch arithmetic (band_plan,
pinned to sg_plan.h's through tests/cpp/plan_test.cc).  On the CPU: each family's conditions, asserted on the
case itself; a positional model of the four kernels (entries, band ownership, the wave's window, the long loop,
the four-wave combine and the stepped scan) equal to the oracle on every family; and the model with each named
mistake, caught by a family.  On the GPU: counts, dynamic, prios and run bit-exact against
tests/call_prios_oracle.py through add + prios and through from_progs.  No tolerance anywhere."""
import os
import re
import subprocess
import time

import numpy as np
import pytest

from tests import call_prios_cases as K
from tests import call_prios_checks as CK
from tests import call_prios_oracle as OR
from tests.conftest import ROOT

U8, U32, U64, I32, I64, F32 = np.uint8, np.uint32, np.uint64, np.int32, np.int64, np.float32
NONE = 0xFFFFFFFF  # kPrioNone
ID_BITS, N_BITS, POS_BITS = 13, 7, 6
SAT = 1 << 24

FAMILIES = ([("band_sizes", n) for n in K.BAND_SIZES]
            + [("production_shape",), ("max_calls",), ("entry_fields",), ("many_long_programs",), ("saturation_edges",)]
            + [("finish_rows", n, d) for n in K.FINISH_SIZES for d in (False, True)])
SMALL = [k for k in FAMILIES if k[0] not in ("max_calls", "production_shape")]
_memo = {}


def _id(key):
    return "-".join(str(x) for x in key)


@pytest.fixture(scope="module", autouse=True)
def _drop_cases():
    yield
    _memo.clear()   # (the 8,192-call matrices are some GB)


def get(key):
    """(case, (counts, dynamic, prios, run)) of a family, built and put through the oracle once, shared, read-only"""
    if key not in _memo:
        c = getattr(K, key[0])(*key[1:])
        exp = OR.everything(c["ids"], c["off"], c["ncalls"], c["mmap"], c["static"], c["enabled"])
        for a in (c["ids"], c["off"], c["static"], c["enabled"]) + exp:
            a.setflags(write=False)
        _memo[key] = (c, exp)
    return _memo[key]


# ---- the positional model ------------------------------------------------------------------------
def pack(cid, n, pos, length):
    return cid | n << ID_BITS | pos << (ID_BITS + N_BITS) | (length - 1) << (ID_BITS + N_BITS + POS_BITS)


def ent_id(e):
    return e & ((1 << ID_BITS) - 1)


def ent_n(e):
    return e >> ID_BITS & ((1 << N_BITS) - 1)


def ent_pos(e):
    return e >> (ID_BITS + N_BITS) & ((1 << POS_BITS) - 1)


def ent_len(e):
    return (e >> (ID_BITS + N_BITS + POS_BITS)) + 1


def model_entries(c):
    """k_prio_merge: (ent, longs).  A first occurrence of an id < ncalls that is not mmap becomes an entry at its
    own place; everything else, and every place of a program longer than SHORT_LEN, stays NONE."""
    ids, off, nc, mm = c["ids"].astype(I64), c["off"].astype(I64), c["ncalls"], c["mmap"]
    ent, longs = np.full(ids.size, NONE, I64), []
    for p in range(off.size - 1):
        a0, a1 = off[p], off[p + 1]
        if a1 - a0 > K.SHORT_LEN:
            longs.append(p)
        elif a1 > a0:
            u, first, n = np.unique(ids[a0:a1], return_index=True, return_counts=True)
            keep = (u < nc) & (u != mm)
            ent[a0 + first[keep]] = pack(u[keep], n[keep], first[keep], a1 - a0)
    return ent, longs


def model_counts(c, bug=None):
    """k_prio_band and k_prio_long on k_prio_merge's entries: (counts, info).  info: the furthest cell of the
    counts a band's flush walks to, and the most cells a band asks of LDS."""
    ids, off, nc, mm = c["ids"].astype(I64), c["off"].astype(I64), c["ncalls"], c["mmap"]
    nids = ids.size
    ent, longs = model_entries(c)
    counts = np.zeros(nc * nc, I64)
    rows, nbands, nparts, part, gridy = K.band_plan(nc, nids)
    # the wave's window: for the entry at place ks, lane reads place ks - pos + lane while lane < len
    live = np.flatnonzero(ent != NONE)
    assert (live // part < gridy).all()                      # every place lies in a part of the grid
    e = ent[live]
    lanes = np.arange(K.SHORT_LEN)
    j = (live - np.minimum(ent_pos(e), live))[:, None] + lanes[None, :]
    lim = ent_len(e) + {"lane_le_len": 1, "lane_lt_len_minus_1": -1}.get(bug, 0)
    e2 = ent[np.minimum(j, nids - 1)]
    ok = (lanes[None, :] < lim[:, None]) & (j < nids) & (e2 != NONE) & (ent_id(e2) != ent_id(e)[:, None]) & (ent_id(e2) < nc)
    pi, pl = np.nonzero(ok)
    pa, pb, pv = ent_id(e)[pi], ent_id(e2[pi, pl]), ent_n(e)[pi] * ent_n(e2[pi, pl])
    reach = lds = 0
    for b in range(nbands):                                  # band ownership: r0 <= id < r1, rows of the band in LDS
        r0 = b * rows
        r1 = r0 + rows + {"band_edge_plus_1": 1, "band_edge_minus_1": -1}.get(bug, 0)
        if bug != "last_band_unclamped":
            r1 = min(r1, nc)
        cells = (r1 - r0) * nc
        reach, lds = max(reach, r0 * nc + cells), max(lds, cells)
        own = (pa >= r0) & (pa < r1)
        cell = (pa[own] - r0) * nc + pb[own]
        assert (cell < cells).all()
        np.add.at(counts, r0 * nc + cell, pv[own])
    # the long loop: block blk takes li = blk, blk + nblocks, ...; hist lives in LDS across them
    long_cap = nids // (K.SHORT_LEN + 1) + 1
    nl, nblocks = min(len(longs), long_cap), min(long_cap, 256)
    c2 = counts.reshape(nc, nc)
    for blk in range(min(nblocks, nl)):
        hist = np.zeros(nc, I64)
        for li in range(blk, nl, nblocks):
            if bug == "long_first_round_only" and li >= nblocks:
                break
            if bug != "long_no_reset":
                hist[:] = 0
            seg = ids[off[longs[li]]:off[longs[li] + 1]]
            hist += np.bincount(seg[(seg < nc) & (seg != mm)], minlength=nc)
            lst = np.flatnonzero(hist).astype(np.uint16).astype(I64)   # (the u16 list)
            prod = np.outer(hist[lst], hist[lst])
            if bug == "long_product_32":
                prod &= 0xFFFFFFFF
            np.fill_diagonal(prod, 0)
            c2[np.ix_(lst, lst)] += prod
    return c2.astype(U64), dict(reach=reach, lds=lds, nlong=nl, rows=rows, nbands=nbands, gridy=gridy)


def model_finish(cnt, static, enabled, bug=None, chunk=512):
    """k_prio_finish: thread t of 256 takes the columns j = t mod 256; wave w = t / 64 reduces its own, four LDS
    slots are combined; the scan goes 256 columns a step: a wave's inclusive sums, the waves before it, the carry."""
    nc = cnt.shape[0]
    steps = -(-nc // 256)
    pad = steps * 256 - nc
    waves = 3 if bug == "combine_three_waves" else 4
    dyn, pr, run = np.empty((nc, nc), F32), np.empty((nc, nc), F32), np.empty((nc, nc), I32)
    on = np.asarray(enabled).astype(bool)

    def by_wave(a, fill):
        a = np.pad(a, ((0, 0), (0, pad)), constant_values=fill)
        return a.reshape(a.shape[0], steps, 4, 64)

    for r in range(0, nc, chunk):
        c = cnt[r:r + chunk]
        if bug == "cast_before_min":
            p = np.minimum(c & U64(0xFFFFFFFF), U64(SAT)).astype(F32)
        else:
            p = (np.minimum(c, U64(SAT)) & U64(0xFFFFFFFF)).astype(F32)
        mx = by_wave(p, F32(0)).max(axis=(1, 3))[:, :waves].max(axis=1)
        mn = by_wave(np.where(p != 0, p, F32(1e10)), F32(1e10)).min(axis=(1, 3))[:, :waves].min(axis=1)
        nz = by_wave(p == 0, False).sum(axis=(1, 3))[:, :waves].sum(axis=1)
        with np.errstate(divide="ignore", invalid="ignore"):
            mn = np.where(nz != 0, mn / (F32(2) * nz.astype(F32)), mn).astype(F32)
            q = np.where(p == 0, mn[:, None], p).astype(F32)
            q = ((q - mn[:, None]) / (mx - mn)[:, None]).astype(F32)
            q = (q * F32(0.9)).astype(F32)
            q = (q + F32(0.1)).astype(F32)
            q = np.where(q > 1, F32(1), q)
        q = np.where(mx[:, None] == 0, F32(1), q).astype(F32)
        dyn[r:r + chunk] = q
        q = (q * static[r:r + chunk]).astype(F32)
        pr[r:r + chunk] = q
        v = (q * F32(1000)).astype(F32).astype(I64)
        v[:, ~on] = 0
        v[~on[r:r + chunk], :] = 0
        incl = np.cumsum(by_wave(v, 0), axis=3)
        ssum = incl[:, :, :, 63]
        before = np.cumsum(ssum, axis=2) - ssum                           # the waves before this one
        total = ssum[:, :, :3 if bug == "carry_three_waves" else 4].sum(axis=2)
        carry = np.cumsum(total, axis=1) - total
        if bug == "carry_dropped":
            carry[:] = 0
        out = (carry[:, :, None, None] + before[:, :, :, None] + incl).reshape(c.shape[0], -1)[:, :nc]
        run[r:r + chunk] = (out & 0xFFFFFFFF).astype(U32).view(I32)
    return dyn, pr, run


ADD_BUGS = ("band_edge_plus_1", "band_edge_minus_1", "last_band_unclamped", "lane_le_len", "lane_lt_len_minus_1",
            "long_no_reset", "long_first_round_only", "long_product_32")
FINISH_BUGS = ("cast_before_min", "combine_three_waves", "carry_dropped", "carry_three_waves")
# the families that must tell each mistake (others may as well)
CAUGHT_BY = {"band_edge_plus_1": "band_sizes", "band_edge_minus_1": "band_sizes", "last_band_unclamped": "band_sizes",
             "lane_le_len": "entry_fields", "lane_lt_len_minus_1": "entry_fields",
             "long_no_reset": "many_long_programs", "long_first_round_only": "many_long_programs",
             "long_product_32": "saturation_edges", "cast_before_min": "saturation_edges",
             "combine_three_waves": "finish_rows", "carry_dropped": "finish_rows", "carry_three_waves": "finish_rows"}


# ---- CPU: the restatement ----------------------------------------------------------------------
def test_band_plan_mirror_and_restated_constants(tmp_path):
    src = open(os.path.join(ROOT, "syzkaller_amd", "csrc", "sg_call_prios.hip")).read()
    hdr = open(os.path.join(ROOT, "syzkaller_amd", "csrc", "sg_internal.h")).read()
    assert "kIdBits = %d, kNBits = %d, kPosBits = %d;" % (ID_BITS, N_BITS, POS_BITS) in src
    assert "kPrioNone = 0xFFFFFFFFu;" in src and "kPrioPart = 1ull << 26;" in src and K.PART_MAX == 1 << 26
    assert "kBandT = %d;" % K.BAND_THREADS in src and "kPT = 256;" in src
    assert "kPrioBandCells = %d;" % K.BAND_CELLS in hdr and "kPrioShort = %d;" % K.SHORT_LEN in hdr
    assert "band_plan(t->ncalls, nids, kPrioBandCells, kBandT, kPrioPart)" in src
    assert "std::min<uint64_t>(long_cap, 256)" in src and "nids / (kPrioShort + 1) + 1" in src
    exe = str(tmp_path / "plan_test")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "syzkaller_amd", "csrc"),
                    "-o", exe, os.path.join(ROOT, "tests", "cpp", "plan_test.cc")], check=True)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60, check=True).stdout
    assert re.search(r"^band_plan digest ([0-9a-f]{16})$", out, flags=re.M).group(1) == K.band_plan_digest()
    table = re.findall(r"^band_plan (\d+) (\d+) (\d+) (\d+) (\d+) (\d+) (\d+)$", out, flags=re.M)
    assert len(table) == 60
    for row in table:
        nc, nids, *want = map(int, row)
        assert K.band_plan(nc, nids) == tuple(want), row
    # the sizes the families stand on
    assert K.band_plan(202, 1)[:2] == (202, 1) and K.band_plan(203, 1)[:2] == (201, 2)
    assert K.bands(320) == [(0, 128), (128, 256), (256, 320)] and 128 * 320 == K.BAND_CELLS
    assert K.band_plan(512, 1)[:2] == (80, 7) and 80 * 512 == K.BAND_CELLS and K.bands(512)[-1] == (480, 512)
    assert K.band_plan(513, 1)[:2] == (79, 7)
    assert K.band_plan(1541, 1)[:2] == (26, 60) and K.bands(1541)[-1] == (1534, 1541)
    assert K.band_plan(8192, 1)[:2] == (5, 1639) and K.bands(8192)[-1] == (8190, 8192)
    assert pack(8191, 127, 63, 64) == NONE and pack(8191, 63, K.MAX_N63_POS, 64) == 0xFC17FFFF


# ---- CPU: what each family relies on -------------------------------------------------------------
@pytest.mark.parametrize("ncalls", K.BAND_SIZES)
def test_band_sizes_conditions(ncalls):
    c, (cnt, dyn, pr, run) = get(("band_sizes", ncalls))
    bands = K.bands(ncalls)
    assert len(bands) == {202: 1, 320: 3, 512: 7, 513: 7}[ncalls] and c["edges"] == [r0 for r0, _ in bands[1:]]
    for r0, r1 in bands:                                       # every band populated at both of its ends
        assert cnt[r0].any() and cnt[r1 - 1].any(), (r0, r1)
    progs = [p.tolist() for p in OR.programs(c["ids"], c["off"])]
    last = ncalls - 1
    for r in c["edges"]:
        assert [r - 1, r] in progs and [r, r - 1, r - 1] in progs and c["mmap"] not in (r - 1, r, last)
        assert any(len(p) == K.SHORT_LEN and {r - 1, r, last} <= set(p) for p in progs), r
        assert cnt[r - 1, r] >= 4 and cnt[r, last] >= 1 and cnt[r - 1, last] >= 1
    assert max(len(p) for p in progs) == (K.SHORT_LEN if c["edges"] else 12)   # the band path alone


def test_production_shape_conditions():
    c, (cnt, dyn, pr, run) = get(("production_shape",))
    rows, nbands, nparts, part, gridy = K.band_plan(c["ncalls"], c["ids"].size)
    assert (c["ncalls"], rows, nbands) == (1541, 26, 60) and gridy > 1 and part < c["ids"].size
    lens = np.diff(c["off"].astype(I64))
    assert lens.size == 3000 and lens.min() == 1 and lens.max() == 30
    hot = np.bincount(c["ids"], minlength=1541)
    assert hot.argmax() == c["mmap"] and not cnt[c["mmap"]].any()
    assert sum(bool(cnt[r0:r1].any()) for r0, r1 in K.bands(1541)) == 60   # every band takes part
    print("production_shape: ids", c["ids"].size, "parts", gridy, "of", part, "largest cell", int(cnt.max()))


def test_max_calls_conditions():
    c, (cnt, dyn, pr, run) = get(("max_calls",))
    assert c["ncalls"] == K.MAX_CALLS == 8192 and c["ids"].size <= 4000
    progs = [p.tolist() for p in OR.programs(c["ids"], c["off"])]
    both = [p for p in progs if set(K.MAX_IDS) <= set(p)]
    assert any(len(p) <= K.SHORT_LEN for p in both) and any(len(p) > K.SHORT_LEN for p in both)
    ent, longs = model_entries(c)
    n63 = [int(e) for e in ent if e != NONE and ent_id(e) == 8191 and ent_n(e) == 63 and ent_len(e) == 64]
    assert n63 == [0xFC17FFFF] and bin(n63[0] ^ NONE).count("1") == 6
    assert K.MAX_DISABLED > 8000 and not c["enabled"][K.MAX_DISABLED] and cnt[K.MAX_DISABLED].any()
    assert cnt[8191, 8190] > 1600 and cnt[8191, 0] >= 4 and cnt[8191, 77] == 63 and len(longs) == 2
    assert not cnt[K.MAX_MMAP].any() and (c["ids"] == K.MAX_MMAP).any()
    assert c["static"].shape == (8192, 8192) and (c["static"] == 0).any() and (c["static"] == 1).any()
    print("max_calls: ids", c["ids"].size, "nonzero rows", int(cnt.any(axis=1).sum()), "largest cell", int(cnt.max()))


def test_entry_fields_conditions():
    c, (cnt, dyn, pr, run) = get(("entry_fields",))
    ids, off = c["ids"], c["off"].astype(I64)
    nids = ids.size
    rows, nbands, nparts, part, gridy = K.band_plan(c["ncalls"], nids)
    assert nids == K.ENTRY_NIDS and (nbands, part, gridy) == (1, c["part"], 13) and part == 4096
    start = {int(o): p for p, o in enumerate(off[:-1])}
    bases = K.entry_bases()
    assert [len(b) for b in bases] == [K.SHORT_LEN] * 5 and len(set(bases[3])) == 64 and len(set(bases[4])) == 1
    assert bases[0].index(11) == 63 and bases[0].count(10) == 63 and bases[2].count(20) == bases[2].count(21) == 32
    for kind, shift, at in c["marks"] + [(3, None, c["straddle"]), (3, None, c["ends_on"])]:
        p = start[at]
        assert ids[off[p]:off[p + 1]].tolist() == bases[kind]
        assert ids[off[p - 1]:off[p]].tolist() == K.ENTRY_BEFORE and ids[off[p + 1]:off[p + 2]].tolist() == K.ENTRY_AFTER
        assert not set(bases[kind]) & set(K.ENTRY_BEFORE + K.ENTRY_AFTER + [K.ENTRY_FILL, K.ENTRY_MMAP])
    for kind in range(5):                                      # a program starts on every place of a 64-place window
        assert {at % 64 for k, _, at in c["marks"] if k == kind} == set(range(64)), kind
    assert c["straddle"] // part + 1 == (c["straddle"] + 63) // part and (c["ends_on"] + 64) % part == 0
    ent, _ = model_entries(c)
    at = c["marks"][0][2]
    assert (ent_id(ent[at + 63]), ent_n(ent[at + 63]), ent_pos(ent[at + 63]), ent_len(ent[at + 63])) == (11, 1, 63, 64)
    assert ent_n(ent[at]) == 63 and ent[at] == pack(10, 63, 0, 64)
    # (the 64-distinct program, placed 65 + 2 times, adds 1 to every pair of 0 .. 63; 64 copies of 30 add nothing)
    assert cnt[20, 21] == 65 * 1024 + 67 and cnt[10, 11] == 2 * 65 * 63 + 67 and cnt[30].max() == 67
    assert cnt[10, 66] == 0 and cnt[10, 65] == 0               # nothing shared with a neighbour


def test_many_long_programs_conditions():
    c, (cnt, dyn, pr, run) = get(("many_long_programs",))
    progs = [p.tolist() for p in OR.programs(c["ids"], c["off"])]
    longs = [p for p in progs if len(p) > K.SHORT_LEN]
    assert len(longs) == 603 > 2 * K.LONG_BLOCKS and c["ids"].size // 65 + 1 >= len(longs)
    assert {len(p) for p in longs[:600]} == set(range(65, 81))
    sets = [set(p) for p in longs[:600]]
    assert all(2 <= len(s) <= 4 for s in sets)
    assert all(not sets[k] & sets[k + 1] for k in range(599))
    assert all(not sets[k] & sets[k + K.LONG_BLOCKS] for k in range(600 - K.LONG_BLOCKS))
    assert [33] * 65 in progs and [K.LONG_MMAP] * 70 in progs and list(range(300)) in progs
    assert any(len(p) <= K.SHORT_LEN and cnt[p[0], p[1]] > 1 for p in progs)   # a short program in a long one's cell
    b = K.many_long_programs(bad=True)
    assert int((b["ids"] >= 300).sum()) == 3 and b["ids"].size == b["want_ids"].size + 3 == c["ids"].size
    assert all(len(p) > K.SHORT_LEN for p in OR.programs(b["ids"], b["off"]) if (p >= 300).any())
    print("many_long_programs: long programs", len(longs), "largest cell", int(cnt.max()))


def test_saturation_edges_conditions():
    c, (cnt, dyn, pr, run) = get(("saturation_edges",))
    for (i, j), v in K.SAT_VALUES.items():
        assert cnt[i, j] == cnt[j, i] == v, (i, j)
    assert 4095 * 4097 == SAT - 1 and 4096 * 4096 == SAT and 65536 * 65537 == (1 << 32) + 65536
    cl = OR.cells(cnt)
    assert cl[0, 1] != cl[2, 3] and cl[2, 3] == cl[4, 5] == cl[6, 7] == F32(SAT) and cl[0, 1] == F32(SAT - 1)
    assert sorted(cnt[6].tolist()) == [0, 0, 0, 0, 0, 1, 2, (1 << 32) + 65536] and c["enabled"][6]
    assert all(len(p) > K.SHORT_LEN for p in OR.programs(c["ids"], c["off"]) if len(p) > 3)
    # a truncated cell changes the row's maximum, and with it every nonzero cell of the row
    t = cnt.copy()
    t[6, 7] &= U64(0xFFFFFFFF)
    assert (CK.bits(OR.normalize(OR.cells(t))[6]) != CK.bits(dyn[6]))[[0, 2]].all()


@pytest.mark.parametrize("ncalls", K.FINISH_SIZES)
def test_finish_rows_conditions(ncalls):
    c, (cnt, dyn, pr, run) = get(("finish_rows", ncalls, False))
    last = ncalls - 1
    c0, c1, c2, c3 = K.finish_cols(ncalls)
    assert (c0 % 256 // 64, c1 % 256 // 64, c2 % 256 // 64, c3 % 256 // 64) == (0, 1, 2, 3) and c3 < ncalls
    assert np.flatnonzero(cnt[K.R_LAST]).tolist() == [last] and np.flatnonzero(cnt[K.R_ONE]).tolist() == [100]
    for r, wmax, wmin in ((K.R_W3, 3, 2), (K.R_W2, 2, 3)):
        row = cnt[r].astype(I64)
        assert {int(j) % 256 // 64 for j in np.flatnonzero(row == row.max())} == {wmax}
        assert {int(j) % 256 // 64 for j in np.flatnonzero(row == row[row > 0].min())} == {wmin}
        assert {int(j) % 256 // 64 for j in np.flatnonzero(row)} == {0, 1, 2, 3}
    assert not cnt[K.R_ZERO].any() and c["enabled"][K.R_ZERO] and (dyn[K.R_ZERO] == 1).all()
    want = (c["static"][K.R_ZERO] * F32(1000)).astype(F32).astype(I64)
    want[c["enabled"] == 0] = 0
    assert run[K.R_ZERO].tolist() == np.cumsum(want).tolist()          # run = 1000 * static, truncated
    assert np.flatnonzero(c["enabled"] == 0).tolist() == [j for j in (255, 256) if j < ncalls]
    d, (dcnt, ddyn, dpr, drun) = get(("finish_rows", ncalls, True))
    assert int((dcnt[K.R_FULL] == 0).sum()) == 1 and d["enabled"][K.R_FULL]   # nzero == 1
    off = np.flatnonzero(d["enabled"] == 0).tolist()
    assert off == (list(range(256, 512)) if ncalls >= 512 else [])
    if ncalls > 256:
        # the last column's sum is above what any one step holds, so a dropped carry shows: in both matrices,
        # but for the one whose last step is disabled as a whole (column 256 of 257, columns 256 .. 511 of 512)
        for dense, r, rr in ((False, K.R_ZERO, run), (True, K.R_FULL, drun)):
            row = rr[r].astype(I64)
            step = [int(row[min(j + 256, ncalls) - 1] - (row[j - 1] if j else 0)) for j in range(0, ncalls, 256)]
            assert min(step) >= 0 and (row[-1] > max(step) > 0) == ((ncalls, dense) not in ((257, False), (512, True))), (r, step)
            assert not (dense and ncalls >= 513) or (step[1] == 0 and step[2] > 0)   # the carry crosses an all-zero step


# ---- CPU: the model against the oracle, and the named mistakes --------------------------------------
@pytest.mark.parametrize("key", FAMILIES, ids=_id)
def test_model_equals_oracle(key):
    c, (cnt, dyn, pr, run) = get(key)
    mc, info = model_counts(c)
    assert np.array_equal(mc, cnt)
    assert info["reach"] == c["ncalls"] ** 2 and info["lds"] <= K.BAND_CELLS
    md, mp, mr = model_finish(cnt, c["static"], c["enabled"])
    assert np.array_equal(CK.bits(md), CK.bits(dyn)) and np.array_equal(CK.bits(mp), CK.bits(pr))
    assert np.array_equal(mr, run)
    print(_id(key), info, "ids", c["ids"].size, "largest cell", int(cnt.max()))


def test_model_with_each_named_mistake_is_caught():
    """Each mistake put into the model changes the result of a family made for it.  One of them changes no value:
    a last band not clamped to ncalls owns no further id, and its further cells stay zero, which the flush skips;
    what changes is how far the flush walks, past the end of the counts (info["reach"])."""
    caught = {b: [] for b in ADD_BUGS + FINISH_BUGS}
    for key in SMALL:
        c, (cnt, dyn, pr, run) = get(key)
        for bug in ADD_BUGS:
            if key[0] == "finish_rows" and key[1:] != (513, False):
                continue                                       # (one of them is enough for the add's mistakes)
            mc, info = model_counts(c, bug)
            if not np.array_equal(mc, cnt) or info["reach"] != c["ncalls"] ** 2:
                caught[bug].append(_id(key))
        for bug in FINISH_BUGS:
            md, mp, mr = model_finish(cnt, c["static"], c["enabled"], bug)
            if not (np.array_equal(CK.bits(md), CK.bits(dyn)) and np.array_equal(mr, run)):
                caught[bug].append(_id(key))
    for bug, by in caught.items():
        print(bug, "->", ", ".join(by))
        assert any(k.startswith(CAUGHT_BY[bug]) for k in by), (bug, by)
    # and where each shows
    sat = {k: v for k, v in caught.items() if "saturation_edges" in v}
    assert set(sat) >= {"long_product_32", "cast_before_min"}
    assert all("band_sizes-202" not in caught[b] for b in ("band_edge_plus_1", "last_band_unclamped"))   # one band
    assert {"band_sizes-320", "band_sizes-512", "band_sizes-513"} <= set(caught["last_band_unclamped"])
    assert all("finish_rows-256-False" not in caught[b] for b in ("carry_dropped", "carry_three_waves"))
    assert all(_id(("finish_rows", n, d)) in caught["carry_dropped"] for n in K.FINISH_SIZES[1:] for d in (False, True))


# ---- GPU ------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("key", FAMILIES, ids=_id)
def test_edges_bit_exact(ctx, key):
    from syzkaller_amd.prio import PrioTable

    c, exp = get(key)
    t0 = time.perf_counter()
    t = PrioTable(c["static"], c["mmap"], c["enabled"], ctx=ctx)
    before = ctx.counter("prio_bad_ids")
    t.add(csr=(c["ids"], c["off"]))
    assert np.array_equal(t.counts(), exp[0]), key
    CK.same(t.prios(), exp, key)
    CK.same(t.from_progs(csr=(c["ids"], c["off"])), exp, key)      # clear + add + finish: nothing doubles
    assert np.array_equal(t.counts(), exp[0]) and ctx.counter("prio_bad_ids") == before
    t.close()
    print(_id(key), "on the GPU and compared: %.2f s" % (time.perf_counter() - t0))


@pytest.mark.gpu
def test_device_form_bad_ids_inside_long_programs(ctx):
    import torch

    from syzkaller_amd._lib import call
    from syzkaller_amd.prio import PrioTable

    c, _ = get(("many_long_programs",))
    b = K.many_long_programs(bad=True)
    exp = OR.everything(b["want_ids"], b["want_off"], b["ncalls"], b["mmap"], c["static"], c["enabled"])
    t = PrioTable(c["static"], c["mmap"], c["enabled"], ctx=ctx)
    d_ids, d_off = CK.to_dev(b["ids"]), CK.to_dev(b["off"])
    n = b["ncalls"] ** 2
    d_dyn = torch.empty(n, dtype=torch.float32, device="cuda")
    d_pr = torch.empty(n, dtype=torch.float32, device="cuda")
    d_run = torch.empty(n, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    before = ctx.counter("prio_bad_ids")
    call("sg_prio_table_add_dev", t.h, d_ids.data_ptr(), d_off.data_ptr(), b["off"].size - 1, b["ids"].size)
    call("sg_call_prios_dev", t.h, d_dyn.data_ptr(), d_pr.data_ptr(), d_run.data_ptr())
    ctx.sync()
    assert ctx.counter("prio_bad_ids") == before + 3
    assert np.array_equal(t.counts(), exp[0])
    shape = (b["ncalls"], b["ncalls"])
    CK.same(tuple(x.cpu().numpy().reshape(shape) for x in (d_dyn, d_pr, d_run)), exp, "device form")
    t.close()
