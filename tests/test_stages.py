"""The stages every feature shares, each run alone through the test-only harness library
(tests/hip/stages_harness.hip, built as syzkaller_amd/libsgstages_test.so and linked against libsyzsig.so) and
compared, exactly, with numpy: scan_counts, radix_sort_u64, radix_pass_runs, the distinct-and-rank stages of
sg_rank.hip, the device helpers of sg_internal.h and the line walk of sg_linewalk.h (against a plain Python
restatement of "split at '\\n'").  Every buffer a stage is given, and its share of the
workspace (its *_ws bound, at an offset of the test's choosing), lies between two guards, and every test asserts
that the guards are intact.  The CPU tests show that the library is there and that each case of
tests/stages_cases.py is where it claims to be."""
import ctypes
import os
import re
import subprocess
from ctypes import POINTER, c_int, c_int32, c_uint8, c_uint32, c_uint64, c_void_p

import numpy as np
import pytest

from tests import stages_cases as K
from tests.conftest import ROOT

HARNESS = os.path.join(ROOT, "syzkaller_amd", "libsgstages_test.so")
P8, P32, P64, PI32 = POINTER(c_uint8), POINTER(c_uint32), POINTER(c_uint64), POINTER(c_int32)

# name -> (restype, argtypes): every entry point the tests use
SGT = {
    "sgt_scan_ws_bytes": (c_uint64, [c_uint64]),
    "sgt_radix_sort_ws": (c_uint64, [c_uint64]),
    "sgt_radix_pass_runs_ws": (c_uint64, [c_uint64, c_uint64]),
    "sgt_rank_ws_bytes": (c_uint64, [c_uint64]),
    "sgt_bits_below": (c_uint64, [c_uint64]),
    "sgt_scan_counts": (c_int, [c_void_p, P32, c_uint64, c_uint64, P64, P32]),
    "sgt_radix_sort": (c_int, [c_void_p, P64, c_uint64, c_uint64, c_uint64, P64, POINTER(c_int), P64, P32]),
    "sgt_radix_pass_runs": (c_int, [c_void_p, P64, c_uint64, P64, P64, c_uint64, c_uint32, c_uint64, P64, P32]),
    "sgt_rank_runs": (c_int, [c_void_p, P64, c_uint64, c_int, c_uint64, P32, P64, P64, P32]),
    "sgt_rank_pack": (c_int, [c_void_p, P32, P32, c_uint64, c_uint64, P64, P64, P32]),
    "sgt_rank_values": (c_int, [c_void_p, P64, c_uint64, c_uint64, c_uint64, P64, P64, P32, P32]),
    "sgt_rank_flag_all": (c_int, [c_void_p, P64, c_uint64, c_uint64, P8, P8, P64, P64, P32]),
    "sgt_rank_fill": (c_int, [c_void_p, P64, c_uint64, c_uint64, P8, P64, c_uint64, P32, P32, P32]),
    "sgt_rank_group_first": (c_int, [c_void_p, P32, P32, c_uint64, c_uint64, c_uint64, P64, P64, P32, P64, P32]),
    "sgt_bounds": (c_int, [c_void_p, P64, c_uint64, P64, c_uint64, P64, P64, P32]),
    "sgt_seg_search": (c_int, [c_void_p, P64, c_uint32, P64, c_uint64, P64, P64, P32]),
    "sgt_wave_add": (c_int, [c_void_p, P32, c_uint64, P32, P32]),
    "sgt_wave_max": (c_int, [c_void_p, PI32, c_uint64, PI32, P32]),
    "sgt_walk_lines": (c_int, [c_void_p, P8, c_uint64, P64, c_uint64, c_uint32, c_uint64, c_uint32, c_uint32, c_uint32,
                               c_uint32, c_uint64, c_uint32, P32, P64, P32]),
}
_PTR = {np.dtype(np.uint8): P8, np.dtype(np.uint32): P32, np.dtype(np.uint64): P64, np.dtype(np.int32): PI32}
_harness = None


def harness():
    global _harness
    if _harness is None:
        from syzkaller_amd import _lib  # noqa: F401  (the product library, loaded first from its own path)

        h = ctypes.CDLL(HARNESS)
        for name, (res, args) in SGT.items():
            f = getattr(h, name)
            f.restype, f.argtypes = res, args
        _harness = h
    return _harness


def ptr(a):
    """A contiguous array as the pointer its dtype asks for (null for None)."""
    if a is None:
        return None
    assert a.flags["C_CONTIGUOUS"]
    return a.ctypes.data_as(_PTR[a.dtype])


def run(name, ctx, *args):
    """One harness call; the guards' mask is its last argument.  Fails on an error code or a damaged guard."""
    from syzkaller_amd._lib import lib

    broken = c_uint32(0xFFFFFFFF)
    rc = getattr(harness(), name)(ctx.h, *args, ctypes.byref(broken))
    assert rc == 0, (name, rc, lib.sg_last_error())
    assert broken.value == 0, "%s: guards damaged, mask 0x%x" % (name, broken.value)


# ---- CPU: the library, and the cases' own conditions ------------------------------
def test_harness_library_exports():
    """The harness exists (a missing library is a failure), loads, and exports every sgt_* name used here and no
    sg_* name; the product library gains nothing from it."""
    from syzkaller_amd import _lib

    assert os.path.exists(HARNESS), "syzkaller_amd/libsgstages_test.so is not built (make -C syzkaller_amd)"
    h = harness()
    for name in SGT:
        getattr(h, name)
    out = subprocess.run(["nm", "-D", "--defined-only", HARNESS], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r" T ([a-z0-9_]+)$", out, flags=re.M))
    assert exported >= set(SGT)
    assert not [n for n in exported if n.startswith("sg_")]
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert not re.findall(r" T (sgt_[a-z0-9_]+)$", out, flags=re.M)


def test_ws_bounds_cover_the_stages_layout():
    """The bounds against the layouts restated from the stages: the scan holds its tile sums twice at the first
    level (sums and bases) and once at every further one, every region rounded up to 256 bytes."""
    h = harness()

    def r256(b):
        return (b + 255) & ~255

    def scan_used(n):
        if n == 0:
            return 0
        t = (n + K.SCAN_TILE - 1) // K.SCAN_TILE
        used = 2 * r256(8 * t)
        while True:
            t2 = (t + K.SCAN_TILE - 1) // K.SCAN_TILE
            used += r256(8 * t2)
            if t2 <= 1:
                return used
            t = t2

    for n in K.SCAN_SIZES + (K.SCAN_THIRD_LEVEL, 2, 4096 ** 3 + 1):
        assert h.sgt_scan_ws_bytes(n) >= scan_used(n), n
    assert scan_used(K.SCAN_SINGLE_COUNT) == 768   # (sums, bases and the sum of the bases' one tile)
    def sort_used(t, tables=0):
        """Counts [256][t] and their offsets (one more), then the pass over runs' tile tables or the sort's 256
        bytes for its AND / OR words, then the scan of the counts."""
        return r256(1024 * t) + r256(8 * (256 * t + 1)) + (tables or 256) + scan_used(256 * t)

    for n in K.SORT_SIZES:
        assert h.sgt_radix_sort_ws(n) >= sort_used((n + K.SORT_TILE - 1) // K.SORT_TILE), n
    for counts in (K.RUN_COUNTS, (1,), (), (0, 0), (K.SORT_TILE,) * 5, (1,) * 100):
        t = sum((c + K.SORT_TILE - 1) // K.SORT_TILE for c in counts)
        bound = h.sgt_radix_pass_runs_ws(sum(counts), len(counts))
        assert bound >= (sort_used(t, r256(8 * t) + r256(4 * t)) if t else 0), counts
    for ng in K.RANK_RUN_SIZES + (1000, 9000):   # v, ka, kb, pos, flags, then the sort and the scan from one tail
        regions = 3 * r256(8 * ng) + r256(8 * (ng + 1)) + r256(4 * ng)
        tail = max(sort_used((ng + K.SORT_TILE - 1) // K.SORT_TILE), scan_used(ng))
        assert h.sgt_rank_ws_bytes(ng) >= regions + tail, ng


def test_scan_cases_are_where_they_claim():
    assert [K.scan_levels(n) for n in (1, 4096, 4097, 4096 * 4096, K.SCAN_THIRD_LEVEL)] == [1, 1, 2, 2, 3]
    assert K.SCAN_THIRD_LEVEL == 4096 * 4096 + 1 and (K.SCAN_THIRD_LEVEL + 4095) // 4096 > 4096
    assert max(K.scan_levels(n) for n in K.SCAN_SIZES) == 2
    for n in (0, 1, 15, 16, 17, 255, 256, 257, 4095, 4096, 4097, 2 * 4096, 4096 * 4096 - 1, 4096 * 4096):
        assert n in K.SCAN_SIZES
    # all 0xFFFFFFFF at 4097: the sum passes 2^32 inside one thread's 16 items, inside a tile and across tiles
    ref = K.scan_reference(K.scan_input(4097, "max"))
    assert ref[2] >= 1 << 32 and ref[16] < ref[4096] < ref[4097] and int(ref[4097]) == 4097 * 0xFFFFFFFF
    rnd = K.scan_input(K.SCAN_THIRD_LEVEL, "random")
    assert rnd.size == K.SCAN_THIRD_LEVEL and rnd.min() == 0 and rnd.max() == 3
    assert {0, 4095, 4096, 3 * 4096} <= set(K.SCAN_EDGE_POSITIONS) and max(K.SCAN_EDGE_POSITIONS) == 3 * 4096


def test_sort_window_rule():
    """The restated rule: windows of 8 bits from the lowest varying bit, a window without a varying bit skipped;
    for a mask that is its own windows' bits, or keys constant in the rest of them, the windows' order is the
    order by key & mask."""
    assert K.sort_windows(K.M64) == list(range(0, 64, 8))
    assert K.sort_windows(0x7FF << 32) == [32, 40]
    assert K.sort_windows(K.M64 ^ 0xF) == [4, 12, 20, 28, 36, 44, 52, 60]      # the last one reaches past bit 63
    assert K.sort_windows(((1 << 24) - 1) << 13) == [13, 21, 29]
    assert K.sort_windows(0xFF | (0xFF << 24)) == [0, 24]                       # the middle digits are skipped
    assert K.sort_windows(1 << 63) == [63] and K.sort_windows(0xF << 60) == [60] and K.sort_windows(1 << 5) == [5]
    assert K.window_bits(1 << 5) == 0xFF << 5 and K.window_bits(0xF << 60) == 0xF << 60
    for mask, (vary, _, mask_order) in K.SORT_MASKS.items():
        for n in (65, 1025):
            vary, keys = K.sort_keys(mask, n)
            eff = K.effective_vary(keys, vary)
            if not vary:
                assert eff == int(np.bitwise_or.reduce(keys ^ keys[0])), mask
            if not eff:
                continue
            outside = K.window_bits(eff) & ~eff & K.M64
            if mask_order:
                assert not int(np.bitwise_or.reduce((keys ^ keys[0]) & np.uint64(outside))), mask
                by_mask = np.argsort(keys & np.uint64(eff), kind="stable")
                assert np.array_equal(np.argsort(K.window_key(keys, eff), kind="stable"), by_mask), mask
                assert np.array_equal(K.sort_reference(keys, vary)[0], keys[by_mask]), mask


def test_sort_cases_are_where_they_claim():
    sizes = set(K.SORT_SIZES)
    assert {0, 1, 2, 63, 64, 65, 1023, 1024, 1025, 8191, 8192, 8193, 2 * 8192 + 1, 17 * 8192 + 5} == sizes
    tiles = (K.SORT_TWO_SCAN_LEVELS + K.SORT_TILE - 1) // K.SORT_TILE
    assert 256 * tiles > K.SCAN_TILE and K.scan_levels(256 * tiles) == 2
    n = 1025
    passes = {m: K.sort_reference(K.sort_keys(m, n)[1], K.SORT_MASKS[m][0])[1] for m in K.SORT_MASKS}
    assert passes["full"] == 8 and passes["deflate_class"] == 2 and passes["low_bit_13"] == 3
    assert passes["low_bit_4"] == 8 and passes["empty_middle"] == 2 and passes["superset"] == 3
    assert passes["single_bit"] == passes["bit_63"] == passes["bits_60_63"] == passes["auto_one_bit"] == 1
    assert passes["auto_equal"] == 0 and passes["auto"] == 5
    assert {p % 2 for p in passes.values()} == {0, 1}                      # results left in a and in b
    # deflate's use: the low 32 bits are the key's index and differ in every key, outside the windows
    vary, keys = K.sort_keys("deflate_class", n)
    assert np.array_equal(keys & np.uint64(0xFFFFFFFF), np.arange(n, dtype=np.uint64))
    assert not K.window_bits(vary) & 0xFFFFFFFF
    want = K.sort_reference(keys, vary)[0]
    assert np.array_equal(want, keys[np.argsort(keys >> np.uint64(32), kind="stable")])
    # the empty middle digit sits on constant key bits; the superset is strict; one bit differs
    vary, keys = K.sort_keys("empty_middle", n)
    assert set(((keys >> np.uint64(8)) & np.uint64(0xFFFF)).tolist()) == {0xABCD}
    vary, keys = K.sort_keys("superset", n)
    diff = int(np.bitwise_or.reduce(keys ^ keys[0]))
    assert diff and diff & ~vary == 0 and diff != vary and diff & ~(0xFFF << 8) == 0
    assert K.sort_windows(vary)[-1] == 20 and not ((keys >> np.uint64(20)) & np.uint64(255)).any()
    vary, keys = K.sort_keys("auto_one_bit", n)
    assert int(np.bitwise_or.reduce(keys ^ keys[0])) == 1 << 37
    assert len(set(K.sort_keys("auto_equal", n)[1].tolist())) == 1
    # partial last waves hold live keys of digit 0 next to dead lanes (key 0, digit 0) in the one-window cases
    for m in ("bit_63", "bits_60_63"):
        for n in (63, 1023, 8191):
            vary, keys = K.sort_keys(m, n)
            last = keys[(n - 1) // 64 * 64:]
            assert last.size == 63 and K.window_key(last, vary)[-1] == 0, (m, n)
            assert (K.window_key(keys, vary) != 0).any()
    for n in K.SORT_DIST_SIZES:
        vary, keys = K.sort_dist("sorted", n)
        assert np.array_equal(K.sort_reference(keys, vary)[0], keys)
        vary, keys = K.sort_dist("reversed", n)
        assert not np.array_equal(K.sort_reference(keys, vary)[0], keys)
        vary, keys = K.sort_dist("equal_windows", n)
        assert len(set(K.window_key(keys, vary).tolist())) == 1 and len(set(keys.tolist())) > 1
        vary, keys = K.sort_dist("one_digit", n)
        assert (K.window_key(keys[:8193], vary) == 7).all() and K.sort_windows(vary) == [8]
    assert 8192 in K.SORT_DIST_SIZES and 8193 in K.SORT_DIST_SIZES


def test_runs_cases_are_where_they_claim():
    src, start, cnt = K.runs_case(K.RUN_COUNTS)
    assert cnt.tolist() == [0, 1, 8191, 8192, 8193, 2 * 8192 + 1] and K.RUN_SHIFTS == (0, 4, 56)
    covered = np.zeros(src.size, bool)
    for s, c in zip(start.tolist(), cnt.tolist()):
        assert not covered[s:s + c].any()
        covered[s:s + c] = True
    assert (src[~covered] == np.uint64(K.POISON)).all() and (~covered).sum() > 100
    assert not (src[covered] == np.uint64(K.POISON)).any()
    assert start[1] > 0 and covered.sum() == cnt.sum()
    ref = K.runs_reference(src, start, cnt, 4)
    assert ref.size == cnt.sum() and np.array_equal(np.sort(ref), np.sort(src[covered]))


def test_rank_cases_are_where_they_claim():
    runs = K.rank_runs_cases()
    for n in (1, 255, 256, 257, 4096, 4097):
        assert runs["equal_%d" % n].size == runs["distinct_%d" % n].size == n
        assert np.unique(runs["equal_%d" % n]).size == 1 and np.unique(runs["distinct_%d" % n]).size == n
    for name, keys in runs.items():
        assert (keys[1:] >= keys[:-1]).all(), name
    assert np.flatnonzero(K.rank_runs_reference(runs["run_ends_256"])[0]).tolist() == [0, 256, 512]
    assert np.flatnonzero(K.rank_runs_reference(runs["run_ends_4096"])[0]).tolist() == [0, 4096, 8192]
    vals = K.rank_values_cases()
    assert np.unique(vals["repeats_exact_vary"][0]).size <= 37 < vals["repeats_exact_vary"][0].size // 100
    assert vals["all_equal_vary_0"][1] == 0 and np.unique(vals["all_equal_vary_0"][0]).size == 1
    assert {0, K.M64} <= set(vals["zero_and_max"][0].tolist())
    for name, (v, vary) in vals.items():
        assert int(np.bitwise_or.reduce(v ^ v[0])) & ~vary == 0, name     # vary covers the bits that differ
    csr = K.csr_cases()
    off, total, sel, _ = csr["selected"]
    lens = np.diff(off.astype(np.int64))
    assert (lens == 0).sum() > 20 and lens.max() > 256 and 0 < sel.sum() < sel.size
    assert ((lens == 0) & (sel != 0)).any()                               # selected and empty: not flagged
    assert (np.diff(csr["decreasing"][0].astype(np.int64)) < 0).any()
    assert (csr["past_total"][0] > np.uint64(total)).any()
    for name, (off, total, sel, garbage) in csr.items():
        assert garbage == (not (off[0] == 0 and (off[1:] >= off[:-1]).all() and int(off[-1]) == total)), name
    gf = K.group_first_cases()
    assert [gf["groups_%d" % g][2] for g in (1, 2, 255, 256, 257)] == [1, 2, 255, 256, 257]
    h = harness()
    assert [h.sgt_bits_below(g) for g in (1, 2, 255, 256, 257)] == [0, 1, 255, 255, 511]
    for name, (g, r, ngroups) in gf.items():
        assert g.max() < ngroups and r.max() < g.size, name
    assert not (gf["groups_257"][0] == 1).any() and (gf["groups_257"][0] == 256).any()
    assert set(gf["one_group_holds_all"][0].tolist()) == {5}


def test_helper_cases_are_where_they_claim():
    b = K.bounds_cases()
    assert sorted(a.size for a, _ in b.values()) == [0, 1, 2, 2, 6, 7, 7, 8, 8]
    for name, (a, probes) in b.items():
        assert (a[1:] >= a[:-1]).all()
        for x in a.tolist():
            assert x in probes and (x == 0 or x - 1 in probes) and (x == K.M64 or x + 1 in probes), name
    off, q = K.seg_cases()
    assert (off[1:] >= off[:-1]).all() and (np.diff(off.astype(np.int64)) == 0).sum() >= 4
    assert (q[:, 0] == q[:, 1]).any() and (q[:, 2] < off[q[:, 0].astype(np.int64)]).any()
    assert K.seg_reference(off, 0, 9, 3) == 3 and K.seg_reference(off, 0, 9, 10) == 5   # the last of equal offsets
    assert K.seg_reference(off, 4, 9, 2) == 4                                        # i below off[lo]: lo
    add = K.wave_add_rows()
    assert np.array_equal(add[:64], np.eye(64, dtype=np.uint32))
    assert (add.astype(np.uint64).sum(axis=1) >= 1 << 32).any()
    mx = K.wave_max_rows()
    assert mx.min() == -1 and (mx[:64].max(axis=1) == 7).all() and ((mx[:64] == 7).sum(axis=1) == 1).all()
    assert (mx[-1] == -1).all()


def _walk_lines(segs, tile_log):
    """[(segment, a0, tile in the segment, record)] of every line of the case over segs, no limit."""
    text, off = K.walk_case(segs, tile_log)[:2]
    tile_off = K.walk_tile_off(off, len(text), tile_log)
    out = []
    for g, lines in enumerate(K.walk_reference(text, off, tile_log, K.WALK_CLS)):
        p = max(i for i in range(len(segs)) if tile_off[i] <= g and off[i] < off[i + 1])
        out += [(p, off[p], g - tile_off[p], r) for r in lines]
    return text, out


def test_walk_cases_are_where_they_claim():
    hdr = open(os.path.join(ROOT, "syzkaller_amd", "csrc", "sg_linewalk.h")).read()
    assert "kWalkStep = %d;" % K.WALK_STEP in hdr and "kWalkLoad = %d;" % (K.WALK_LOAD // K.WALK_STEP) in hdr
    assert "kLineGroup = %d;" % K.WALK_GROUP in hdr and "cb += kWalkLoad * kWalkStep;" in hdr
    # the restatement, by hand: two segments, the second from an odd place; a line is its first byte's tile's
    text = b"ab(\n\n=" + b"x" * 70 + b"\nq"
    ref = K.walk_reference(text, [0, 5, len(text)], 6, K.WALK_CLS)
    assert ref == [[(0, 3, 1, 2, 0), (4, 4, 0, 0, 0)], [(5, 76, 2, 0, 5)], [(77, 78, 0, 0, 0)]]
    assert K.walk_tile_off([0, 5, len(text)], len(text), 6) == [0, 1, 3]
    assert K.walk_origin(5, 5, 6) == 5 and K.walk_origin(5, 68, 6) == 5 and K.walk_origin(5, 69, 6) == 68
    for tile_log in K.WALK_TILE_LOGS:
        tile = 1 << tile_log
        # ownership: the line behind a '\n' at te + d starts at te + d + 1 and is the tile's that holds that byte
        segs = K.walk_ownership_segs(tile_log)
        _, lines = _walk_lines(segs, tile_log)
        k = 0
        for edge in (1, 2):
            owners = []
            for d in K.WALK_OWNER_SHIFTS:
                mine = [(t, r) for p, a0, t, r in lines if p == k]
                assert len(mine) == 2 and mine[1][1][0] - off_of(segs, k) == edge * tile + d + 1
                owners.append(mine[1][0])
                k += 1
            assert owners == [edge - 1, edge - 1, edge, edge, edge]
        tail = [[(t, r[1] - r[0]) for p, a0, t, r in lines if p == k + i] for i in range(4)]
        assert tail == [[(0, tile - 1)], [(0, tile - 2), (0, 1)], [(0, tile - 1), (1, 1)], [(0, tile)]]
        # segments: the lengths, odd starts, empty lines
        segs = K.walk_segment_segs(tile_log)
        assert {0, 1, tile - 1, tile, tile + 1} <= {len(g) for g in segs} and b"\n" in segs and b"\n\n\n" in segs
        text, lines = _walk_lines(segs, tile_log)
        assert sum(a0 % 2 for p, a0, t, r in lines) > len(lines) // 3
        assert sum(r[0] == r[1] for p, a0, t, r in lines) >= 5
        at = segs.index(b"xxxx")
        assert segs[at - 1][-1:] == b"\n" and segs[at - 1][-2:-1] == b"=" and segs[at + 1][:2] == b"\n("
        assert [r[1:] for p, a0, t, r in lines if p == at] == [(off_of(segs, at) + 4, 0, 0, 0)]
    # spans, a tile a step: three tiles and more, and SPAN lines that leave the owner's first load
    text, lines = _walk_lines(K.walk_span_segs(), 6)
    long = [(p, a0, t, r) for p, a0, t, r in lines if r[1] - r[0] >= 150]
    assert len(long) == 16 and all((r[1] - 1 - a0) // 64 - t >= 2 for p, a0, t, r in long)
    past = [r for p, a0, t, r in long if r[1] - K.walk_origin(a0, r[0], 6) > K.WALK_LOAD]
    assert len(past) >= 8 and {t > 0 for p, a0, t, r in long} == {False, True}
    assert sum(text[r[1]:r[1] + 1] == b"\n" for p, a0, t, r in long) == 8     # the others end with their segment
    assert all(r[2] == 3 for p, a0, t, r in long)
    assert {r[1] - r[0] for p, a0, t, r in long} == {150, K.WALK_MAX_LINE - 1, 300, 600}
    # classes: each one on both sides of a step's and of a load's edge, counted from where its owner reads
    for tile_log in K.WALK_TILE_LOGS:
        text, lines = _walk_lines(K.walk_class_segs(), tile_log)
        assert all(r[1] - r[0] < K.WALK_MAX_LINE for p, a0, t, r in lines)
        for k in (0, 1):
            rel = {r[3 + k] - K.walk_origin(a0, r[0], tile_log) for p, a0, t, r in lines if r[2] >> k & 1}
            assert {K.WALK_STEP - 1, 0} <= {x % K.WALK_STEP for x in rel}
            if tile_log == 8:     # (at 6 a line below the limit ends inside its owner's first load)
                assert {K.WALK_LOAD - 1, K.WALK_LOAD} <= rel
            first = {r[3 + k] - r[0] for p, a0, t, r in lines if r[2] >> k & 1}
            last = {r[1] - 1 - r[3 + k] for p, a0, t, r in lines if r[2] >> k & 1}
            assert 0 in first and 0 in last
        assert {r[2] for p, a0, t, r in lines} == {0, 1, 2, 3}
        assert any(r[2] == 3 and r[3] < r[4] for p, a0, t, r in lines) and any(r[2] == 3 and r[3] > r[4] for p, a0, t, r in lines)
    # the limit: every place of a step, on both sides
    for tile_log in K.WALK_TILE_LOGS:
        text, lines = _walk_lines(K.walk_limit_segs(), tile_log)
        for n in (K.WALK_MAX_LINE - 1, K.WALK_MAX_LINE, K.WALK_MAX_LINE + 1):
            places = {(r[0] - K.walk_origin(a0, r[0], tile_log)) % K.WALK_STEP for p, a0, t, r in lines if r[1] - r[0] == n}
            assert places == set(range(K.WALK_STEP)), (tile_log, n)
    # the store group
    text, lines = _walk_lines(K.walk_dense_segs(), 8)
    per = {}
    for p, a0, t, r in lines:
        per[(p, t)] = per.get((p, t), 0) + 1
    assert [per[(2 * i, 0)] for i in range(5)] == [per[(2 * i + 1, 1)] for i in range(5)] == list(K.WALK_DENSE_COUNTS)
    assert K.WALK_GROUP == 64 and all((p, 1 + p % 2) not in per for p in range(10))
    # a wave's share: several tiles each; with and without a shorter last share; with and without idle waves
    shares = []
    for nwaves in K.WALK_FEW_WAVES:
        for case in walk_share_cases(nwaves):
            ntiles = len(K.walk_reference(case[0], case[1], case[2], case[4]))
            per = (ntiles + nwaves - 1) // nwaves
            assert per >= 2 and case[5] == nwaves
            shares.append((ntiles % per != 0, (nwaves - 1) * per >= ntiles))
    assert {a for a, _ in shares} == {b for _, b in shares} == {False, True}


def off_of(segs, k):
    return sum(len(g) for g in segs[:k])


# ---- GPU: scan_counts ---------------------------------------------------------------
def gpu_scan(ctx, counts, ws_used):
    out = np.full(counts.size + 1, 0x1111111111111111, np.uint64)
    run("sgt_scan_counts", ctx, ptr(counts), counts.size, ws_used, ptr(out))
    return out


@pytest.mark.gpu
def test_scan_counts_sizes(ctx):
    k = 0
    for n in K.SCAN_SIZES:
        patterns = ("random",) if n > 1 << 20 else ("random", "ones", "zero")
        for pattern in patterns:
            counts = K.scan_input(n, pattern, seed=n)
            ws_used = K.WS_USED[k % 3]
            k += 1
            assert np.array_equal(gpu_scan(ctx, counts, ws_used), K.scan_reference(counts)), (n, pattern, ws_used)


@pytest.mark.gpu
def test_scan_counts_values(ctx):
    """Sums past 2^32 at every level, and a single count at the first, last and tile-edge places."""
    for ws_used in K.WS_USED:
        counts = K.scan_input(4097, "max")
        assert np.array_equal(gpu_scan(ctx, counts, ws_used), K.scan_reference(counts)), ws_used
    n = 3 * 4096 + 1
    for k, at in enumerate(K.SCAN_EDGE_POSITIONS):
        counts = K.scan_one_hot(n, at)
        assert np.array_equal(gpu_scan(ctx, counts, K.WS_USED[k % 3]), K.scan_reference(counts)), at


@pytest.mark.gpu
def test_scan_counts_single_count_stays_in_its_bound(ctx):
    """One count, at every workspace offset: the guard behind scan_ws_bytes(1) is what this is about."""
    assert K.SCAN_SINGLE_COUNT == 1
    for ws_used in K.WS_USED:
        for value in (0, 7, 0xFFFFFFFF):
            out = gpu_scan(ctx, np.array([value], np.uint32), ws_used)
            assert out.tolist() == [0, value], (ws_used, value)


@pytest.mark.gpu
@pytest.mark.parametrize("pattern", ["random", "ones"])
def test_scan_counts_third_level(ctx, pattern):
    """4096 * 4096 + 1 counts: the first size at which the tile sums' own tile sums are scanned in turn."""
    counts = K.scan_input(K.SCAN_THIRD_LEVEL, pattern)
    out = gpu_scan(ctx, counts, 256)
    ref = K.scan_reference(counts)
    assert int(out[-1]) == int(ref[-1])
    assert np.array_equal(out, ref)


# ---- GPU: radix_sort_u64 ------------------------------------------------------------
def gpu_sort(ctx, keys, vary, ws_used):
    """(result, which): which buffer *sorted named, a (0) or b (1)."""
    n = keys.size
    out = np.full(n, 0x2222222222222222, np.uint64)
    a_after = np.full(n, 0x3333333333333333, np.uint64)
    which = c_int(-2)
    run("sgt_radix_sort", ctx, ptr(keys), n, vary, ws_used, ptr(out), ctypes.byref(which), ptr(a_after))
    return out, which.value, a_after


def check_sort(ctx, keys, vary, ws_used, what):
    got, which, a_after = gpu_sort(ctx, keys, vary, ws_used)
    want, passes = K.sort_reference(keys, vary)
    assert which == passes % 2, (what, which, passes)       # an even pass count leaves the result in a
    assert np.array_equal(got, want), what
    if passes == 0:
        assert np.array_equal(a_after, keys), what          # nothing to sort: a untouched


@pytest.mark.gpu
@pytest.mark.parametrize("mask", list(K.SORT_MASKS))
def test_radix_sort_masks(ctx, mask):
    for k, n in enumerate(K.SORT_SIZES):
        vary, keys = K.sort_keys(mask, n)
        check_sort(ctx, keys, vary, K.WS_USED[k % 3], (mask, n))


@pytest.mark.gpu
@pytest.mark.parametrize("dist", K.SORT_DISTS)
def test_radix_sort_distributions(ctx, dist):
    for k, n in enumerate(K.SORT_DIST_SIZES):
        vary, keys = K.sort_dist(dist, n)
        check_sort(ctx, keys, vary, K.WS_USED[k % 3], (dist, n))


# ---- GPU: radix_pass_runs -------------------------------------------------------------
def check_runs(ctx, counts, shift, ws_used):
    src, start, cnt = K.runs_case(counts, seed=shift)
    n = int(cnt.sum())
    dst = np.full(n, 0x4444444444444444, np.uint64)
    run("sgt_radix_pass_runs", ctx, ptr(src), src.size, ptr(start), ptr(cnt), len(counts), shift, ws_used, ptr(dst))
    assert not (dst == np.uint64(K.POISON)).any(), (counts, shift)
    assert np.array_equal(dst, K.runs_reference(src, start, cnt, shift)), (counts, shift)


@pytest.mark.gpu
@pytest.mark.parametrize("shift", K.RUN_SHIFTS)
def test_radix_pass_runs(ctx, shift):
    check_runs(ctx, K.RUN_COUNTS, shift, 0)
    check_runs(ctx, K.RUN_COUNTS[::-1], shift, 256)
    check_runs(ctx, (1,), shift, 1 << 20)
    check_runs(ctx, (), shift, 0)
    check_runs(ctx, (0, 0), shift, 256)


# ---- GPU: the rank stages -----------------------------------------------------------------
@pytest.mark.gpu
def test_rank_runs(ctx):
    for k, (name, keys) in enumerate(K.rank_runs_cases().items()):
        n = keys.size
        flags, pos, u = K.rank_runs_reference(keys)
        for want_u in (1, 0):
            gf = np.zeros(n, np.uint32)
            gp = np.zeros(n + 1, np.uint64)
            gu = np.zeros(n, np.uint64)
            run("sgt_rank_runs", ctx, ptr(keys), n, want_u, K.WS_USED[k % 3], ptr(gf), ptr(gp), ptr(gu))
            assert np.array_equal(gf, flags) and np.array_equal(gp, pos), name
            assert int(gp[n]) == u.size, name
            if want_u:
                assert np.array_equal(gu[:u.size], u), name
                assert (gu[u.size:] == np.uint64(0xEEEEEEEEEEEEEEEE)).all(), name      # nothing past the distinct keys
            else:
                assert (gu == np.uint64(0xEEEEEEEEEEEEEEEE)).all(), name               # u null: nothing written


@pytest.mark.gpu
def test_rank_values_and_pack(ctx):
    for k, (name, (v, vary)) in enumerate(K.rank_values_cases().items()):
        ng = v.size
        u = np.zeros(ng, np.uint64)
        nu = c_uint64(0)
        rank = np.zeros(ng, np.uint32)
        run("sgt_rank_values", ctx, ptr(v), ng, vary, K.WS_USED[k % 3], ptr(u), ctypes.byref(nu), ptr(rank))
        want = np.unique(v)
        assert nu.value == want.size, name
        assert np.array_equal(u[:want.size], want), name
        assert np.array_equal(rank, np.searchsorted(want, v).astype(np.uint32)), name
    rng = np.random.default_rng(12)
    for k, ng in enumerate((1, 255, 256, 257, 1000)):
        hi = rng.integers(0, 1 << 32, size=ng, dtype=np.uint32)
        lo = rng.integers(0, 1 << 32, size=ng, dtype=np.uint32)
        hi[0], lo[0] = 0xFFFFFFFF, 0xFFFFFFFF
        gv, gka = np.zeros(ng, np.uint64), np.zeros(ng, np.uint64)
        run("sgt_rank_pack", ctx, ptr(hi), ptr(lo), ng, K.WS_USED[k % 3], ptr(gv), ptr(gka))
        want = (hi.astype(np.uint64) << np.uint64(32)) | lo.astype(np.uint64)
        assert np.array_equal(gv, want) and np.array_equal(gka, want), ng


@pytest.mark.gpu
def test_rank_flag_all_and_fill(ctx):
    for name, (off, total, sel, garbage) in K.csr_cases().items():
        ngroups = off.size - 1
        flag = np.full(ngroups, 9, np.uint8)
        gbase = np.zeros(ngroups, np.uint64)
        scal = np.full(2, 9, np.uint64)
        run("sgt_rank_flag_all", ctx, ptr(off), ngroups, total, ptr(sel), ptr(flag), ptr(gbase), ptr(scal))
        ranges = [K.csr_range(off, c, total) for c in range(ngroups)]
        lens = np.array([r1 - r0 for r0, r1 in ranges], np.int64)
        if sel is None:
            assert (flag == 1).all() and scal.tolist() == [0, 0], name
            assert gbase.tolist() == [r0 for r0, _ in ranges], name
            ng = total
        else:
            want_flag = (sel != 0) & (lens > 0)
            assert np.array_equal(flag, want_flag.astype(np.uint8)), name
            assert scal.tolist() == [int(want_flag.sum()), int(lens[want_flag].sum())], name
            # the places come from an atomic counter: any order, but a disjoint exact cover of [0, scal[1])
            cover = np.zeros(int(scal[1]), np.int64)
            for c in np.flatnonzero(want_flag):
                assert int(gbase[c]) + lens[c] <= scal[1], (name, c)
                cover[int(gbase[c]):int(gbase[c]) + lens[c]] += 1
            assert (cover == 1).all(), name
            assert (gbase[~want_flag] == 0).all(), name
            ng = int(scal[1])
        if ng == 0:
            continue
        gidx = np.zeros(ng, np.uint32)
        ggroup = np.zeros(ng, np.uint32)
        run("sgt_rank_fill", ctx, ptr(off), ngroups, total, ptr(flag), ptr(gbase), ng, ptr(gidx), ptr(ggroup))
        assert (gidx < max(total, 1)).all() and (ggroup < ngroups).all(), name   # csr_range's promise
        if garbage and sel is None:
            # lists may overlap or leave places out: a place holds its own member (the place of member m is m) or,
            # never assigned, member 0 of group 0
            at = np.arange(ng)
            assert ((gidx == at) | ((gidx == 0) & (ggroup == 0))).all(), name
            continue
        want_idx = np.zeros(ng, np.uint32)
        want_grp = np.zeros(ng, np.uint32)
        for c in np.flatnonzero(flag):
            r0, r1 = ranges[c]
            g0 = int(gbase[c])
            want_idx[g0:g0 + r1 - r0] = np.arange(r0, r1)
            want_grp[g0:g0 + r1 - r0] = c
        assert np.array_equal(gidx, want_idx) and np.array_equal(ggroup, want_grp), name


@pytest.mark.gpu
def test_rank_group_first(ctx):
    for k, (name, (g, r, ngroups)) in enumerate(K.group_first_cases().items()):
        ng = g.size
        first = np.full(ngroups, 9, np.uint64)
        keys = np.zeros(ng, np.uint64)
        flags = np.zeros(ng, np.uint32)
        pos = np.zeros(ng + 1, np.uint64)
        run("sgt_rank_group_first", ctx, ptr(g), ptr(r), ng, ngroups, K.WS_USED[k % 3], ptr(first), ptr(keys),
            ptr(flags), ptr(pos))
        wkeys, wflags, wpos, wfirst = K.group_first_reference(g, r, ngroups)
        assert np.array_equal(keys, wkeys) and np.array_equal(flags, wflags) and np.array_equal(pos, wpos), name
        assert np.array_equal(first, wfirst), name
        absent = np.setdiff1d(np.arange(ngroups), g)
        assert (first[absent] == 0).all(), name                              # groups without members keep 0


# ---- GPU: the line walk ----------------------------------------------------------------------
FILL64 = np.uint64(0xEEEEEEEEEEEEEEEE)


def check_walk(ctx, case, nclasses=2):
    """One harness call against the restatement: every tile's count and records, exactly; of a line of max_line
    bytes or more one record with the true start and max_line <= e - s <= the true length, its classes those of
    [s, e), and none for its remainder; nothing written behind a tile's records.  With nclasses below 2 the walk is
    the one of fewer classes, and the classes left out are never met."""
    text, off, tile_log, max_line, cls, nwaves, per_tile = case
    cls2, cls = cls, cls[:nclasses]
    want = K.walk_reference(text, off, tile_log, cls)
    ntiles = len(want)
    assert ntiles and max(len(w) for w in want) <= per_tile
    cnt = np.full(ntiles, 0xFFFFFFFF, np.uint32)
    rec = np.zeros((ntiles, per_tile, 5), np.uint64)
    t8 = np.frombuffer(text, np.uint8).copy()
    o64 = np.array(off, np.uint64)
    run("sgt_walk_lines", ctx, ptr(t8) if t8.size else None, t8.size, ptr(o64), len(off) - 1, tile_log, max_line, nclasses,
        cls2[0], cls2[1], nwaves, ntiles, per_tile, ptr(cnt), ptr(rec))
    assert cnt.tolist() == [len(w) for w in want]
    for g, lines in enumerate(want):
        got = [tuple(r) for r in rec[g, :len(lines)].tolist()]
        for k, (s, e, _, _, _) in enumerate(lines):
            if e - s >= max_line:
                assert got[k][0] == s and max_line <= got[k][1] - s <= e - s, (g, k, got[k], s, e)
                e = got[k][1]
            assert got[k] == K.walk_record(text, s, e, cls), (g, k)
        assert (rec[g, len(lines):] == FILL64).all(), g


@pytest.mark.gpu
@pytest.mark.parametrize("tile_log", K.WALK_TILE_LOGS)
def test_walk_lines_ownership_and_segments(ctx, tile_log):
    check_walk(ctx, K.walk_case(K.walk_ownership_segs(tile_log), tile_log))
    check_walk(ctx, K.walk_case(K.walk_segment_segs(tile_log), tile_log))
    check_walk(ctx, K.walk_case([b""] * 3 + [b"r"], tile_log))


@pytest.mark.gpu
@pytest.mark.parametrize("tile_log", K.WALK_TILE_LOGS)
def test_walk_lines_classes(ctx, tile_log):
    segs = K.walk_class_segs()
    check_walk(ctx, K.walk_case(segs, tile_log))
    check_walk(ctx, K.walk_case(segs, tile_log, cls=K.WALK_CLS[::-1]))
    check_walk(ctx, K.walk_case(segs, tile_log), nclasses=1)
    check_walk(ctx, K.walk_case(segs, tile_log), nclasses=0)
    # a class byte of 0: what is read behind a segment's end, or behind the text's, is no byte of any class
    zero = [g.replace(b"(", b"\0") for g in segs] + [b"nothing", b"\0"]
    check_walk(ctx, K.walk_case(zero, tile_log, cls=(0, K.WALK_CLS[1])))


@pytest.mark.gpu
def test_walk_lines_spans(ctx):
    segs = K.walk_span_segs()
    check_walk(ctx, K.walk_case(segs, 6))
    check_walk(ctx, K.walk_case(segs, 6, max_line=K.WALK_NO_LIMIT))
    check_walk(ctx, K.walk_case(segs, 8, max_line=K.WALK_NO_LIMIT))


@pytest.mark.gpu
@pytest.mark.parametrize("tile_log", K.WALK_TILE_LOGS)
def test_walk_lines_limit_at_step_positions(ctx, tile_log):
    check_walk(ctx, K.walk_case(K.walk_limit_segs(), tile_log))
    check_walk(ctx, K.walk_case(K.walk_limit_segs(), tile_log), nclasses=0)


@pytest.mark.gpu
def test_walk_lines_store_group(ctx):
    check_walk(ctx, K.walk_case(K.walk_dense_segs(), 8, per_tile=130))
    check_walk(ctx, K.walk_case(K.walk_dense_segs(), 6))
    check_walk(ctx, K.walk_case(K.walk_dense_segs(), 8, per_tile=130), nclasses=0)


def walk_share_cases(nwaves):
    return [K.walk_case(K.walk_class_segs() + K.walk_dense_segs(), tile_log, nwaves=nwaves, per_tile=130)
            for tile_log in K.WALK_TILE_LOGS]


@pytest.mark.gpu
@pytest.mark.parametrize("nwaves", K.WALK_FEW_WAVES)
def test_walk_lines_more_tiles_than_waves(ctx, nwaves):
    """A wave's share of several consecutive tiles (test_walk_cases_are_where_they_claim: whole shares, a shorter
    last one, and waves without a share)."""
    for case in walk_share_cases(nwaves):
        check_walk(ctx, case)


# ---- GPU: the device helpers -----------------------------------------------------------------
@pytest.mark.gpu
def test_lb64_ub64(ctx):
    for name, (a, probes) in K.bounds_cases().items():
        lb = np.zeros(probes.size, np.uint64)
        ub = np.zeros(probes.size, np.uint64)
        run("sgt_bounds", ctx, ptr(a), a.size, ptr(probes), probes.size, ptr(lb), ptr(ub))
        assert np.array_equal(lb, np.searchsorted(a, probes, side="left").astype(np.uint64)), name
        assert np.array_equal(ub, np.searchsorted(a, probes, side="right").astype(np.uint64)), name


@pytest.mark.gpu
def test_seg_search(ctx):
    off, q = K.seg_cases()
    og = np.zeros(q.shape[0], np.uint64)
    ol = np.zeros(q.shape[0], np.uint64)
    run("sgt_seg_search", ctx, ptr(off), off.size, ptr(q), q.shape[0], ptr(og), ptr(ol))
    want = np.array([K.seg_reference(off, *map(int, row)) for row in q], np.uint64)
    assert np.array_equal(og, want), "global pointer"
    assert np.array_equal(ol, want), "LDS pointer"
    below = q[:, 2] < off[q[:, 0].astype(np.int64)]
    assert np.array_equal(og[below], q[below, 0])                               # i below off[lo]: lo


@pytest.mark.gpu
def test_wave_scans(ctx):
    add = K.wave_add_rows()
    out = np.zeros_like(add)
    run("sgt_wave_add", ctx, ptr(add), add.shape[0], ptr(out))
    assert np.array_equal(out, np.cumsum(add.astype(np.uint64), axis=1).astype(np.uint32))   # (wraps at 2^32)
    mx = K.wave_max_rows()
    outm = np.zeros_like(mx)
    run("sgt_wave_max", ctx, ptr(mx), mx.shape[0], ptr(outm))
    assert np.array_equal(outm, np.maximum.accumulate(mx, axis=1))
