"""Cases of tests/test_stages.py: inputs for the stages every feature shares (scan_counts, radix_sort_u64,
radix_pass_runs, the distinct-and-rank stages, the device helpers of sg_internal.h, the line walk of
sg_linewalk.h), each at the edge it is named for, with the numpy references they are compared to.

What is restated here from the stages, and nothing else of them:
  the scan works in tiles of SCAN_TILE counts, and a level of tile sums is scanned in turn while it has more than
      one tile (scan_levels);
  the sort works in tiles of SORT_TILE keys, a wave's step is 64 of them, and it scans 256 counts per tile;
  the sort's windows: 8-bit digits from ctz(vary) upwards in steps of 8, a window kept when vary has a bit in it
      (sort_windows); the result is the stable order by the kept windows, most significant last-sorted, and every
      other bit of a key travels with it as payload (window_key, sort_reference);
  csr_range's clamp (csr_range);
  the line walk reads WALK_STEP bytes a step and WALK_LOAD bytes a load, from its segment's start in the head tile
      and from one byte before its tile in every other (walk_origin), and stores WALK_GROUP lines at a time.
The CPU tests of test_stages.py show that each case is where it claims to be; the expected values are numpy's."""
import numpy as np

M64 = (1 << 64) - 1
SCAN_TILE = 4096
SORT_TILE = 8192
WS_USED = (0, 256, 1 << 20)


def u64(x):
    return np.asarray(x, dtype=np.uint64)


# ---- scan_counts ----------------------------------------------------------------
def scan_levels(n):
    """Levels of tile sums a scan of n counts goes through: 1 up to one tile, 2 up to SCAN_TILE tiles, then 3."""
    levels = 0
    while True:
        n = (n + SCAN_TILE - 1) // SCAN_TILE
        levels += 1
        if n <= 1:
            return levels


SCAN_SIZES = (0, 1, 15, 16, 17, 255, 256, 257, 4095, 4096, 4097, 2 * 4096, 4096 * 4096 - 1, 4096 * 4096)
# a single count: sums, bases and the sum that the scan of the bases' one tile writes behind them, 768 bytes, where
# scan_ws_bytes(1) once promised 512 (the write landed in whatever region the caller's plan had placed next)
SCAN_SINGLE_COUNT = 1
SCAN_THIRD_LEVEL = 4096 * 4096 + 1   # the first size whose tile sums fill more than one tile of tile sums
SCAN_EDGE_POSITIONS = (0, 15, 16, 4095, 4096, 4097, 2 * 4096 - 1, 2 * 4096, 3 * 4096)  # in a vector of 3 * 4096 + 1


def scan_input(n, pattern, seed=0):
    if pattern == "random":
        return np.random.default_rng(1000 + seed).integers(0, 4, size=n, dtype=np.uint32)
    if pattern == "ones":
        return np.ones(n, np.uint32)
    if pattern == "zero":
        return np.zeros(n, np.uint32)
    if pattern == "max":
        return np.full(n, 0xFFFFFFFF, np.uint32)
    raise ValueError(pattern)


def scan_one_hot(n, at, value=0xFFFFFFFF):
    v = np.zeros(n, np.uint32)
    v[at] = value
    return v


def scan_reference(counts):
    """[n + 1]: the exclusive prefix, then the total."""
    out = np.zeros(counts.size + 1, np.uint64)
    np.cumsum(counts.astype(np.uint64), out=out[1:])
    return out


# ---- radix_sort_u64 ---------------------------------------------------------------
def sort_windows(vary):
    """The shifts of the 8-bit digits the sort runs for this (non-zero) vary, least significant first."""
    lo = (vary & -vary).bit_length() - 1
    return [s for s in range(lo, vary.bit_length(), 8) if (vary >> s) & 255]


def window_bits(vary):
    m = 0
    for s in sort_windows(vary):
        m |= (255 << s) & M64
    return m


def window_key(keys, vary):
    """The kept windows of each key, concatenated (at most 8 of 8 bits: a uint64)."""
    wk = np.zeros(keys.size, np.uint64)
    for i, s in enumerate(sort_windows(vary)):
        wk |= ((keys >> np.uint64(s)) & np.uint64(255)) << np.uint64(8 * i)
    return wk


def effective_vary(keys, vary):
    """vary as given, or what the auto-detect finds: the bits in which the keys differ."""
    if vary or keys.size == 0:
        return vary
    return int(np.bitwise_and.reduce(keys)) ^ int(np.bitwise_or.reduce(keys))


def sort_reference(keys, vary):
    """(expected keys, passes): the stable order by the windows; fewer than two keys or no varying bit: as they are."""
    vary = effective_vary(keys, vary)
    if keys.size < 2 or not vary:
        return keys.copy(), 0
    return keys[np.argsort(window_key(keys, vary), kind="stable")], len(sort_windows(vary))


SORT_SIZES = (0, 1, 2, 63, 64, 65, 1023, 1024, 1025, 8191, 8192, 8193, 2 * 8192 + 1, 17 * 8192 + 5)
SORT_TWO_SCAN_LEVELS = 17 * 8192 + 5   # 256 counts a tile over 18 tiles: more than one tile of counts


def _rand(rng, n):
    return rng.integers(0, 1 << 64, size=n, dtype=np.uint64)


def _mask_full(rng, n):
    return _rand(rng, n)


def _mask_top(rng, n):
    k = _rand(rng, n)
    if n:
        k[-1] &= np.uint64((1 << 60) - 1)   # the last key's top digit is 0, as a dead lane's is
    return k


def _mask_class(rng, n):
    return (rng.integers(0, 0x800, size=n, dtype=np.uint64) << np.uint64(32)) | np.arange(n, dtype=np.uint64)


def _mask_empty_middle(rng, n):
    return (_rand(rng, n) & u64(M64 ^ (0xFFFF << 8))) | u64(0xABCD << 8)


def _mask_superset(rng, n):   # (the top window, bits 20..27, holds digit 0 in every key, as a dead lane's key does)
    return (_rand(rng, n) & u64(0xFFF << 8)) | u64(0x5A5A00003000000F)


def _mask_auto(rng, n):
    return (_rand(rng, n) & u64(((1 << 40) - 1) << 3)) | u64(0xC000000000000005)


def _mask_auto_equal(rng, n):
    return np.full(n, 0x0123456789ABCDEF, np.uint64)


def _mask_auto_one_bit(rng, n):
    return u64(0x00FF00000000FF00) | (rng.integers(0, 2, size=n, dtype=np.uint64) << np.uint64(37))


# name -> (vary, keys(rng, n), mask_order): mask_order says the windows' order is the order by key & vary, which
# holds when the keys are constant in the window bits outside vary
SORT_MASKS = {
    "full": (M64, _mask_full, True),
    "deflate_class": (0x7FF << 32, _mask_class, True),             # sg_deflate.hip's and sg_inflate.hip's use
    "low_bit_4": (M64 ^ 0xF, _mask_full, True),                   # windows at 4, 12, .. 60: the top one passes bit 63
    "low_bit_13": (((1 << 24) - 1) << 13, _mask_full, True),      # three windows at odd shifts, an odd pass count
    "empty_middle": (0xFF | (0xFF << 24), _mask_empty_middle, True),
    "single_bit": (1 << 5, _mask_full, False),                    # the window is bits 5..12 all the same
    "bit_63": (1 << 63, _mask_top, True),
    "bits_60_63": (0xF << 60, _mask_top, True),
    "superset": (((1 << 24) - 1) << 4, _mask_superset, True),     # the keys differ in bits 8..19 only
    "auto": (0, _mask_auto, False),
    "auto_equal": (0, _mask_auto_equal, False),
    "auto_one_bit": (0, _mask_auto_one_bit, False),
}


def sort_keys(mask, n, seed=0):
    vary, gen, _ = SORT_MASKS[mask]
    return vary, gen(np.random.default_rng([list(SORT_MASKS).index(mask), n, seed]), n)


SORT_DISTS = ("sorted", "reversed", "equal_windows", "one_digit")
SORT_DIST_SIZES = (65, 8192, 8193, 2 * 8192 + 1)


def sort_dist(dist, n):
    """(vary, keys): key distributions over vary = bits 13..36 (three windows) and, for one_digit, one window."""
    rng = np.random.default_rng(77 + n)
    vary = ((1 << 24) - 1) << 13
    if dist in ("sorted", "reversed"):
        keys = _rand(rng, n)
        keys = keys[np.argsort(keys & u64(vary), kind="stable")]
        return vary, keys[::-1].copy() if dist == "reversed" else keys
    if dist == "equal_windows":   # only payload differs: the order must stay
        return vary, (_rand(rng, n) & u64(M64 ^ vary)) | u64(0x123456 << 13)
    if dist == "one_digit":       # the first min(n, 8193) keys hold digit 7: a whole tile of one digit, and one more
        d = rng.integers(0, 256, size=n, dtype=np.uint64)
        d[:8193] = 7
        return 0xFF << 8, (d << np.uint64(8)) | (np.arange(n, dtype=np.uint64) << np.uint64(20)) | u64(0xC3)
    raise ValueError(dist)


# ---- radix_pass_runs ----------------------------------------------------------------
POISON = 0xDEADBEEFDEADBEEF
RUN_COUNTS = (0, 1, 8191, 8192, 8193, 2 * 8192 + 1)
RUN_SHIFTS = (0, 4, 56)
RUN_GAPS = (5, 0, 3, 100, 1, 64, 7)   # keys of poison before each run and after the last one


def runs_case(counts, seed=0):
    """(src, run_start, run_cnt): the runs in a buffer whose gaps hold POISON; no key of a run equals it."""
    rng = np.random.default_rng(500 + seed)
    parts, start = [], []
    at = 0
    for i, c in enumerate(counts):
        gap = RUN_GAPS[i % len(RUN_GAPS)]
        parts.append(np.full(gap, POISON, np.uint64))
        at += gap
        start.append(at)
        k = _rand(rng, c)
        k[k == np.uint64(POISON)] = 1
        parts.append(k)
        at += c
    parts.append(np.full(RUN_GAPS[len(counts) % len(RUN_GAPS)], POISON, np.uint64))
    return np.concatenate(parts), u64(start), u64(list(counts))


def runs_reference(src, run_start, run_cnt, shift):
    cat = np.concatenate([src[int(s):int(s) + int(c)] for s, c in zip(run_start, run_cnt)] + [np.zeros(0, np.uint64)])
    digit = (cat >> np.uint64(shift)) & np.uint64(255)
    return cat[np.argsort(digit, kind="stable")]


# ---- the rank stages -------------------------------------------------------------------
RANK_RUN_SIZES = (1, 255, 256, 257, 4096, 4097)


def rank_runs_cases():
    """name -> sorted keys."""
    out = {}
    for n in RANK_RUN_SIZES:
        out["equal_%d" % n] = np.full(n, 0x7777777777777777, np.uint64)
        out["distinct_%d" % n] = np.arange(n, dtype=np.uint64) * np.uint64(3) + np.uint64(1 << 40)
        out["repeats_%d" % n] = np.sort(np.random.default_rng(n).integers(0, max(n // 3, 1), size=n, dtype=np.uint64))
    # runs that end exactly on 256 and on 4096: a new run starts at the first place of a block and of a scan tile
    out["run_ends_256"] = np.repeat(u64([5, 9, 11]), [256, 256, 100])
    out["run_ends_4096"] = np.repeat(u64([0, 1, M64]), [4096, 4096, 5])
    return out


def rank_runs_reference(sorted_keys):
    n = sorted_keys.size
    flags = np.ones(n, np.uint32)
    flags[1:] = sorted_keys[1:] != sorted_keys[:-1]
    return flags, scan_reference(flags), np.unique(sorted_keys)


def rank_values_cases():
    """name -> (values, vary)."""
    rng = np.random.default_rng(31)
    pool = _rand(rng, 37)
    rep = pool[rng.integers(0, pool.size, size=5000)]
    ends = np.concatenate([rep[:1000], u64([0, M64, 0, M64, 1, M64 - 1])])
    rng.shuffle(ends)
    same = np.full(300, 0xFEDCBA9876543210, np.uint64)
    diff = int(np.bitwise_and.reduce(rep)) ^ int(np.bitwise_or.reduce(rep))
    return {
        "repeats_exact_vary": (rep, diff),
        "repeats_all_bits": (rep, M64),
        "all_equal_vary_0": (same, 0),
        "all_equal_all_bits": (same, M64),
        "one_value": (same[:1], 0),
        "zero_and_max": (ends, M64),
    }


def csr_range(off, i, total):
    """sgd::csr_range: list i of a CSR over `total` members, clamped to them."""
    r0 = min(int(off[i]), total)
    r1 = min(max(int(off[i + 1]), r0), total)
    return r0, r1


def csr_cases():
    """name -> (off, total, sel or None, garbage): garbage offsets promise nothing but bounds."""
    rng = np.random.default_rng(41)
    lens = rng.integers(0, 9, size=300)
    lens[rng.integers(0, 300, size=60)] = 0      # empty groups
    lens[17] = 1000                              # more than 256 members: the fill's stride loop
    lens[299] = 257
    off = u64(np.concatenate([[0], np.cumsum(lens)]))
    total = int(off[-1])
    sel = (rng.integers(0, 3, size=300) > 0).astype(np.uint8)
    sel[17] = 1
    decreasing = off.copy()
    decreasing[100:200] = decreasing[100:200][::-1]
    past = off.copy()
    past[250:] += np.uint64(total)
    past[7] = np.uint64(M64)
    return {
        "plain": (off, total, None, False),
        "selected": (off, total, sel, False),
        "none_selected": (off, total, np.zeros(300, np.uint8), False),
        "one_group": (u64([0, 700]), 700, None, False),
        "decreasing": (decreasing, total, None, True),
        "past_total": (past, total, None, True),
        "past_total_selected": (past, total, sel, True),
    }


GROUP_FIRST_GROUPS = (1, 2, 255, 256, 257)


def group_first_cases():
    """name -> (ggroup, rank, ngroups): places in no order, ranks below the number of places."""
    out = {}
    for ngroups in GROUP_FIRST_GROUPS:
        rng = np.random.default_rng(ngroups)
        ng = 3 * ngroups + 50
        g = rng.integers(0, ngroups, size=ng).astype(np.uint32)
        if ngroups > 2:
            g[g == 1] = 0                        # a group without members
            g[g == ngroups - 2] = ngroups - 1
        out["groups_%d" % ngroups] = (g, rng.integers(0, ng // 4 + 1, size=ng).astype(np.uint32), ngroups)
    rng = np.random.default_rng(9)
    out["one_group_holds_all"] = (np.full(9000, 5, np.uint32), rng.integers(0, 500, size=9000).astype(np.uint32), 9)
    return out


def group_first_reference(ggroup, rank, ngroups):
    """(sorted keys, flags, pos, first)."""
    keys = np.sort((ggroup.astype(np.uint64) << np.uint64(32)) | rank.astype(np.uint64))
    flags, pos, _ = rank_runs_reference(keys)
    first = np.zeros(ngroups, np.uint64)
    for i in range(keys.size - 1, -1, -1):       # the lowest place of each group wins
        first[int(keys[i]) >> 32] = pos[i]
    return keys, flags, pos, first


# ---- the device helpers ------------------------------------------------------------------
def bounds_cases():
    """name -> (ascending array, probes): every value below, between, equal to and above the elements."""
    arrays = {
        "n0": [], "n1": [10], "n2": [10, 20], "n7": [2, 4, 6, 8, 10, 12, 14], "n8": [2, 4, 6, 8, 10, 12, 14, 16],
        "ties2": [5, 5], "ties7": [1, 3, 3, 3, 7, 7, 9], "ties8": [4, 4, 4, 4, 4, 4, 4, 4],
        "ends": [0, 0, 1, M64 - 1, M64, M64],
    }
    out = {}
    for name, a in arrays.items():
        probes = {0, 1, M64 - 1, M64}
        for x in a:
            probes |= {max(x - 1, 0), x, min(x + 1, M64)}
        out[name] = (u64(a), u64(sorted(probes)))
    return out


def seg_cases():
    """(off, queries [nq, 3] of {lo, hi, i}): lo == hi, ties, i below off[lo], i past the last offset."""
    off = u64([0, 3, 3, 3, 10, 10, 11, 20, 20, 50])
    q = []
    for lo in range(off.size):
        for hi in range(lo, off.size):
            for i in (0, 2, 3, 4, 9, 10, 11, 19, 20, 21, 49, 50, 51, M64):
                q.append((lo, hi, i))
    return off, u64(q).reshape(-1, 3)


def seg_reference(off, lo, hi, i):
    """The largest r in [lo, hi] with off[r] <= i; lo when there is none (i below off[lo])."""
    r = lo
    for k in range(lo, hi + 1):
        if int(off[k]) <= i:
            r = k
    return r


def wave_add_rows():
    """[rows, 64] uint32: the 64 one-hot rows, random rows whose sums wrap 2^32, small rows, zeroes and ones."""
    rng = np.random.default_rng(64)
    rows = [np.eye(64, dtype=np.uint32)]
    rows.append(rng.integers(0, 1 << 32, size=(16, 64), dtype=np.uint32))
    rows.append(rng.integers(0, 5, size=(8, 64), dtype=np.uint32))
    rows.append(np.zeros((1, 64), np.uint32))
    rows.append(np.ones((1, 64), np.uint32))
    rows.append(np.full((1, 64), 0xFFFFFFFF, np.uint32))
    return np.concatenate(rows)


def wave_max_rows():
    """[rows, 64] int32 over values >= -1: lane j holds 7 and the rest -1, random rows, all -1."""
    rng = np.random.default_rng(65)
    one = np.full((64, 64), -1, np.int32)
    one[np.arange(64), np.arange(64)] = 7
    rows = [one, rng.integers(-1, 1 << 31, size=(16, 64)).astype(np.int32),
            rng.integers(-1, 4, size=(8, 64)).astype(np.int32), np.full((1, 64), -1, np.int32)]
    return np.concatenate(rows)


# ---- the line walk (sg_linewalk.h) ----------------------------------------------------------
WALK_STEP = 64
WALK_LOAD = 256
WALK_GROUP = 64
WALK_MAX_LINE = 192
WALK_NO_LIMIT = 1 << 20
WALK_TILE_LOGS = (6, 8)
WALK_CLS = (ord("("), ord("="))
NL = 10


def walk_tile_off(off, nbytes, tile_log):
    """[nseg + 1]: the first tile of each segment, in segment order."""
    out = [0]
    for p in range(len(off) - 1):
        a0, a1 = csr_range(off, p, nbytes)
        out.append(out[-1] + ((a1 - a0 + (1 << tile_log) - 1) >> tile_log))
    return out


def walk_origin(a0, s, tile_log):
    """Where the wave that owns a line starting at s begins to read: its steps and loads count from there."""
    t = (s - a0) >> tile_log
    return a0 if t == 0 else a0 + (t << tile_log) - 1


def walk_record(text, s, e, cls):
    """(s, e, met, first0, first1) of the line [s, e): the classes met in it and the leftmost place of each."""
    met, first = 0, [0, 0]
    for k, c in enumerate(cls):     # (one or no class: the others are never met)
        at = text.find(bytes([c]), s, e)
        if at >= 0:
            met |= 1 << k
            first[k] = at
    return (s, e, met, first[0], first[1])


def walk_reference(text, off, tile_log, cls):
    """Per tile, the records of the lines that start in it: each segment split at '\n', a trailing fragment without
    '\n' a line, nothing behind a final '\n', a line in the tile that holds its first byte.  No limit here."""
    tile_off = walk_tile_off(off, len(text), tile_log)
    tiles = [[] for _ in range(tile_off[-1])]
    for p in range(len(off) - 1):
        a0, a1 = csr_range(off, p, len(text))
        s = a0
        while s < a1:
            e = text.find(b"\n", s, a1)
            e = a1 if e < 0 else e
            tiles[tile_off[p] + ((s - a0) >> tile_log)].append(walk_record(text, s, e, cls))
            s = e + 1
    return tiles


def walk_case(segs, tile_log, max_line=WALK_MAX_LINE, cls=WALK_CLS, nwaves=0, per_tile=80):
    """(text, off, tile_log, max_line, cls, nwaves, per_tile) over the segments, back to back; nwaves 0: a wave a
    tile."""
    text = b"".join(segs)
    off = [0]
    for g in segs:
        off.append(off[-1] + len(g))
    ntiles = walk_tile_off(off, len(text), tile_log)[-1]
    return text, off, tile_log, max_line, cls, nwaves or (max(ntiles, 1) + 3) // 4 * 4, per_tile


WALK_OWNER_SHIFTS = (-3, -2, -1, 0, 1)   # the '\n' at te + d: the next line starts at te - 2 .. te + 2


def walk_ownership_segs(tile_log):
    """For the tile edge te behind the head tile and the one behind the second tile, a '\n' at te - 3 .. te + 1 in
    a segment of three tiles and a bit; then the segment's own end: a final '\n', and a last line of one byte."""
    tile = 1 << tile_log
    segs = []
    for edge in (1, 2):
        for d in WALK_OWNER_SHIFTS:
            g = bytearray(b"o" * (3 * tile + 5))
            g[edge * tile + d] = NL
            segs.append(bytes(g))
    segs.append(b"p" * (tile - 1) + b"\n")          # nothing follows the final '\n', the tile's last byte
    segs.append(b"p" * (tile - 2) + b"\nq")         # a line that is the tile's and the segment's last byte
    segs.append(b"p" * (tile - 1) + b"\nq")         # the same behind the tile edge: the second tile's
    segs.append(b"p" * tile + b"\n")                # a final '\n' alone in the second tile: it owns nothing
    return segs


def walk_span_segs():
    """Lines over three tiles and more of 64 bytes, from the head tile and from a later one, with and without a
    last '\n'; SPAN_LONG of them also leave the owner's first load."""
    segs = []
    for lead in (b"", b"k" * 70 + b"\n"):
        for n in (150, WALK_MAX_LINE - 1, 300, 600):
            body = b"s" * 20 + b"(" + b"s" * (n - 41) + b"=" + b"s" * 19
            segs.append(lead + body + b"\nt\n")
            segs.append(lead + body)
    return segs


WALK_CLASS_EDGES = (64, 128, 256, 320, 512)


def walk_class_segs():
    """The hand-written rules, then for every edge E and d in -2 .. 1 a line [E + d - 90, E + d + 40) with '(' at
    E + d and '=' one further, between two lines of filler."""
    segs = [
        b"(abc\n=abc\n", b"abc(\nabc=\n", b"(\n=\n", b"abc(", b"abc=",
        b"a(b\nccc\n", b"a=b\nccc\n",                   # the previous line's class is not carried over
        b"aaa\n(b\n", b"aaa\n=b\n", b"\n(=\n",         # a class behind the line's '\n' in the same step is not its
        b"a(b=c\n", b"a=b(c\n", b"a((b(=c==\n", b"==((\n",
    ]
    for edge in WALK_CLASS_EDGES:
        for d in (-2, -1, 0, 1):
            at = edge + d
            s = at - 90
            lead = bytearray(b"f" * s)               # lines of 100 bytes, the last one up to the '\n' at s - 1
            lead[s - 1::-100] = b"\n" * len(lead[s - 1::-100])
            segs.append(bytes(lead) + b"c" * 90 + b"(=" + b"c" * 38 + b"\n" + b"g" * 9)
    return segs


def walk_segment_segs(tile_log):
    """Lengths 0, 1, tile - 1, tile, tile + 1 (the first leaves every later start odd), with and without '\n's; only
    "\n"; "\n\n\n"; and a segment without '\n' or class byte between neighbours that begin and end with them."""
    tile = 1 << tile_log
    segs = [b"u"]
    for n in (0, 1, tile - 1, tile, tile + 1):
        segs.append(b"v" * n)
        segs.append((b"w(\n=" * tile)[:n])
    segs += [b"\n", b"\n\n\n", b"(=\n", b"xxxx", b"\n(=", b"(=\n", b"", b"yy", b"\n"]
    return segs


def walk_limit_segs(max_line=WALK_MAX_LINE):
    """Lines of max_line - 1, max_line and max_line + 1 bytes from each of the 64 places of a step, a '(' early and
    a '=' as the last byte, and a short line behind each."""
    segs = []
    for n in (max_line - 1, max_line, max_line + 1):
        for o in range(WALK_STEP):
            lead = b"z" * (o - 1) + b"\n" if o else b""
            segs.append(lead + b"L" * 5 + b"(" + b"L" * (n - 7) + b"=" + b"\nt(\n")
    return segs


WALK_DENSE_COUNTS = (63, 64, 65, 128, 129)
WALK_FEW_WAVES = (4, 8, 12)   # against 188 tiles of 64 bytes and 75 of 256 (walk_class_segs + walk_dense_segs)


def walk_dense_segs():
    """Tiles of 256 bytes in which n lines start: n - 1 empty ones (129 lines of a byte of content and its '\\n'
    do not start in 256 bytes, so a line here is its '\\n' alone, s == e) and one that runs to the segment's end
    in the next tile; as the head tile, and behind a tile of one line.  The records differ in s only, which is
    what "written once, in order" is read from."""
    segs = []
    for n in WALK_DENSE_COUNTS:
        dense = b"\n" * (n - 1) + b"d" * (256 - (n - 1)) + b"d" * 10
        segs.append(dense)
        segs.append(b"h" * 255 + b"\n" + dense)
    return segs
