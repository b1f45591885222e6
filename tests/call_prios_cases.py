"""Inputs of tests/test_call_prios.py: the worked example with its matrices
written out, the 12-call corpus of the parity test, random corpora per matrix
size, and the saturation program.  And of tests/test_call_prios_edges.py: the
band plan of k_prio_band restated (band_plan) and the deterministic families
that sit on the constants of sg_call_prios.hip."""
import numpy as np

U8, U32, U64, F32 = np.uint8, np.uint32, np.uint64, np.float32
NO_CALL = 0xFFFFFFFF

BAND_CELLS = 40960  # ctx.counter("prio_band_cells")
SHORT_LEN = 64      # ctx.counter("prio_short_len")
# the smallest matrix whose rows no longer fit one band: 203 * 203 = 41209 cells
BAND_EDGE = 203
SIZES = (1, 63, 64, 65, BAND_EDGE, 257)


def csr(progs):
    off = np.zeros(len(progs) + 1, U64)
    if progs:
        off[1:] = np.cumsum([len(p) for p in progs])
    ids = np.concatenate([np.asarray(p, U32) for p in progs]) if progs else np.zeros(0, U32)
    return ids.astype(U32), off


# ---- the worked example ---------------------------------------------------------------
EX_NCALLS, EX_MMAP = 4, 3
EX_PROGS = [[0, 1], [0, 1, 1], [2, 3, 0], [3, 3]]
EX_COUNTS = np.array([[0, 3, 1, 0], [3, 0, 0, 0], [1, 0, 0, 0], [0, 0, 0, 0]], U64)
_ONE, _TENTH = 1065353216, 1036831949  # float32 1.0 and 0.1
EX_DYNAMIC_BITS = np.array([[_TENTH, _ONE, 1051778923, _TENTH],
                            [_ONE, _TENTH, _TENTH, _TENTH],
                            [_ONE, _TENTH, _TENTH, _TENTH],
                            [_ONE, _ONE, _ONE, _ONE]], U32)
EX_STATIC = np.array([[1, .5, .1, 1], [.5, 1, 1, .1], [.1, 1, 1, .25], [1, .1, .25, 1]], F32)
EX_ENABLED = np.array([1, 1, 0, 1], U8)
EX_RUN = np.array([[100, 600, 600, 700], [500, 600, 600, 610], [0, 0, 0, 0], [1000, 1100, 1100, 2100]], np.int32)


# ---- the 12-call corpus ------------------------------------------------------------------
def corpus12():
    """40 programs of 1 to 9 calls over 12 calls, mmap_id 3.  Call 11 is in no program (an all-zero row besides
    mmap's), ids repeat inside programs, and call 5 is disabled (a disabled row and column)."""
    rng = np.random.default_rng(20240611)
    progs = [rng.integers(0, 11, size=int(rng.integers(1, 10))).tolist() for _ in range(40)]
    static = rng.integers(0, 1001, size=(12, 12)).astype(F32) / F32(1000)
    enabled = np.ones(12, U8)
    enabled[5] = 0
    return progs, 12, 3, static.astype(F32), enabled


# ---- random corpora ------------------------------------------------------------------------
def random_case(ncalls, seed, nprogs=60):
    """Programs of 0 to 12 calls with skewed ids, one of SHORT_LEN, one of SHORT_LEN + 1 and one of 300 calls (the
    long path), an mmap-only program; a static matrix with exact 0 and 1 cells; some calls disabled."""
    rng = np.random.default_rng(seed)
    mmap_id = int(rng.integers(0, ncalls)) if ncalls > 1 else 0

    def draw(k):
        return np.minimum(rng.zipf(1.3, size=k) - 1, ncalls - 1).astype(U32) if ncalls > 1 else np.zeros(k, U32)

    progs = [draw(int(rng.integers(0, 13))).tolist() for _ in range(nprogs)]
    for k in (SHORT_LEN, SHORT_LEN + 1, 300):
        progs.insert(int(rng.integers(0, len(progs))), draw(k).tolist())
    progs.insert(3, [mmap_id] * 5)
    progs.insert(7, [])
    progs.append(rng.integers(0, ncalls, size=9).astype(U32).tolist())  # uniform ids: the far bands too
    static = rng.integers(0, 1001, size=(ncalls, ncalls)).astype(F32) / F32(1000)
    static[rng.integers(0, ncalls), rng.integers(0, ncalls)] = 1
    static[rng.integers(0, ncalls), rng.integers(0, ncalls)] = 0
    enabled = (rng.random(ncalls) < 0.85).astype(U8)
    enabled[int(rng.integers(0, ncalls))] = 1
    return progs, ncalls, mmap_id, static.astype(F32), enabled


# ---- saturation ----------------------------------------------------------------------------
SAT_N = 4097                      # 4097 * 4097 = 16,785,409 > 2^24
SAT_PROG = [0] * SAT_N + [1] * SAT_N


# ---- Choose ---------------------------------------------------------------------------------
def draws_from(values):
    """intn of a fixed list: value k of the list modulo n; intn.used counts the draws taken."""
    it = iter(values)

    def intn(n):
        intn.used += 1
        return next(it) % n

    intn.used = 0
    return intn


# ---- the band plan ---------------------------------------------------------------------------
BAND_THREADS = 1024   # kBandT
PART_MAX = 1 << 26    # kPrioPart
MAX_CALLS = 8192      # SG_PRIO_MAX_CALLS
PLAN_NIDS = (1, 4095, 4096, 4097, PART_MAX - 1, PART_MAX, PART_MAX + 1, (1 << 32) - 1)


def band_plan(ncalls, nids):
    """sg_plan.h's band_plan restated: (rows, nbands, nparts, part, gridy).  tests/cpp/plan_test.cc prints a digest
    of the C++ function over every ncalls and PLAN_NIDS and a table of some sizes; the edge file compares both."""
    def up(a, b):
        return (a + b - 1) // b

    rows = max(1, min(BAND_CELLS // ncalls, ncalls))
    nbands = up(ncalls, rows)
    nparts = max(min(up(2048, nbands), up(nids, 4 * BAND_THREADS)), up(nids, PART_MAX))
    part = up(up(nids, nparts), BAND_THREADS) * BAND_THREADS
    return rows, nbands, nparts, part, up(nids, part)


def band_plan_digest():
    h = 14695981039346656037
    for ncalls in range(1, MAX_CALLS + 1):
        for nids in PLAN_NIDS:
            for v in band_plan(ncalls, nids):
                h = ((h ^ v) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    return "%016x" % h


def bands(ncalls):
    """[(r0, r1)] of the row bands"""
    rows, nbands = band_plan(ncalls, 1)[:2]
    return [(b * rows, min(b * rows + rows, ncalls)) for b in range(nbands)]


# ---- the edge families -------------------------------------------------------------------------
def static_enabled(ncalls, rng, on=()):
    """random_case's static matrix (exact 0 and 1 cells) and enabled mask; the calls of `on` enabled"""
    static = rng.integers(0, 1001, size=(ncalls, ncalls)).astype(F32) / F32(1000)
    static[rng.integers(0, ncalls), rng.integers(0, ncalls)] = 1
    static[rng.integers(0, ncalls), rng.integers(0, ncalls)] = 0
    enabled = (rng.random(ncalls) < 0.85).astype(U8)
    enabled[int(rng.integers(0, ncalls))] = 1
    for i in on:
        enabled[i] = 1
    return static.astype(F32), enabled


def case(progs, ncalls, mmap_id, static, enabled, **marks):
    ids, off = progs if isinstance(progs, tuple) else csr(progs)
    return dict(ids=ids, off=off, ncalls=ncalls, mmap=mmap_id, static=static, enabled=enabled, **marks)


BAND_SIZES = (202, 320, 512, 513)
BAND_MMAP = 3


def band_sizes(ncalls):
    """Uniform ids, so every band is populated; at each band edge r the programs [r - 1, r], [r, r - 1, r - 1] and
    one of SHORT_LEN calls holding r - 1, r and the last call."""
    rng = np.random.default_rng(7000 + ncalls)
    last = ncalls - 1
    edges = [r0 for r0, _ in bands(ncalls)[1:]]
    progs = [rng.integers(0, ncalls, size=int(rng.integers(2, 13))).tolist() for _ in range(400)]
    progs.append([0, last])
    for r in edges:
        fill = rng.integers(0, ncalls, size=SHORT_LEN - 3).tolist()
        progs += [[r - 1, r], [r, r - 1, r - 1], fill[:20] + [r - 1] + fill[20:40] + [r] + fill[40:] + [last]]
    static, enabled = static_enabled(ncalls, rng)
    return case(progs, ncalls, BAND_MMAP, static, enabled, edges=edges)


PROD_CALLS = 1541


def production_shape():
    """scripts/exp/call_prios_rate.py's corpus, 3,000 programs of it: 1 to 30 calls, ids Zipf(1.2) through a fixed
    permutation of the calls, mmap the hottest call."""
    rng = np.random.default_rng(1541)
    lens = rng.integers(1, 31, size=3000)
    off = np.zeros(lens.size + 1, U64)
    off[1:] = np.cumsum(lens)
    perm = rng.permutation(PROD_CALLS)
    ids = perm[(rng.zipf(1.2, size=int(off[-1])) - 1) % PROD_CALLS].astype(U32)
    static, enabled = static_enabled(PROD_CALLS, rng)
    return case((ids, off), PROD_CALLS, int(perm[0]), static, enabled)


MAX_IDS = (8191, 8190, 4096, 255, 256, 0)   # the id field's ends, its top bit alone, the u16 list about a byte
MAX_MMAP, MAX_DISABLED, MAX_N63_POS = 5000, 8100, 1


def max_calls():
    """ncalls = MAX_CALLS: MAX_IDS together in short programs and in a long one, a SHORT_LEN-call program whose
    entry for id 8191 has n = 63 (0xFC17FFFF, next to kPrioNone's all ones), a disabled call above 8,000, and 300
    short programs of uniform ids.  The static matrix is a 64 x 64 block tiled."""
    rng = np.random.default_rng(8192)
    s = list(MAX_IDS)
    progs = [s, s[::-1] + [8191], s + list(range(100, 160)) + s, [77] + [8191] * 63, [MAX_DISABLED, 8191, 5],
             [MAX_MMAP, 8191, 0], [8191] * 40 + [8190] * 40]
    progs += [rng.integers(0, MAX_CALLS, size=int(rng.integers(1, 13))).tolist() for _ in range(300)]
    block = rng.integers(0, 1001, size=(64, 64)).astype(F32) / F32(1000)
    block[3, 5], block[7, 2] = 1, 0
    static = np.tile(block.astype(F32), (MAX_CALLS // 64, MAX_CALLS // 64))
    enabled = (rng.random(MAX_CALLS) < 0.85).astype(U8)
    enabled[MAX_DISABLED] = 0
    enabled[[8191, 0]] = 1
    return case(progs, MAX_CALLS, MAX_MMAP, static, enabled)


ENTRY_CALLS, ENTRY_MMAP, ENTRY_FILL = 70, 69, 68
ENTRY_BEFORE, ENTRY_AFTER = [64, 65], [66, 67]
ENTRY_NIDS = 13 * 4096


def entry_bases():
    """The SHORT_LEN-call programs: a first occurrence at place 63 (and n = 63 beside n = 1); the same two ids the
    other way round; 32 and 32 (a pair that adds 1,024); 64 distinct ids; 64 copies of one id (no pair)."""
    a, b, n = 10, 11, SHORT_LEN
    return [[a] * (n - 1) + [b], [b] + [a] * (n - 1), [20] * (n // 2) + [21] * (n // 2), list(range(n)), [30] * n]


def _fill(n):
    return [[ENTRY_FILL] * min(SHORT_LEN, n - k) for k in range(0, n, SHORT_LEN)]


def entry_fields():
    """Every base program directly between two short programs of other ids, behind 0 .. 64 filler places (groups
    padded to a multiple of 64 places, so the program starts at place 2 + shift of a wave's 64-place window);
    then a 64-distinct program across a part edge and one that ends on the next, the stream filled up to
    ENTRY_NIDS places (13 parts of 4,096).  marks: (kind, shift, first place) per base program placed."""
    progs, marks, at = [], [], 0

    def put(ps):
        nonlocal at
        for p in ps:
            progs.append(p)
            at += len(p)

    for kind, base in enumerate(entry_bases()):
        for shift in range(SHORT_LEN + 1):
            put(_fill(shift) + [ENTRY_BEFORE])
            marks.append((kind, shift, at))
            put([base, ENTRY_AFTER])
            put(_fill(-at % SHORT_LEN))
    part = band_plan(ENTRY_CALLS, ENTRY_NIDS)[3]
    distinct = entry_bases()[3]
    edge = (at // part + 1) * part
    put(_fill(edge - 30 - 2 - at) + [ENTRY_BEFORE])
    straddle = at
    put([distinct, ENTRY_AFTER])
    put(_fill(edge + part - SHORT_LEN - 2 - at) + [ENTRY_BEFORE])
    ends_on = at
    put([distinct, ENTRY_AFTER])
    put(_fill(ENTRY_NIDS - at))
    rng = np.random.default_rng(70)
    static, enabled = static_enabled(ENTRY_CALLS, rng)
    return case(progs, ENTRY_CALLS, ENTRY_MMAP, static, enabled, marks=marks, straddle=straddle, ends_on=ends_on, part=part)


LONG_CALLS, LONG_MMAP, LONG_BLOCKS = 300, 7, 256
LONG_BAD = ((5, 10, 300), (300, 0, 0xFFFFFFFF), (599, -1, 8192))  # (program, place, the out-of-range id)


def many_long_programs(bad=False):
    """600 programs of 65 to 80 calls over four ids each, the id sets of programs k and k + 1 and of k and
    k + LONG_BLOCKS disjoint; 65 copies of one id; 70 of mmap; every call once; a few short programs in their cells.
    bad: the device-form twin, LONG_BAD's three ids put in place of ids inside long programs (the expectation is
    the corpus without those three places)."""
    progs = []
    for k in range(600):
        base = 7 * k % 290
        progs.append([base + (t * t + t // 5 + k) % 4 for t in range(65 + k % 16)])
    progs += [[33] * 65, [LONG_MMAP] * 70, list(range(LONG_CALLS)), [33, 34], [0, 1, 2, 3], [299, 0], [7, 8, 9]]
    want = None
    if bad:
        want = [list(p) for p in progs]
        for p, k, x in LONG_BAD:
            progs[p][k] = x
            del want[p][k]
    rng = np.random.default_rng(300)
    static, enabled = static_enabled(LONG_CALLS, rng)
    c = case(progs, LONG_CALLS, LONG_MMAP, static, enabled)
    if bad:
        c["want_ids"], c["want_off"] = csr(want)
    return c


SAT_CALLS = 8
SAT_VALUES = {(0, 1): (1 << 24) - 1, (2, 3): 1 << 24, (4, 5): (1 << 24) + 1, (6, 7): (1 << 32) + 65536}


def saturation_edges():
    """Cells of exactly 2^24 - 1 (4,095 * 4,097), 2^24 (4,096 * 4,096), 2^24 + 1 (the same and one short pair) and
    65,536 * 65,537 = 2^32 + 65,536, the last in row 6 beside cells of 1 and 2: truncated to 32 bits it is 65,536,
    which changes the row's maximum and so every cell of its dynamic row.  No mmap: all eight calls are in use."""
    progs = [[0] * 4095 + [1] * 4097, [2] * 4096 + [3] * 4096, [4] * 4096 + [5] * 4096, [4, 5],
             [6] * 65536 + [7] * 65537, [6, 0], [6, 2, 2]]
    rng = np.random.default_rng(8)
    static, enabled = static_enabled(SAT_CALLS, rng, on=(6,))
    return case(progs, SAT_CALLS, NO_CALL, static, enabled)


FINISH_SIZES = (256, 257, 512, 513, 1025)
R_LAST, R_W3, R_W2, R_ONE, R_ZERO, R_FULL = 10, 20, 30, 40, 50, 60


def finish_cols(ncalls):
    """(c0, c1, c2, c3): columns of waves 0 to 3 of a 256-column step, the last two in the highest step that has both"""
    hi = 256 * ((ncalls - 201) // 256)
    return 5, 70, hi + 130, hi + 200


def finish_rows(ncalls, dense):
    """Rows crafted through short programs; no mmap (its column would be a second zero of the dense row).
    sparse: R_LAST's only nonzero cell is the last column; R_W3 has its maximum (3) in wave 3's columns only and
    its nonzero minimum (1) in wave 2's only, R_W2 the reverse, both with cells of 2 in waves 0 and 1; R_ONE has
    one nonzero cell; R_ZERO is in no program; columns 255 and 256 are disabled and no other.
    dense (the counts are symmetric, so a row without zeros needs a matrix of its own): R_FULL with every other
    call, nzero == 1; from 512 calls on the whole step of columns 256 .. 511 is disabled, below every call is
    enabled."""
    rng = np.random.default_rng(9000 + ncalls)
    last = ncalls - 1
    c0, c1, c2, c3 = finish_cols(ncalls)
    if dense:
        others = [x for x in range(ncalls) if x != R_FULL]
        progs = [[R_FULL] * (1 + k // 62 % 2) + others[k:k + 62] for k in range(0, len(others), 62)]
    else:
        progs = [[R_LAST, last], [R_ONE, 100]]
        for r, mx, mn in ((R_W3, c3, c2), (R_W2, c2, c3)):
            progs += [[r, mx, mx, mx], [r, mn], [r, c0, c0], [r, c1, c1]]
        pool = np.array([x for x in range(ncalls) if x not in (R_LAST, R_W3, R_W2, R_ONE, R_ZERO)])
        progs += [pool[rng.integers(0, pool.size, size=int(rng.integers(2, 9)))].tolist() for _ in range(100)]
    static, _ = static_enabled(ncalls, rng)
    enabled = np.ones(ncalls, U8)
    if not dense:
        enabled[255:257] = 0
    elif ncalls >= 512:
        enabled[256:512] = 0
    return case(progs, ncalls, NO_CALL, static, enabled)
