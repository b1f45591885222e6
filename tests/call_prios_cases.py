"""Inputs of tests/test_call_prios.py: the worked example with its matrices
written out, the 12-call corpus of the parity test, random corpora per matrix
size, and the saturation program."""
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
