"""Inputs of the cover-report line-table tests (tests/test_cover_lines.py): a
"world" is the symbol table, the call sites and the frames of every symbolised
PC with File / Func as strings; intern() turns it into sg_cover_table_create's
arrays.  Hand-written worlds with their expected fileSet results written out,
the unit-edge worlds, and a seeded random world."""
import functools

import numpy as np

U32, U64 = np.uint32, np.uint64
K = 0xffffffff81000000  # kernel text
BASE = 0xffffffff


def cov_of(pcs):
    """The cover words whose RestorePC(., BASE) - 5 gives pcs."""
    return ((np.asarray(pcs, dtype=U64) + U64(5)) & U64(0xffffffff)).astype(U32)


class World:
    def __init__(self, syms, sites, frames):
        """syms: [(start, end)] sorted by start, ends non-decreasing; sites: call-site PCs; frames: {pc: [(func,
        file, line), ...]} in `addr2line -afi` order (inlined first, the outermost function last).  Every site gets a
        (maybe empty) entry."""
        self.sym_start = np.array([s for s, _ in syms], dtype=U64)
        self.sym_end = np.array([e for _, e in syms], dtype=U64)
        self.sites = np.array(sorted(sites), dtype=U64)
        self.frames = {int(pc): list(fr) for pc, fr in frames.items()}
        for pc in self.sites.tolist():
            self.frames.setdefault(pc, [])

    def symbolize(self, pcs):
        return [(pc, fn, fl, ln) for pc in pcs for fn, fl, ln in self.frames.get(int(pc), [])]


def intern(world, frames=None):
    """(tab_pcs, frame_off, frame_file, frame_line, frame_func, files, funcs): ids in order of first appearance
    walking the PCs upwards; files / funcs list the names by id."""
    frames = world.frames if frames is None else frames
    tab = sorted(frames)
    files, funcs = {}, {}
    off, ff, fl, fn = [0], [], [], []
    for pc in tab:
        for func, file, line in frames[pc]:
            ff.append(files.setdefault(file, len(files)))
            fn.append(funcs.setdefault(func, len(funcs)))
            fl.append(line)
        off.append(len(ff))
    return (np.array(tab, dtype=U64), np.array(off, dtype=U64), np.array(ff, dtype=U32), np.array(fl, dtype=U32),
            np.array(fn, dtype=U32), sorted(files, key=files.get), sorted(funcs, key=funcs.get))


# ---- hand-written ----------------------------------------------------------------
def hand_world():
    syms = [(K + 0x1000, K + 0x10ff), (K + 0x2000, K + 0x20ff), (K + 0x3000, K + 0x30ff),
            (K + 0x6000, K + 0x60ff), (K + 0x6080, K + 0x617f)]  # the last two overlap
    frames = {
        K + 0x1010: [("f1", "a.c", 10)],
        K + 0x1018: [("f1", "a.c", 11)],                                          # in the table, not a call site
        K + 0x1020: [],                                                           # a site with no frames
        K + 0x1030: [("inl_h", "h.h", 5), ("inl_g", "h.h", 9), ("f1", "a.c", 12)],  # a chain of 3 across 2 files
        K + 0x2010: [("f2", "b.c", 20)],
        K + 0x2020: [("inl_h", "h.h", 6), ("f2", "b.c", 21)],
        K + 0x2030: [("f2", "only_unc.c", 3)],
        K + 0x3010: [("f3", "c.c", 30)],
        K + 0x5000: [("stray", "s.c", 1)],                                        # outside every symbol
        K + 0x6010: [("g1", "g.c", 1)],
        K + 0x6090: [("g1", "g.c", 2)],
        K + 0x60a0: [("g1", "g.c", 3)],
        K + 0x6100: [("g2", "g.c", 50)],
    }
    sites = [K + o for o in (0x1010, 0x1020, 0x1030, 0x2010, 0x2020, 0x2030, 0x3010, 0x6010, 0x6090, 0x60a0, 0x6100)]
    return World(syms, sites, frames)


T, F = True, False
# (name, cover PCs in query order, expected fileSet, expected covered frames over the distinct PCs)
HAND = [
    # f1 is touched: its other sites are uncovered; 0x1020 has no frames; of 0x1030's chain only the f1 frame is kept
    # (inl_h and inl_g were never covered, though their symbol is touched); h.h gets no entry
    ("dropped_inlines", [0x1010], {"a.c": [(10, T), (12, F)]}, 1),
    # duplicate and unsorted cover; h.h:6 (inl_h at a site of f2) is kept only because inl_h was covered inlined at
    # 0x1030, in f1; only_unc.c is created by an uncovered frame alone; c.c (f3 untouched) has no entry
    ("inline_chain", [0x2010, 0x1030, 0x2010],
     {"a.c": [(10, F), (12, T)], "h.h": [(5, T), (6, F), (9, T)], "b.c": [(20, T), (21, F)], "only_unc.c": [(3, F)]}, 4),
    # a covered PC outside every symbol, and one in the table that is no call site (it still touches f1)
    ("stray_and_non_site", [0x5000, 0x1018], {"s.c": [(1, T)], "a.c": [(10, F), (11, T), (12, F)]}, 2),
    # overlapping symbols: 0x6090 lands in g1 and is deleted; 0x6100 lands in g2, whose range re-adds 0x6090 and
    # 0x60a0: 0x6090 is both covered and uncovered, its line is covered
    ("both_covered_and_uncovered", [0x6090, 0x6100], {"g.c": [(1, F), (2, T), (3, F), (50, T)]}, 2),
    # the only covered PC has no frames: nothing is kept, ncovered_frames == 0 ("does not have debug info")
    ("no_frames", [0x1020], {}, 0),
]


def hand_cov(pcs):
    return cov_of([K + o for o in pcs])


# ---- unit edges --------------------------------------------------------------------
def slots_world(n):
    """n table PCs in one symbol and one file, PC i at line i + 1: n slots.  Every fifth PC is no call site (its
    slot is set only when covered)."""
    frames = {K + 0x100 + 16 * i: [("f", "a.c", i + 1)] for i in range(n)}
    sites = [K + 0x100 + 16 * i for i in range(n) if i % 5]
    return World([(K, K + 0x100 + 16 * n)], sites, frames)


def slots_cover(n, rng):
    """Two covers of slots_world(n): a third of the PCs, and all of them in random order."""
    pcs = np.array([K + 0x100 + 16 * i for i in range(n)], dtype=U64)
    return [cov_of(pcs[rng.random(n) < 0.34]) if n > 1 else cov_of(pcs), cov_of(rng.permutation(pcs))]


SLOT_COUNTS = [1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025]  # the 64-bit word, the wave's chunk, the workgroup's tile


def ids_world(n=40):
    """Symbol k with its own func and file, ids k (bits 31, 32, 33 of the bitmaps among them), two sites each."""
    syms, frames, sites = [], {}, []
    for k in range(n):
        s = K + 0x100 * k
        syms.append((s, s + 0xff))
        frames[s + 0x10] = [("fn%d" % k, "file%d.c" % k, 1)]
        frames[s + 0x20] = [("fn%d" % k, "file%d.c" % k, 2)]
        sites += [s + 0x10, s + 0x20]
    return World(syms, sites, frames)


def frames_world():
    """Sites with 0, 1, 2, 3, 64 and 65 frames in one symbol (a site's frames are one thread's loop)."""
    frames, sites = {}, []
    for i, nf in enumerate([0, 1, 2, 3, 64, 65, 1, 0]):
        pc = K + 0x10 + 16 * i
        frames[pc] = [("inl%d" % (j % 3), "h%d.h" % (j % 2), 100 * i + j + 1) for j in range(nf - 1)]
        if nf:
            frames[pc].append(("f", "a.c", i + 1))
        sites.append(pc)
    return World([(K, K + 0xfff)], sites, frames)


# ---- random --------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def random_world(seed=7, nsym=12000, helpers=300):
    """About 150k sites and 220k frames: symbols of 1..24 sites (every 50th symbol overlapping its successor), the
    outermost frame in the symbol's own file, inline chains drawn from a small pool of header helpers with a heavy
    tail (a few header lines are hit from thousands of sites), some sites without frames, and table PCs that are
    no call sites."""
    rng = np.random.default_rng(seed)
    syms, frames, sites = [], {}, []
    pool = (rng.zipf(1.3, size=400000) - 1) % helpers
    pi = 0
    at = K
    for k in range(nsym):
        ns = int(rng.integers(1, 25))
        size = 16 * ns + 16
        start, end = at, at + size - 1
        if k % 50 == 49:
            end += 64  # reaches into the next symbol
        if syms and end < syms[-1][1]:
            end = syms[-1][1]
        syms.append((start, end))
        file = "dir%d/file%d.c" % (k % 37, k % 1500)
        for i in range(ns):
            pc = start + 8 + 16 * i
            r = rng.random()
            if r < 0.04:
                frames[pc] = []
            else:
                chain = []
                nin = 0 if r < 0.70 else int(rng.integers(1, 4)) if r < 0.98 else int(rng.integers(4, 12))
                for _ in range(nin):
                    h = int(pool[pi]); pi += 1
                    chain.append(("helper%d" % h, "include/h%d.h" % (h % 40), 10 + h % 7))
                chain.append(("func%d" % k, file, 1 + i))
                frames[pc] = chain
            if rng.random() < 0.93:
                sites.append(pc)
        at += size + int(rng.integers(0, 3)) * 16
    return World(syms, sites, frames)


@functools.lru_cache(maxsize=None)
def random_cover(seed=11, nq=100000, missing=0):
    """nq cover words over the random world in random order: 90% from the table PCs of a tenth of the symbols, the
    rest anywhere; with `missing`, that many PCs that the table does not hold (some twice)."""
    w = random_world()
    rng = np.random.default_rng(seed)
    tab = np.array(sorted(w.frames), dtype=U64)
    sym = np.searchsorted(w.sym_start, tab, side="right") - 1
    hot = rng.random(w.sym_start.size) < 0.10
    pool = tab[hot[sym] & (rng.random(tab.size) < 0.6)]
    q = np.concatenate([rng.choice(pool, size=nq - nq // 10), rng.choice(tab, size=nq // 10 - missing)])
    if missing:
        extra = tab[rng.integers(0, tab.size, size=missing - missing // 3)] + U64(3)  # table PCs are 8 mod 16
        q = np.concatenate([q, extra, extra[: missing // 3]])
    return cov_of(rng.permutation(q))
