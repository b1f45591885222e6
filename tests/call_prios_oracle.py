"""Test oracle of the call priorities: prog/prio.go:133-229 restated twice with
numpy float32.  `literal_*` follow the reference loop by loop with float32
scalars (the triple loop of calcDynamicPrio adds 1.0 to a float32 cell, and
normalizePrio runs cell by cell); the closed form takes the exact integer
counts sum_p n_p(i) * n_p(j), reads a cell as float32(min(count, 2^24)) (1.0
added to a float32 is exact up to 2^24 and then sticks) and normalises a row
at a time with float32 arrays, every operation still rounded to float32.
tests/test_call_prios.py shows that the two agree.  Pinned by restatement
only: no Go toolchain."""
import bisect

import numpy as np

F32, U64, I64 = np.float32, np.uint64, np.int64
NO_CALL = 0xFFFFFFFF
SAT = 1 << 24


def programs(ids, off):
    ids, off = np.asarray(ids), np.asarray(off)
    return [ids[int(off[p]):int(off[p + 1])] for p in range(off.size - 1)]


# ---- the literal form ---------------------------------------------------------------
def literal_cells(progs, ncalls, mmap_id):
    """prio.go:134-151: the float32 matrix before normalizePrio."""
    prios = np.zeros((ncalls, ncalls), F32)
    one = F32(1.0)
    for p in progs:
        for id0 in p:
            for id1 in p:
                if id0 == id1 or id0 == mmap_id or id1 == mmap_id:
                    continue
                prios[id0, id1] = F32(prios[id0, id1] + one)
    return prios


def literal_normalize(cells):
    """prio.go:158-192, cell by cell with float32 scalars."""
    out = np.array(cells, dtype=F32, copy=True)
    for prio in out:
        mx, mn, nzero = F32(0), F32(1e10), 0
        for p in prio:
            if mx < p:
                mx = p
            if p != 0 and mn > p:
                mn = p
            if p == 0:
                nzero += 1
        if nzero != 0:
            mn = F32(mn / F32(F32(2) * F32(nzero)))
        for i in range(prio.size):
            p = prio[i]
            if mx == 0:
                prio[i] = 1
                continue
            if p == 0:
                p = mn
            p = F32(F32(F32(F32(p - mn) / F32(mx - mn)) * F32(0.9)) + F32(0.1))
            if p > 1:
                p = F32(1)
            prio[i] = p
    return out


def literal_run(prios, enabled):
    """prio.go:214-227; a disabled row (nil in Go) is None."""
    n = prios.shape[0]
    run = []
    for i in range(n):
        if not enabled[i]:
            run.append(None)
            continue
        row, s = [], 0
        for j in range(n):
            if enabled[j]:
                s += int(F32(prios[i, j] * F32(1000)))
            row.append(s)
        run.append(row)
    return run


# ---- the closed form ----------------------------------------------------------------
def counts(ids, off, ncalls, mmap_id):
    """count[i][j] = sum_p n_p(i) * n_p(j), i != j, neither mmap: exact, uint64."""
    ids, off = np.asarray(ids).astype(I64), np.asarray(off).astype(I64)
    c = np.zeros((ncalls, ncalls), I64)
    for p in range(off.size - 1):
        seg = ids[off[p]:off[p + 1]]
        if seg.size == 0:
            continue
        u, n = np.unique(seg, return_counts=True)
        c[np.ix_(u, u)] += np.outer(n, n)
    c[np.arange(ncalls), np.arange(ncalls)] = 0
    if mmap_id != NO_CALL:
        c[mmap_id, :] = 0
        c[:, mmap_id] = 0
    return c.astype(U64)


def cells(cnt):
    """The reference's float32 cell of an exact count."""
    return np.minimum(cnt, U64(SAT)).astype(F32)


def normalize(cl):
    """normalizePrio a row at a time; float32 arrays round every operation to float32."""
    cl = np.asarray(cl, F32)
    out = np.empty_like(cl)
    for i, prio in enumerate(cl):
        mx = prio.max()
        if mx == 0:
            out[i] = 1
            continue
        nz = prio != 0
        mn = prio[nz].min() if nz.any() else F32(1e10)
        nzero = int(prio.size - nz.sum())
        if nzero:
            mn = F32(mn / F32(F32(2) * F32(nzero)))
        p = np.where(nz, prio, mn).astype(F32)
        q = ((p - mn) / F32(mx - mn)).astype(F32)
        q = (q * F32(0.9)).astype(F32)
        q = (q + F32(0.1)).astype(F32)
        out[i] = np.minimum(q, F32(1))
    return out


def normalize_fused(cl):
    """What a contracted build would give: q * 0.9 + 0.1 with one rounding (the product of two float32 is exact in
    float64).  Only to show that the parity cases can tell the two apart."""
    cl = np.asarray(cl, F32)
    out = np.empty_like(cl)
    for i, prio in enumerate(cl):
        mx = prio.max()
        if mx == 0:
            out[i] = 1
            continue
        nz = prio != 0
        mn = prio[nz].min()
        nzero = int(prio.size - nz.sum())
        if nzero:
            mn = F32(mn / F32(F32(2) * F32(nzero)))
        p = np.where(nz, prio, mn).astype(F32)
        q = ((p - mn) / F32(mx - mn)).astype(F32)
        q = (q.astype(np.float64) * np.float64(F32(0.9)) + np.float64(F32(0.1))).astype(F32)
        out[i] = np.minimum(q, F32(1))
    return out


def run_sums(prios, enabled):
    """BuildChoiceTable's matrix form: a disabled row is all zeros."""
    prios = np.asarray(prios, F32)
    en = np.ones(prios.shape[0], bool) if enabled is None else np.asarray(enabled).astype(bool)
    v = (prios * F32(1000)).astype(F32).astype(I64)  # truncation
    v[:, ~en] = 0
    run = np.cumsum(v, axis=1)
    run[~en, :] = 0
    return run.astype(np.int32)


def everything(ids, off, ncalls, mmap_id, static, enabled):
    """(counts, dynamic, prios, run) of a corpus, closed form."""
    cnt = counts(ids, off, ncalls, mmap_id)
    dyn = normalize(cells(cnt))
    pr = (dyn * np.asarray(static, F32)).astype(F32)
    return cnt, dyn, pr, run_sums(pr, enabled)


def choose(run, enabled, draws, call):
    """ChoiceTable.Choose (prio.go:231-247) with the draws of r.Intn given as an iterator of functions' results:
    draws(n) returns the next number in [0, n).  enabledCalls ascending."""
    en = np.asarray(enabled).astype(bool)
    calls = [i for i in range(en.size) if en[i]]
    row = run[call] if call >= 0 else None
    if row is None:
        return calls[draws(len(calls))]
    while True:
        x = draws(int(row[-1]))
        i = bisect.bisect_left(list(row), x)
        if not en[i]:
            continue
        return i
