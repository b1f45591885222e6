"""TEST INFRASTRUCTURE ONLY: the batches of tests/test_minimize_pred.py.  Each
builder returns (lists, attempts): the newSignal lists and the attempts (cand,
call1, run) of tests/minimize_pred_oracle.py, a run being the list of its
calls' u64 KCOV buffers."""
import functools

import numpy as np

from tests import minimize_pred_oracle as MP
from tests import triage_runs_oracle as TR

U32, U64 = np.uint32, np.uint64
S = 0xFFFFFFFF
TEXT = 0xFFFFFFFF81000000
A, B, C = TEXT + 16, TEXT + 32, TEXT + 48
WAVE = 64          # lanes of a wave
LONG = 8300        # PCs of the long call: more than one LDS chunk of tin_intersect holds


def tr(rng, n, nvals, base=0):
    """A call's trace: n PCs of a pool of nvals kernel-text PCs starting at slot base."""
    pool = TEXT + 16 * (base + rng.choice(1 << 16, size=max(nvals, 1), replace=False).astype(U64))
    return pool[rng.integers(0, max(nvals, 1), size=n)]


def sig_of(run, call):
    info = TR.run_info(run, call)
    return info[0] if info is not None else TR.EMPTY


def canon(run, call):
    return np.unique(sig_of(run, call))


@functools.lru_cache(maxsize=None)
def planted():
    """Every exit of the closure as an attempt of its own, and one list shared
    by five attempts in shuffled order."""
    rng = np.random.default_rng(60)
    R = [tr(rng, 60, 20), tr(rng, 150, 40), tr(rng, 30, 8)]
    R2 = [R[0], np.concatenate([R[1], tr(rng, 25, 9, 1 << 17)]), R[2]]   # the same call with extra PCs: still holds it
    D = [tr(rng, 60, 20, 1 << 19), tr(rng, 150, 40, 1 << 19)]
    shared = canon(R, 1)
    one = int(sig_of([[5]], 0)[0])
    assert one == 5
    lists = [[],                            # 0
             [3525549802],                  # 1: edge B-after-A
             [678886622],                   # 2: what call 1 of [[A, B], [A, B, C]] is left with
             [16, 2639983419],              # 3: two PCs equal below bit 32
             [5, 5],                        # 4: a repeat
             [5, S],                        # 5: the sentinel
             shared,                        # 6
             [5]]                           # 7
    wide = [[0x1_0000_0010, 0x2_0000_0010]]
    att = [(0, 1, [[A, B], [A, B]]),        # no Signal left: not executed, whatever the list
           (1, 1, [[A, B], [A, B]]),
           (2, 1, [[A, B], [A, B, C]]),     # OK
           (1, 1, [[A, B], [A, B, C]]),     # LOST: the edge is in the call's own trace, the table dropped it
           (1, 0, [[A, B, C]]),             # the same trace as call 0: OK
           (6, 1, R),                       # the shared list, first of five
           (3, 0, wide),                    # truncation before hashing
           (0, 0, [[A]]),                   # the empty list: executed
           (0, 0, []),                      # ... and not
           (6, 1, D),                       # shared: LOST
           (4, 0, [[5]]),                   # LOST
           (5, 0, [[5]]),                   # LOST
           (7, 0, [[5]]),                   # OK
           (6, 1, R[:1]),                   # shared: exactly call1 calls
           (7, 0, []),                      # an execution with no calls
           (7, 2, [[5], [5]]),              # exactly call1 calls
           (6, 1, R2),                      # shared: OK
           (7, 1, [[5], []]),               # call1 holds 0 PCs
           (6, 1, [R[0], R[1][:0], R[2]]),  # shared: call1 holds 0 PCs
           (7, 1, [[9], [5]])]              # call 1 of two
    return lists, att


PLANTED_STATUS = [1, 1, 0, 2, 0, 0, 0, 0, 1, 2, 2, 2, 0, 1, 1, 1, 0, 1, 1, 0]


@functools.lru_cache(maxsize=None)
def random_batch(seed=61, n=48, nlists=12):
    """n attempts on nlists lists: executions of 0..5 calls of 0..300 PCs from
    pools of 8..40 values, so that a call often finds its edges in the table
    already."""
    rng = np.random.default_rng(seed)
    bases, lists = [], []
    for k in range(nlists):
        ncalls = int(rng.integers(1, 6))
        pool, base = int(rng.integers(8, 41)), int(rng.integers(0, 4)) << 17
        run = [tr(rng, int(rng.integers(0, 301)), pool, base) for _ in range(ncalls)]
        call = int(rng.integers(0, ncalls))
        if run[call].size == 0:
            run[call] = tr(rng, 40, pool, base)
        full = canon(run, call)
        take = full if rng.integers(3) == 0 else rng.choice(full, size=int(rng.integers(0, full.size + 1)), replace=False)
        bases.append((run, call, pool, base))
        lists.append(np.sort(take).astype(U32))
    att = []
    for e in range(n):
        k = int(rng.integers(0, nlists))
        run, call, pool, base = bases[k]
        kind = int(rng.integers(0, 7))
        if kind == 0:                                    # as it was
            r, c = run, call
        elif kind == 1 and call > 0:                     # an earlier call removed: the table starts emptier
            i = int(rng.integers(0, call))
            r, c = run[:i] + run[i + 1:], call - 1
        elif kind == 2:                                  # an earlier call added, from the same pool
            r, c = [np.concatenate(run)] + run, call + 1
        elif kind == 3:                                  # the call cut short
            r, c = run[:call] + [run[call][: run[call].size // 2]] + run[call + 1:], call
        elif kind == 4:                                  # not executed: too few calls, none, or no PCs
            r, c = [run[:call], [], run[:call] + [run[call][:0]]][int(rng.integers(0, 3))], call
        elif kind == 5:                                  # somewhere else entirely
            r, c = [tr(rng, 80, 30, base + (1 << 20)) for _ in run], call
        else:                                            # another list's execution
            r, c = bases[int(rng.integers(0, nlists))][:2]
        att.append((k, c, list(r)))
    return lists, att


@functools.lru_cache(maxsize=None)
def long_call():
    """One call of LONG consecutive distinct PCs and its Signal in trace order
    (edge t is pcs[t] ^ hash(pcs[t - 1])): LONG distinct values."""
    pcs = TEXT + 16 * np.arange(LONG, dtype=U64)
    sig = sig_of([pcs], 0)
    assert sig.size == LONG and np.unique(sig).size == LONG
    return pcs, sig


def without(pcs, t):
    """The trace with edge t gone and every other edge kept: a PC from elsewhere in front of pcs[t]."""
    return np.concatenate([pcs[:t], [U64(TEXT + (1 << 30) + 16 * t)], pcs[t:]])


@functools.lru_cache(maxsize=None)
def length_edges():
    """Lists of 1 .. 8193 values on both sides of a wave's width and of the LDS
    chunk, against a Signal with all of the list and with all but one value,
    and Signals of 1 .. LONG values around a wave's and the workgroup's
    widths.  Returns (lists, attempts, expected status)."""
    pcs, sig = long_call()
    order = np.argsort(sig)                               # order[i]: the trace position of the i-th smallest signal
    ssig = sig[order]
    lists, att, exp = [], [], []
    for n in (1, 63, 64, 65, 8191, 8192, 8193):
        k = len(lists)
        lists.append(ssig[:n])
        att.append((k, 0, [pcs]))
        exp.append(MP.OK)
        for i in sorted({0, n - 1} | {i for i in (63, 64, 8191, 8192) if i < n}):
            att.append((k, 0, [without(pcs, int(order[i]))]))
            exp.append(MP.LOST)
    for m in (1, 63, 64, 65, 255, 256, 257, LONG):
        head = np.sort(sig[:m])
        base = len(lists)
        lists += [head,                                   # all of Signal
                  head[: min(m, WAVE)],                   # a wave's width of it
                  sig[m - 1: m],                          # its last value alone
                  np.sort(sig[: m + 1]) if m < LONG else np.sort(np.append(head, U32(7))),  # one value more than it has
                  [7]]                                    # a value it lacks
        att += [(base + j, 0, [pcs[:m]]) for j in range(5)]
        exp += [MP.OK, MP.OK, MP.OK, MP.LOST, MP.LOST]
    return lists, att, np.array(exp, dtype=np.int32)
