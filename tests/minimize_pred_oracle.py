"""TEST INFRASTRUCTURE ONLY: the checker of sg_minimize_pred_from_kcov.

The closure triageInput hands to prog.Minimize (syz-fuzzer/fuzzer.go:578-591)
restated, one statement per reference step, from tests/triage_runs_oracle.py
(run_info: the execution), O.canonicalize and O.foreach (the literal two-pointer
loop).  execute()'s own new-signal check (:665-691) is oracle.pyoracle's trace
triage: the executor's signal of every call, then the sequential loop.
"""
import numpy as np

from oracle import pyoracle as O
from tests import triage_runs_oracle as TR

U32, U64 = np.uint32, np.uint64
OK, NOT_EXECUTED, LOST = 0, 1, 2
EMPTY = np.zeros(0, dtype=U32)


def predicate(new, run, call1):
    """One predicate call: new is newSignal, run the shortened program's
    execution (a list of its calls' KCOV buffers, u64 PCs)."""
    info = TR.run_info(run, call1)                                           # :579 execute()
    if info is None or len(info[0]) == 0:                                    # :580-582
        return NOT_EXECUTED
    sig, m = O.canonicalize(info[0])                                         # :584
    if len(O.foreach(O.INTER, new, sig[:m])) != len(new):                    # :587-589
        return LOST
    return OK                                                                # :590


def run_signal(run):
    """info[c].Signal of every call of one execution: (vals, off)."""
    calls = [np.asarray(c, dtype=U64).reshape(-1) for c in run]
    if not calls:
        return EMPTY, np.zeros(1, dtype=U64)
    call_off = np.concatenate([[0], np.cumsum([c.size for c in calls])]).astype(U64)
    pcs32 = (np.concatenate(calls) & U64(0xFFFFFFFF)).astype(U32)
    return O.exec_signal(pcs32, call_off, [0, len(calls)])                   # a fresh table per execution


def batch(lists, attempts, maxset=None, newset=None):
    """attempts: a list of (cand, call1, run); lists: the newSignal lists.
    Returns the status array and, with maxset (an O.OSet, updated; newset
    likewise), also (rec_new, sig_vals, sig_off) as sg_minimize_pred_from_kcov."""
    status = np.array([predicate(np.asarray(lists[k], dtype=U32), run, c1) for k, c1, run in attempts], dtype=np.int32)
    if maxset is None:
        return status
    sigs = []                                                                # per call, in batch order
    selected = []
    for _, c1, run in attempts:
        v, off = run_signal(run)
        sigs += [v[int(off[c]):int(off[c + 1])] for c in range(len(run))]
        selected += [c == c1 for c in range(len(run))]
    all_off = np.concatenate([[0], np.cumsum([s.size for s in sigs])]).astype(U64)
    all_vals = np.concatenate(sigs).astype(U32) if sigs else EMPTY
    rec_new = O.triage_flags_only(maxset, newset, all_vals, all_off)         # fuzzer.go:665-691, every call in order
    kept = [s if (rec_new[c] or selected[c]) else EMPTY for c, s in enumerate(sigs)]  # :678-683 and info[call1]
    sig_off = np.concatenate([[0], np.cumsum([s.size for s in kept])]).astype(U64)
    sig_vals = np.concatenate(kept).astype(U32) if kept else EMPTY
    return status, rec_new, sig_vals, sig_off


def to_arrays(lists, attempts):
    """The flat arguments of sg_minimize_pred_from_kcov: new_vals, new_off,
    cand, call, pcs, call_off, prog_off."""
    ls = [np.asarray(x, dtype=U32).reshape(-1) for x in lists]
    new_off = np.concatenate([[0], np.cumsum([x.size for x in ls])]).astype(U64)
    calls = [np.asarray(x, dtype=U64).reshape(-1) for _, _, run in attempts for x in run]
    prog_off = np.concatenate([[0], np.cumsum([len(run) for _, _, run in attempts])]).astype(U64)
    call_off = np.concatenate([[0], np.cumsum([x.size for x in calls])]).astype(U64)
    return (np.concatenate(ls) if ls else EMPTY, new_off, np.array([a[0] for a in attempts], dtype=U32),
            np.array([a[1] for a in attempts], dtype=U32), np.concatenate(calls) if calls else np.zeros(0, dtype=U64),
            call_off, prog_off)
