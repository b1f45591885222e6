"""TEST INFRASTRUCTURE ONLY: the checker of sg_comps_pairs and
sg_hints_from_kcov (the product never imports it).

pairs_of restates the loop body of the executor output reader
(pkg/ipc/ipc_linux.go:266-302), one statement per reference step, over
full-width operands: the triples {type, arg1', arg2'} that
kcov_comparison_t::write leaves (executor/executor.h:632-645), not the wire
words.  batch composes it with tests/exec_comps_oracle.py (the executor's
sort, unique and write) and tests/hints_oracle.py (shrinkExpand).
"""
import numpy as np

from tests import exec_comps_oracle as X
from tests import hints_oracle as H

COMP_SIZE_MASK, COMP_CONST_MASK = 6, 1  # ipc_linux.go:41-43
OK, COMPS_TYPE = H.OK, H.COMPS_TYPE
M64 = (1 << 64) - 1


def pairs_of(triples):
    """One call's triples [(type, arg1, arg2)] -> (status, [(key, value)]): the
    reader's AddComp calls in its order; (COMPS_TYPE, []) when the reader
    returns at :266-270, before it assigns Comps (:304)."""
    added = []  # :258 compMap, as its AddComp sequence
    for typ, arg1, arg2 in triples:  # :259
        typ, arg1, arg2 = int(typ), int(arg1), int(arg2)
        if typ > COMP_CONST_MASK | COMP_SIZE_MASK:  # :266
            return COMPS_TYPE, []
        is_const = (typ & COMP_CONST_MASK) != 0  # :273
        _, op1, op2 = X.write((typ, arg1, arg2))  # the operands at full width (executor.h:632-645; idempotent)
        if op1 == op2:  # :290
            continue
        added.append((op2, op1))  # :294
        if is_const:  # :295
            continue
        added.append((op1, op2))  # :302
    return OK, added  # :304


def pairs_batch(comp_off, comps):
    """The batch contract of sg_comps_pairs: (status[], pair_lists[])."""
    rows = np.asarray(comps, dtype=np.uint64).reshape(-1, 3).tolist()
    status, lists = [], []
    for c in range(len(comp_off) - 1):
        st, added = pairs_of(rows[int(comp_off[c]):int(comp_off[c + 1])])
        status.append(st)
        lists.append(added)
    return status, lists


def pairs_arrays(lists):
    """pair_lists -> (pairs u64[n, 2], pair_off)."""
    off = np.concatenate([[0], np.cumsum([len(x) for x in lists])]).astype(np.uint64)
    flat = [kv for x in lists for kv in x]
    return np.array(flat, dtype=np.uint64).reshape(len(flat), 2), off


def batch(recs, call_off, vals, val_off):
    """The contract of sg_hints_from_kcov: raw records and values -> (status[],
    pair_lists[], replacers[]): per value slot its replacers, ascending."""
    comp_off, comps, _, _ = X.batch(recs, call_off)
    status, lists = pairs_batch(comp_off, comps)
    reps = []
    for c, added in enumerate(lists):
        m = H.comp_map(added)
        for i in range(int(val_off[c]), int(val_off[c + 1])):
            reps.append(sorted(H.shrink_expand(int(vals[i]), m)))
    return status, lists, reps


def reps_arrays(reps):
    """per-slot replacer lists -> (reps u64, rep_off)."""
    off = np.concatenate([[0], np.cumsum([len(x) for x in reps])]).astype(np.uint64)
    return np.array([x for s in reps for x in s], dtype=np.uint64), off
