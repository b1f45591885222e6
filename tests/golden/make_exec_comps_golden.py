"""Regenerate tests/golden/exec_comps_golden.npz from the reference executor.

Run where the reference checkout exists (as make_golden.py):
    python tests/golden/make_exec_comps_golden.py

The calls of tests/exec_comps_cases.golden_calls() go through the comparison
branch of handle_completion (executor/executor.h:379-387) built from the
reference's OWN compiled code: oracle/_ref/libref_executor.so (oracle/Makefile)
exports kcov_comparison_t's operator< (:665-673), operator== (:659-663) and
write (:621-657).  Per call: a sort under the reference operator<, std::unique's
rule (keep the first of a run) under the reference operator==, then the
reference write() on each survivor, with a callback that appends the word;
arg1 / arg2 are read back from the struct write() extended in place.  pc takes
no part in either operator and is never written, so any correct sort under
that comparator yields what std::sort yields.
The fixture holds data only: the input records, and the reference's triples,
words and offsets.
"""
import ctypes
import functools
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)


class KcovComparison(ctypes.Structure):  # executor.h:118-123
    _fields_ = [("type", ctypes.c_uint64), ("arg1", ctypes.c_uint64), ("arg2", ctypes.c_uint64), ("pc", ctypes.c_uint64)]


WRITE_ONE = ctypes.CFUNCTYPE(ctypes.c_void_p, ctypes.c_uint32)


def reference():
    from oracle import pyoracle

    pyoracle.build()
    R = ctypes.CDLL(pyoracle.REF_SO)
    P = ctypes.POINTER(KcovComparison)
    lt = getattr(R, "_ZNK17kcov_comparison_tltERKS_")
    eq = getattr(R, "_ZNK17kcov_comparison_teqERKS_")
    wr = getattr(R, "_ZN17kcov_comparison_t5writeEPFPjjE")
    lt.restype = eq.restype = ctypes.c_bool
    lt.argtypes = eq.argtypes = [P, P]
    wr.restype = None
    wr.argtypes = [P, WRITE_ONE]
    return lt, eq, wr


def ref_call(ref, recs):
    lt, eq, wr = ref
    cs = [KcovComparison(*r) for r in recs]

    def cmp(a, b):
        return -1 if lt(ctypes.byref(a), ctypes.byref(b)) else (1 if lt(ctypes.byref(b), ctypes.byref(a)) else 0)

    cs.sort(key=functools.cmp_to_key(cmp))  # :384
    kept = []  # :385
    for c in cs:
        if not kept or not eq(ctypes.byref(kept[-1]), ctypes.byref(c)):
            kept.append(c)
    words = []

    def write_one(v):
        words.append(v)
        return None

    cb = WRITE_ONE(write_one)
    triples = []
    for c in kept:  # :386-387
        wr(ctypes.byref(c), cb)
        triples.append((c.type, c.arg1, c.arg2))
    return triples, words


def main():
    from tests import exec_comps_cases as EC

    ref = reference()
    calls = EC.golden_calls()
    recs, call_off = EC.to_arrays(calls)
    comp_off, word_off, comps, words = [0], [0], [], []
    for c in calls:
        t, w = ref_call(ref, c)
        comps += t
        words += w
        comp_off.append(len(comps))
        word_off.append(len(words))
    path = os.path.join(HERE, "exec_comps_golden.npz")
    np.savez_compressed(path, recs=recs, call_off=call_off, comp_off=np.array(comp_off, np.uint64),
                        comps=np.array(comps, np.uint64).reshape(len(comps), 3), word_off=np.array(word_off, np.uint64),
                        words=np.array(words, np.uint64).astype(np.uint32))
    print("exec comps golden: calls=%d records=%d comps=%d words=%d bytes=%d" %
          (len(calls), recs.shape[0], len(comps), len(words), os.path.getsize(path)))


if __name__ == "__main__":
    main()
