"""TEST INFRASTRUCTURE ONLY: the checker of sg_exec_comps.

Pure-Python restatement of the comparison branch of handle_completion
(executor/executor.h:379-387) with kcov_comparison_t's operator< (:665-673),
operator== (:659-663) and write (:621-657), one statement per reference step.
Its parity is pinned by tests/golden/exec_comps_golden.npz, which the
reference's own compiled code produced (tests/golden/make_exec_comps_golden.py).
"""
import functools

import numpy as np

M64 = (1 << 64) - 1
KCOV_CMP_CONST = 1  # executor.h:109-114
KCOV_CMP_SIZE_MASK = 6
KCOV_CMP_SIZE1, KCOV_CMP_SIZE2, KCOV_CMP_SIZE4, KCOV_CMP_SIZE8 = 0, 2, 4, 6


def less(a, b):
    """operator< (:665-673) over records (type, arg1, arg2, pc)."""
    if a[0] != b[0]:
        return a[0] < b[0]
    if a[1] != b[1]:
        return a[1] < b[1]
    return a[2] < b[2]


def equal(a, b):
    """operator== (:659-663)."""
    return a[0] == b[0] and a[1] == b[1] and a[2] == b[2]


def _sext(x, bits):
    x &= (1 << bits) - 1
    return (x | (M64 ^ ((1 << bits) - 1))) & M64 if x >> (bits - 1) else x


def write(rec):
    """write() (:621-657): (the words it emits, arg1 and arg2 as it leaves them)."""
    typ, arg1, arg2 = rec[0], rec[1], rec[2]
    words = [typ & 0xFFFFFFFF]  # :624
    size = typ & KCOV_CMP_SIZE_MASK  # :632
    if size == KCOV_CMP_SIZE1:
        arg1, arg2 = _sext(arg1, 8), _sext(arg2, 8)  # :634-635
    elif size == KCOV_CMP_SIZE2:
        arg1, arg2 = _sext(arg1, 16), _sext(arg2, 16)  # :638-639
    elif size == KCOV_CMP_SIZE4:
        arg1, arg2 = _sext(arg1, 32), _sext(arg2, 32)  # :642-643
    if size != KCOV_CMP_SIZE8:  # :646-651
        words += [arg1 & 0xFFFFFFFF, arg2 & 0xFFFFFFFF]
    else:  # :653-656
        words += [arg1 & 0xFFFFFFFF, arg1 >> 32, arg2 & 0xFFFFFFFF, arg2 >> 32]
    return words, arg1, arg2


def call_comps(recs):
    """executor.h:379-387 for one call: recs = [(type, arg1, arg2, pc)].
    Returns (triples [(type, arg1', arg2')], words)."""
    start = sorted(recs, key=functools.cmp_to_key(lambda a, b: -1 if less(a, b) else (1 if less(b, a) else 0)))  # :384
    kept = []  # :385 std::unique: the first of every run of equal records
    for r in start:
        if not kept or not equal(kept[-1], r):
            kept.append(r)
    triples, words = [], []
    for r in kept:  # :386-387
        w, arg1, arg2 = write(r)
        words += w
        triples.append((r[0], arg1, arg2))
    return triples, words


def batch(recs, call_off):
    """The batch contract of sg_exec_comps: (comp_off, comps u64[n, 3],
    word_off, words u32)."""
    recs = np.asarray(recs, dtype=np.uint64).reshape(-1, 4)
    rows = recs.tolist()
    comp_off, word_off, comps, words = [0], [0], [], []
    for c in range(len(call_off) - 1):
        t, w = call_comps([tuple(x) for x in rows[int(call_off[c]):int(call_off[c + 1])]])
        comps += t
        words += w
        comp_off.append(len(comps))
        word_off.append(len(words))
    return (np.array(comp_off, dtype=np.uint64), np.array(comps, dtype=np.uint64).reshape(len(comps), 3),
            np.array(word_off, dtype=np.uint64), np.array(words, dtype=np.uint64).astype(np.uint32))
