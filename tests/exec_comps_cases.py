"""Seeded KCOV_TRACE_CMP buffers for the sg_exec_comps tests and for the golden
fixture's generator: calls as lists of (type, arg1, arg2, pc)."""
import numpy as np

M64 = (1 << 64) - 1
PC0 = 0xFFFFFFFF81000000  # kernel text; the low PC bits vary, as a loop's do

EDGE_OPERANDS = [0, 1, 0x7F, 0x80, 0xFF, 0x17F, 0x180, 0x7FFF, 0x8000, 0xFFFF, 0x18000, 0x7FFFFFFF, 0x80000000,
                 0xFFFFFFFF, 0x100000005, 0x5, 0x180000000, 1 << 63, (1 << 63) - 1, M64, M64 - 1, 0xFFFFFFFF00000080]


def pool(rng, n):
    """n distinct (type, arg1, arg2): types 0..7, operands from the edge list
    and random values of 8 to 64 bits."""
    seen, out = set(), []
    while len(out) < n:
        typ = int(rng.integers(0, 8))
        ops = []
        for _ in range(2):
            if rng.integers(0, 3) == 0:
                ops.append(EDGE_OPERANDS[int(rng.integers(0, len(EDGE_OPERANDS)))])
            else:
                ops.append(int(rng.integers(0, 1 << 63, dtype=np.uint64)) >> int(rng.integers(0, 56)))
        key = (typ, ops[0], ops[1])
        if key not in seen:
            seen.add(key)
            out.append(key)
    return out


def draw(rng, p, n):
    """n records drawn from the pool p, each with a pc of its own."""
    return [p[int(i)] + (PC0 + 4 * int(pc),) for i, pc in zip(rng.integers(0, len(p), size=n),
                                                                rng.integers(0, 1 << 12, size=n))]


def distinct(rng, n, types=8):
    """n records, all distinct in (type, arg1, arg2), in random order."""
    a1 = rng.permutation(n)
    return [(int(i) % types, int(x) * 0x9E3779B97F4A7C15 & M64, int(rng.integers(0, 1 << 62)), PC0 + 4 * int(i))
            for i, x in enumerate(a1)]


def edge_calls(rng):
    """The named edge cases, each one call of at most 300 records."""
    p = pool(rng, 60)
    calls = {"empty": [], "one": draw(rng, p, 1)}
    calls["two_equal"] = [(4, 7, 9, PC0), (4, 7, 9, PC0 + 8)]
    calls["two_reversed"] = [(4, 9, 7, PC0), (4, 7, 9, PC0)]
    for n in (63, 64, 65, 255, 256, 257):
        calls["pool_%d" % n] = draw(rng, p, n)
    # equal (type, arg1, arg2), different pc: one entry
    calls["pcs"] = [(2, 0x1234, 0x8000, PC0 + 4 * i) for i in range(40)] + [(2, 0x1234, 0x8001, PC0)]
    # operands that differ only above the operand's width: two entries, equal words
    calls["above_width"] = [(4, 0x100000005, 1, PC0), (4, 0x5, 1, PC0), (0, 0x17F, 0x27F, PC0), (0, 0x7F, 0x7F, PC0),
                            (2, 0x18000, 0x8000, PC0), (2, 0x8000, 0x18000, PC0), (5, 0xFFFFFFFF00000080, 0x80, PC0),
                            (5, 0x80, 0x80, PC0)]
    # every size class and the const bit, the sign bit of the width set and clear
    calls["sizes"] = [(t, a, b, PC0) for t in range(8) for a, b in
                      ((0x7F, 0x80), (0x7FFF, 0x8000), (0x7FFFFFFF, 0x80000000), ((1 << 63) - 1, 1 << 63),
                       (0xFF, 0xFFFF), (0xFFFFFFFF, M64))]
    # a type above 32 bits sorts after every small type and writes its low word
    calls["big_type"] = [((1 << 32) + 1, 3, 4, PC0), (7, M64, M64, PC0), (1, 3, 4, PC0), ((1 << 32) + 1, 3, 4, PC0 + 4),
                         ((1 << 32) + 7, 1 << 40, 2, PC0), (M64, M64, M64, PC0), (M64, 0, 0, PC0), (1 << 63, 5, 6, PC0)]
    calls["extremes"] = [(t, a, b, PC0) for t in (0, 3, 4, 6, 7) for a in (0, 1 << 63, M64) for b in (0, 1 << 63, M64)]
    calls["distinct_300"] = distinct(rng, 300)
    calls["equal_300"] = [(6, 1 << 63, 0xFFFFFFFF, PC0 + 4 * (i % 7)) for i in range(300)]
    # any u64 in every field
    calls["random_fields"] = [tuple(int(x) for x in rng.integers(0, 1 << 64, size=4, dtype=np.uint64)) for _ in range(120)]
    calls["random_fields"] += calls["random_fields"][:40]
    return calls


def to_arrays(calls):
    """calls (lists of 4-tuples) -> (recs u64[n, 4], call_off)."""
    off = np.concatenate([[0], np.cumsum([len(c) for c in calls])]).astype(np.uint64)
    flat = [r for c in calls for r in c]
    return np.array(flat, dtype=np.uint64).reshape(len(flat), 4), off


def golden_calls():
    """The calls the golden fixture records: the edge cases, 20 pool calls of
    up to 300 records, and one full buffer (16,383 records, kCoverSize 64 Ki
    words) drawn from 500 distinct triples."""
    rng = np.random.default_rng(20171013)
    calls = list(edge_calls(rng).values())
    p = pool(rng, 90)
    for _ in range(20):
        calls.append(draw(rng, p, int(rng.integers(0, 301))))
    calls.append(draw(rng, pool(rng, 500), 16383))
    return calls
