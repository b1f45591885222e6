"""Seeded comps-mode executor output batches and argument values for the hint
tests: regions written the reader's way (oracle/ipc_oracle.py write_call,
widths="reader"), operands and values drawn from one small pool so that
values meet comparison operands."""
import collections
import json
import os

import numpy as np

from oracle import ipc_oracle as I
from tests import hints_oracle as H

M64 = (1 << 64) - 1
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "hints_kats.json")


def load_kats():
    with open(GOLDEN) as f:
        return json.load(f)


def kat_constants():
    """Every number of the reference tables: inputs, keys, values, results."""
    k = load_kats()["tests"]
    vals = set()
    for name in ("TestHintsCheckConstArg", "TestHintsShrinkExpand"):
        for c in k[name]:
            vals.add(int(c["in"], 0))
            vals.update(int(x, 0) for x in c["res"])
    for cases in k.values():
        for c in cases:
            for key, vs in c["comps"]:
                vals.add(int(key, 0))
                vals.update(int(v, 0) for v in vs)
    return sorted(vals)


def pool(rng):
    """About 90 operands: the KAT constants, the sign-boundary values, 40
    random u64 and 20 random values below 2^16."""
    p = list(kat_constants())
    for b in (0x80, 0x8000, 0x80000000):
        width = b.bit_length()
        p += [b, (b | ~((1 << width) - 1)) & M64]
    p += [0xFF, 0xFFFF, 0xFFFFFFFF, M64, 1 << 32, 4096, 0, 1, 2]
    p += [int(x) for x in rng.integers(0, 1 << 64, size=40, dtype=np.uint64)]
    p += [int(x) for x in rng.integers(0, 1 << 16, size=20, dtype=np.uint64)]
    return p


def comparisons(rng, p, n, types=None):
    """n comparisons (type, op1, op2) over the pool; types: a list to cycle."""
    out = []
    for j in range(n):
        typ = int(types[j % len(types)]) if types else int(rng.integers(0, 8))
        a1 = p[int(rng.integers(0, len(p)))]
        a2 = a1 if rng.integers(0, 8) == 0 else p[int(rng.integers(0, len(p)))]
        out.append((typ, a1, a2))
    return out


def assemble(programs):
    """programs: a list of (region words, ncalls, call_nums) -> the batch arrays."""
    out_off = np.concatenate([[0], np.cumsum([len(r) for r, _, _ in programs])]).astype(np.uint64)
    call_off = np.concatenate([[0], np.cumsum([n for _, n, _ in programs])]).astype(np.uint64)
    out = np.array([w for r, _, _ in programs for w in r], dtype=np.uint64).astype(np.uint32)
    nums = np.concatenate([np.asarray(c, np.uint32) for _, _, c in programs] + [np.zeros(0, np.uint32)])
    return out, out_off, call_off, nums.astype(np.uint32)


def batch(seed, nprog=60, maxcalls=6, maxcomps=200, maxvals=12):
    """A comps-mode batch: (out, out_off, call_off, call_nums, vals, val_off);
    every program parses (status OK).  Some calls do not execute, some have no
    comparisons, some no values."""
    rng = np.random.default_rng(seed)
    p = pool(rng)
    programs, vals, nvals = [], [], []
    for _ in range(nprog):
        ncalls = int(rng.integers(0, maxcalls + 1))
        nums = rng.integers(0, 4000, size=ncalls).astype(np.uint32)
        order = [int(c) for c in rng.permutation(ncalls) if rng.integers(0, 10) != 0]
        words = [len(order)]
        for ci in order:
            sig = rng.integers(0, 1 << 32, size=int(rng.integers(0, 20)), dtype=np.uint64)
            cov = rng.integers(0x81000000, 0x82000000, size=int(rng.integers(0, 10)), dtype=np.uint64)
            ncomps = 0 if rng.integers(0, 6) == 0 else int(rng.integers(1, maxcomps + 1))
            words += I.write_call(ci, int(nums[ci]), 0, 0, sig, cov, comparisons(rng, p, ncomps), "reader")
        programs.append((words, ncalls, nums))
        for _ in range(ncalls):
            nv = 0 if rng.integers(0, 6) == 0 else int(rng.integers(1, maxvals + 1))
            vals += [p[int(rng.integers(0, len(p)))] for _ in range(nv)]
            nvals.append(nv)
    val_off = np.concatenate([[0], np.cumsum(nvals)]).astype(np.uint64)
    return assemble(programs) + (np.array(vals, dtype=np.uint64), val_off)


def expected_replacers(pair_lists, vals, val_off):
    """The oracle over a batch: per value slot its replacers ascending, and
    the number of candidates: the (slot, AddComp call) matches before any
    deduplication, repeated pairs counted as often as they were added."""
    reps, cands = [], [0]
    for r, added in enumerate(pair_lists):
        m = H.comp_map(added)
        times = collections.Counter(added)

        def on_match(mutant, new_v):
            cands[0] += times[(mutant, new_v)]

        for i in range(int(val_off[r]), int(val_off[r + 1])):
            reps.append(sorted(H.shrink_expand(int(vals[i]), m, on_match)))
    return reps, cands[0]


def pairs_csr(pair_lists):
    """Per-record AddComp lists -> (pairs[n, 2], pair_off)."""
    off = np.concatenate([[0], np.cumsum([len(x) for x in pair_lists])]).astype(np.uint64)
    flat = [kv for x in pair_lists for kv in x]
    return np.array(flat, dtype=np.uint64).reshape(len(flat), 2), off
