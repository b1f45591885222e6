#!/usr/bin/env python3
"""Rate of the call priorities, sg_call_prios_from_progs and its parts, at the
size of the reference's amd64 target: 1,541 calls, 500k programs of 1 to 30
calls (uniform), call ids Zipf(1.2) over the calls through a fixed random
permutation, so the hot calls are scattered over the id range as in a real
target; mmap is the hottest call (that this resembles a corpus is an
ASSUMPTION, not a measurement of one).  A random static matrix, a tenth of the
calls disabled.  One JSON line.  After a warm-up, timed repetitions of the legs
on the same input, each timed by a host clock from the call to its return
(every leg ends with its results on the host; call_ms is the median of the
repetitions, call_ms_min_max their range):
  from_progs  sg_call_prios_from_progs: ids and offsets in, the three matrices out
  add         sg_prio_table_clear + sg_prio_table_add (ids and offsets in)
  finish      sg_call_prios on the resident counts (the three matrices out)
  baseline    the TEST ORACLE's closed form (tests/call_prios_oracle.py: exact
              counts n_i * n_j, min(count, 2^24), normalizePrio row by row, the
              static multiply and the masked running sums) in numpy on the
              CPU, with the counts as float32 matrix products over chunks of
              programs small enough to stay exact.  It is numpy, not Go: the
              reference's own triple loop was not run.
The GPU results are compared with the baseline's, bit for bit.  Then, in a pass
of its own, the kernels (sg_ctx_kernel_time): k_prio_merge, k_prio_band and
k_prio_long of the add, and k_prio_finish."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from syzkaller_amd import cover as C  # noqa: E402
from syzkaller_amd import prio as P  # noqa: E402
from tests import call_prios_oracle as OR  # noqa: E402

U8, U32, U64, F32 = np.uint8, np.uint32, np.uint64, np.float32
CHUNK = 8192  # programs per matrix product: a cell gains at most 8192 * 15 * 15 < 2^24, exact in float32


def corpus(nprogs, ncalls, maxlen, s, rng):
    lens = rng.integers(1, maxlen + 1, size=nprogs)
    off = np.zeros(nprogs + 1, U64)
    off[1:] = np.cumsum(lens)
    perm = rng.permutation(ncalls)
    ranks = (rng.zipf(s, size=int(off[-1])) - 1) % ncalls
    return perm[ranks].astype(U32), off, int(perm[0])


def baseline_counts(ids, off, ncalls, mmap_id):
    """The oracle's counts for a large corpus: per chunk of programs the matrix N[p][i] = n_p(i), and N^T N."""
    off = off.astype(np.int64)
    nprogs = off.size - 1
    prog = np.repeat(np.arange(nprogs, dtype=np.int64), np.diff(off))
    cnt = np.zeros((ncalls, ncalls), np.int64)
    for p0 in range(0, nprogs, CHUNK):
        p1 = min(p0 + CHUNK, nprogs)
        a, b = off[p0], off[p1]
        n = np.bincount((prog[a:b] - p0) * ncalls + ids[a:b].astype(np.int64), minlength=(p1 - p0) * ncalls)
        n = n.reshape(p1 - p0, ncalls).astype(F32)
        part = n.T @ n
        assert part.max() < (1 << 24)
        cnt += part.astype(np.int64)
    cnt[np.arange(ncalls), np.arange(ncalls)] = 0
    if mmap_id != OR.NO_CALL:
        cnt[mmap_id, :] = 0
        cnt[:, mmap_id] = 0
    return cnt.astype(U64)


def wall(fn, n):
    ms = []
    for _ in range(n):
        t0 = time.perf_counter()
        fn()
        ms.append((time.perf_counter() - t0) * 1e3)
    return round(float(np.median(ms)), 3), [round(min(ms), 3), round(max(ms), 3)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=1541)
    ap.add_argument("--programs", type=int, default=500000)
    ap.add_argument("--max-len", type=int, default=30)
    ap.add_argument("--zipf", type=float, default=1.2)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--baseline-reps", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "call_prios_rate.jsonl"))
    a = ap.parse_args()
    ctx = C.Context(0)
    rng = np.random.default_rng(7)
    ids, off, mmap_id = corpus(a.programs, a.calls, a.max_len, a.zipf, rng)
    static = (rng.integers(0, 1001, size=(a.calls, a.calls)).astype(F32) / F32(1000)).astype(F32)
    enabled = (rng.random(a.calls) < 0.9).astype(U8)
    table = P.PrioTable(static, mmap_id, enabled, ctx=ctx)
    got, base = {}, {}

    def from_progs():
        got["fused"] = table.from_progs(csr=(ids, off))

    def add():
        table.clear()
        table.add(csr=(ids, off))

    def finish():
        got["parts"] = table.prios()

    def baseline():
        cnt = baseline_counts(ids, off, a.calls, mmap_id)
        dyn = OR.normalize(OR.cells(cnt))
        pr = (dyn * static).astype(F32)
        base["all"] = (cnt, dyn, pr, OR.run_sums(pr, enabled))

    for fn in (from_progs, add, finish):
        wall(fn, a.warmup)
    b_ms, b_spread = wall(baseline, a.baseline_reps)
    cnt, dyn, pr, run = base["all"]
    assert np.array_equal(table.counts(), cnt), "counts disagree with the oracle"
    for k in ("fused", "parts"):
        for x, y, what in zip(got[k], (dyn, pr, run), ("dynamic", "prios", "run")):
            assert np.array_equal(x.view(U32), y.view(U32)), f"{k}: {what} disagrees with the oracle"
    w, spread = {}, {}
    for name, fn in (("from_progs", from_progs), ("add", add), ("finish", finish)):
        w[name], spread[name] = wall(fn, a.reps)
    w["baseline"], spread["baseline"] = b_ms, b_spread
    ctx.timing(True)
    names = ("prio_merge", "prio_band", "prio_long", "prio_finish")
    t0 = {k: ctx.kernel_time(k)[0] for k in names}
    for _ in range(a.reps):
        from_progs()
    ctx.sync()
    kern = {k: round((ctx.kernel_time(k)[0] - t0[k]) / a.reps, 4) for k in names}
    ctx.timing(False)
    pairs = int(cnt.sum())
    res = {"metric": "call_prios_rate", "calls": a.calls, "programs": a.programs, "ids": int(off[-1]), "zipf": a.zipf,
           "pair_increments": pairs, "nonzero_cells": int((cnt != 0).sum()), "max_cell": int(cnt.max()),
           "cells_above_2_24": int((cnt > (1 << 24)).sum()), "reps": a.reps, "baseline_reps": a.baseline_reps,
           "baseline": "tests/call_prios_oracle.py closed form, numpy on the CPU (not Go)",
           "call_ms": w, "call_ms_min_max": spread, "kernel_ms": kern,
           "from_progs_over_baseline": round(w["from_progs"] / w["baseline"], 5),
           "pair_increments_per_s_kernel": round(pairs / ((kern["prio_merge"] + kern["prio_band"] + kern["prio_long"]) * 1e-3))}
    print(json.dumps(res), flush=True)
    table.close()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(json.dumps(res) + "\n")


if __name__ == "__main__":
    main()
