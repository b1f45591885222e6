#!/usr/bin/env python3
"""Rate of the fused hint-seed call, sg_hints_from_kcov_dev, on comps-mode KCOV
buffers of the size a fuzzer produces: 4,096 programs x 8 calls x 2,048 records
{type, arg1, arg2, pc} with 16 argument values per call drawn from the hint
tests' pool (tests/hints_cases.py pool), built on the device.  Two inputs, one
JSON line each, as exec_comps_rate.py builds them:
  pool  types 0..7, operands drawn from the same pool;
  loop  every call draws its records from 64 triples of its own (an ASSUMPTION
        about real buffers, not a measurement of them).
After a warm-up, timed repetitions alternate the fused call with, on the same
input, the three separate device calls (sg_exec_comps_dev without words,
sg_comps_pairs_dev, sg_hints_replacers_dev): the mean device time of each whole
route (HIP events around it, kernel timing off).  Then, in passes of their own,
each route's kernels (sg_ctx_kernel_time: exec_comps_call, exec_comps_emit,
comps_pairs, hints_join, hints_sort).  The two routes' outputs are compared.  comps_pairs_over_emit is
the pairs kernels' time over exec_comps_emit's on the same triples (emit
without the words here: 24 B read and 24 B written per comparison; the pairs
kernels read 24 B twice and write at most 32 B)."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from scripts.exp.exec_comps_rate import build  # noqa: E402
from syzkaller_amd._lib import call  # noqa: E402
from syzkaller_amd.cover import Context  # noqa: E402
from tests.hints_cases import pool  # noqa: E402

NAMES = ("exec_comps_call", "exec_comps_emit", "comps_pairs", "hints_join", "hints_sort")


def route_times(ctx, fns, n):
    """Mean ms between HIP events around each of fns, n runs each, the routes
    alternated, kernel timing off."""
    ev = [[(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(n)] for _ in fns]
    for i in range(n):
        for fn, e in zip(fns, ev):
            e[i][0].record()
            fn()
            e[i][1].record()
    ctx.sync()
    torch.cuda.synchronize()
    return [round(sum(a.elapsed_time(b) for a, b in e) / n, 4) for e in ev]


def kernel_times(ctx, fn, n):
    """Mean ms per kernel name over n runs of fn (sg_ctx_kernel_time), in a pass of its own."""
    ctx.timing(True)
    base = {k: ctx.kernel_time(k)[0] for k in NAMES}
    for _ in range(n):
        fn()
    ctx.sync()
    ms = {k: round((ctx.kernel_time(k)[0] - base[k]) / n, 4) for k in NAMES}
    ctx.timing(False)
    return ms


def run(ctx, kind, P, C, M, V, warmup, reps):
    ncall, nrecs, nvals = P * C, P * C * M, P * C * V
    dev = "cuda"
    recs = build(kind, ncall, M, 1)
    g = torch.Generator(device=dev)
    g.manual_seed(2)
    pl = torch.from_numpy(np.array(pool(np.random.default_rng(1)), dtype=np.uint64).view(np.int64)).to(dev)
    vals = pl[torch.randint(0, pl.numel(), (nvals,), device=dev, generator=g)].contiguous()
    call_off = torch.arange(ncall + 1, device=dev, dtype=torch.int64) * M
    val_off = torch.arange(ncall + 1, device=dev, dtype=torch.int64) * V
    rcap = 128 * nvals
    out = {}
    for route in ("fused", "separate"):
        out[route] = (torch.empty(ncall, dtype=torch.int32, device=dev),
                      torch.empty(nvals + 1, dtype=torch.int64, device=dev),
                      torch.empty(rcap, dtype=torch.int64, device=dev))
    comp_off = torch.empty(ncall + 1, dtype=torch.int64, device=dev)
    comps = torch.empty(3 * nrecs, dtype=torch.int64, device=dev)
    pair_off = torch.empty(ncall + 1, dtype=torch.int64, device=dev)
    pairs = torch.empty(4 * nrecs, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()

    def fused():
        st, ro, rp = out["fused"]
        call("sg_hints_from_kcov_dev", ctx.h, recs.data_ptr(), call_off.data_ptr(), ncall, nrecs, val_off.data_ptr(),
             vals.data_ptr(), nvals, st.data_ptr(), ro.data_ptr(), rp.data_ptr(), rcap)

    def separate():
        st, ro, rp = out["separate"]
        call("sg_exec_comps_dev", ctx.h, recs.data_ptr(), call_off.data_ptr(), ncall, nrecs, comp_off.data_ptr(),
             comps.data_ptr(), nrecs, None, None, 0)
        call("sg_comps_pairs_dev", ctx.h, comp_off.data_ptr(), comps.data_ptr(), ncall, nrecs, st.data_ptr(),
             pair_off.data_ptr(), pairs.data_ptr(), 2 * nrecs)
        call("sg_hints_replacers_dev", ctx.h, pair_off.data_ptr(), pairs.data_ptr(), ncall, val_off.data_ptr(),
             vals.data_ptr(), nvals, ro.data_ptr(), rp.data_ptr(), rcap)

    for _ in range(warmup):
        fused()
        separate()
    ctx.sync()
    ncomps, npairs = int(comp_off[-1]), int(pair_off[-1])
    nreps = int(out["fused"][1][-1])
    assert nreps <= rcap and npairs <= 2 * nrecs
    (f_st, f_ro, f_rp), (s_st, s_ro, s_rp) = out["fused"], out["separate"]
    assert torch.equal(f_st, s_st) and torch.equal(f_ro, s_ro) and torch.equal(f_rp[:nreps], s_rp[:nreps]), \
        "the two routes disagree"
    assert bool((f_st == 0).all())
    res = {"metric": "hint_seed_rate", "input": kind, "programs": P, "calls": C, "records_per_call": M,
           "vals_per_call": V, "reps": reps, "records": nrecs, "comparisons": ncomps, "pairs": npairs,
           "value_slots": nvals, "replacers": nreps}
    res["candidates"] = ctx.counter("hints_candidates")
    f_ms, s_ms = route_times(ctx, (fused, separate), reps)
    f_k, s_k = kernel_times(ctx, fused, reps), kernel_times(ctx, separate, reps)
    res["fused"] = {"call_ms": f_ms, "kernel_ms": f_k}
    res["separate"] = {"call_ms": s_ms, "kernel_ms": s_k}
    res["fused_over_separate"] = round(f_ms / s_ms, 4) if s_ms > 0 else None
    emit = s_k["exec_comps_emit"]
    res["comps_pairs_over_emit"] = round(s_k["comps_pairs"] / emit, 3) if emit > 0 else None
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--programs", type=int, default=4096)
    ap.add_argument("--calls", type=int, default=8)
    ap.add_argument("--records", type=int, default=2048)
    ap.add_argument("--vals", type=int, default=16)
    ap.add_argument("--inputs", default="pool,loop")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=10)
    a = ap.parse_args()
    torch.cuda.set_device(0)
    ctx = Context(0)
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    for kind in a.inputs.split(","):
        run(ctx, kind, a.programs, a.calls, a.records, a.vals, a.warmup, a.reps)


if __name__ == "__main__":
    main()
