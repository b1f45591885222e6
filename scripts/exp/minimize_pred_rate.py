#!/usr/bin/env python3
"""Rate of the fused minimisation predicate, sg_minimize_pred_from_kcov_dev, on
a batch of the size -procs Minimize runs produce together: 4,096 attempts, each
the execution of a shortened program of 16 calls x 1,024 PCs
(sg_gen_zipf_traces_dev, Zipf 1.1 over 2^20 ranks, widened to u64 with the high
word 0xffffffff; that Zipf traces resemble real buffers is an ASSUMPTION, not a
measurement of them), call1 uniform.  Attempt e tests a list of its own: 1..32
values of call1's executor list as sg_exec_signal_dev gives it, one value in
eight replaced by a value the call lacks, so that a share of the attempts is
LOST.  One JSON line.  After a warm-up, timed repetitions alternate four legs on
the same input, each timed by a host clock from the call to the end of a stream
synchronise:
  fused            the device call without sets
  fused_sets       the device call with maxSignal and newSignal
  chain            the entry points the library had before: truncate (torch),
                   sg_exec_signal_dev on every call, the lists to the host,
                   the host form of sg_triage_subset on the selected calls'
                   lists, the not-executed rule in numpy
  chain_sets       sg_triage_traces_dev, then the chain
The sets are cleared before each timed call of the two legs that use them,
outside the timed window.  Then, in a pass of its own, the kernels of the fused
call (sg_ctx_kernel_time: minimize_pred is the predicate, exec_signal and
exec_compact the executor).  All legs' statuses are compared."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from syzkaller_amd import cover as C  # noqa: E402
from syzkaller_amd._lib import call  # noqa: E402

UNIVERSE_SEED = 1
NAMES = ("minimize_pred", "exec_signal", "exec_compact")


def wall_times(ctx, legs, n):
    """Mean ms per leg over n runs, the legs alternated and their order rotated from run to run (the leg after
    the host-bound chain meets an idle, down-clocked GPU): legs are (prep, fn), prep outside the window."""
    ms = [0.0] * len(legs)
    for i in range(n):
        for k in [(i + j) % len(legs) for j in range(len(legs))]:
            prep, fn = legs[k]
            if prep:
                prep()
            ctx.sync()
            t0 = time.perf_counter()
            fn()
            ctx.sync()
            ms[k] += (time.perf_counter() - t0) * 1e3
    return [round(x / n, 4) for x in ms]


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


def run(ctx, N, CALLS, M, warmup, reps):
    dev = "cuda"
    ncalls, npcs = N * CALLS, N * CALLS * M
    lo = torch.empty(npcs, dtype=torch.int32, device=dev)
    call("sg_gen_zipf_traces_dev", ctx.h, UNIVERSE_SEED, 7, 1.1, 1 << 20, 0, N, CALLS, M, lo.data_ptr())
    ctx.sync()
    pcs = (lo.to(torch.int64) & 0xFFFFFFFF) | (-1 << 32)
    del lo
    call_off = torch.arange(ncalls + 1, device=dev, dtype=torch.int64) * M
    prog_off = torch.arange(N + 1, device=dev, dtype=torch.int64) * CALLS
    rng = np.random.default_rng(3)
    call1 = rng.integers(0, CALLS, size=N).astype(np.uint32)
    sel = np.arange(N, dtype=np.int64) * CALLS + call1
    d_call = torch.from_numpy(call1.view(np.int32)).to(dev)
    d_cand = torch.arange(N, device=dev, dtype=torch.int32)
    pcs32 = torch.empty(npcs, dtype=torch.int32, device=dev)
    xsig = torch.empty(npcs, dtype=torch.int32, device=dev)
    xoff = torch.empty(ncalls + 1, dtype=torch.int64, device=dev)
    flags = torch.empty(ncalls, dtype=torch.uint8, device=dev)
    host = {}

    def chain():
        pcs32.copy_(pcs)  # (uint32_t)pc: the low word
        call("sg_exec_signal_dev", ctx.h, pcs32.data_ptr(), call_off.data_ptr(), prog_off.data_ptr(), N, ncalls, npcs,
             xsig.data_ptr(), xoff.data_ptr())
        off = xoff.cpu().numpy().view(np.uint64)
        vals = xsig[: int(off[-1])].cpu().numpy().view(np.uint32)
        lens = (off[sel + 1] - off[sel]).astype(np.uint64)
        r_off = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
        r_vals = np.concatenate([vals[int(off[c]):int(off[c + 1])] for c in sel])
        host["lists"], host["bytes"] = (r_vals, r_off), int(off.nbytes + vals.nbytes)
        if "new" in host:
            ok = C.triage_subset(host["new"][0], host["new"][1], r_vals, r_off, ctx=ctx)
            host["status"] = np.where(lens == 0, 1, np.where(ok != 0, 0, 2)).astype(np.int32)

    chain()
    r_vals, r_off = host["lists"]
    news = []
    for e in range(N):
        have = np.unique(r_vals[int(r_off[e]):int(r_off[e + 1])])
        take = rng.choice(have, size=min(int(rng.integers(1, 33)), have.size), replace=False)
        swap = rng.integers(0, 8, size=take.size) == 0
        take = np.where(swap, take ^ np.uint32(1), take)  # a neighbour: a PC 16 bytes on hashes elsewhere
        news.append(np.unique(take[take != 0xFFFFFFFF]))
    new_vals, new_off = C.to_csr(news)
    host["new"] = (new_vals, new_off)
    nnew = int(new_off[-1])
    d_nv = torch.from_numpy(new_vals.view(np.int32)).to(dev)
    d_no = torch.from_numpy(new_off.view(np.int64)).to(dev)
    ms, ns = C.SignalSet(ctx), C.SignalSet(ctx)
    cms, cns = C.SignalSet(ctx), C.SignalSet(ctx)
    out = {k: torch.empty(N, dtype=torch.int32, device=dev) for k in ("fused", "fused_sets")}
    rec_new = torch.empty(ncalls, dtype=torch.uint8, device=dev)
    sig_off = torch.empty(ncalls + 1, dtype=torch.int64, device=dev)
    sig_vals = torch.empty(npcs, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()

    def fused(key, sets):
        def fn():
            call("sg_minimize_pred_from_kcov_dev", ctx.h, ms.h if sets else None, ns.h if sets else None, d_nv.data_ptr(),
                 d_no.data_ptr(), N, nnew, d_cand.data_ptr(), d_call.data_ptr(), N, pcs.data_ptr(), call_off.data_ptr(),
                 prog_off.data_ptr(), ncalls, npcs, out[key].data_ptr(), rec_new.data_ptr() if sets else None,
                 sig_off.data_ptr() if sets else None, sig_vals.data_ptr() if sets else None, npcs if sets else 0)
        return fn

    def chain_sets():
        pcs32.copy_(pcs)
        call("sg_triage_traces_dev", ctx.h, cms.h, cns.h, pcs32.data_ptr(), call_off.data_ptr(), npcs, ncalls,
             flags.data_ptr())
        chain()

    def clear(*sets):
        return lambda: [s.clear() for s in sets]

    legs = [(None, fused("fused", False)), (clear(ms, ns), fused("fused_sets", True)), (None, chain),
            (clear(cms, cns), chain_sets)]
    names = ("fused", "fused_sets", "chain", "chain_sets")
    wall_times(ctx, legs, warmup)
    status = host["status"]
    for key, t in out.items():
        assert np.array_equal(t.cpu().numpy(), status), key + " disagrees with the chain"
    assert torch.equal(rec_new, flags) and np.array_equal(ms.export(), cms.export()), "set updates disagree"
    res = {"metric": "minimize_pred_rate", "attempts": N, "calls": CALLS, "pcs_per_call": M, "pcs": npcs, "reps": reps,
           "list_values": nnew, "signals_of_selected_calls": int(r_off[-1]), "chain_download_bytes": host["bytes"],
           "status_counts": np.bincount(status, minlength=3).tolist()}
    res["call_ms"] = dict(zip(names, wall_times(ctx, legs, reps)))
    res["kernel_ms"] = kernel_times(ctx, legs[0][1], reps)
    w = res["call_ms"]
    res["fused_over_chain"] = round(w["fused"] / w["chain"], 4)
    res["fused_sets_over_chain_sets"] = round(w["fused_sets"] / w["chain_sets"], 4)
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--attempts", type=int, default=4096)
    ap.add_argument("--calls", type=int, default=16)
    ap.add_argument("--pcs", type=int, default=1024)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=10)
    a = ap.parse_args()
    torch.cuda.set_device(0)
    ctx = C.Context(0)
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    run(ctx, a.attempts, a.calls, a.pcs, a.warmup, a.reps)


if __name__ == "__main__":
    main()
