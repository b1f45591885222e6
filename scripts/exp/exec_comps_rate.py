#!/usr/bin/env python3
"""Rate of sg_exec_comps_dev on comps-mode KCOV buffers of the size a fuzzer
produces: 4,096 programs x 8 calls x 2,048 records {type, arg1, arg2, pc},
built on the device.  Three inputs, one JSON line each:
  pool      types 0..7, operands drawn from the hint tests' pool
            (tests/hints_cases.py pool, about 90 values), as hints_rate.py;
  loop      every call draws its records from 64 triples of its own: the
            repeats a loop's comparisons leave (an ASSUMPTION about real
            buffers, not a measurement of them);
  distinct  every record of a call distinct.
Each line states the repeat ratio 1 - comparisons / records that its input
has.  After a warm-up, timed repetitions run the auto path (every call on the
fast shapes here) and then, on the same input, the general path for every call
(option exec_comps_path = 0).  Per path: the mean device time of the whole call
(HIP events around it) and of its kernels (sg_ctx_kernel_time: exec_comps_call,
exec_comps_general, exec_comps_emit), the algorithmic bytes (32 B per record
in, 24 B per triple and 4 B per word out) and the fraction of the 8 TB/s HBM
peak they make over the whole call."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from syzkaller_amd._lib import call  # noqa: E402
from syzkaller_amd.cover import Context  # noqa: E402
from tests.hints_cases import pool  # noqa: E402

HBM_PEAK = 8.0e12
NAMES = ("exec_comps_call", "exec_comps_general", "exec_comps_emit")
PC0 = -0x7F000000  # 0xFFFFFFFF81000000 as int64


def build(kind, ncall, M, seed):
    dev = "cuda"
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    recs = torch.empty((ncall, M, 4), dtype=torch.int64, device=dev)
    if kind == "pool":
        pl = torch.from_numpy(np.array(pool(np.random.default_rng(seed)), dtype=np.uint64).view(np.int64)).to(dev)
        recs[:, :, 0] = torch.randint(0, 8, (ncall, M), device=dev, generator=g)
        recs[:, :, 1] = pl[torch.randint(0, pl.numel(), (ncall, M), device=dev, generator=g)]
        recs[:, :, 2] = pl[torch.randint(0, pl.numel(), (ncall, M), device=dev, generator=g)]
    elif kind == "loop":
        K = 64
        trip = torch.randint(-(1 << 62), 1 << 62, (ncall, K, 3), device=dev, generator=g)
        trip[:, :, 0] = torch.randint(0, 8, (ncall, K), device=dev, generator=g)
        pick = torch.randint(0, K, (ncall, M), device=dev, generator=g)
        recs[:, :, :3] = torch.gather(trip, 1, pick[:, :, None].expand(ncall, M, 3))
    else:  # distinct: arg1 a permutation of 0 .. M - 1 per call, scattered over 64 bits by an odd multiplier
        perm = torch.argsort(torch.rand((ncall, M), device=dev, generator=g), dim=1)
        recs[:, :, 0] = torch.randint(0, 8, (ncall, M), device=dev, generator=g)
        recs[:, :, 1] = perm * -0x61C8864680B583EB
        recs[:, :, 2] = torch.randint(-(1 << 62), 1 << 62, (ncall, M), device=dev, generator=g)
    recs[:, :, 3] = PC0 + 4 * torch.randint(0, 1 << 12, (ncall, M), device=dev, generator=g)
    return recs.reshape(-1).contiguous()


def run(ctx, kind, P, C, M, warmup, reps, general_reps):
    ncall, nrecs = P * C, P * C * M
    dev = "cuda"
    recs = build(kind, ncall, M, 1)
    call_off = torch.arange(ncall + 1, device=dev, dtype=torch.int64) * M
    comp_off = torch.empty(ncall + 1, dtype=torch.int64, device=dev)
    word_off = torch.empty(ncall + 1, dtype=torch.int64, device=dev)
    comps = torch.empty(3 * nrecs, dtype=torch.int64, device=dev)
    words = torch.empty(5 * nrecs, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()

    def one():
        call("sg_exec_comps_dev", ctx.h, recs.data_ptr(), call_off.data_ptr(), ncall, nrecs, comp_off.data_ptr(),
             comps.data_ptr(), nrecs, word_off.data_ptr(), words.data_ptr(), 5 * nrecs)

    res = {"metric": "exec_comps_rate", "input": kind, "programs": P, "calls": C, "records_per_call": M,
           "records": nrecs}
    ref = None
    for path, n in ((-1, reps), (0, general_reps)):
        if n <= 0:
            continue
        ctx.set_option("exec_comps_path", path)
        for _ in range(warmup):
            one()
        ctx.sync()
        ncomps, nwords, general = int(comp_off[-1]), int(word_off[-1]), ctx.counter("exec_comps_general")
        sums = (int(comp_off.sum()), int(comps[: 3 * ncomps].sum()), int(word_off.sum()), int(words[:nwords].sum()))
        if ref is None:
            ref = sums
        assert sums == ref, "the two paths disagree"
        ctx.timing(True)
        base = {k: ctx.kernel_time(k)[0] for k in NAMES}
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(n)]
        for a, b in ev:
            a.record()
            one()
            b.record()
        ctx.sync()
        torch.cuda.synchronize()
        ms = {k: round((ctx.kernel_time(k)[0] - base[k]) / n, 4) for k in NAMES}
        ctx.timing(False)
        total = sum(a.elapsed_time(b) for a, b in ev) / n
        nbytes = 32 * nrecs + 24 * ncomps + 4 * nwords
        res.update({"comparisons": ncomps, "words": nwords, "repeat_ratio": round(1 - ncomps / nrecs, 4),
                    "algorithmic_bytes": nbytes})
        res["auto" if path < 0 else "general"] = {
            "reps": n, "calls_on_general_path": general, "call_ms": round(total, 4), "kernel_ms": ms,
            "hbm_fraction": round(nbytes / (total * 1e-3) / HBM_PEAK, 4)}
    ctx.set_option("exec_comps_path", -1)
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--programs", type=int, default=4096)
    ap.add_argument("--calls", type=int, default=8)
    ap.add_argument("--records", type=int, default=2048)
    ap.add_argument("--inputs", default="pool,loop,distinct")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--general-reps", type=int, default=3)
    a = ap.parse_args()
    torch.cuda.set_device(0)
    ctx = Context(0)
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    for kind in a.inputs.split(","):
        run(ctx, kind, a.programs, a.calls, a.records, a.warmup, a.reps, a.general_reps)


if __name__ == "__main__":
    main()
