#!/usr/bin/env python3
"""C2 triage steps on the default regime (bench.py's generator, starting
maxSignal and triage call), one at a time with a sync after each, and the
split bucket stage's counters after every step as one JSON line: was the launch
split, the summary's full blocks, did the second phase run map-free
(flag_skip_all_flagged), the records queued.  argv[1]: steps (default 8)."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import bench  # noqa: E402
from bench import call  # noqa: E402
from syzkaller_amd.cover import Context, SignalSet  # noqa: E402


def main():
    steps = int(sys.argv[1]) if len(sys.argv) > 1 else 8
    cfg = {"programs": 65536, "calls": 16, "pcs_per_call": 1024, "zipf_s": 1.1, "ranks": 1 << 20}
    torch.cuda.set_device(0)
    ctx = Context(0)
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    g = bench.Gen(cfg)
    warm = g.zipf(ctx, cfg, 2_000_000)
    batches = [g.zipf(ctx, cfg, 1_000 + k) for k in range(steps)]
    rec_new = torch.empty(max(b.nrec for b in batches), dtype=torch.uint8, device="cuda")
    maxsig, newsig, m0set = SignalSet(ctx), SignalSet(ctx), SignalSet(ctx)
    bench.build_m0(ctx, m0set, warm, cfg["calls"], 16 << 20, rec_new)
    del warm
    for k, b in enumerate(batches):
        call("sg_set_copy", maxsig.h, m0set.h)
        u0, a0 = ctx.counter("flag_skip_used"), ctx.counter("flag_skip_all_flagged")
        bench.triage(ctx, maxsig, newsig, b, rec_new)
        torch.cuda.synchronize()
        print(json.dumps({"step": k, "nrec": b.nrec, "blocks": -(-b.nrec // 4096),
                          "split": ctx.counter("flag_skip_used") - u0,
                          "full_blocks": ctx.counter("flag_skip_full_blocks"),
                          "all_flagged": ctx.counter("flag_skip_all_flagged") - a0,
                          "queued": int(rec_new[: b.nrec].sum().item())}), flush=True)


if __name__ == "__main__":
    main()
