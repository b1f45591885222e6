#!/usr/bin/env python3
"""Rate of db.compact() on the GPU: sg_db_compact of an opened database of --programs synthetic programs against the
reference's work restated, one thread of C zlib over the same records in Go's framing (serializeRecord's loop,
pkg/db/db.go:137-165), at level 9 (flate.BestCompression, what pkg/db asks for) and at level 1 (the cheapest
setting a Go user could choose) -- C zlib, a harder baseline than Go's compress/flate.  The texts and their size
distribution are scripts/exp/db_open_rate.py's (lognormal, median --median bytes, sigma --sigma, clipped to [16 B,
64 KiB]): an ASSUMPTION, the reference publishes no corpus.  One JSON line, also written to
profiles/db_compact_rate.jsonl.

  compact_ms        sg_db_compact from call to return (host clock; the call ends in a wait), median of --reps after
                    --warmup
  kernel_ms         per kernel through sg_ctx_kernel_time, in a pass of its own (timing slows the host)
  not_kernel_ms     compact_ms - the kernels: the keys' upload, the two waits, the download of the file
  download_ms       a device-to-host copy of the file's size alone
  baseline9_ms, baseline1_ms   the zlib loops (median of --base-reps), with the bytes of their streams
  forms             the call's streams per form, from the context's counters
The compacted file is opened again and every text compared."""
import argparse
import hashlib
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import numpy as np  # noqa: E402

from hub_state_rate import make_corpus, make_names, wall  # noqa: E402
from syzkaller_amd import _lib  # noqa: E402
from syzkaller_amd import cover as C  # noqa: E402
from syzkaller_amd import db as D  # noqa: E402
from syzkaller_amd.cover import _p8  # noqa: E402
from tests import db_cases as K  # noqa: E402

U8 = np.uint8
KERNELS = ("deflate_keys", "deflate_sort", "scan", "deflate_count", "deflate_long", "deflate_write", "db_frames")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--programs", type=int, default=500000)
    ap.add_argument("--median", type=float, default=512.0)
    ap.add_argument("--sigma", type=float, default=1.0)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--base-reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "db_compact_rate.jsonl"))
    a = ap.parse_args()
    reps = max(a.reps, 5)  # (the issue's floor: a median of at least 5)
    import torch

    ctx = C.Context(0)
    n = a.programs
    progs = make_corpus(n, make_names(), a.median, a.sigma, 7)
    keys = [hashlib.sha1(p).hexdigest().encode() for p in progs]
    text_bytes = sum(len(p) for p in progs)

    # ---- the baselines: serializeRecord's loop, one thread of C zlib ----
    def loop(level):
        ms, streams = [], None
        for _ in range(a.base_reps):
            t0 = time.perf_counter()
            streams = [K.go_stream(p, level) for p in progs]
            ms.append((time.perf_counter() - t0) * 1e3)
        return ms, streams

    base1, streams1 = loop(1)
    bytes1 = sum(map(len, streams1))
    del streams1
    base9, streams9 = loop(9)
    bytes9 = sum(map(len, streams9))
    data = K.db_header() + b"".join(K.db_record(keys[k], None, 1 + k // 1000, stream=streams9[k]) for k in range(n))
    del streams9
    frame_bytes = len(data) - bytes9

    # ---- sg_db_compact of the opened database ----
    db = D.DB(data, ctx)
    assert len(db) == n and db.end == 0
    cap = 8 + 29 * n + db.key_bytes + db.text_bytes + 5 * (db.text_bytes // 65535 + 1)
    out = np.empty(cap, U8)
    nout = _lib.c_size_t()

    def compact():
        _lib.call("sg_db_compact", db.h, _p8(out), cap, _lib.ctypes.byref(nout))

    wall(compact, a.warmup)
    forms = {f: ctx.counter("deflate_%s_streams" % f) for f in ("stored", "fixed", "dynamic")}
    assert sum(forms.values()) == n
    file_bytes = nout.value
    compacted = out[:file_bytes].tobytes()
    compact_ms, compact_spread = wall(compact, reps)
    assert out[:nout.value].tobytes() == compacted, "sg_db_compact is not deterministic"
    db.close()
    again = D.DB(compacted, ctx)
    k2, s2, t2 = again.export()
    assert t2 == progs and k2 == keys and again.uncompacted == n and again.end == 0, "the compacted file reads back wrong"
    again.close()

    src = torch.empty(file_bytes, dtype=torch.uint8, device="cuda")
    dst = torch.empty(file_bytes, dtype=torch.uint8)

    def down():
        dst.copy_(src)
        torch.cuda.synchronize()

    wall(down, 2)
    download_ms, _ = wall(down, 5)

    # ---- the kernels, timed by events in a pass of their own ----
    db = D.DB(data, ctx)
    ctx.timing(True)
    ctx.sync()
    k0 = {k: ctx.kernel_time(k)[0] for k in KERNELS}
    for _ in range(reps):
        compact()
    kern = {k: round((ctx.kernel_time(k)[0] - k0[k]) / reps, 4) for k in KERNELS}
    ctx.timing(False)
    db.close()
    ksum = sum(kern.values())  # (the sort's own scans are in "scan" and in "deflate_sort": db_open_rate.py's convention)
    b9, b1 = float(np.median(base9)), float(np.median(base1))
    res = {"metric": "db_compact_rate", "programs": n, "text_bytes": text_bytes, "length_median_assumed": a.median,
           "length_sigma": a.sigma, "reps": reps, "base_reps": a.base_reps,
           "baseline": "zlib.compressobj(level, DEFLATED, -15) per record in Go's framing, one CPU thread, C zlib",
           "compact_ms": compact_ms, "compact_ms_min_max": compact_spread,
           "baseline9_ms": round(b9, 1), "baseline9_ms_min_max": [round(min(base9), 1), round(max(base9), 1)],
           "baseline1_ms": round(b1, 1), "baseline1_ms_min_max": [round(min(base1), 1), round(max(base1), 1)],
           "compact_over_baseline9": round(compact_ms / b9, 5), "compact_over_baseline1": round(compact_ms / b1, 5),
           "kernel_ms": kern, "kernels_ms": round(ksum, 3), "not_kernel_ms": round(compact_ms - ksum, 3),
           "not_kernel_share": round((compact_ms - ksum) / compact_ms, 4), "download_ms": download_ms,
           "file_bytes": file_bytes, "frame_bytes": frame_bytes, "stream_bytes": file_bytes - frame_bytes,
           "stream_bytes_level9": bytes9, "stream_bytes_level1": bytes1,
           "streams_over_level9": round((file_bytes - frame_bytes) / bytes9, 4),
           "streams_over_level1": round((file_bytes - frame_bytes) / bytes1, 4), "forms": forms,
           "long_streams": ctx.counter("deflate_long_streams")}
    print(json.dumps(res), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(json.dumps(res) + "\n")


if __name__ == "__main__":
    main()
