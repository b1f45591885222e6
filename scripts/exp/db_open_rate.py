#!/usr/bin/env python3
"""Rate of db.Open on the GPU: sg_db_open of a database of --programs synthetic programs, each value compressed at
zlib level 9 in Go's framing (sync flush, then the final empty stored block), against a single-thread loop of
zlib.decompressobj(-15) over the same records -- C zlib, a harder baseline than Go's compress/flate.  The texts and
their size distribution are scripts/exp/hub_state_rate.py's (lognormal, median --median bytes, sigma --sigma, clipped
to [16 B, 64 KiB]): an ASSUMPTION, the reference publishes no corpus.  One JSON line, also written to
profiles/db_open_rate.jsonl.

  open_ms           sg_db_open from call to return (host clock; the call ends in a wait), median of --reps after
                    --warmup, the database destroyed outside the clock
  kernel_ms         per kernel through sg_ctx_kernel_time, in a pass of its own (timing slows the host)
  scan_ms           sg_db_scan alone: the host's framing pass
  upload_ms         the file's bytes host to device alone (a pageable copy of the same size)
  not_kernel_ms     open_ms - the kernels: the upload, the two waits with their read-backs, the host's scan and
                    key resolution
  verify_ms         sg_db_verify over the resident texts (loadDB's loop)
  baseline_ms       the zlib loop; baseline_scan_ms the Python framing before it (not counted)
Every text is compared with the baseline's."""
import argparse
import json
import os
import sys
import time
import zlib

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
from tests import db_oracle as OR  # noqa: E402

U8, U64 = np.uint8, np.uint64
KERNELS = ("inflate_keys", "inflate_sort", "scan", "inflate_count", "inflate_long", "inflate_write")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--programs", type=int, default=500000)
    ap.add_argument("--median", type=float, default=512.0)
    ap.add_argument("--sigma", type=float, default=1.0)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "db_open_rate.jsonl"))
    a = ap.parse_args()
    reps = max(a.reps, 5)  # (the issue's floor: a median of at least 5)
    import hashlib

    import torch

    ctx = C.Context(0)
    n = a.programs
    progs = make_corpus(n, make_names(), a.median, a.sigma, 7)
    t0 = time.perf_counter()
    data = K.db_header() + b"".join(K.db_record(hashlib.sha1(p).hexdigest().encode(), p, 1 + k // 1000)
                                    for k, p in enumerate(progs))
    build_s = time.perf_counter() - t0
    file = np.frombuffer(data, U8)
    text_bytes = sum(len(p) for p in progs)

    # ---- the baseline: framing in Python (not counted), then one thread of C zlib ----
    t0 = time.perf_counter()
    recs, end = OR.scan(data)
    base_scan_ms = (time.perf_counter() - t0) * 1e3
    assert end == 0 and len(recs) == n
    streams = [data[vp:vp + vl] for _, _, _, vp, vl in recs]
    base = []
    for _ in range(reps):
        t0 = time.perf_counter()
        texts = [zlib.decompressobj(-15).decompress(s) for s in streams]
        base.append((time.perf_counter() - t0) * 1e3)
    assert texts == progs
    base_ms = float(np.median(base))

    # ---- sg_db_open ----
    h = [None]

    def close():
        if h[0] is not None:
            _lib.lib.sg_db_destroy(h[0])
            h[0] = None

    def open_():
        hh = _lib.c_void_p()
        _lib.call("sg_db_open", ctx.h, _p8(file), file.size, _lib.ctypes.byref(hh))
        h[0] = hh

    wall(open_, a.warmup, close)
    close()
    db = D.DB(data, ctx)
    keys, seqs, got = db.export()
    assert got == progs and len(db) == n and db.uncompacted == n and db.end == 0, "sg_db_open disagrees with zlib"
    bad, max_seq = db.verify()
    assert not bad.any() and max_seq == 1 + (n - 1) // 1000, "sg_db_verify"
    verify_ms, verify_spread = wall(lambda: db.verify(), reps)
    db.close()
    open_ms, open_spread = wall(open_, reps, close)
    close()

    nrec, e = _lib.c_size_t(), _lib.c_int()

    def scan():
        _lib.call("sg_db_scan", _p8(file), file.size, None, None, None, None, None, 0, _lib.ctypes.byref(nrec),
                  _lib.ctypes.byref(e))

    scan_ms, _ = wall(scan, 5)
    src = torch.from_numpy(file.copy())
    dst = torch.empty(file.size, dtype=torch.uint8, device="cuda")

    def up():
        dst.copy_(src)
        torch.cuda.synchronize()

    wall(up, 2)
    upload_ms, _ = wall(up, 5)

    # ---- the kernels, timed by events in a pass of their own ----
    ctx.timing(True)
    ctx.sync()
    k0 = {k: ctx.kernel_time(k)[0] for k in KERNELS}
    for _ in range(reps):
        open_()
        close()
    kern = {k: round((ctx.kernel_time(k)[0] - k0[k]) / reps, 4) for k in KERNELS}
    ctx.timing(False)
    ksum = sum(kern.values())
    res = {"metric": "db_open_rate", "programs": n, "file_bytes": len(data), "stream_bytes": sum(map(len, streams)),
           "text_bytes": text_bytes, "length_median_assumed": a.median, "length_sigma": a.sigma, "reps": reps,
           "level": 9, "framing": "sync flush + final empty stored block (Go's writer as read from its source: unpinned)",
           "baseline": "zlib.decompressobj(-15) per record, one CPU thread, C zlib (not Go's compress/flate)",
           "open_ms": open_ms, "open_ms_min_max": open_spread, "baseline_ms": round(base_ms, 1),
           "baseline_ms_min_max": [round(min(base), 1), round(max(base), 1)], "baseline_scan_ms": round(base_scan_ms, 1),
           "open_over_baseline": round(open_ms / base_ms, 4), "kernel_ms": kern, "kernels_ms": round(ksum, 3),
           "not_kernel_ms": round(open_ms - ksum, 3), "not_kernel_share": round((open_ms - ksum) / open_ms, 4),
           "scan_ms": scan_ms, "upload_ms": upload_ms, "verify_ms": verify_ms, "verify_ms_min_max": verify_spread,
           "long_streams": ctx.counter("inflate_long_streams"), "build_s": round(build_s, 1)}
    print(json.dumps(res), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(json.dumps(res) + "\n")


if __name__ == "__main__":
    main()
