#!/usr/bin/env python3
"""Rate of the program identities: sg_prog_hashes, sg_prog_hashes_dev, sg_hub_sync and sg_sigset_add_progs on
500k programs whose lengths are lognormal (median --median bytes, sigma --sigma), clipped to [16 B, 64 KiB]
(--clip lowers the upper end: SHA-1 is a serial chain, and the longest program alone bounds the kernel from
below), with random bytes.  The reference publishes no program-size figures: the median is an ASSUMPTION.  One JSON
line.  After a warm-up, timed repetitions of the legs on the same input, each timed by a host clock from the
call to its return (call_ms is the median of the repetitions, call_ms_min_max their range):
  prog_hashes      sg_prog_hashes: texts and offsets in, the identities out
  prog_hashes_dev  sg_prog_hashes_dev on device-resident texts, then a context sync
  hub_sync         sg_hub_sync on a set that holds the same corpus with 1 % of the programs replaced (the set
                   is put back into that state before every repetition, outside the clock)
  add_progs        sg_sigset_add_progs into an empty set (cleared outside the clock)
  baseline         a hashlib.sha1 loop plus a dict on this machine's CPU: OpenSSL through Python, one thread.
                   It is not Go: the reference's own loop (manager.go:1053-1069) was not run.
The GPU results are compared with the baseline's.  Then, in a pass of its own, the kernels
(sg_ctx_kernel_time) of one sg_hub_sync; "scan" is every prefix scan of the call, those inside
"sha1_sort" included."""
import argparse
import hashlib
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from syzkaller_amd import _lib  # noqa: E402
from syzkaller_amd import corpus as P  # noqa: E402
from syzkaller_amd import cover as C  # noqa: E402
from syzkaller_amd.cover import _p8, _p64  # noqa: E402

U8, U64 = np.uint8, np.uint64
KERNELS = ("sha1_keys", "sha1_sort", "scan", "sha1_short", "sha1_long", "sigset_insert", "sigset_flags", "sigset_compact",
           "hub_sync_diff", "hub_sync_gather")


def wall(fn, n, before=None):
    ms = []
    for _ in range(n):
        if before:
            before()
        t0 = time.perf_counter()
        fn()
        ms.append((time.perf_counter() - t0) * 1e3)
    return round(float(np.median(ms)), 3), [round(min(ms), 3), round(max(ms), 3)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--programs", type=int, default=500000)
    ap.add_argument("--median", type=float, default=512.0)
    ap.add_argument("--sigma", type=float, default=1.0)
    ap.add_argument("--clip", type=int, default=65536, help="the longest program, in bytes")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--baseline-reps", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "prog_hashes_rate.jsonl"))
    a = ap.parse_args()
    import torch

    ctx = C.Context(0)
    rng = np.random.default_rng(7)
    n = a.programs
    lens = np.clip(rng.lognormal(np.log(a.median), a.sigma, size=n), 16, a.clip).astype(np.int64)
    off = np.zeros(n + 1, U64)
    off[1:] = np.cumsum(lens)
    nbytes = int(off[-1])
    data = rng.integers(0, 256, size=nbytes, dtype=U8)
    # the hub's state: the same corpus with 1 % of the programs replaced (their first bytes changed)
    old = data.copy()
    repl = rng.choice(n, size=n // 100, replace=False)
    old[off[repl].astype(np.int64)] ^= 0xFF
    sigs = np.empty((n, 20), U8)
    hub, fresh = P.SigSet(n, ctx=ctx), P.SigSet(n, ctx=ctx)
    add, dels, nd, flags = np.zeros(n, U8), np.empty((n, 20), U8), _lib.c_size_t(), np.zeros(n, U8)
    d_data = torch.from_numpy(data).to("cuda")
    d_off = torch.from_numpy(off.view(np.int64)).to("cuda")
    d_sigs = torch.empty(20 * n, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()

    def prog_hashes():
        _lib.call("sg_prog_hashes", ctx.h, _p8(data), _p64(off), n, _p8(sigs), None)

    def prog_hashes_dev():
        _lib.call("sg_prog_hashes_dev", ctx.h, d_data.data_ptr(), d_off.data_ptr(), n, nbytes, d_sigs.data_ptr())
        ctx.sync()

    def hub_reset():
        hub.clear()
        _lib.call("sg_sigset_add_progs", hub.h, _p8(old), _p64(off), n, None, _p8(flags))

    def hub_sync():
        _lib.call("sg_hub_sync", hub.h, _p8(data), _p64(off), n, None, _p8(add), _p8(dels), n, _lib.ctypes.byref(nd))

    def add_progs():
        _lib.call("sg_sigset_add_progs", fresh.h, _p8(data), _p64(off), n, None, _p8(flags))

    base = {}

    def baseline():
        view = memoryview(data)
        o = off.astype(np.int64).tolist()
        hubmap = base["hub"]
        corpus, adds = {}, []
        for k in range(n):  # manager.go:1053-1061
            h = hashlib.sha1(view[o[k]:o[k + 1]]).digest()
            corpus[h] = True
            if h not in hubmap:
                adds.append(k)
        base["del"] = [h for h in hubmap if h not in corpus]  # :1063-1069
        base["add"], base["corpus"] = adds, corpus

    view, o = memoryview(old), off.astype(np.int64).tolist()
    base["hub"] = {hashlib.sha1(view[o[k]:o[k + 1]]).digest(): True for k in range(n)}
    wall(prog_hashes, a.warmup)
    wall(prog_hashes_dev, a.warmup)
    wall(hub_sync, a.warmup, hub_reset)
    wall(add_progs, a.warmup, fresh.clear)
    b_ms, b_spread = wall(baseline, a.baseline_reps)
    # the GPU's results against the baseline's
    exp = np.frombuffer(b"".join(base["corpus"]), U8).reshape(-1, 20)
    assert exp.shape[0] == n, "the corpus' programs are distinct"
    assert np.array_equal(sigs, exp), "sg_prog_hashes disagrees with hashlib"
    assert np.array_equal(d_sigs.cpu().numpy().reshape(n, 20), exp), "sg_prog_hashes_dev disagrees with hashlib"
    assert np.flatnonzero(add).tolist() == base["add"] and nd.value == len(base["del"]) == n // 100
    assert dels[: nd.value].tobytes() == b"".join(base["del"]), "a.Del disagrees"
    assert np.array_equal(hub.export(), exp) and flags.all() and np.array_equal(fresh.export(), exp)
    w, spread = {}, {}
    w["prog_hashes"], spread["prog_hashes"] = wall(prog_hashes, a.reps)
    w["prog_hashes_dev"], spread["prog_hashes_dev"] = wall(prog_hashes_dev, a.reps)
    w["hub_sync"], spread["hub_sync"] = wall(hub_sync, a.reps, hub_reset)
    w["add_progs"], spread["add_progs"] = wall(add_progs, a.reps, fresh.clear)
    w["baseline"], spread["baseline"] = b_ms, b_spread
    ctx.timing(True)
    hub_reset()
    ctx.sync()
    t0 = {k: ctx.kernel_time(k)[0] for k in KERNELS}
    for _ in range(a.reps):
        hub_sync()
        ctx.sync()
        t1 = {k: ctx.kernel_time(k)[0] for k in KERNELS}
        hub_reset()
        ctx.sync()
        t2 = {k: ctx.kernel_time(k)[0] for k in KERNELS}
        for k in KERNELS:  # (the reset's own kernels are not the sync's)
            t0[k] += t2[k] - t1[k]
    kern = {k: round((ctx.kernel_time(k)[0] - t0[k]) / a.reps, 4) for k in KERNELS}
    ctx.timing(False)
    blocks = int(((lens + 8) // 64 + 1).sum())
    res = {"metric": "prog_hashes_rate", "programs": n, "bytes": nbytes, "sha1_blocks": blocks,
           "length_median_assumed": a.median, "length_sigma": a.sigma, "max_length": int(lens.max()),
           "long_path_programs": int((lens > P.SHA1_LONG).sum()), "replaced": int(n // 100),
           "reps": a.reps, "baseline_reps": a.baseline_reps,
           "baseline": "hashlib.sha1 loop plus dict (OpenSSL through Python, one CPU thread; not Go)",
           "call_ms": w, "call_ms_min_max": spread, "hub_sync_kernel_ms": kern,
           "hub_sync_over_baseline": round(w["hub_sync"] / w["baseline"], 5),
           "sha1_short_blocks_per_s": round(blocks / (kern["sha1_short"] * 1e-3)) if kern["sha1_short"] else None,
           "sha1_short_bytes_per_s": round(nbytes / (kern["sha1_short"] * 1e-3)) if kern["sha1_short"] else None}
    print(json.dumps(res), flush=True)
    hub.close()
    fresh.close()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(json.dumps(res) + "\n")


if __name__ == "__main__":
    main()
