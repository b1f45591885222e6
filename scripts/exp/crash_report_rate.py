#!/usr/bin/env python3
"""Rate of the crash-report calls, sg_crash_scan, sg_crash_parse and sg_console_output, over a synthetic crash store:
--logs stored crash logs (1,024), each with up to 1 MiB of console and fuzzer output before the oops and up to
128 KiB after it -- vm/vm.go's two constants (:121-143).  A log is console lines (a timestamp prefix and a message)
and the fuzzer's lines (`executing program`, program text) in front, an oops of some sixty lines (a KASAN header, a
call trace with `?` frames, a taint line, the panic_on_warn panic past rank 40), and more of the same behind.  The
sizes are uniform in [1/16, 1] of the two limits.  The line-length distribution and the mix are recorded as `assumed`.

Every result is compared before anything is timed: all three calls on the first --check-logs logs with
tests/crash_report_oracle.py, and the device forms with the host forms on the whole store.

Per call, after a warm-up call, the median of --reps timed calls (host clock, call to return):
  host   the host form: the batch uploaded from pageable memory, the results on the host
  dev    the device form over a resident batch, the results left on the device (its one wait included)
with the upload timed apart (upload_ms: the batch from pageable memory to the device, by torch), and in a pass of
its own the named kernels (sg_ctx_kernel_time).  text_bytes_per_s is the batch's bytes over the device form's call,
frac_stream that rate over 6.2 TB/s, the streaming read DESIGN.md section 4 measures.

parse_batch end to end, with two ignores: its three steps (the scan, the regexps over the record lines, the parse)
and what the host then does per log (extractDescription's expressions, the replacements), so the share left on the
host is visible.

The baseline is tests/crash_report_oracle.py parse_bounds on the first --baseline-logs logs, named as what it is:
Python on one thread, not Go.  Nothing is scaled."""
import argparse
import json
import os
import re
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from syzkaller_amd import _lib  # noqa: E402
from syzkaller_amd import cover as C  # noqa: E402
from syzkaller_amd import report as R  # noqa: E402
from tests import crash_report_oracle as OR  # noqa: E402

U8, U32, U64 = np.uint8, np.uint32, np.uint64
STREAM = 6.2e12
BEFORE, AFTER = 1 << 20, 128 << 10
KERNELS = ("crash_lines", "crash_flags", "crash_line", "crash_records", "crash_logs", "crash_copy", "scan")


def pool(rng, nbytes):
    """nbytes or so of calm output and its line starts: 60 % console lines, 40 % fuzzer lines"""
    lines, size, t = [], 0, 100.0
    while size < nbytes:
        if rng.random() < 0.6:
            t += rng.random()
            ln = b"[%12.6f] " % t + rng.choice([b"audit: type=1400 audit(%d.%d): avc: denied { read } for pid=%d comm=\"syz-executor%d\"",
                                               b"netlink: %d bytes leftover after parsing attributes in process `syz-executor%d'.",
                                               b"device lo entered promiscuous mode %d %d", b"IPVS: Creating netns size=%d id=%d"])
            ln = ln.replace(b"%d", b"%d" % rng.randrange(100000))
        elif rng.random() < 0.1:
            ln = b"executing program %d:" % rng.randrange(8)
        else:
            ln = b"r%d = syz_open_dev$tun(&(0x7f0000%04x000)=\"%s\", 0x%x, 0x%x)" % (
                rng.randrange(20), rng.randrange(1 << 16), b"2f6465762f" * rng.randrange(1, 30), rng.randrange(64), rng.randrange(1 << 12))
        lines.append(ln + b"\n")
        size += len(ln) + 1
    data = b"".join(lines)
    starts = np.cumsum([0] + [len(x) for x in lines])
    return data, starts


def oops(rng):
    t = 500.0 + rng.random()
    p = lambda: b"[%12.6f] " % t  # noqa: E731
    out = [p() + b"=================================================================="]
    out.append(p() + b"BUG: KASAN: use-after-free in ip6_send_skb+0x%x/0x340 at addr ffff8800%08x" % (rng.randrange(256), rng.randrange(1 << 32)))
    out.append(p() + b"Read of size 8 by task syz-executor%d/%d" % (rng.randrange(8), rng.randrange(30000)))
    out.append(p() + b"Call Trace:")
    for k in range(50):
        q = b" ? " if rng.random() < 0.3 else b" "
        out.append(p() + b" [<ffffffff81%06x>]%sfunc_%d+0x%x/0x%x" % (rng.randrange(1 << 24), q, rng.randrange(500), rng.randrange(4096), rng.randrange(4096)))
    out.insert(8, p() + OR.TAINT)
    out.append(p() + b"Kernel panic - not syncing: panic_on_warn set ...")
    out.append(p() + b"Kernel Offset: disabled")
    out.append(p() + b"Rebooting in 86400 seconds..")
    return b"".join(x + b"\n" for x in out)


def store(nlogs, seed):
    import random

    rng = random.Random(seed)
    data, starts = pool(rng, 6 << 20)
    logs = []
    for _ in range(nlogs):
        parts = []
        for lim in (BEFORE, AFTER):
            want = rng.randrange(lim // 16, lim)
            i = rng.randrange(0, len(starts) - 1)
            a = int(starts[i])
            b = int(starts[np.searchsorted(starts, min(a + want, len(data)), side="right") - 1])
            parts.append(data[a:b])
        logs.append(parts[0] + oops(rng) + parts[1])
    return logs


def wall(fn, reps):
    ms = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ms.append((time.perf_counter() - t0) * 1e3)
    return round(float(np.median(ms)), 3), [round(min(ms), 3), round(max(ms), 3)]


def kernel_times(ctx, fn, reps):
    ctx.timing(True)
    fn()
    base = {k: ctx.kernel_time(k)[0] for k in KERNELS}
    for _ in range(reps):
        fn()
    ctx.sync()
    ms = {k: round((ctx.kernel_time(k)[0] - base[k]) / reps, 4) for k in KERNELS}
    ctx.timing(False)
    return {k: v for k, v in ms.items() if v}


def main():
    import torch

    ap = argparse.ArgumentParser()
    ap.add_argument("--logs", type=int, default=1024)
    ap.add_argument("--check-logs", type=int, default=16)
    ap.add_argument("--baseline-logs", type=int, default=16)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "crash_report_rate.jsonl"))
    a = ap.parse_args()
    ctx = C.Context(0)
    logs = store(a.logs, 5)
    data, off = R.to_batch(logs)
    nlogs, nbytes = len(logs), int(data.size)
    lens = np.diff(np.flatnonzero(data[: 64 << 20] == 10))
    assumed = {"before_bytes": [BEFORE // 16, BEFORE], "after_bytes": [AFTER // 16, AFTER], "console_line_share": 0.6,
               "line_bytes_mean": round(float(lens.mean()), 1), "line_bytes_p50_p99": [int(np.percentile(lens, 50)), int(np.percentile(lens, 99))],
               "oops_lines": 57}
    rows = []

    # ---- compare first: the oracle on a subset, the device forms on everything
    sub = logs[: a.check_logs]
    recs = R.crash_scan(sub, ctx)
    want = [(l,) + r for l, log in enumerate(sub) for r in OR.scan(log)]
    assert list(zip(recs.log.tolist(), recs.line_start.tolist(), recs.line_end.tolist(), recs.oops.tolist(), recs.match.tolist())) == want
    pb = R.parse_bounds_batch(sub, None, ctx)
    for l, log in enumerate(sub):
        o, s, e, dp, dl, t = OR.parse_bounds(log)
        assert (int(pb.oops[l]), int(pb.start[l]), int(pb.end[l]), int(pb.desc_pos[l]), int(pb.desc_len[l]), pb.text(l)) == (o, s, e, dp, dl, t)
    assert R.console_output_batch(sub, ctx) == [OR.console_output(x) for x in sub]
    del recs, pb

    got = {}
    t0 = time.perf_counter()
    d_data = torch.from_numpy(data).to("cuda")
    torch.cuda.synchronize()
    up = [(time.perf_counter() - t0) * 1e3]
    for _ in range(a.reps):
        t0 = time.perf_counter()
        d_data.copy_(torch.from_numpy(data))
        torch.cuda.synchronize()
        up.append((time.perf_counter() - t0) * 1e3)
    upload_ms = round(float(np.median(up[1:])), 3)
    d_off = torch.from_numpy(off.view(np.int64)).to("cuda")
    buf = lambda n: torch.empty(n + 16, dtype=torch.uint8, device="cuda")  # noqa: E731
    host = lambda t, dt, n: t.cpu().numpy()[: n * np.dtype(dt).itemsize].view(dt)  # noqa: E731

    def row(metric, host_fn, dev_fn, extra):
        host_ms, host_mm = wall(host_fn, a.reps)
        dev_ms, dev_mm = wall(dev_fn, a.reps)
        km = kernel_times(ctx, dev_fn, a.reps)
        r = {"metric": metric, "logs": nlogs, "text_bytes": nbytes, "assumed": assumed, "reps": a.reps,
             "upload_ms": upload_ms, "call_ms": {"host": host_ms, "dev": dev_ms},
             "call_ms_min_max": {"host": host_mm, "dev": dev_mm}, "kernel_ms": km, "device_ms": round(sum(km.values()), 4),
             "text_bytes_per_s": round(nbytes / (dev_ms * 1e-3), 0), "frac_stream": round(nbytes / (dev_ms * 1e-3) / STREAM, 5)}
        r.update(extra)
        rows.append(r)
        print(json.dumps(r), flush=True)

    # ---- sg_crash_scan
    def scan_host():
        got["scan"] = R.crash_scan(logs, ctx, cap=1 << 17)

    scan_host()
    k = len(got["scan"])
    sc = [buf(nlogs), buf(4 * k), buf(8 * k), buf(8 * k), buf(4 * k), buf(8 * k), buf(8), buf(24)]

    def scan_dev():
        q = [x.data_ptr() for x in sc]
        _lib.call("sg_crash_scan_dev", ctx.h, d_data.data_ptr(), d_off.data_ptr(), nlogs, nbytes, *q[:6], k, q[6], q[7])
        ctx.sync()

    scan_dev()
    s = got["scan"]
    assert int(host(sc[6], U64, 1)[0]) == k and np.array_equal(host(sc[0], U8, nlogs), s.contains) and s.contains.all()
    for x, dt, w in zip(sc[1:6], (U32, U64, U64, U32, U64), (s.log, s.line_start, s.line_end, s.oops, s.match)):
        assert np.array_equal(host(x, dt, k), w)
    stats = s.stats.tolist()
    row("crash_scan_rate", scan_host, scan_dev, {"lines": stats[0], "records": k})

    # ---- sg_crash_parse
    def parse_host():
        got["parse"] = R.parse_bounds_batch(logs, None, ctx, cap=64 << 20)

    parse_host()
    b = got["parse"]
    nt = int(b.text_off[nlogs])
    pc = [buf(4 * nlogs)] + [buf(8 * nlogs) for _ in range(4)] + [buf(8 * nlogs + 8), buf(nt), buf(24)]

    def parse_dev():
        q = [x.data_ptr() for x in pc]
        _lib.call("sg_crash_parse_dev", ctx.h, d_data.data_ptr(), d_off.data_ptr(), nlogs, nbytes, None, None, 0, *q[:7], nt, q[7])
        ctx.sync()

    parse_dev()
    assert np.array_equal(host(pc[0], np.int32, nlogs), b.oops) and (b.oops == 0).all()
    for x, w in zip(pc[1:5], (b.start, b.end, b.desc_pos, b.desc_len)):
        assert np.array_equal(host(x, U64, nlogs), w)
    assert np.array_equal(host(pc[5], U64, nlogs + 1), b.text_off) and np.array_equal(host(pc[6], U8, nt), b.text_bytes)
    row("crash_parse_rate", parse_host, parse_dev, {"lines": int(b.stats[0]), "console_lines": int(b.stats[1]), "text_out_bytes": nt})

    # ---- sg_console_output
    def cons_host():
        got["cons"] = R.console_output_batch(logs, ctx)

    cons_host()
    total = sum(len(x) for x in got["cons"])
    cc = [buf(8 * nlogs + 8), buf(total)]

    def cons_dev():
        _lib.call("sg_console_output_dev", ctx.h, d_data.data_ptr(), d_off.data_ptr(), nlogs, nbytes, cc[0].data_ptr(),
                  cc[1].data_ptr(), total, None)
        ctx.sync()

    cons_dev()
    assert bytes(host(cc[1], U8, total)) == b"".join(got["cons"])
    row("console_output_rate", cons_host, cons_dev, {"out_bytes": total})
    del d_data, sc, pc, cc

    # ---- parse_batch end to end, with ignores, step by step
    igs = [re.compile(rb"WARNING: suspicious"), re.compile(rb"Kernel panic - not syncing: panic_on_warn")]
    t = [time.perf_counter()]
    recs = R.crash_scan(logs, ctx, cap=1 << 17)
    t.append(time.perf_counter())
    ignored = R._ignored_lines(logs, recs, igs)
    t.append(time.perf_counter())
    pb = R.parse_bounds_batch(logs, ignored, ctx, cap=64 << 20)
    t.append(time.perf_counter())
    descs = []
    for l, log in enumerate(logs):
        st, dp = int(pb.start[l]), int(pb.desc_pos[l])
        descs.append(R.finish_description(R.extract_description(log[st:], int(pb.oops[l]), log[dp:dp + int(pb.desc_len[l])])))
    t.append(time.perf_counter())
    whole = R.parse_batch(logs, igs, ctx)
    t.append(time.perf_counter())
    assert [w[0] for w in whole] == descs and all(d == b"KASAN: use-after-free Read in ip6_send_skb" for d in descs)
    assert sum(len(s) for s in ignored) == nlogs and (pb.end < b.end).all()
    step = [round((y - x) * 1e3, 1) for x, y in zip(t, t[1:])]
    rows.append({"metric": "parse_batch_end_to_end", "logs": nlogs, "text_bytes": nbytes, "ignores": 2,
                 "step_ms": {"scan": step[0], "ignores_over_record_lines": step[1], "parse": step[2],
                             "descriptions_on_host": step[3]}, "record_lines": len({(int(x), int(y)) for x, y in zip(recs.log, recs.line_start)}),
                 "parse_batch_ms": step[4], "host_share": round((step[1] + step[3]) / sum(step[:4]), 3),
                 "note": "scan and parse are host forms: each uploads the batch from pageable memory and joins the logs in Python"})
    print(json.dumps(rows[-1]), flush=True)

    # ---- the baseline: the sequential Python restatement, on a subset
    base = logs[: a.baseline_logs]
    t0 = time.perf_counter()
    for log in base:
        OR.parse_bounds(log)
    base_s = time.perf_counter() - t0
    bb = sum(len(x) for x in base)
    rows.append({"metric": "crash_parse_baseline", "what": "tests/crash_report_oracle.py parse_bounds: Python on one thread, not Go",
                 "logs": len(base), "text_bytes": bb, "s": round(base_s, 2), "text_bytes_per_s": round(bb / base_s, 0)})
    print(json.dumps(rows[-1]), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        for r in rows:
            f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
