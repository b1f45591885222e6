#!/usr/bin/env python3
"""Rate of the cover report's text ingest, sg_objdump_pcs and sg_nm_symbols, at the size of cover_lines_rate.py's
world(): 50,000 symbols of 100 call sites each, rendered as kernel-style text.

  objdump  one line per call site as `objdump -d --no-show-raw-insn` prints it, in address order, among lines that
           are no call site.  Every line is 69 bytes.  The share of other lines is what brings the text to 1 GB
           or more -- two other lines per site -- and is recorded as `assumed`: a real vmlinux has more of them.
  nm       `nm -nS` lines: each symbol as t or T, and between them as many data symbols (d, D, r, b) again.
  addr2line  `addr2line -afi` output for all the sites: a PC line and the world's frames, two lines each (7.3M
           frames, 5,500 files, 70,000 functions), through sg_addr2line_frames[_dev]; its rate is the text's bytes
           over the device form's whole call, interning included.

Per stage, after a warm-up call, the median of --reps timed calls (call_ms_min_max their range), each timed by a
host clock from the call to its return:
  host    the host form: the text uploaded from pageable memory, the results on the host
  dev     the device form over a resident text, the results left on the device (its one wait included)
and in a pass of its own the named kernels (sg_ctx_kernel_time).  scan_bytes_per_s is the text's bytes over the
time of the two walks (each reads the text once), and frac_stream that rate over 6.2 TB/s, the streaming read
DESIGN.md section 4 measures.  The results are compared with the world's arrays.

The baseline is the path a caller had before: the same text through the sequential Python parser of
tests/cover_ingest_oracle.py, on the first --baseline-bytes of the objdump text (cut at a line end; the size is in
the row), on the whole nm text, and on the first quarter of that many bytes of the addr2line text (records and
bytes in the row), there with the dict interning CoverReport does.  Then the fused build
(CoverTable.from_text: sg_cover_table_from_text over the nm and addr2line texts), and the report end to end:
CoverReport(callable) fed by those Python parsers -- the only path there was -- against CoverReport.from_tools on
the same three texts of a world of --report-symbols symbols (the size is in the row).  Nothing is scaled."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import numpy as np  # noqa: E402

from cover_lines_rate import world  # noqa: E402
from syzkaller_amd import _lib  # noqa: E402
from syzkaller_amd import cover as C  # noqa: E402
from tests import cover_ingest_oracle as OR  # noqa: E402

U8, U32, U64 = np.uint8, np.uint32, np.uint64
STREAM = 6.2e12
SITE = b"0000000000000000:\tcallq  ffffffff815cc1d0 <__sanitizer_cov_trace_pc>\n"
OTHER = b"0000000000000000:\tmov    %rax,0x10(%rbp)".ljust(len(SITE) - 1) + b"\n"
HEX = np.frombuffer(b"0123456789abcdef", U8)


def stamp(rows, col, vals):
    """rows[:, col:col+16] = the 16 hex digits of vals"""
    for d in range(16):
        rows[:, col + d] = HEX[((vals >> U64(60 - 4 * d)) & U64(15)).astype(np.intp)]


def objdump_text(sites, others_per_site):
    per = others_per_site + 1
    rows = np.empty((sites.size, per, len(SITE)), dtype=U8)
    rows[:, :others_per_site, :] = np.frombuffer(OTHER, U8)
    rows[:, others_per_site, :] = np.frombuffer(SITE, U8)
    for k in range(per):
        stamp(rows[:, k, :], 0, sites - U64(4 * (others_per_site - k)))
    return rows.reshape(-1)


def nm_text(ss, size):
    n = ss.size
    line = b"0000000000000000 0000000000000000 t sym_0000000000000000\n"
    rows = np.empty((n, 2, len(line)), dtype=U8)
    rows[:] = np.frombuffer(line, U8)
    idx = np.arange(n, dtype=U64)
    for k in range(2):
        stamp(rows[:, k, :], 0, ss + U64(8 * k))
        stamp(rows[:, k, :], 17, np.full(n, size, dtype=U64))
        stamp(rows[:, k, :], 40, idx)
    rows[:, 0, 34] = np.frombuffer(b"tT", U8)[(idx % U64(2)).astype(np.intp)]
    rows[:, 1, 34] = np.frombuffer(b"dDrb", U8)[(idx % U64(4)).astype(np.intp)]
    return rows.reshape(-1)


def a2l_text(W):
    """`addr2line -afi` output for every site of the world, and the sentinel's record"""
    sites, off, file, line, func = W[2], W[3].astype(np.int64), W[4], W[5], W[6]
    frames = [b"fn_%d\n/src/d%d/f_%d.c:%d\n" % (fu, fi % 97, fi, ln)
              for fu, fi, ln in zip(func.tolist(), file.tolist(), line.tolist())]
    parts, o = [], off.tolist()
    for j, pc in enumerate(sites.tolist()):
        parts.append(b"0x%016x\n" % pc)
        parts += frames[o[j]:o[j + 1]]
    parts.append(b"0xffffffffffffffff\n??\n??:0\n")
    return np.frombuffer(b"".join(parts), U8)


def wall(fn, reps):
    ms = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ms.append((time.perf_counter() - t0) * 1e3)
    return round(float(np.median(ms)), 3), [round(min(ms), 3), round(max(ms), 3)]


def kernel_times(ctx, fn, names, reps):
    ctx.timing(True)
    fn()
    base = {k: ctx.kernel_time(k)[0] for k in names}
    for _ in range(reps):
        fn()
    ctx.sync()
    ms = {k: round((ctx.kernel_time(k)[0] - base[k]) / reps, 4) for k in names}
    ctx.timing(False)
    return ms


def main():
    import torch

    ap = argparse.ArgumentParser()
    ap.add_argument("--symbols", type=int, default=50000)
    ap.add_argument("--sites-per-symbol", type=int, default=100)
    ap.add_argument("--min-bytes", type=int, default=1_000_000_000)
    ap.add_argument("--baseline-bytes", type=int, default=128 << 20)
    ap.add_argument("--report-symbols", type=int, default=30000)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cover_ingest_rate.jsonl"))
    a = ap.parse_args()
    ctx = C.Context(0)
    ss, se, sites = world(a.symbols, a.sites_per_symbol, np.random.default_rng(5))[:3]
    others = max(-(-a.min_bytes // (len(SITE) * sites.size)) - 1, 0)
    od = objdump_text(sites, others)
    size = int(se[0] - ss[0]) - 14          # ReadSymbols rounds it up to the stride
    nm = nm_text(ss, size)
    p8 = lambda x: x.ctypes.data_as(_lib.P8)  # noqa: E731
    nc, nf = np.frombuffer(b"callq ", U8), np.frombuffer(b" <__sanitizer_cov_trace_pc>", U8)
    rows = []

    # ---- objdump
    got = {}
    d_od = torch.from_numpy(od).to("cuda")
    d_pcs = torch.empty(sites.size + 1, dtype=torch.int64, device="cuda")
    d_info = torch.zeros(3, dtype=torch.int64, device="cuda")

    def od_host():
        got["pcs"] = C.objdump_pcs(od, ctx=ctx)

    def od_dev():
        _lib.call("sg_objdump_pcs_dev", ctx.h, d_od.data_ptr(), od.size, p8(nc), nc.size, p8(nf), nf.size, d_pcs.data_ptr(),
                  sites.size + 1, d_info.data_ptr())
        ctx.sync()

    od_host()
    od_dev()
    assert np.array_equal(got["pcs"], sites) and d_info.cpu().tolist() == [sites.size, 0, 0]
    assert np.array_equal(d_pcs.cpu().numpy()[:sites.size].view(U64), sites)
    host_ms, host_mm = wall(od_host, a.reps)
    dev_ms, dev_mm = wall(od_dev, a.reps)
    km = kernel_times(ctx, od_dev, ("objdump_scan", "objdump_emit", "objdump_sort"), a.reps)
    walks = km["objdump_scan"] + km["objdump_emit"]
    cut = bytes(od[:a.baseline_bytes // len(SITE) * len(SITE)])
    t0 = time.perf_counter()
    base_pcs = OR.objdump_pcs(cut)
    base_ms = (time.perf_counter() - t0) * 1e3
    assert np.array_equal(np.array(base_pcs, dtype=U64), sites[:len(base_pcs)])
    rows.append({"metric": "objdump_pcs_rate", "text_bytes": int(od.size), "lines": int(od.size // len(SITE)),
                 "sites": int(sites.size), "assumed": {"other_lines_per_site": others,
                                                        "other_line_share": round(others / (others + 1), 4)},
                 "reps": a.reps, "call_ms": {"host": host_ms, "dev": dev_ms},
                 "call_ms_min_max": {"host": host_mm, "dev": dev_mm}, "kernel_ms": km,
                 "device_ms": round(sum(km.values()), 4),
                 "scan_bytes_per_s": round(2 * od.size / (walks * 1e-3), 0) if walks else None,
                 "frac_stream": round(2 * od.size / (walks * 1e-3) / STREAM, 4) if walks else None,
                 "dev_call_text_bytes_per_s": round(od.size / (dev_ms * 1e-3), 0),
                 "baseline": {"what": "tests/cover_ingest_oracle.py objdump_pcs", "text_bytes": len(cut),
                              "sites": len(base_pcs), "ms": round(base_ms, 1),
                              "text_bytes_per_s": round(len(cut) / (base_ms * 1e-3), 0)}})
    print(json.dumps(rows[-1]), flush=True)
    del d_od, cut

    # ---- nm
    d_nm = torch.from_numpy(nm).to("cuda")
    k = ss.size
    bufs = [torch.empty(k + 1, dtype=torch.int64, device="cuda") for _ in range(7)]

    def nm_host():
        got["nm"] = C.nm_symbols(nm, ctx=ctx)

    def nm_dev():
        _lib.call("sg_nm_symbols_dev", ctx.h, d_nm.data_ptr(), nm.size, *[b.data_ptr() for b in bufs], k + 1,
                  d_info.data_ptr())
        ctx.sync()

    nm_host()
    nm_dev()
    s = got["nm"]
    assert np.array_equal(s.sym_start, ss) and np.array_equal(s.sym_end, se + U64(1)) and len(s) == k
    assert np.array_equal(s.order, np.arange(k)) and d_info.cpu().tolist() == [k, 0, 0]
    host_ms, host_mm = wall(nm_host, a.reps)
    dev_ms, dev_mm = wall(nm_dev, a.reps)
    km = kernel_times(ctx, nm_dev, ("nm_scan", "nm_emit", "nm_order"), a.reps)
    walks = km["nm_scan"] + km["nm_emit"]
    text = bytes(nm)
    t0 = time.perf_counter()
    base = OR.nm_sorted(OR.nm_symbols(text))
    base_ms = (time.perf_counter() - t0) * 1e3
    assert base[0] == ss.tolist()
    rows.append({"metric": "nm_symbols_rate", "text_bytes": int(nm.size), "lines": 2 * k, "symbols": k, "reps": a.reps,
                 "call_ms": {"host": host_ms, "dev": dev_ms}, "call_ms_min_max": {"host": host_mm, "dev": dev_mm},
                 "kernel_ms": km, "device_ms": round(sum(km.values()), 4),
                 "scan_bytes_per_s": round(2 * nm.size / (walks * 1e-3), 0) if walks else None,
                 "frac_stream": round(2 * nm.size / (walks * 1e-3) / STREAM, 6) if walks else None,
                 "baseline": {"what": "tests/cover_ingest_oracle.py nm_symbols + nm_sorted", "text_bytes": len(text),
                              "ms": round(base_ms, 1), "text_bytes_per_s": round(len(text) / (base_ms * 1e-3), 0)}})
    print(json.dumps(rows[-1]), flush=True)
    del d_nm

    # ---- addr2line
    W = world(a.symbols, a.sites_per_symbol, np.random.default_rng(5))
    a2l = a2l_text(W)
    off, file, line, func = W[3], W[4], W[5], W[6]
    d_a2l = torch.from_numpy(a2l).to("cuda")
    nrec, nfr = sites.size, int(off[-1])
    sizes = (8 * nrec, 8 * (nrec + 1), 4 * nfr, 8 * nfr, 4 * nfr, 8 * nfr, 4 * nfr, 8 * nfr, 4 * nfr, 48)
    abuf = [torch.empty(m + 8, dtype=torch.uint8, device="cuda") for m in sizes]

    def a2l_host():
        got["a2l"] = C.addr2line_frames(a2l, nrec, ctx=ctx)

    def a2l_dev():
        q = [t.data_ptr() for t in abuf]
        _lib.call("sg_addr2line_frames_dev", ctx.h, d_a2l.data_ptr(), a2l.size, nrec, q[0], q[1], q[2], q[3], q[4], nfr,
                  q[5], q[6], q[7], q[8], 64, q[9])
        ctx.sync()

    a2l_host()
    a2l_dev()
    fr = got["a2l"]
    assert np.array_equal(fr.rec_pc, sites) and np.array_equal(fr.frame_off, off) and np.array_equal(fr.frame_line, line)
    # ids are dense in order of first occurrence: the same partition of the frames as the world's ids
    for mine, theirs in ((fr.frame_file, file), (fr.frame_func, func)):
        first = np.unique(theirs, return_index=True)[1]
        assert np.array_equal(mine[np.sort(first)], np.arange(first.size)) and np.unique(
            mine.astype(U64) << U64(32) | theirs.astype(U64)).size == first.size
    assert abuf[9].cpu().numpy()[:48].view(U64).tolist() == [nfr, fr.nfiles, fr.nfuncs, 0, 0, 0]
    host_ms, host_mm = wall(a2l_host, a.reps)
    dev_ms, dev_mm = wall(a2l_dev, a.reps)
    km = kernel_times(ctx, a2l_dev, ("a2l_lines", "a2l_records", "a2l_frames", "a2l_intern"), a.reps)
    nb = min(a.baseline_bytes // 4, a2l.size)
    brec = max(1, int(nrec * nb // a2l.size) - 2)
    text = bytes(a2l[:nb])
    t0 = time.perf_counter()
    recs = OR.addr2line_frames(text, brec)
    OR.intern(recs)
    base_ms = (time.perf_counter() - t0) * 1e3
    assert [pc for pc, _ in recs] == sites[:brec].tolist()
    rows.append({"metric": "addr2line_frames_rate", "text_bytes": int(a2l.size), "records": nrec, "frames": nfr,
                 "files": fr.nfiles, "funcs": fr.nfuncs, "reps": a.reps, "call_ms": {"host": host_ms, "dev": dev_ms},
                 "call_ms_min_max": {"host": host_mm, "dev": dev_mm}, "kernel_ms": km,
                 "device_ms": round(sum(km.values()), 4),
                 "dev_call_text_bytes_per_s": round(a2l.size / (dev_ms * 1e-3), 0),
                 "frac_stream": round(a2l.size / (dev_ms * 1e-3) / STREAM, 5),
                 "baseline": {"what": "tests/cover_ingest_oracle.py addr2line_frames + intern", "text_bytes": len(text),
                              "records": brec, "ms": round(base_ms, 1),
                              "text_bytes_per_s": round(len(text) / (base_ms * 1e-3), 0)}})
    print(json.dumps(rows[-1]), flush=True)
    del d_a2l, abuf

    # ---- the fused build: the three texts to an sg_cover_table, the frames never on the host
    ref = C.CoverTable(ss, se, sites, sites, off, file, line, func, int(file.max()) + 1, int(func.max()) + 1, ctx=ctx)

    def fused():
        t, files, funcs = C.CoverTable.from_text(nm, sites, a2l, ctx=ctx)
        got["fused"] = (t.nslots, len(files), len(funcs))
        t.close()

    fused()
    assert got["fused"] == (ref.nslots, fr.nfiles, fr.nfuncs)
    ref.close()
    fused_ms, fused_mm = wall(fused, a.reps)
    km = kernel_times(ctx, fused, ("nm_scan", "nm_emit", "nm_order", "a2l_lines", "a2l_records", "a2l_frames", "a2l_intern",
                                   "cover_table_build"), a.reps)
    rows.append({"metric": "cover_table_from_text_rate", "text_bytes": int(nm.size + a2l.size), "records": nrec,
                 "frames": nfr, "reps": a.reps, "call_ms": fused_ms, "call_ms_min_max": fused_mm, "kernel_ms": km,
                 "device_ms": round(sum(km.values()), 4), "text_bytes_per_s": round((nm.size + a2l.size) / (fused_ms * 1e-3), 0),
                 "frac_stream": round((nm.size + a2l.size) / (fused_ms * 1e-3) / STREAM, 5),
                 "note": "call_ms: the host form, both texts uploaded from pageable memory, the names sliced out in Python"})
    print(json.dumps(rows[-1]), flush=True)

    # ---- the report end to end against the path a caller had before: CoverReport(callable) fed by the Python
    # parsers of the same three texts, at --report-symbols symbols (stated in the row; nothing is scaled)
    W2 = world(a.report_symbols, a.sites_per_symbol, np.random.default_rng(6))
    ss2, se2, sites2 = W2[:3]
    nm2, od2, a2l2 = nm_text(ss2, size), objdump_text(sites2, others), a2l_text(W2)
    nm2b, od2b, a2l2b = bytes(nm2), bytes(od2), bytes(a2l2)

    def symbolize(pcs):
        recs = OR.addr2line_frames(a2l2b, len(pcs))
        return [(pc, fn.decode(), fl.decode(), ln) for pc, frs in recs for fn, fl, ln, _, _ in frs]

    t0 = time.perf_counter()
    bs, be, _ = OR.nm_sorted(OR.nm_symbols(nm2b))
    r_old = C.CoverReport(np.array(bs, U64), np.array(be, U64), OR.objdump_pcs(od2b), symbolize, ctx=ctx)
    old_s = time.perf_counter() - t0
    new_ms = []
    for _ in range(3):
        t0 = time.perf_counter()
        r_new = C.CoverReport.from_tools(nm2, od2, lambda pcs: a2l2, ctx=ctx)
        new_ms.append((time.perf_counter() - t0) * 1e3)
        if len(new_ms) < 3:
            r_new.close()
    assert r_new.names == r_old.names and r_new.files == r_old.files and r_new.funcs == r_old.funcs
    cov = ((sites2[::37] + U64(5)) & U64(0xffffffff)).astype(U32)
    assert r_new.file_set(cov, 0xffffffff) == r_old.file_set(cov, 0xffffffff)
    rows.append({"metric": "cover_report_from_tools", "symbols": int(ss2.size), "sites": int(sites2.size),
                 "frames": int(W2[3][-1]), "text_bytes": {"nm": len(nm2b), "objdump": len(od2b), "addr2line": len(a2l2b)},
                 "baseline": {"what": "CoverReport(callable) fed by tests/cover_ingest_oracle.py over the same texts",
                              "s": round(old_s, 2)},
                 "from_tools_ms": round(float(np.median(new_ms)), 2), "from_tools_ms_all": [round(x, 2) for x in new_ms],
                 "speedup": round(old_s * 1e3 / float(np.median(new_ms)), 1)})
    print(json.dumps(rows[-1]), flush=True)
    r_new.close()
    r_old.close()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        for r in rows:
            f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
