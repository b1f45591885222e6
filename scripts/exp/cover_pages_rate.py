#!/usr/bin/env python3
"""Rate of the cover report's file bodies, sg_cover_pages / sg_cover_pages_set,
on cover_lines_rate.py's table and covers (its world(), the same seed): 5M
sites, 5,500 files, covers of 100k and 1M PCs in PC order and in random order.
The sources are synthetic and their sizes an ASSUMPTION, not a measurement of
a kernel tree: every file is a run of blocks of 100 C-like lines (tab-indented,
12 to 90 bytes, now and then a '<', '>' or '&'), as many blocks as cover the
highest line the table lists for the file -- about 30 KiB for a source file of
1,000 lines, 3 KiB for a header.  One JSON line per cover.  After a warm-up,
timed repetitions alternate three legs on the same input, each timed by a host
clock from the call to its return (every leg ends with its results on the
host; call_ms is the median of the repetitions, call_ms_min_max their range):
  fused      sg_cover_pages on the two tables
  fused_set  sg_cover_pages_set on a set holding the cover (filled outside the
             window)
  chain      what a caller had before: sg_cover_lines, then parseFile and the
             render loop on the host in the fastest form bytes gives (whole-file
             bytes.replace in an order that equals the one-pass replacer, one
             split, the listed lines wrapped in the list, one join) -- reading
             no file: the sources are in memory
The bodies of the three are compared.  Then, in a pass of its own, the kernels
of the fused call (sg_ctx_kernel_time) and the copy kernel against its floor:
(stored bytes of the report's files + body bytes) over 4.8 TB/s of read + write
bytes, DESIGN.md section 8's copy rate.  The first lines are the two table
builds; the last is the download of a buffer of the bodies' size into pageable
and into pinned host memory (torch), which is what decides whether staging the
bodies through pinned memory could pay."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import numpy as np  # noqa: E402

from cover_lines_rate import BASE, U32, U64, wall_times, world  # noqa: E402
from syzkaller_amd import cover as C  # noqa: E402

NAMES = ("lines_rows", "lines_cov", "lines_unc", "lines_compact", "pages_marks", "pages_tiles", "pages_copy")
COPY_RATE = 4.8e12  # read + write bytes per second
COVERED = (b"<span id='covered'>", b"</span> /*covered*/")   # cover.go:133-135 (the join supplies the '\n')
UNCOVERED = (b"<span id='uncovered'>", b"</span>")           # cover.go:138-140
BLOCK_LINES = 100


def sources(file, line, nfiles, rng):
    """A source per file id: blocks of BLOCK_LINES C-like lines, enough to cover the table's highest line of it."""
    top = np.zeros(nfiles, dtype=np.int64)
    np.maximum.at(top, file.astype(np.int64), line.astype(np.int64))
    words = [b"if", b"(err", b"<", b"0)", b"goto", b"out;", b"return", b"ret", b"&", b"mask;", b"struct", b"page",
             b"*p", b"=", b"list_entry(pos,", b"->next", b">", b"limit", b"spin_lock(&dev->lock);", b"/*", b"*/", b"{", b"}"]
    blocks = []
    for _ in range(64):
        lines = []
        for _ in range(BLOCK_LINES):
            n = int(rng.integers(0, 12))
            ln = b"\t" * int(rng.integers(0, 4)) + b" ".join(words[int(k)] for k in rng.integers(0, len(words), size=n))
            lines.append(ln[:90])
        blocks.append(b"\n".join(lines) + b"\n")
    out = []
    for f in range(nfiles):
        nb = (int(top[f]) + BLOCK_LINES - 1) // BLOCK_LINES
        out.append(b"".join(blocks[int(k)] for k in rng.integers(0, len(blocks), size=nb)))
    return out, top


def host_pages(file_off, lines, covered, srcs):
    """parseFile (cover.go:198-217) and the render loop (cover.go:128-147) per file of the report: (bodies, coverage)."""
    bodies, coverage = [], np.zeros(len(srcs), dtype=U32)
    fo = file_off.tolist()
    for f in np.flatnonzero(np.diff(file_off.astype(np.int64)) > 0).tolist():
        data = srcs[f]
        cut = data.rfind(b"\n") + 1
        esc = data[:cut].replace(b"&", b"&amp;").replace(b"<", b"&lt;").replace(b">", b"&gt;").replace(b"\t", b"        ")
        ls = esc.split(b"\n")
        if cut < len(data):
            ls[-1] = data[cut:]  # the raw fragment
        else:
            ls.pop()
        n = len(ls)
        cov = 0
        for ln, c in zip(lines[fo[f]:fo[f + 1]].tolist(), covered[fo[f]:fo[f + 1]].tolist()):
            if ln <= n:
                pre, suf = COVERED if c else UNCOVERED
                ls[ln - 1] = pre + ls[ln - 1] + suf
                cov += c
        ls.append(b"")
        bodies.append(b"\n".join(ls) if n else b"")
        coverage[f] = cov
    return b"".join(bodies), coverage


def kernel_times(ctx, fn, n):
    ctx.timing(True)
    base = {k: ctx.kernel_time(k)[0] for k in NAMES}
    for _ in range(n):
        fn()
    ctx.sync()
    ms = {k: round((ctx.kernel_time(k)[0] - base[k]) / n, 4) for k in NAMES}
    ctx.timing(False)
    return ms


def download_probe(nbytes, reps):
    """ms to bring nbytes from the device into pageable and into pinned host memory."""
    import torch

    dev = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    host = {"pageable": torch.empty(nbytes, dtype=torch.uint8), "pinned": torch.empty(nbytes, dtype=torch.uint8).pin_memory()}
    ms = {k: [] for k in host}
    for i in range(reps + 1):
        for k, h in host.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            h.copy_(dev)
            torch.cuda.synchronize()
            if i:
                ms[k].append((time.perf_counter() - t0) * 1e3)
    return {k: round(float(np.median(v)), 3) for k, v in ms.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--symbols", type=int, default=50000)
    ap.add_argument("--sites-per-symbol", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cover_pages_rate.jsonl"))
    a = ap.parse_args()
    ctx = C.Context(0)
    rng = np.random.default_rng(5)
    W = world(a.symbols, a.sites_per_symbol, rng)
    ss, se, sites, off, file, line, func, nfiles, nfuncs = W
    rows = []

    def emit(row):
        rows.append(row)
        print(json.dumps(row), flush=True)

    ctx.timing(True)
    t0 = time.perf_counter()
    table = C.CoverTable(ss, se, sites, sites, off, file, line, func, nfiles, nfuncs, ctx=ctx)
    emit({"metric": "cover_table_build", "sites": int(sites.size), "frames": int(off[-1]), "slots": table.nslots,
          "files": nfiles, "call_ms": round((time.perf_counter() - t0) * 1e3, 2),
          "device_ms": round(ctx.kernel_time("cover_table_build")[0], 3)})
    hot = rng.random(ss.size) < 0.10  # (cover_lines_rate.py's draws, in its order)
    pool = sites[np.repeat(hot, a.sites_per_symbol) & (rng.random(sites.size) < 0.5)]
    covers = [(nq, ((rng.choice(pool, size=nq) + U64(5)) & U64(0xffffffff)).astype(U32)) for nq in (100_000, 1_000_000)]
    srcs, top = sources(file, line, nfiles, np.random.default_rng(6))
    soff = np.zeros(nfiles + 1, dtype=U64)
    soff[1:] = np.cumsum([len(s) for s in srcs])
    raw = np.frombuffer(b"".join(srcs), dtype=np.uint8)
    t0 = time.perf_counter()
    src = C.SourceTable(np.ones(nfiles, dtype=np.uint8), raw, soff, ctx=ctx)
    build_ms = (time.perf_counter() - t0) * 1e3
    flo, nlines, stored, nraw = src.counts()
    emit({"metric": "src_table_build", "files": nfiles, "lines": nlines, "raw_bytes": nraw, "stored_bytes": stored,
          "call_ms": round(build_ms, 2), "device_ms": round(ctx.kernel_time("src_table_build")[0], 3),
          "assumed": "synthetic sources: blocks of 100 C-like lines up to the table's highest line per file"})
    ctx.timing(False)
    del raw
    nl = np.diff(flo.astype(np.int64))
    nbytes = 0
    for nq, drawn in covers:
        for order in ("pc_order", "random"):
            cov = np.sort(drawn) if order == "pc_order" else drawn
            cset = C.SignalSet(ctx)
            C.SignalAdd(cset, cov)
            got = {}

            def fused():
                got["fused"] = C.cover_pages(table, src, cov, BASE)

            def fused_set():
                got["fused_set"] = C.cover_pages(table, src, cset, BASE)

            def chain():
                res = C.cover_lines(table, cov, BASE)
                got["chain"] = host_pages(res[0], res[1], res[2], srcs)

            legs = [fused, fused_set, chain]
            wall_times(legs, a.warmup)
            for k in ("fused", "fused_set"):
                assert got[k][9] is None and got[k][5].size == 0
                assert got[k][7].tobytes() == got["chain"][0], k + " disagrees with the chain"
                assert np.array_equal(got[k][8], got["chain"][1]), k + ": coverage disagrees with the chain"
            med, spread = wall_times(legs, a.reps)
            w = dict(zip(("fused", "fused_set", "chain"), med))
            file_off, lines, covered, _, _, _, body_off, bodies, coverage, _ = got["fused"]
            inrep = np.diff(file_off.astype(np.int64)) > 0
            mark_file = np.repeat(np.arange(nfiles), np.diff(file_off.astype(np.int64)))
            inside = lines.astype(np.int64) <= nl[mark_file]
            ins = int((inside * np.where(covered > 0, 38, 28)).sum())
            nbytes = int(bodies.size)
            moved = (nbytes - ins) + nbytes  # stored bytes of the report's files, read; the bodies, written
            kms = kernel_times(ctx, fused, a.reps)
            emit({"metric": "cover_pages_rate", "queries": nq, "order": order, "distinct": int(len(cset)), "reps": a.reps,
                  "files_out": int(inrep.sum()), "lines_out": int(lines.size), "lines_wrapped": int(inside.sum()),
                  "body_bytes": nbytes, "stored_bytes_read": nbytes - ins, "call_ms": w,
                  "call_ms_min_max": dict(zip(("fused", "fused_set", "chain"), spread)),
                  "fused_over_chain": round(w["fused"] / w["chain"], 4),
                  "fused_set_over_chain": round(w["fused_set"] / w["chain"], 4), "kernel_ms": kms,
                  "copy_floor_ms": round(moved / COPY_RATE * 1e3, 4),
                  "copy_over_floor": round(kms["pages_copy"] / (moved / COPY_RATE * 1e3), 2) if moved else None,
                  "copy_tb_per_s": round(moved / (kms["pages_copy"] * 1e-3) / 1e12, 3) if kms["pages_copy"] else None})
            cset.close()
    emit({"metric": "download_probe", "bytes": nbytes, "ms": download_probe(nbytes, a.reps)})
    src.close()
    table.close()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        for r in rows:
            f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
