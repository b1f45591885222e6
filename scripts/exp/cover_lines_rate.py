#!/usr/bin/env python3
"""Rate of the cover report's line tables, sg_cover_lines / sg_cover_lines_set,
at the C5 size: 50,000 functions of 100 call sites each (5M sites, every site
symbolised), about 1.5 frames per site -- the outermost frame in one of 5,000
source files, inline chains of helpers drawn Zipf(1.2) from 20,000 of them in
500 headers, so a few header lines are shared by thousands of sites (that this
resembles a vmlinux's line table is an ASSUMPTION, not a measurement of one).
Covers of 100k and 1M PCs drawn from the sites of a tenth of the functions, in
PC order and in random order.  One JSON line per cover.  After a warm-up, timed
repetitions alternate three legs on the same input, each timed by a host clock
from the call to its return (every leg ends with its results on the host;
call_ms is the median of the repetitions, call_ms_min_max their range):
  fused      sg_cover_lines on the table
  fused_set  sg_cover_lines_set on a set holding the cover (filled outside the
             window): the distinct PCs in PC order, nothing uploaded
  chain      the route the library had before: sg_cover_uncovered (its tables
             validated and uploaded per call), then fileSet on the host as
             vectorised numpy over the same frame table
The three results are compared.  Then, in a pass of its own, the kernels of the
fused call (sg_ctx_kernel_time).  The first line is the table build."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from syzkaller_amd import cover as C  # noqa: E402

U32, U64 = np.uint32, np.uint64
K, BASE = 0xffffffff81000000, 0xffffffff
NAMES = ("lines_rows", "report_sorted_q", "report_count_q", "report_scatter_q", "report_chunks", "report_sites",
         "lines_cov", "lines_unc", "lines_compact")


def world(nsym, per, rng):
    """(sym_start, sym_end, sites, frame_off, file, line, func, nfiles, nfuncs); tab_pcs = sites."""
    stride = 16 * per + 16
    ss = U64(K) + (stride * np.arange(nsym, dtype=np.int64)).astype(U64)
    se = ss + U64(stride - 1)
    sites = (ss[:, None] + U64(8) + (16 * np.arange(per, dtype=np.int64)).astype(U64)[None, :]).reshape(-1)
    n = sites.size
    r = rng.random(n)
    ninl = np.where(r < 0.70, 0, np.where(r < 0.90, 1, np.where(r < 0.98, 2, 5))).astype(np.int64)
    off = np.zeros(n + 1, dtype=np.int64)
    off[1:] = np.cumsum(ninl + 1)
    nfr = int(off[-1])
    site_of = np.repeat(np.arange(n, dtype=np.int64), ninl + 1)
    outer = np.zeros(nfr, dtype=bool)
    outer[off[1:] - 1] = True
    sym, idx = site_of // per, site_of % per
    ncfiles, nhelp, nhdr = 5000, 20000, 500
    h = (rng.zipf(1.2, size=nfr) - 1) % nhelp
    func = np.where(outer, sym, nsym + h)
    file = np.where(outer, sym % ncfiles, ncfiles + h % nhdr)
    line = np.where(outer, 1 + idx + per * (sym // ncfiles), 10 + h % 50)
    return ss, se, sites, off.astype(U64), file.astype(U32), line.astype(U32), func.astype(U32), ncfiles + nhdr, \
        nsym + nhelp


def host_file_set(cov, unc, W, key):
    """fileSet (cover.go:165-196) over the frame table, vectorised: (file_off, lines, covered)."""
    ss, se, sites, off, file, line, func, nfiles, nfuncs = W
    off = off.astype(np.int64)

    def frames_of(pcs):
        j = np.searchsorted(sites, pcs)
        j = np.unique(j[(j < sites.size) & (sites[np.minimum(j, sites.size - 1)] == pcs)])
        cnt = off[j + 1] - off[j]
        if cnt.sum() == 0:
            return np.zeros(0, dtype=np.int64)
        return np.repeat(off[j] - np.concatenate([[0], np.cumsum(cnt)[:-1]]), cnt) + np.arange(int(cnt.sum()))

    pcs = (U64(BASE << 32) + cov.astype(U64) - U64(5))
    ic, iu = frames_of(pcs), frames_of(unc)
    funcs = np.zeros(nfuncs, dtype=bool)
    funcs[func[ic]] = True
    kc = np.unique(key[ic])
    ku = np.unique(key[iu][funcs[func[iu]]])
    al = np.union1d(kc, ku)
    covered = np.isin(al, kc, assume_unique=True).astype(np.uint8)
    file_off = np.searchsorted(al >> U64(32), np.arange(nfiles + 1, dtype=U64)).astype(U64)
    return file_off, (al & U64(0xffffffff)).astype(U32), covered


def wall_times(legs, n):
    """Per leg the median and the (min, max) ms over n runs, the legs alternated and their order rotated."""
    ms = [[] for _ in legs]
    for i in range(n):
        for k in [(i + j) % len(legs) for j in range(len(legs))]:
            t0 = time.perf_counter()
            legs[k]()
            ms[k].append((time.perf_counter() - t0) * 1e3)
    return [round(float(np.median(x)), 4) for x in ms], [[round(min(x), 4), round(max(x), 4)] for x in ms]


def kernel_times(ctx, fn, n):
    ctx.timing(True)
    base = {k: ctx.kernel_time(k)[0] for k in NAMES}
    for _ in range(n):
        fn()
    ctx.sync()
    ms = {k: round((ctx.kernel_time(k)[0] - base[k]) / n, 4) for k in NAMES}
    ctx.timing(False)
    return ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--symbols", type=int, default=50000)
    ap.add_argument("--sites-per-symbol", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cover_lines_rate.jsonl"))
    a = ap.parse_args()
    ctx = C.Context(0)
    rng = np.random.default_rng(5)
    W = world(a.symbols, a.sites_per_symbol, rng)
    ss, se, sites, off, file, line, func, nfiles, nfuncs = W
    key = (file.astype(U64) << U64(32)) | line.astype(U64)
    rows = []
    ctx.timing(True)
    t0 = time.perf_counter()
    table = C.CoverTable(ss, se, sites, sites, off, file, line, func, nfiles, nfuncs, ctx=ctx)
    build_ms = (time.perf_counter() - t0) * 1e3
    rows.append({"metric": "cover_table_build", "symbols": int(ss.size), "sites": int(sites.size), "frames": int(off[-1]),
                 "slots": table.nslots, "files": nfiles, "funcs": nfuncs, "call_ms": round(build_ms, 2),
                 "device_ms": round(ctx.kernel_time("cover_table_build")[0], 3)})
    ctx.timing(False)
    print(json.dumps(rows[-1]), flush=True)
    hot = rng.random(ss.size) < 0.10
    pool = sites[np.repeat(hot, a.sites_per_symbol) & (rng.random(sites.size) < 0.5)]
    for nq in (100_000, 1_000_000):
        drawn = ((rng.choice(pool, size=nq) + U64(5)) & U64(0xffffffff)).astype(U32)
        for order in ("pc_order", "random"):
            cov = np.sort(drawn) if order == "pc_order" else drawn
            cset = C.SignalSet(ctx)
            C.SignalAdd(cset, cov)
            got = {}

            def fused():
                got["fused"] = C.cover_lines(table, cov, BASE)

            def fused_set():
                got["fused_set"] = C.cover_lines(table, cset, BASE)

            def chain():
                unc = C.cover_uncovered(cov, BASE, ss, se, sites, ctx=ctx)
                got["unc"] = unc.size
                got["chain"] = host_file_set(cov, unc, W, key)

            legs = [fused, fused_set, chain]
            wall_times(legs, a.warmup)
            for k in ("fused", "fused_set"):
                for x, y in zip(got[k][:3], got["chain"]):
                    assert np.array_equal(x, y), k + " disagrees with the chain"
                assert got[k][5].size == 0
            med, spread = wall_times(legs, a.reps)
            w = dict(zip(("fused", "fused_set", "chain"), med))
            res = {"metric": "cover_lines_rate", "queries": nq, "order": order, "distinct": int(len(cset)), "reps": a.reps,
                   "uncovered_pcs": got["unc"], "lines_out": int(got["fused"][1].size),
                   "covered_frames": int(got["fused"][4]), "call_ms": w,
                   "call_ms_min_max": dict(zip(("fused", "fused_set", "chain"), spread)),
                   "fused_over_chain": round(w["fused"] / w["chain"], 4),
                   "fused_set_over_chain": round(w["fused_set"] / w["chain"], 4),
                   "kernel_ms": kernel_times(ctx, fused, a.reps)}
            rows.append(res)
            print(json.dumps(res), flush=True)
            cset.close()
    table.close()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        for r in rows:
            f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
