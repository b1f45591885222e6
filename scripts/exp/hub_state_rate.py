#!/usr/bin/env python3
"""Rate of the hub's corpus on the GPU: sg_call_sets, sg_call_sets_dev, sg_hubcorpus_add / _pending / _purge and a
full HubState.Sync, on --programs synthetic program texts.  A text is 1..30 lines `rN = name$variant(0x...,
&(0x...)=...)` with names from a 4,096-name dictionary; its length follows the lognormal of
scripts/exp/prog_hashes_rate.py (median --median bytes, sigma --sigma, clipped to [16 B, 64 KiB]).  That is an
ASSUMPTION: the reference publishes no corpus.  Setting: 8 managers whose call masks differ (manager m lacks the
names with id % 16 == m), each holding a random half of the corpus.  One JSON line.

Legs, after a warm-up, medians of --reps repetitions, host clock from call to return:
  call_sets        sg_call_sets: texts and offsets in, statuses, line offsets, spans and ids out
  call_sets_dev    sg_call_sets_dev on device-resident texts, then a context sync
  add              sg_hubcorpus_add of the whole corpus into an empty corpus (a fresh one per repetition, made
                   outside the clock; the dictionary already holds the names)
  pending_seq0     sg_hubcorpus_pending for a manager at seq 0
  pending_caught   ... for a manager whose seq is the hub's
  purge            sg_hubcorpus_purge with the 8 managers' sets (the corpus is rebuilt outside the clock)
  sync             HubState.Sync with 1 % of the corpus added and 1 % of the manager's deleted (Python included)
Baseline: tests/hub_state_oracle.py on this machine's CPU -- Python, one thread, NOT Go; its pending and purge
walk dicts of parsed records (it does not re-parse the texts as state.go:277 does, which favours it).  Every GPU
result of the run is compared with the baseline's.  With --scan-only the script only repeats sg_call_sets_dev:
that is the run to put under a kernel trace."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from syzkaller_amd import _lib  # noqa: E402
from syzkaller_amd import cover as C  # noqa: E402
from syzkaller_amd import hub as H  # noqa: E402
from syzkaller_amd.corpus import SigSet, texts_csr  # noqa: E402
from syzkaller_amd.cover import _p8, _p32, _p64  # noqa: E402
from tests import hub_state_oracle as OR  # noqa: E402

U8, U32, U64 = np.uint8, np.uint32, np.uint64
KERNELS = ("call_set_tiles", "call_set_scan", "call_set_status", "call_set_emit", "name_lookup", "scan")
READ_RATE = 6.2e12  # bytes/s: the streaming read rate DESIGN 8 records


def wall(fn, n, before=None):
    ms = []
    for _ in range(n):
        if before:
            before()
        t0 = time.perf_counter()
        fn()
        ms.append((time.perf_counter() - t0) * 1e3)
    return round(float(np.median(ms)), 3), [round(min(ms), 3), round(max(ms), 3)]


def make_names(n=4096):
    return [b"call%d$v%d" % (k // 8, k % 8) for k in range(n)]


def make_corpus(n, names, median, sigma, seed, tag=b""):
    """n distinct program texts."""
    rng = np.random.default_rng(seed)
    lens = np.clip(rng.lognormal(np.log(median), sigma, size=n), 16, 65536).astype(np.int64)
    ncalls = rng.integers(1, 31, size=n)
    pick = rng.integers(0, len(names), size=int(ncalls.sum()))  # (more than the lines: short programs have fewer)
    pad = b"0x0, " * 14000
    progs, at = [], 0
    for k in range(n):
        c = min(int(ncalls[k]), max(1, int(lens[k]) // 48))  # (a line is 40 bytes at least)
        per = max(int(lens[k]) // c - 40, 0)
        lines = [b"r%d = %s(0x%x, &(0x7f0000%06x)=%s0x1)" % (j, names[pick[at + j]], k, j, pad[:per - per % 5])
                 for j in range(c)]
        at += c
        progs.append(b"\n".join(lines) + b"\n" + tag)
    return progs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--programs", type=int, default=500000)
    ap.add_argument("--median", type=float, default=512.0)
    ap.add_argument("--sigma", type=float, default=1.0)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--scan-only", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hub_state_rate.jsonl"))
    a = ap.parse_args()
    import torch

    ctx = C.Context(0)
    n, nm = a.programs, 8
    names = make_names()
    progs = make_corpus(n, names, a.median, a.sigma, 7)
    b, off = texts_csr(progs)
    nbytes = int(off[-1])
    table = H.NameTable(ctx)
    table.add(names)
    cap = int(np.count_nonzero(b == 0x28))
    d_b, d_off = torch.from_numpy(b).to("cuda"), torch.from_numpy(off.view(np.int64)).to("cuda")
    d_st = torch.empty(n, dtype=torch.uint8, device="cuda")
    d_lo = torch.empty(n + 1, dtype=torch.int64, device="cuda")
    d_pos = torch.empty(cap, dtype=torch.int64, device="cuda")
    d_len, d_id = torch.empty(cap, dtype=torch.int32, device="cuda"), torch.empty(cap, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()

    def call_sets_dev():
        _lib.call("sg_call_sets_dev", ctx.h, table.h, d_b.data_ptr(), d_off.data_ptr(), n, nbytes, d_st.data_ptr(),
                  d_lo.data_ptr(), d_pos.data_ptr(), d_len.data_ptr(), d_id.data_ptr(), cap)
        ctx.sync()

    if a.scan_only:
        wall(call_sets_dev, a.warmup + a.reps)
        print(json.dumps({"scan_only": True, "programs": n, "bytes": nbytes}))
        return

    st, lo = np.zeros(n, U8), np.zeros(n + 1, U64)
    pos, ln, ids = np.zeros(cap, U64), np.zeros(cap, U32), np.zeros(cap, U32)
    nl = _lib.c_size_t()

    def call_sets():
        _lib.call("sg_call_sets", ctx.h, table.h, _p8(b), _p64(off), n, _p8(st), _p64(lo), _p64(pos), _p32(ln), _p32(ids),
                  cap, _lib.ctypes.byref(nl))

    # ---- the baseline, and the state both sides start from -------------------------
    base_ms = {}
    t0 = time.perf_counter()
    est, elo, epos, eln, enames = OR.call_sets(progs)
    base_ms["call_sets"] = base_ms["call_sets_dev"] = round((time.perf_counter() - t0) * 1e3, 1)
    otab = OR.ONameTable()
    otab.add(names)
    ocorpus = OR.OHubCorpus(otab)
    t0 = time.perf_counter()
    seqs = (1 + np.arange(n) // 1000).astype(U64)  # a thousand programs per sync of the hub's past
    hub_seq = int(seqs.max())
    _, enew, ekeys = ocorpus.add(progs, seqs.tolist())
    base_ms["add"] = round((time.perf_counter() - t0) * 1e3, 1)
    assert enew.all(), "the corpus' programs are distinct"
    rng = np.random.default_rng(11)
    halves = [np.sort(rng.choice(n, size=n // 2, replace=False)) for _ in range(nm)]
    calls = [[x for i, x in enumerate(names) if i % 16 != m] for m in range(nm)]
    osets = []
    for m in range(nm):
        s = OR.OSet()
        s.m = {ekeys[k].tobytes(): True for k in halves[m]}
        osets.append(s)
    sets = [SigSet(n, ctx=ctx) for _ in range(nm)]
    for s, h in zip(sets, halves):
        assert s.add_new(ekeys[h]).all()
    masks = [table.mask(c) for c in calls]

    corpus = [None]

    def fresh_corpus():
        if corpus[0] is not None:
            corpus[0].close()
        corpus[0] = H.HubCorpus(table)

    is_new, sigs, nunk = np.zeros(n, U8), np.zeros((n, 20), U8), _lib.c_size_t()

    def add():
        _lib.call("sg_hubcorpus_add", corpus[0].h, None, _p8(b), _p64(off), n, _p64(seqs), _p8(st), _p8(is_new), _p8(sigs),
                  None, None, 0, _lib.ctypes.byref(nunk))

    def refill():
        fresh_corpus()
        add()

    out_s, out_q = np.zeros((n, 20), U8), np.zeros(n, U64)
    pn, pmax, pmore = _lib.c_size_t(), _lib.c_uint64(), _lib.c_uint64()

    def pending(mgr_seq):
        _lib.call("sg_hubcorpus_pending", corpus[0].h, sets[0].h, mgr_seq, hub_seq, _p64(masks[0]), masks[0].size, 1000,
                  _p8(out_s), _p64(out_q), n, _lib.ctypes.byref(pn), _lib.ctypes.byref(pmax), _lib.ctypes.byref(pmore))

    dels, nd = np.zeros((n, 20), U8), _lib.c_size_t()
    arr = (_lib.c_void_p * nm)(*[s.h.value for s in sets])

    def purge():
        _lib.call("sg_hubcorpus_purge", corpus[0].h, arr, nm, _p8(dels), n, _lib.ctypes.byref(nd))

    w, spread = {}, {}
    wall(call_sets, a.warmup)
    assert nl.value == int(elo[-1]) and np.array_equal(st, est) and np.array_equal(lo, elo), "sg_call_sets: statuses"
    assert np.array_equal(pos[:nl.value], epos) and np.array_equal(ln[:nl.value], eln), "sg_call_sets: spans"
    assert ids[:nl.value].tolist() == [otab.ids[x] for x in enames], "sg_call_sets: ids"
    w["call_sets"], spread["call_sets"] = wall(call_sets, a.reps)
    wall(call_sets_dev, a.warmup)
    assert np.array_equal(d_st.cpu().numpy(), est) and np.array_equal(d_lo.cpu().numpy().view(U64), elo)
    assert np.array_equal(d_pos.cpu().numpy().view(U64)[:nl.value], epos)
    assert np.array_equal(d_id.cpu().numpy().view(U32)[:nl.value], ids[:nl.value]), "sg_call_sets_dev"
    w["call_sets_dev"], spread["call_sets_dev"] = wall(call_sets_dev, a.reps)
    wall(add, a.warmup, fresh_corpus)
    assert nunk.value == 0 and is_new.all() and np.array_equal(sigs, ekeys)
    for g, e in zip(corpus[0].export(), ocorpus.export()):
        assert np.array_equal(g, e), "sg_hubcorpus_add: the records"
    w["add"], spread["add"] = wall(add, a.reps, fresh_corpus)
    omask = otab.mask(calls[0])
    for leg, mgr_seq in (("pending_seq0", 0), ("pending_caught", hub_seq)):
        t0 = time.perf_counter()
        ekeys_p, eseqs_p, emax, emore = ocorpus.pending(osets[0], mgr_seq, hub_seq, omask, 1000)
        base_ms[leg] = round((time.perf_counter() - t0) * 1e3, 1)
        wall(lambda: pending(mgr_seq), a.warmup)
        assert (pn.value, pmax.value, pmore.value) == (len(ekeys_p), emax, emore), leg
        assert out_s[:pn.value].tobytes() == b"".join(ekeys_p), leg
        w[leg], spread[leg] = wall(lambda: pending(mgr_seq), a.reps)
    pending(0)
    sel0 = {"kept": pn.value, "more": pmore.value}
    t0 = time.perf_counter()
    edels = ocorpus.purge(osets)
    base_ms["purge"] = round((time.perf_counter() - t0) * 1e3, 1)
    wall(purge, a.warmup, refill)
    assert dels[:nd.value].tobytes() == b"".join(edels), "sg_hubcorpus_purge"
    for g, e in zip(corpus[0].export(), ocorpus.export()):
        assert np.array_equal(g, e), "sg_hubcorpus_purge: the records"
    w["purge"], spread["purge"] = wall(purge, a.reps, refill)
    purged = nd.value
    corpus[0].close()
    for s in sets:
        s.close()

    # ---- a full Sync: both states built directly (Connect would parse every half again) ----
    hs, ohs = H.HubState(ctx), OR.OHubState()
    hs.table.add(names)
    ohs.table.add(names)
    hs.corpusSeq = ohs.corpusSeq = hub_seq
    hs.Corpus.add(csr=(b, off), seqs=seqs)
    ohs.Corpus.add(progs, seqs.tolist())
    hs.texts = {ekeys[k].tobytes(): progs[k] for k in range(n)}
    ohs.texts = dict(hs.texts)
    for m in range(nm):
        mg, og = H._Manager("m%d" % m, ctx), OR._OManager()
        mg.Connected = og.Connected = True
        mg.Calls, og.Calls = set(calls[m]), set(calls[m])
        mg.Corpus.add_new(ekeys[halves[m]])
        og.Corpus.m = {ekeys[k].tobytes(): True for k in halves[m]}
        hs.Managers["m%d" % m], ohs.Managers["m%d" % m] = mg, og
    hs.purgeCorpus()
    ohs.purgeCorpus()
    nsync = a.warmup + a.reps
    fresh = make_corpus(nsync * (n // 100), names, a.median, a.sigma, 99, tag=b"# new\n")
    sync_ms, base_sync = [], []
    for r in range(nsync):
        name = "m%d" % (r % nm)
        add_r = fresh[r * (n // 100):(r + 1) * (n // 100)]
        held = list(ohs.Managers[name].Corpus.m)
        del_r = [held[i].hex() for i in rng.choice(len(held), size=n // 100, replace=False)]
        t0 = time.perf_counter()
        got = hs.Sync(name, add_r, del_r)
        sync_ms.append((time.perf_counter() - t0) * 1e3)
        t0 = time.perf_counter()
        exp = ohs.Sync(name, add_r, del_r)
        base_sync.append((time.perf_counter() - t0) * 1e3)
        assert got == exp, "HubState.Sync"
        assert hs.Corpus.count() == len(ohs.Corpus.recs) and hs.texts.keys() == ohs.texts.keys()
    for g, e in zip(hs.Corpus.export(), ohs.Corpus.export()):
        assert np.array_equal(g, e), "HubState: the records"
    w["sync"] = round(float(np.median(sync_ms[a.warmup:])), 3)
    spread["sync"] = [round(min(sync_ms[a.warmup:]), 3), round(max(sync_ms[a.warmup:]), 3)]
    base_ms["sync"] = round(float(np.median(base_sync[a.warmup:])), 1)
    hs.close()

    # ---- the scan's kernels, timed by events in a pass of their own ----
    ctx.timing(True)
    ctx.sync()
    t0 = {k: ctx.kernel_time(k)[0] for k in KERNELS}
    for _ in range(a.reps):
        call_sets_dev()
    kern = {k: round((ctx.kernel_time(k)[0] - t0[k]) / a.reps, 4) for k in KERNELS}
    ctx.timing(False)
    floor_ms = nbytes / READ_RATE * 1e3
    res = {"metric": "hub_state_rate", "programs": n, "bytes": nbytes, "call_lines": int(elo[-1]), "names": len(names),
           "managers": nm, "length_median_assumed": a.median, "length_sigma": a.sigma, "reps": a.reps,
           "baseline": "tests/hub_state_oracle.py (Python, one CPU thread, dicts of parsed records; not Go)",
           "call_ms": w, "call_ms_min_max": spread, "baseline_ms": base_ms,
           "over_baseline": {k: round(w[k] / base_ms[k], 5) for k in w if base_ms.get(k)},
           "pending_seq0": sel0, "purged": purged, "call_sets_dev_kernel_ms": kern,
           "scan_read_floor_ms": round(floor_ms, 4),
           "scan_fraction_of_read_floor": round(floor_ms / kern["call_set_scan"], 4) if kern["call_set_scan"] else None}
    print(json.dumps(res), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(json.dumps(res) + "\n")


if __name__ == "__main__":
    main()
