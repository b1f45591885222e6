#!/usr/bin/env python3
"""Rate of sg_exec_cover_dev (dedup = 1) on KCOV buffers of the size a fuzzer
produces: 4,096 programs x 8 calls x 2,048 PCs, built on the device.  Two
inputs, one JSON line each:
  zipf      sg_gen_zipf_traces_dev (Zipf 1.1 over 2^20 ranks, the benchmark's
            traces) widened to u64 with the high word 0xffffffff: the
            "loop-like" end, where repeats dominate.  That Zipf traces resemble
            real triage buffers is an ASSUMPTION, not a measurement of them;
  distinct  every PC of a call distinct.
Each line states the repeat ratio 1 - cover / PCs that its input has.  After a
warm-up, timed repetitions run the auto path (every call on the fast shapes
here) and then, on the same input, the general path for every call (option
exec_cover_path = 0).  Per path: the mean device time of the whole call (HIP
events around it) and of its kernels (sg_ctx_kernel_time: exec_cover_call,
exec_cover_general, exec_cover_emit), the algorithmic bytes (8 B per PC in, 4 B
per PC out, as the issue counts them) and the fraction of the 8 TB/s HBM peak
they make over the whole call.

A last line measures the fused triage call, sg_triage_runs_from_kcov_dev, on
4,096 candidates x 3 runs x 4 calls x 1,024 PCs: each candidate's runs are one
Zipf program with 2 % of the PCs of every run redrawn (flaky coverage),
inp.signal is the signal of its call in run 0, and a third of that signal is
already in the corpus.  Alternated in one process with the same work as
separate calls: sg_exec_signal_dev and sg_exec_cover_dev on the device, their
lists copied to the host, then sg_triage_newsig, sg_triage_intersect per run
and sg_merge_batch(SG_OP_UNION) per run on host arrays (the only forms those
three have), with the glue between them vectorised in numpy.  The outputs are
checked equal.  Reported: the HIP-event mean of the fused call, the wall-clock
means of both, and their ratio."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

import time  # noqa: E402

import numpy as np  # noqa: E402
import torch  # noqa: E402

from syzkaller_amd._lib import call  # noqa: E402
from syzkaller_amd._lib import P32, P64  # noqa: E402
from syzkaller_amd.cover import Context, SignalSet  # noqa: E402

HBM_PEAK = 8.0e12
NAMES = ("exec_cover_call", "exec_cover_general", "exec_cover_emit")
UNIVERSE_SEED = 7


def build(ctx, kind, P, C, M, seed):
    dev = "cuda"
    if kind == "zipf":
        lo = torch.empty(P * C * M, dtype=torch.int32, device=dev)
        call("sg_gen_zipf_traces_dev", ctx.h, UNIVERSE_SEED, seed, 1.1, 1 << 20, 0, P, C, M, lo.data_ptr())
        ctx.sync()
        return (lo.to(torch.int64) & 0xFFFFFFFF) | (-1 << 32)  # the high word 0xffffffff
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    # distinct: a permutation of 0 .. M - 1 per call, scattered over 64 bits by an odd multiplier
    perm = torch.argsort(torch.rand((P * C, M), device=dev, generator=g), dim=1)
    return (perm * -0x61C8864680B583EB).reshape(-1).contiguous()


def run(ctx, kind, P, C, M, warmup, reps, general_reps):
    ncall, npcs = P * C, P * C * M
    dev = "cuda"
    pcs = build(ctx, kind, P, C, M, 1)
    call_off = torch.arange(ncall + 1, device=dev, dtype=torch.int64) * M
    cov_off = torch.empty(ncall + 1, dtype=torch.int64, device=dev)
    cov = torch.empty(npcs, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()

    def one():
        call("sg_exec_cover_dev", ctx.h, pcs.data_ptr(), call_off.data_ptr(), ncall, npcs, 1, cov_off.data_ptr(),
             cov.data_ptr(), npcs)

    res = {"metric": "exec_cover_rate", "input": kind, "programs": P, "calls": C, "pcs_per_call": M, "pcs": npcs}
    ref = None
    for path, n in ((-1, reps), (0, general_reps)):
        if n <= 0:
            continue
        ctx.set_option("exec_cover_path", path)
        for _ in range(warmup):
            one()
        ctx.sync()
        ncov, general = int(cov_off[-1]), ctx.counter("exec_cover_general")
        sums = (int(cov_off.sum()), int(cov[:ncov].to(torch.int64).sum()))
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
        nbytes = 8 * npcs + 4 * npcs
        res.update({"cover": ncov, "repeat_ratio": round(1 - ncov / npcs, 4), "algorithmic_bytes": nbytes})
        res["auto" if path < 0 else "general"] = {
            "reps": n, "calls_on_general_path": general, "call_ms": round(total, 4), "kernel_ms": ms,
            "hbm_fraction": round(nbytes / (total * 1e-3) / HBM_PEAK, 4)}
    ctx.set_option("exec_cover_path", -1)
    print(json.dumps(res), flush=True)


def _np64(t):
    return t.cpu().numpy().view(np.uint64)


def _np32(t):
    return t.cpu().numpy().view(np.uint32)


def _gather(vals, off, idx):
    """The CSR of segments idx of (vals, off), vectorised."""
    lens = (off[idx + 1] - off[idx]).astype(np.int64)
    out_off = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    src = np.repeat(off[idx].astype(np.int64) - out_off[:-1].astype(np.int64), lens) + np.arange(int(out_off[-1]))
    return vals[src], out_off


def run_fused(ctx, n, R, C, M, warmup, reps):
    dev = "cuda"
    nexec, ncalls, npcs = n * R, n * R * C, n * R * C * M
    base = build(ctx, "zipf", n, C, M, 11).reshape(n, 1, C * M)
    other = build(ctx, "zipf", n * R, C, M, 12).reshape(n, R, C * M)
    g = torch.Generator(device=dev)
    g.manual_seed(13)
    noise = torch.rand((n, R, C * M), device=dev, generator=g) < 0.02
    pcs = torch.where(noise, other, base.expand(n, R, C * M)).reshape(-1).contiguous()
    del other, noise
    call_off = torch.arange(ncalls + 1, device=dev, dtype=torch.int64) * M
    prog_off = torch.arange(nexec + 1, device=dev, dtype=torch.int64) * C
    call_idx = (torch.arange(n, device=dev, dtype=torch.int32) % C).contiguous()
    minimized = torch.zeros(n, dtype=torch.uint8, device=dev)
    h_prog_off, h_call = _np64(prog_off), call_idx.cpu().numpy().astype(np.int64)
    # the separate device calls' outputs
    pcs32 = torch.empty(npcs, dtype=torch.int32, device=dev)
    t_sig, t_sig_off = torch.empty(npcs, dtype=torch.int32, device=dev), torch.empty(ncalls + 1, dtype=torch.int64, device=dev)
    t_cov, t_cov_off = torch.empty(npcs, dtype=torch.int32, device=dev), torch.empty(ncalls + 1, dtype=torch.int64, device=dev)

    def device_lists():
        pcs32.copy_(pcs)  # (uint32_t)pc: the low word
        call("sg_exec_signal_dev", ctx.h, pcs32.data_ptr(), call_off.data_ptr(), prog_off.data_ptr(), nexec, ncalls, npcs,
             t_sig.data_ptr(), t_sig_off.data_ptr())
        call("sg_exec_cover_dev", ctx.h, pcs.data_ptr(), call_off.data_ptr(), ncalls, npcs, 1, t_cov_off.data_ptr(),
             t_cov.data_ptr(), npcs)
        ctx.sync()
        so, co = _np64(t_sig_off), _np64(t_cov_off)
        return _np32(t_sig[: int(so[-1])]), so, _np32(t_cov[: int(co[-1])]), co

    # inp.signal: the call's signal in run 0; a third of it goes into the corpus
    sig, so, _, _ = device_lists()
    first = h_prog_off[np.arange(n) * R].astype(np.int64) + h_call
    inp_sig, inp_off = _gather(sig, so, first)
    corpus = SignalSet(ctx)
    seen = np.ascontiguousarray(inp_sig[::3])
    call("sg_set_add", corpus.h, seen.ctypes.data_as(P32), seen.size)
    nsig = int(inp_off[-1])
    d_sig = torch.from_numpy(inp_sig.view(np.int32).copy()).to(dev)
    d_sig_off = torch.from_numpy(inp_off.view(np.int64).copy()).to(dev)
    status = torch.empty(n, dtype=torch.int32, device=dev)
    new_off, cov_off = torch.empty(n + 1, dtype=torch.int64, device=dev), torch.empty(n + 1, dtype=torch.int64, device=dev)
    new_vals, cov_vals = torch.empty(nsig, dtype=torch.int32, device=dev), torch.empty(npcs, dtype=torch.int32, device=dev)

    def fused():
        call("sg_triage_runs_from_kcov_dev", ctx.h, corpus.h, d_sig.data_ptr(), d_sig_off.data_ptr(), n, nsig,
             call_idx.data_ptr(), minimized.data_ptr(), R, pcs.data_ptr(), call_off.data_ptr(), prog_off.data_ptr(), ncalls,
             npcs, status.data_ptr(), new_off.data_ptr(), new_vals.data_ptr(), nsig, cov_off.data_ptr(),
             cov_vals.data_ptr(), npcs)

    def chained():
        sig, so, cov, co = device_lists()
        nv, no = np.empty(max(nsig, 1), np.uint32), np.zeros(n + 1, np.uint64)
        call("sg_triage_newsig", ctx.h, corpus.h, inp_sig.ctypes.data_as(P32), inp_off.ctypes.data_as(P64), n,
             nv.ctypes.data_as(P32), no.ctypes.data_as(P64))
        nv = np.ascontiguousarray(nv[: int(no[-1])])
        had = np.diff(no.astype(np.int64)) > 0
        cover = cover_off = None
        for i in range(R):
            c = h_prog_off[np.arange(n) * R + i].astype(np.int64) + h_call
            rv, ro = _gather(sig, so, c)
            rv = np.ascontiguousarray(rv)
            lens = np.zeros(n, np.uint64)
            call("sg_triage_intersect", ctx.h, nv.ctypes.data_as(P32), no.ctypes.data_as(P64), rv.ctypes.data_as(P32),
                 ro.ctypes.data_as(P64), n, lens.ctypes.data_as(P64))
            keep = np.repeat(no[:-1].astype(np.int64), lens.astype(np.int64))
            new_o = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
            keep += np.arange(int(new_o[-1])) - np.repeat(new_o[:-1].astype(np.int64), lens.astype(np.int64))
            nv, no = np.ascontiguousarray(nv[keep]), new_o
            cv, cvo = _gather(cov, co, c)
            cv = np.ascontiguousarray(cv)
            if cover is None:
                cover, cover_off = cv, cvo
                continue
            al, bl = np.diff(cover_off.astype(np.int64)).astype(np.uint64), np.diff(cvo.astype(np.int64)).astype(np.uint64)
            ob = np.concatenate([[0], np.cumsum(al + bl)]).astype(np.uint64)
            out, ol = np.empty(max(int(ob[-1]), 1), np.uint32), np.zeros(n, np.uint64)
            ab, bb = np.ascontiguousarray(cover_off[:-1]), np.ascontiguousarray(cvo[:-1])
            call("sg_merge_batch", ctx.h, 2, cover.ctypes.data_as(P32), cover.size, ab.ctypes.data_as(P64),
                 al.ctypes.data_as(P64), cv.ctypes.data_as(P32), cv.size, bb.ctypes.data_as(P64), bl.ctypes.data_as(P64), n,
                 out.ctypes.data_as(P32), out.size, ob.ctypes.data_as(P64), ol.ctypes.data_as(P64))
            # pack the merged lists: pair k's result is out[ob[k] : ob[k] + ol[k])
            lens64 = ol.astype(np.int64)
            c_off = np.concatenate([[0], np.cumsum(lens64)]).astype(np.uint64)
            src = np.repeat(ob[:-1].astype(np.int64) - c_off[:-1].astype(np.int64), lens64) + np.arange(int(c_off[-1]))
            cover, cover_off = np.ascontiguousarray(out[src]), c_off
        left = np.diff(no.astype(np.int64)) > 0
        st = np.where(~had, 1, np.where(left, 0, 3)).astype(np.int32)  # SG_TIN_NO_NEW / SG_TIN_OK / SG_TIN_FLAKY
        return st, nv, no, cover, cover_off

    for _ in range(warmup):
        fused()
        chained()
    ctx.sync()
    # the outputs agree
    st, nv, no, cover, cover_off = chained()
    fused()
    ctx.sync()
    f_st, f_no, f_co = status.cpu().numpy(), _np64(new_off), _np64(cov_off)
    f_nv, f_cv = _np32(new_vals[: int(f_no[-1])]), _np32(cov_vals[: int(f_co[-1])])
    assert np.array_equal(f_st, st), "statuses differ"
    ok = np.flatnonzero(st == 0)
    assert np.array_equal(f_nv, nv), "newSignal differs"  # (a candidate that is not OK has an empty list on both sides)
    e_cv, e_co = _gather(cover, cover_off, ok)
    g_cv, g_co = _gather(f_cv, f_co, ok)
    assert np.array_equal(e_cv, g_cv) and np.array_equal(e_co, g_co), "inputCover differs"
    assert int(f_co[-1]) == int(g_co[-1])
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    names = ("exec_signal", "exec_cover_call", "exec_cover_emit", "tinput_diff", "triage_runs_round", "triage_runs_cover")
    t_fused = t_chain = 0.0
    kms = {k: 0.0 for k in names}
    for a, b in ev:  # alternated
        ctx.timing(True)
        t0 = time.perf_counter()
        a.record()
        fused()
        b.record()
        ctx.sync()
        t_fused += time.perf_counter() - t0
        for k in names:
            kms[k] += ctx.kernel_time(k)[0]
        ctx.timing(False)
        t0 = time.perf_counter()
        chained()
        t_chain += time.perf_counter() - t0
    torch.cuda.synchronize()
    res = {"metric": "triage_runs_rate", "candidates": n, "runs": R, "calls": C, "pcs_per_call": M, "pcs": npcs,
           "inp_signal": nsig, "status_counts": np.bincount(st, minlength=4).tolist(),
           "new_signal": int(f_no[-1]), "input_cover": int(f_co[-1]), "wide": ctx.counter("triage_runs_wide"),
           "fused": {"reps": reps, "event_ms": round(sum(a.elapsed_time(b) for a, b in ev) / reps, 4),
                     "wall_ms": round(1e3 * t_fused / reps, 4), "kernel_ms": {k: round(v / reps, 4) for k, v in kms.items()}},
           "chained": {"reps": reps, "wall_ms": round(1e3 * t_chain / reps, 4)},
           "chained_over_fused_wall": round(t_chain / t_fused, 2)}
    print(json.dumps(res), flush=True)
    corpus.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--programs", type=int, default=4096)
    ap.add_argument("--calls", type=int, default=8)
    ap.add_argument("--pcs", type=int, default=2048)
    ap.add_argument("--inputs", default="zipf,distinct,fused")
    ap.add_argument("--candidates", type=int, default=4096)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--general-reps", type=int, default=10)
    a = ap.parse_args()
    torch.cuda.set_device(0)
    ctx = Context(0)
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    for kind in a.inputs.split(","):
        if kind == "fused":
            run_fused(ctx, a.candidates, 3, 4, 1024, a.warmup, a.reps)
        else:
            run(ctx, kind, a.programs, a.calls, a.pcs, a.warmup, a.reps, a.general_reps)


if __name__ == "__main__":
    main()
