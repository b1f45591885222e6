"""TEST INFRASTRUCTURE ONLY: the checker of sg_triage_runs_from_kcov.

triageInput (syz-fuzzer/fuzzer.go:521-576) restated, one statement per
reference step, composed from oracle.pyoracle (exec_signal, signal_diff,
canonicalize, and foreach, which is the literal two-pointer loop, so wide PCs
are exact too) and tests/exec_cover_oracle.py (the cover branch).
"""
import numpy as np

from oracle import pyoracle as O
from tests import exec_cover_oracle as XC

U32, U64 = np.uint32, np.uint64
OK, NO_NEW, NOT_EXECUTED, FLAKY = 0, 1, 2, 3
EMPTY = np.zeros(0, dtype=U32)


def run_info(run, call):
    """execute1 with FlagCollectCover | FlagDedupCover for one execution: run is
    the list of its calls' KCOV buffers (u64 PCs).  Returns None when
    info[call] does not exist, else (info[call].Signal, info[call].Cover)."""
    if len(run) <= call:
        return None
    calls = [np.asarray(c, dtype=U64).reshape(-1) for c in run[: call + 1]]  # (later calls cannot change this one)
    call_off = np.concatenate([[0], np.cumsum([c.size for c in calls])]).astype(U64)
    pcs32 = (np.concatenate(calls) & U64(0xFFFFFFFF)).astype(U32)           # executor.h:394 (uint32_t)cover_data[i]
    sig, so = O.exec_signal(pcs32, call_off, [0, len(calls)])                # :389-401, a fresh table per execution
    signal = sig[int(so[call]):int(so[call + 1])]
    cover = XC.call_cover(calls[call], dedup=True)                           # :402-415
    return signal, cover


def triage_input(corpus, signal, call, runs, minimized):
    """One candidate: (status, newSignal, inputCover); corpus is an O.OSet."""
    new = O.signal_diff(corpus, signal)                                      # fuzzer.go:527
    if len(new) == 0:                                                        # :529-531
        return NO_NEW, EMPTY, EMPTY
    a, n = O.canonicalize(new)                                               # :532
    new = a[:n]
    cover = EMPTY                                                            # :539
    if minimized:                                                            # :543
        for run in runs:                                                     # :545
            info = run_info(run, call)
            if info is None or len(info[1]) == 0:                            # :547-549
                continue
            cover = info[1].copy()                                           # :550
            break                                                            # :551
        return OK, new, cover
    notexecuted = False                                                      # :555
    for run in runs:                                                         # :556
        info = run_info(run, call)
        if info is None or len(info[0]) == 0:                                # :558
            if notexecuted:                                                  # :560-562
                return NOT_EXECUTED, EMPTY, EMPTY
            notexecuted = True                                               # :563
            continue
        sig, cov = info
        c, m = O.canonicalize(sig)
        new = O.foreach(O.INTER, new, c[:m])                                 # :567
        if len(new) == 0:                                                    # :568-570
            return FLAKY, EMPTY, EMPTY
        if len(cover) == 0:                                                  # :571
            cover = cov.copy()                                               # :572
        else:
            cover = O.foreach(O.UNION, cover, cov)                           # :574
    return OK, new, cover


def batch(corpus, cands):
    """cands: a list of (signal, call, runs, minimized).  Returns (status,
    new_vals, new_off, cov_vals, cov_off) as sg_triage_runs_from_kcov."""
    res = [triage_input(corpus, *c) for c in cands]
    status = np.array([r[0] for r in res], dtype=np.int32)
    news, covs = [r[1] for r in res], [r[2] for r in res]
    new_off = np.concatenate([[0], np.cumsum([len(x) for x in news])]).astype(U64)
    cov_off = np.concatenate([[0], np.cumsum([len(x) for x in covs])]).astype(U64)
    new_vals = np.concatenate(news).astype(U32) if news else EMPTY
    cov_vals = np.concatenate(covs).astype(U32) if covs else EMPTY
    return status, new_vals, new_off, cov_vals, cov_off


def to_arrays(cands):
    """The flat arguments of sg_triage_runs_from_kcov for cands (every candidate
    with the same number of runs): sig_vals, sig_off, call, minimized, nruns,
    pcs, call_off, prog_off."""
    nruns = len(cands[0][2]) if cands else 3
    assert all(len(c[2]) == nruns for c in cands)
    sigs = [np.asarray(c[0], dtype=U32).reshape(-1) for c in cands]
    sig_off = np.concatenate([[0], np.cumsum([s.size for s in sigs])]).astype(U64)
    calls = [np.asarray(x, dtype=U64).reshape(-1) for c in cands for r in c[2] for x in r]
    prog_off = np.concatenate([[0], np.cumsum([len(r) for c in cands for r in c[2]])]).astype(U64)
    call_off = np.concatenate([[0], np.cumsum([x.size for x in calls])]).astype(U64)
    return (np.concatenate(sigs) if sigs else EMPTY, sig_off, np.array([c[1] for c in cands], dtype=U32),
            np.array([1 if c[3] else 0 for c in cands], dtype=np.uint8), nruns,
            np.concatenate(calls) if calls else np.zeros(0, dtype=U64), call_off, prog_off)
