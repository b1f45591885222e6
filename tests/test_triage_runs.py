"""triageInput's loop from raw KCOV buffers (syz-fuzzer/fuzzer.go:521-576):
sg_triage_runs_from_kcov.  On the CPU the boundary and the test oracle
(tests/triage_runs_oracle.py) on hand-written cases; on the GPU the host and
device forms exact against the oracle, every exit of the loop planted as a
candidate of its own, and the fused call against the separate entry points
chained on the host side."""
import functools
import os
import re
import subprocess

import numpy as np
import pytest

from oracle import pyoracle as O
from tests import exec_cover_oracle as XC
from tests import triage_runs_cases as K
from tests import triage_runs_oracle as TR
from tests.conftest import ROOT

U32, U64 = np.uint32, np.uint64
S = 0xFFFFFFFF
M64 = (1 << 64) - 1
TEXT = 0xFFFFFFFF81000000
FILL32 = 0xA5A5A5A5
NAMES = ("sg_triage_runs_from_kcov", "sg_triage_runs_from_kcov_dev")


def tr(rng, n, nvals, base=0):
    """A call's trace: n PCs of a pool of nvals kernel-text PCs starting at slot base."""
    pool = TEXT + 16 * (base + rng.choice(1 << 16, size=max(nvals, 1), replace=False).astype(U64))
    return pool[rng.integers(0, max(nvals, 1), size=n)]


def sig_of(run, call):
    info = TR.run_info(run, call)
    return info[0] if info is not None else TR.EMPTY


# ---- CPU: the boundary ---------------------------------------------------------
def test_header_binding_and_library():
    from syzkaller_amd import _lib
    from syzkaller_amd import cover as C

    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "syzsig.h")).read(), flags=re.S)
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r" T (sg_[a-z0-9_]+)$", out, flags=re.M))
    for name in NAMES:
        assert re.search(r"\bint %s\s*\(" % name, src), name
        assert name in _lib.SIGNATURES and name in exported, name
    for name, v in (("OK", TR.OK), ("NO_NEW", TR.NO_NEW), ("NOT_EXECUTED", TR.NOT_EXECUTED), ("FLAKY", TR.FLAKY)):
        assert re.search(r"#define SG_TIN_%s %d\b" % (name, v), src) and getattr(_lib, "TIN_" + name) == v
    assert callable(C.triage_runs_from_kcov) and callable(C.TriageInput)


def test_null_context_is_einval():
    from syzkaller_amd import _lib

    z = np.zeros(4, U64)
    p64, p32 = z.ctypes.data_as(_lib.P64), z.view(U32).ctypes.data_as(_lib.P32)
    st = np.zeros(1, np.int32).ctypes.data_as(_lib.POINTER(_lib.c_int32))
    assert _lib.lib.sg_triage_runs_from_kcov(None, None, p32, p64, 0, p32, z.view(np.uint8).ctypes.data_as(_lib.P8), 3,
                                             p64, p64, p64, st, p64, p32, 0, p64, p32, 0) == _lib.SG_EINVAL
    assert _lib.lib.sg_triage_runs_from_kcov_dev(None, None, None, None, 0, 0, None, None, 3, None, None, None, 0, 0,
                                                 None, None, None, 0, None, None, 0) == _lib.SG_EINVAL


# ---- CPU: the oracle on hand-written cases ---------------------------------------
def test_oracle_cover_fold():
    empty = O.OSet()
    # Union of [5, 5] and [5]: each value at its largest count (cover.go:63-102)
    wide, one = [0x1_0000_0005, 0x2_0000_0005], [5]
    assert XC.call_cover(wide).tolist() == [5, 5]
    st, new, cov = TR.triage_input(empty, [5], 0, [[wide], [one], [one]], False)
    assert (st, new.tolist(), cov.tolist()) == (TR.OK, [5], [5, 5])
    st, new, cov = TR.triage_input(empty, [5], 0, [[one], [wide], [one]], False)
    assert (st, cov.tolist()) == (TR.OK, [5, 5])
    # a copy keeps 0xFFFFFFFF, Union drops it
    run = [[TEXT + 16, M64]]
    s1 = int(sig_of(run, 0)[0])
    assert s1 == 0x81000010 and XC.call_cover(run[0]).tolist() == [0x81000010, S]
    st, new, cov = TR.triage_input(empty, [s1], 0, [run, [], []], True)
    assert (st, new.tolist(), cov.tolist()) == (TR.OK, [s1], [0x81000010, S])
    st, new, cov = TR.triage_input(empty, [s1], 0, [run, [], run], False)
    assert (st, cov.tolist()) == (TR.OK, [0x81000010])
    st, new, cov = TR.triage_input(empty, [s1], 0, [run], False)  # one run: the copy alone
    assert (st, cov.tolist()) == (TR.OK, [0x81000010, S])
    # a cover of sentinels only: Union returns nothing, and the next run is copied again
    alls = [[M64]]
    st, new, cov = TR.triage_input(empty, [S, 7], 0, [alls, alls, alls], False)
    assert st == TR.FLAKY  # Intersection drops the sentinel: nothing of newSignal is left


def test_oracle_statuses():
    rng = np.random.default_rng(50)
    R = [tr(rng, 30, 9), tr(rng, 40, 12), tr(rng, 20, 5)]
    D = [tr(rng, 30, 9, 1 << 17), tr(rng, 40, 12, 1 << 17)]
    sig = sig_of(R, 1)
    assert sig.size > 3
    corpus = O.OSet(sig[:2])
    expect_new = np.unique(sig[2:])
    st, new, cov = TR.triage_input(corpus, sig, 1, [R, R, R], False)
    assert st == TR.OK and np.array_equal(new, expect_new) and np.array_equal(cov, XC.call_cover(R[1]))
    assert TR.triage_input(corpus, sig[:2], 1, [R, R, R], False)[0] == TR.NO_NEW
    assert TR.triage_input(corpus, sig[:2], 1, [R, R, R], True)[0] == TR.NO_NEW
    assert TR.triage_input(corpus, sig, 1, [[], R, R], False)[0] == TR.OK           # skipped once
    assert TR.triage_input(corpus, sig, 1, [R, R, R[:1]], False)[0] == TR.OK
    assert TR.triage_input(corpus, sig, 1, [[], R[:1], R], False)[0] == TR.NOT_EXECUTED
    assert TR.triage_input(corpus, sig, 1, [[], R, []], False)[0] == TR.NOT_EXECUTED
    st, new, cov = TR.triage_input(corpus, sig, 1, [D, R, R], False)
    assert st == TR.FLAKY and new.size == 0 and cov.size == 0
    assert TR.triage_input(corpus, sig, 1, [R, R, D], False)[0] == TR.FLAKY
    # minimized: the first run with any cover, whatever its signal
    st, new, cov = TR.triage_input(corpus, sig, 1, [[], D, R], True)
    assert st == TR.OK and np.array_equal(new, expect_new) and np.array_equal(cov, XC.call_cover(D[1]))
    st, new, cov = TR.triage_input(corpus, sig, 1, [[], [], R[:1]], True)
    assert st == TR.OK and cov.size == 0
    # a call whose edges its program's earlier call already holds: a trace, a cover, no signal
    dup = [R[1], R[1]]
    assert sig_of(dup, 1).size == 0 and TR.run_info(dup, 1)[1].size > 0
    assert TR.triage_input(corpus, sig, 1, [dup, R, R], False)[0] == TR.OK
    assert TR.triage_input(corpus, sig, 1, [dup, dup, R], False)[0] == TR.NOT_EXECUTED
    assert np.array_equal(TR.triage_input(corpus, sig, 1, [dup, R, R], True)[2], XC.call_cover(R[1]))


def test_oracle_signal_agrees_with_the_compiled_reference():
    if O.ref_executor() is None:
        pytest.skip("oracle/_ref is not built")
    rng = np.random.default_rng(51)
    for _ in range(20):
        run = [tr(rng, int(n), 50) for n in rng.integers(0, 300, size=4)]
        call = int(rng.integers(0, 4))
        pcs32 = (np.concatenate(run) & U64(S)).astype(U32)
        off = np.concatenate([[0], np.cumsum([c.size for c in run])]).astype(U64)
        ref, so = O.ref_exec_signal(pcs32, off, [0, 4])
        assert np.array_equal(sig_of(run, call), ref[int(so[call]):int(so[call + 1])])


# ---- the candidates ----------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _planted():
    """(corpus values, candidates, the index of the one wide candidate)."""
    rng = np.random.default_rng(52)
    R = [tr(rng, 60, 20), tr(rng, 150, 40), tr(rng, 30, 8), tr(rng, 90, 30)]
    R2 = [R[0], np.concatenate([R[1], tr(rng, 25, 9, 1 << 17)]), R[2]]   # the same call with extra PCs
    R3 = [tr(rng, 10, 4, 1 << 18), np.concatenate([tr(rng, 12, 5, 1 << 18), R[1]])]
    D = [tr(rng, 60, 20, 1 << 19), tr(rng, 150, 40, 1 << 19), tr(rng, 9, 3, 1 << 19)]
    dup = [R2[1], R2[1], R[2]]
    sig = sig_of(R, 1)
    corpus = np.concatenate([sig[:5], sig_of(D, 0)[:7]])
    junk = np.array([S, S, 3, 3, 0], U32)
    c = []
    c.append((sig[:5], 1, [R, R, R], False))                      # NO_NEW
    c.append((sig[:5], 1, [R, R, R], True))                       # ... whatever minimized says
    c.append((sig, 1, [R, R2, R3], False))                        # OK over three different runs
    c.append((sig, 1, [[], R, R2], False))                        # not executed at run 0 only
    c.append((sig, 1, [R, R2, R[:1]], False))                     # ... at run 2 only (a short execution)
    c.append((sig, 1, [[], R[:1], R], False))                     # at runs 0 and 1
    c.append((sig, 1, [[], R, []], False))                        # at runs 0 and 2
    c.append((sig, 1, [dup, R, R2], False))                       # a trace without signal: skipped once
    c.append((sig, 1, [dup, dup, R], False))                      # ... twice
    c.append((sig, 1, [dup, R, R2], True))                        # minimized still takes its cover
    c.append((sig, 1, [D, tr(rng, 5, 2).reshape(1, -1).tolist() * 2, [[1, 2, 3]] * 2], False))  # FLAKY at run 0, garbage after
    c.append((sig, 1, [R, R2, D], False))                         # FLAKY at run 2
    c.append((sig, 1, [R, D, R2], True))                          # minimized: the first non-empty run is 0
    c.append((sig, 1, [[], D, R], True))                          # ... 1
    c.append((sig, 1, [[], R[:1], R3], True))                     # ... 2
    c.append((sig, 1, [[], [R[0], []], R[:1]], True))             # ... none
    c.append((sig_of(R, 0), 0, [R, R, R2], False))                # inp.call 0
    c.append((sig_of(R, 3), 3, [R, R, R], False))                 # the last call
    c.append((sig, 4, [R, R, R], False))                          # past the execution's calls
    c.append((sig, 4, [R, R, R], True))
    sent = [[TEXT + 16, TEXT + 32, M64, M64]]
    s_sent = sig_of(sent, 0)
    c.append((s_sent, 0, [sent, [], []], True))                   # a cover with 0xFFFFFFFF: one copy keeps it
    c.append((s_sent, 0, [sent, [], sent], False))                # two counted runs: Union drops it
    c.append((s_sent, 0, [sent, sent, sent], False))
    rep1 = [[0x1_0000_0005, 0x2_0000_0005, 0x2_0000_0009]]       # [5, 5, 9]: repeats, non-decreasing
    rep2 = [[0x1_0000_0005, 0x1_0000_0009, 0x2_0000_0009, 0x3_0000_0009]]  # [5, 9, 9, 9]
    c.append((sig_of(rep1, 0), 0, [rep1, rep2, rep1], False))
    c.append((np.concatenate([junk, sig, junk, sig]), 1, [R, R, R2], False))  # inp.signal with 0xFFFFFFFF and duplicates
    b0 = tr(rng, 3000, 2500, 1 << 20)
    big = [[b0], [np.concatenate([b0, tr(rng, 800, 700, 1 << 20)])], [np.concatenate([b0, tr(rng, 500, 400, 1 << 20)])]]
    c.append((sig_of(big[0], 0)[:40], 0, big, False))             # about 6,500 cover values: the LDS sort
    h0 = tr(rng, 9000, 5000, 1 << 21)
    low = np.array([int(h0.min()) & S], U64)                      # high word 0: the smallest value, a second time
    huge = [[np.concatenate([h0, low])], [np.concatenate([h0, tr(rng, 900, 800, 1 << 21)])],
            [np.concatenate([h0[:8000], low])]]
    c.append((sig_of(huge[0], 0)[:40], 0, huge, False))           # about 12,000, one value twice: past the LDS sort
    wide = len(c)
    w1 = [[0x2_0000_0005, 0x1_0000_0010, 0x1_0000_0003]]          # cover [3, 0x10, 5]: not non-decreasing
    w2 = [[0x1_0000_0005, 0x3_0000_0010, 0x2_0000_0003]]          # the same low words: cover [5, 3, 0x10]
    c.append((sig_of(w1, 0), 0, [w1, w2, w1], False))
    c.append((sig, 1, [R2, R, R3], False))                        # a narrow one next to it
    return corpus, c, wide


@functools.lru_cache(maxsize=None)
def _planted_oracle():
    corpus, cands, _ = _planted()
    return TR.batch(O.OSet(corpus), cands)


def _random(seed, n):
    """n candidates of 1 to 6 calls and 0 to 400 PCs per call, built so that every status occurs."""
    rng = np.random.default_rng(seed)
    corpus_parts, cands = [], []
    for k in range(n):
        ncalls = int(rng.integers(1, 7))
        base = int(rng.integers(0, 8)) << 17
        R = [tr(rng, int(rng.integers(0, 401)), int(rng.integers(1, 120)), base) for _ in range(ncalls)]
        call = int(rng.integers(0, ncalls))
        if R[call].size == 0:
            R[call] = tr(rng, 17, 6, base)
        sig = sig_of(R, call)
        kind = rng.choice(5, p=[0.46, 0.12, 0.14, 0.14, 0.14])
        noisy = [R[:call] + [np.concatenate([R[call], tr(rng, int(rng.integers(0, 30)), 10, base + (1 << 16))])] + R[call + 1:]
                 for _ in range(3)]
        runs = [R, noisy[1], noisy[2]]
        D = [tr(rng, 50, 20, base + (1 << 20)) for _ in range(ncalls)]
        if kind == 1:                                   # everything already in the corpus
            corpus_parts.append(sig)
        elif kind == 2:                                 # not executed twice
            i, j = rng.choice(3, size=2, replace=False)
            runs[i] = [] if rng.integers(2) else R[:call]
            runs[j] = [] if rng.integers(2) else R[:call] + [np.zeros(0, U64)] + R[call + 1:]
        elif kind == 3:                                 # one run somewhere else entirely
            runs[int(rng.integers(3))] = D
        elif kind == 4:                                 # not executed once
            runs[int(rng.integers(3))] = []
        else:
            corpus_parts.append(sig[: sig.size // 3])
        minimized = bool(rng.integers(5) == 0) and kind not in (2, 3)
        cands.append((np.concatenate([sig, sig[:3]]), call, runs, minimized))
    return np.concatenate(corpus_parts).astype(U32), cands


@functools.lru_cache(maxsize=None)
def _random300():
    corpus, cands = _random(53, 300)
    return corpus, cands, TR.batch(O.OSet(corpus), cands)


def test_random_candidates_reach_every_status():
    _, _, exp = _random300()
    counts = np.bincount(exp[0], minlength=4)
    assert counts[TR.OK] >= 100 and (counts[1:] >= 10).all(), counts
    _, cands, wide = _planted()
    st = _planted_oracle()[0]
    assert set(st.tolist()) == {TR.OK, TR.NO_NEW, TR.NOT_EXECUTED, TR.FLAKY} and st[wide] == TR.OK


# ---- GPU -----------------------------------------------------------------------
def _corpus(ctx, values):
    from syzkaller_amd import cover as C

    s = C.SignalSet(ctx)
    C.SignalAdd(s, values)
    return s


def _dev(ctx, corpus, arrs, new_cap=None, cov_cap=None):
    """sg_triage_runs_from_kcov_dev through torch buffers; the payloads prefilled."""
    import torch

    from syzkaller_amd._lib import call

    sv, so, cl, mn, nruns, pcs, co, po = arrs
    n, nsig, ncalls, npcs = so.size - 1, int(so[-1]), co.size - 1, int(co[-1])
    d = "cuda"

    def up(a, dt):
        a = np.ascontiguousarray(a)
        pad = np.zeros(8, a.dtype)
        return torch.from_numpy(np.concatenate([a.reshape(-1), pad]).view(dt).copy()).to(d)

    t = [up(sv, np.int32), up(so, np.int64), up(cl, np.int32), up(mn, np.uint8), up(pcs, np.int64), up(co, np.int64),
         up(po, np.int64)]
    new_cap = nsig if new_cap is None else new_cap
    cov_cap = npcs if cov_cap is None else cov_cap
    status = torch.full((n + 1,), -7, dtype=torch.int32, device=d)
    new_off = torch.full((n + 1,), -1, dtype=torch.int64, device=d)
    cov_off = torch.full((n + 1,), -1, dtype=torch.int64, device=d)
    nv = torch.from_numpy(np.full(new_cap + 8, FILL32, U32).view(np.int32)).to(d)
    cv = torch.from_numpy(np.full(cov_cap + 8, FILL32, U32).view(np.int32)).to(d)
    torch.cuda.synchronize()
    call("sg_triage_runs_from_kcov_dev", ctx.h, corpus.h, t[0].data_ptr(), t[1].data_ptr(), n, nsig, t[2].data_ptr(),
         t[3].data_ptr(), nruns, t[4].data_ptr(), t[5].data_ptr(), t[6].data_ptr(), ncalls, npcs, status.data_ptr(),
         new_off.data_ptr(), nv.data_ptr(), new_cap, cov_off.data_ptr(), cv.data_ptr(), cov_cap)
    ctx.sync()
    return (status.cpu().numpy()[:n], nv.cpu().numpy().view(U32), new_off.cpu().numpy().view(U64),
            cv.cpu().numpy().view(U32), cov_off.cpu().numpy().view(U64))


def _same(got, exp, tag):
    for g, e, name in zip(got, exp, ("status", "new_vals", "new_off", "cov_vals", "cov_off")):
        assert np.array_equal(g, e), (tag, name)


def _check(ctx, ctx_option, corpus_vals, cands, exp, wide=None, paths=(-1, 0), counters=None):
    """Host form and device form on each exec_cover path against exp; counters: the device counters (name ->
    value) every one of those calls leaves."""
    from syzkaller_amd import cover as C

    def counted(tag):
        if wide is not None:
            assert ctx.counter("triage_runs_wide") == wide, tag
        got = {name: ctx.counter(name) for name in counters or ()}
        assert got == (counters or {}), tag

    corpus = _corpus(ctx, corpus_vals)
    before = corpus.export()
    arrs = TR.to_arrays(cands)
    for path in paths:
        ctx_option(ctx, "exec_cover_path", path)
        _same(C.triage_runs_from_kcov(corpus, *arrs, ctx=ctx), exp, ("host", path))
        counted(("host", path))
        st, nv, no, cv, vo = _dev(ctx, corpus, arrs)
        n_new, n_cov = int(exp[2][-1]), int(exp[4][-1])
        _same((st, nv[:n_new], no, cv[:n_cov], vo), exp, ("dev", path))
        assert (nv[n_new:] == FILL32).all() and (cv[n_cov:] == FILL32).all(), path
        counted(("dev", path))
    assert np.array_equal(corpus.export(), before)  # corpusSignal is only read
    corpus.close()


@pytest.mark.gpu
def test_planted_candidates(ctx, ctx_option):
    corpus, cands, _ = _planted()
    exp = _planted_oracle()
    st = exp[0].tolist()
    assert st[:12] == [TR.NO_NEW, TR.NO_NEW, TR.OK, TR.OK, TR.OK, TR.NOT_EXECUTED, TR.NOT_EXECUTED, TR.OK, TR.NOT_EXECUTED,
                       TR.OK, TR.FLAKY, TR.FLAKY]
    oc = O.OSet(corpus)
    routes = K.counters([K.shape(oc, c) for c in cands])  # the route of every cover fold, from the oracle alone
    assert routes["triage_runs_ranked"] == 1 and routes["triage_runs_foreach"] == 1 and routes["triage_runs_wide"] == 1
    _check(ctx, ctx_option, corpus, cands, exp, wide=1, counters=routes)


@pytest.mark.gpu
def test_one_run_no_candidates_one_candidate(ctx, ctx_option):
    corpus, cands, _ = _planted()
    one = [(s, c, r[:1], m) for s, c, r, m in cands]
    _check(ctx, ctx_option, corpus, one, TR.batch(O.OSet(corpus), one), wide=1)
    for sub in (cands[2:3], cands[:1]):
        _check(ctx, ctx_option, corpus, sub, TR.batch(O.OSet(corpus), sub), wide=0, paths=(-1,))
    from syzkaller_amd import cover as C

    s = _corpus(ctx, corpus)
    got = C.triage_runs_from_kcov(s, [], [0], [], [], 3, [], [0], [0], ctx=ctx)
    assert got[0].size == 0 and got[2].tolist() == [0] and got[4].tolist() == [0]
    sig, call, runs, mini = cands[2]
    st, new, cov = C.TriageInput(s, sig, call, runs, mini)
    e = TR.triage_input(O.OSet(corpus), sig, call, runs, mini)
    assert st == e[0] == TR.OK and np.array_equal(new, e[1]) and np.array_equal(cov, e[2])
    s.close()


@pytest.mark.gpu
def test_random_candidates(ctx, ctx_option):
    corpus, cands, exp = _random300()
    _check(ctx, ctx_option, corpus, cands, exp, wide=0)


@pytest.mark.gpu
def test_composition_of_the_separate_entry_points(ctx):
    """The fused result equals sg_triage_newsig, sg_exec_signal, sg_exec_cover,
    sg_triage_intersect and sg_merge(SG_OP_UNION) chained on the host side, for
    the candidates whose covers are ascending."""
    from syzkaller_amd import cover as C

    corpus_vals, cands, wide = _planted()
    rc, rcands = _random(54, 40)
    cands = [c for i, c in enumerate(cands) if i != wide] + rcands
    corpus_vals = np.concatenate([corpus_vals, rc])
    corpus = _corpus(ctx, corpus_vals)
    sv, so, cl, mn, nruns, pcs, co, po = arrs = TR.to_arrays(cands)
    f_st, f_nv, f_no, f_cv, f_vo = C.triage_runs_from_kcov(corpus, *arrs, ctx=ctx)
    new_vals, new_off = C.triage_newsig(corpus, sv, so, ctx=ctx)
    sig, sig_off = C.exec_signal((pcs & U64(S)).astype(U32), co, po, ctx=ctx)
    cov, cov_off = C.exec_cover(pcs, co, ctx=ctx)
    for k, (_, call, runs, mini) in enumerate(cands):
        new = new_vals[int(new_off[k]):int(new_off[k + 1])].copy()
        cover, status, skipped = TR.EMPTY, TR.OK, False
        if new.size == 0:
            status = TR.NO_NEW
        for i in range(nruns):
            if status != TR.OK:
                break
            e = k * nruns + i
            c = int(po[e]) + call
            have = c < int(po[e + 1])
            s_i = sig[int(sig_off[c]):int(sig_off[c + 1])] if have else TR.EMPTY
            c_i = cov[int(cov_off[c]):int(cov_off[c + 1])] if have else TR.EMPTY
            if mini:
                if c_i.size:
                    cover = c_i.copy()
                    break
                continue
            if s_i.size == 0:
                if skipped:
                    status = TR.NOT_EXECUTED
                skipped = True
                continue
            ln = np.zeros(1, U64)
            buf = new.copy()
            C.call("sg_triage_intersect", ctx.h, C._p32(buf), C._p64(np.array([0, buf.size], U64)), C._p32(s_i),
                   C._p64(np.array([0, s_i.size], U64)), 1, C._p64(ln))
            new = buf[: int(ln[0])]
            if new.size == 0:
                status = TR.FLAKY
            elif cover.size == 0:
                cover = c_i.copy()
            else:
                cover = C.Union(cover, c_i, ctx=ctx)
        if status != TR.OK:
            new, cover = TR.EMPTY, TR.EMPTY
        assert f_st[k] == status, k
        assert np.array_equal(f_nv[int(f_no[k]):int(f_no[k + 1])], new), k
        assert np.array_equal(f_cv[int(f_vo[k]):int(f_vo[k + 1])], cover), k
    corpus.close()


@pytest.mark.gpu
def test_capacity_convention_and_arguments(ctx, ctx_option):
    import torch

    from syzkaller_amd import _lib
    from syzkaller_amd.cover import _p8, _p32, _p64

    lib, h, E = _lib.lib, ctx.h, _lib.SG_EINVAL
    corpus_vals, cands, _ = _planted()
    cands = cands[:8]
    exp = TR.batch(O.OSet(corpus_vals), cands)
    corpus = _corpus(ctx, corpus_vals)
    sv, so, cl, mn, nruns, pcs, co, po = arrs = TR.to_arrays(cands)
    n, n_new, n_cov = len(cands), int(exp[2][-1]), int(exp[4][-1])
    assert n_new > 1 and n_cov > 1
    pst = lambda a: a.ctypes.data_as(_lib.POINTER(_lib.c_int32))  # noqa: E731
    st, no, vo = np.zeros(n, np.int32), np.zeros(n + 1, U64), np.zeros(n + 1, U64)
    nv, cv = np.full(n_new, FILL32, U32), np.full(n_cov, FILL32, U32)

    def args(new_cap, cov_cap):
        return (corpus.h, _p32(sv), _p64(so), n, _p32(cl), _p8(mn), nruns, _p64(pcs), _p64(co), _p64(po), pst(st),
                _p64(no), _p32(nv), new_cap, _p64(vo), _p32(cv), cov_cap)

    # one short: the offsets and the status are filled, that payload untouched (each payload by its own cap)
    assert lib.sg_triage_runs_from_kcov(h, *args(n_new - 1, n_cov - 1)) == 0
    assert np.array_equal(st, exp[0]) and np.array_equal(no, exp[2]) and np.array_equal(vo, exp[4])
    assert (nv == FILL32).all() and (cv == FILL32).all()
    assert lib.sg_triage_runs_from_kcov(h, *args(n_new, n_cov - 1)) == 0
    assert np.array_equal(nv, exp[1]) and (cv == FILL32).all()
    assert lib.sg_triage_runs_from_kcov(h, *args(n_new, n_cov)) == 0
    assert np.array_equal(cv, exp[3])
    d = _dev(ctx, corpus, arrs, new_cap=n_new - 1, cov_cap=n_cov - 1)
    assert np.array_equal(d[0], exp[0]) and np.array_equal(d[2], exp[2]) and np.array_equal(d[4], exp[4])
    assert (d[1] == FILL32).all() and (d[3] == FILL32).all()
    # SG_EINVAL: a NULL where a pointer is required, another context's set, bad offsets, nruns outside 1..8
    a = args(n_new, n_cov)

    def but(i, v):
        return a[:i] + (v,) + a[i + 1:]

    assert lib.sg_triage_runs_from_kcov(None, *a) == E
    for i in (0, 1, 2, 4, 5, 7, 8, 9, 10, 11, 12, 14, 15):
        assert lib.sg_triage_runs_from_kcov(h, *but(i, None)) == E, i
    for bad_runs in (0, 9):
        assert lib.sg_triage_runs_from_kcov(h, *but(6, bad_runs)) == E
    for i, off in ((2, so), (8, co), (9, po)):
        bad = off.copy()
        bad[0] = 1
        assert lib.sg_triage_runs_from_kcov(h, *but(i, _p64(bad))) == E, i
        bad = off.copy()
        bad[-1] = 0
        assert lib.sg_triage_runs_from_kcov(h, *but(i, _p64(bad))) == E, i
    t = torch.zeros(64, dtype=torch.int64, device="cuda")
    p = t.data_ptr()
    dev = lib.sg_triage_runs_from_kcov_dev
    good = [h, corpus.h, p, p, 1, 1, p, p, 3, p, p, p, 1, 1, p, p, p, 1, p, p, 1]
    for i in (0, 1, 2, 3, 6, 7, 9, 10, 11, 14, 15, 16, 18, 19):
        assert dev(*(good[:i] + [None] + good[i + 1:])) == E, i
    for i, v in ((8, 0), (8, 9), (4, 1 << 28), (12, 1 << 31), (13, 1 << 32), (5, 1 << 32)):
        assert dev(*(good[:i] + [v] + good[i + 1:])) == E, (i, v)
    corpus.close()
