"""prog.Minimize's predicate from raw KCOV buffers (syz-fuzzer/fuzzer.go:578-591):
sg_minimize_pred_from_kcov.  On the CPU the boundary and the test oracle
(tests/minimize_pred_oracle.py) on hand-written cases; on the GPU the host form
and the device form -- the latter also with every input and output 4 bytes (u32,
bytes) or 8 bytes (u64) off 16-byte alignment -- bit-exact against the oracle:
every exit planted as an attempt of its own, a random batch, list and Signal
lengths at the edges of the wave, the workgroup and the LDS chunk, execute()'s
set updates, the fused call against the separate entry
points, and the call-removal loop of prog.Minimize driven end to end."""
import functools
import os
import re
import subprocess

import numpy as np
import pytest

from oracle import pyoracle as O
from tests import minimize_pred_cases as K
from tests import minimize_pred_oracle as MP
from tests import triage_runs_oracle as TR
from tests.conftest import ROOT

U32, U64 = np.uint32, np.uint64
S = 0xFFFFFFFF
FILL32 = 0xA5A5A5A5
NAMES = ("sg_minimize_pred_from_kcov", "sg_minimize_pred_from_kcov_dev")
A, B, C3 = K.A, K.B, K.C


# ---- CPU: the boundary ---------------------------------------------------------
def test_header_binding_and_library():
    from syzkaller_amd import _lib
    from syzkaller_amd import cover as C

    text = open(os.path.join(ROOT, "include", "syzsig.h")).read()
    assert "syz-fuzzer/fuzzer.go:578-591" in text and "prog/mutation.go:256-450" in text
    src = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r" T (sg_[a-z0-9_]+)$", out, flags=re.M))
    for name in NAMES:
        assert re.search(r"\bint %s\s*\(" % name, src), name
        assert name in _lib.SIGNATURES and name in exported, name
    for name, v in (("OK", MP.OK), ("NOT_EXECUTED", MP.NOT_EXECUTED), ("LOST", MP.LOST)):
        assert re.search(r"#define SG_MP_%s %d\b" % (name, v), src) and getattr(_lib, "MP_" + name) == v
    assert callable(C.minimize_pred_from_kcov) and callable(C.MinimizePred)


def _host_args(lists, att, sets=(None, None)):
    """The ctypes arguments of the host form after ctx, and the arrays they point into."""
    from syzkaller_amd import _lib
    from syzkaller_amd.cover import _p8, _p32, _p64

    nv, no, cd, cl, pcs, co, po = arrs = MP.to_arrays(lists, att)
    n, ncalls = len(att), co.size - 1
    st, rn = np.zeros(max(n, 1), np.int32), np.zeros(max(ncalls, 1), np.uint8)
    so, sv = np.zeros(ncalls + 1, U64), np.zeros(max(pcs.size, 1), U32)
    keep = arrs + (st, rn, so, sv)
    return (sets[0], sets[1], _p32(nv), _p64(no), no.size - 1, _p32(cd), _p32(cl), n, _p64(pcs), _p64(co), _p64(po),
            st.ctypes.data_as(_lib.POINTER(_lib.c_int32)), _p8(rn), _p64(so), _p32(sv), pcs.size), keep


def test_invalid_arguments_are_einval():
    """Every check the host form makes before it touches the context: a context
    that is only a readable block of memory is enough."""
    from syzkaller_amd import _lib
    from syzkaller_amd.cover import _p32, _p64

    lib, E = _lib.lib, _lib.SG_EINVAL
    good, keep = _host_args([[5], [7, 9]], [(0, 0, [[5]]), (1, 0, [[7, 9]])])
    assert lib.sg_minimize_pred_from_kcov(None, *good) == E
    assert lib.sg_minimize_pred_from_kcov_dev(None, None, None, None, None, 0, 0, None, None, 0, None, None, None, 0, 0,
                                              None, None, None, None, 0) == E
    fake = np.zeros(4096, np.uint8).ctypes.data_as(_lib.c_void_p)  # never read: each case below returns first

    def but(i, v):
        return good[:i] + (v,) + good[i + 1:]

    set_like = np.zeros(64, np.uint8).ctypes.data_as(_lib.c_void_p)
    assert lib.sg_minimize_pred_from_kcov(fake, *but(1, set_like)) == E           # newsig without maxsig
    assert lib.sg_minimize_pred_from_kcov_dev(fake, None, set_like, None, good[3], 2, 0, None, None, 0, None, good[9],
                                              good[10], 0, 0, None, None, None, None, 0) == E
    assert lib.sg_minimize_pred_from_kcov(fake, *but(5, _p32(np.array([0, 2], U32)))) == E  # cand[1] == ncand
    bad = np.array([5, 9, 7], U32)
    assert lib.sg_minimize_pred_from_kcov(fake, *but(2, _p32(bad))) == E           # a decreasing list
    for i in (3, 9, 10):                                                           # offsets: not from 0, decreasing
        off = keep[{3: 1, 9: 5, 10: 6}[i]]
        for j, v in ((0, 1), (-1, 0)):
            o = off.copy()
            o[j] = v
            if not np.array_equal(o, off):
                assert lib.sg_minimize_pred_from_kcov(fake, *but(i, _p64(o))) == E, (i, j)
    for i in (3, 5, 6, 9, 10, 11):                                                 # NULL offsets, cand, call, status
        assert lib.sg_minimize_pred_from_kcov(fake, *but(i, None)) == E, i


# ---- CPU: the oracle on hand-written cases ---------------------------------------
def test_oracle_hand_cases():
    # a call whose edges the program's earlier call already put in the table: no Signal, not executed
    assert K.sig_of([[A, B], [A, B]], 1).size == 0
    assert MP.predicate([], [[A, B], [A, B]], 1) == MP.NOT_EXECUTED
    # [[A, B], [A, B, C]], call 1: only C-after-B is left.  B-after-A is in the call's own trace and still LOST:
    # a shortcut around the executor's cross-call table gets this one wrong
    assert K.sig_of([[A, B], [A, B, C3]], 1).tolist() == [678886622]
    assert 3525549802 in K.sig_of([[A, B, C3]], 0).tolist()
    assert MP.predicate([3525549802], [[A, B], [A, B, C3]], 1) == MP.LOST
    assert MP.predicate([678886622], [[A, B], [A, B, C3]], 1) == MP.OK
    assert MP.predicate([3525549802], [[A, B, C3]], 0) == MP.OK
    # truncation before hashing
    wide = [[0x1_0000_0010, 0x2_0000_0010]]
    assert K.sig_of(wide, 0).tolist() == [16, 2639983419]
    assert MP.predicate([16, 2639983419], wide, 0) == MP.OK
    # the empty list: "not executed" comes first
    assert MP.predicate([], [[A]], 0) == MP.OK
    assert MP.predicate([], [], 0) == MP.NOT_EXECUTED and MP.predicate([], [[A]], 1) == MP.NOT_EXECUTED
    assert MP.predicate([], [[A], []], 1) == MP.NOT_EXECUTED
    # a repeat and the sentinel are always LOST
    assert K.sig_of([[5]], 0).tolist() == [5]
    assert MP.predicate([5], [[5]], 0) == MP.OK
    assert MP.predicate([5, 5], [[5]], 0) == MP.LOST
    assert MP.predicate([5, S], [[5]], 0) == MP.LOST
    assert MP.predicate([5, S], [[5, 0xFFFFFFFFFFFFFFFF]], 0) == MP.LOST


@functools.lru_cache(maxsize=None)
def _planted_oracle():
    return MP.batch(*K.planted())


@functools.lru_cache(maxsize=None)
def _random_oracle():
    return MP.batch(*K.random_batch())


@functools.lru_cache(maxsize=None)
def _edges_oracle():
    lists, att, _ = K.length_edges()
    return MP.batch(lists, att)


def test_oracle_batches():
    assert _planted_oracle().tolist() == K.PLANTED_STATUS
    lists, att = K.planted()
    assert sum(1 for k, _, _ in att if k == 6) == 5                     # the shared list
    counts = np.bincount(_random_oracle(), minlength=3)
    assert (counts >= 5).all(), counts                                   # all three statuses occur
    lists, att = K.random_batch()
    assert len(att) == 48 and len(lists) == 12
    assert np.array_equal(_edges_oracle(), K.length_edges()[2])           # the construction does what it says


# ---- GPU -----------------------------------------------------------------------
def _dev(ctx, arrs, sets=None, shift=0, sig_cap=None):
    """sg_minimize_pred_from_kcov_dev through torch buffers, every array `shift`
    elements into its allocation; the outputs prefilled."""
    import torch

    from syzkaller_amd._lib import call

    nv, no, cd, cl, pcs, co, po = arrs
    n, ncand, nnew, ncalls, npcs = po.size - 1, no.size - 1, int(no[-1]), co.size - 1, int(co[-1])
    views = {4: np.int32, 8: np.int64, 1: np.uint8}

    def up(a):
        a = np.ascontiguousarray(a)
        full = np.concatenate([np.zeros(shift, a.dtype), a.reshape(-1), np.zeros(8, a.dtype)])
        t = torch.from_numpy(full.view(views[a.itemsize]).copy()).to("cuda")
        return t, t.data_ptr() + shift * a.itemsize

    def out(count, fill, dtype):
        t = torch.from_numpy(np.full(shift + count + 8, fill, dtype).view(views[np.dtype(dtype).itemsize])).to("cuda")
        return t, t.data_ptr() + shift * np.dtype(dtype).itemsize

    ins = [up(a) for a in (nv, no, cd, cl, pcs, co, po)]
    sig_cap = npcs if sig_cap is None else sig_cap
    st, rn = out(n, -7 & S, U32), out(ncalls, 0xEE, np.uint8)
    so, sv = out(ncalls + 1, (1 << 64) - 1, U64), out(sig_cap, FILL32, U32)
    torch.cuda.synchronize()
    p = [x[1] for x in ins]
    ms, ns = (sets[0].h, sets[1].h if sets[1] is not None else None) if sets else (None, None)
    call("sg_minimize_pred_from_kcov_dev", ctx.h, ms, ns, p[0], p[1], ncand, nnew, p[2], p[3], n, p[4], p[5], p[6],
         ncalls, npcs, st[1], rn[1] if sets else None, so[1] if sets else None, sv[1] if sets else None,
         sig_cap if sets else 0)
    ctx.sync()
    h = [t.cpu().numpy() for t in (st[0], rn[0], so[0], sv[0])]
    status = h[0].view(np.int32)
    assert (status[:shift] == -7).all() and (status[shift + n:] == -7).all()
    if not sets:
        assert (h[1] == 0xEE).all() and (h[2].view(U64) == (1 << 64) - 1).all() and (h[3].view(U32) == FILL32).all()
        return status[shift: shift + n]
    rec_new, sig_off, sig_vals = h[1], h[2].view(U64), h[3].view(U32)
    assert (rec_new[:shift] == 0xEE).all() and (rec_new[shift + ncalls:] == 0xEE).all()
    assert (sig_off[:shift] == (1 << 64) - 1).all() and (sig_off[shift + ncalls + 1:] == (1 << 64) - 1).all()
    sig_off = sig_off[shift: shift + ncalls + 1]
    total = int(sig_off[-1])
    wrote = total if total <= sig_cap else 0
    assert (sig_vals[:shift] == FILL32).all() and (sig_vals[shift + wrote:] == FILL32).all()
    return status[shift: shift + n], rec_new[shift: shift + ncalls], sig_vals[shift: shift + wrote], sig_off


def _check(ctx, lists, att, exp):
    """The host form and the device form (aligned, and off alignment) against exp."""
    from syzkaller_amd import cover as C

    arrs = MP.to_arrays(lists, att)
    got = C.minimize_pred_from_kcov(*arrs, ctx=ctx)
    assert np.array_equal(got, exp), ("host", np.flatnonzero(got != exp))
    for shift in (0, 1):
        got = _dev(ctx, arrs, shift=shift)
        assert np.array_equal(got, exp), ("dev", shift, np.flatnonzero(got != exp))


@pytest.mark.gpu
def test_every_exit(ctx):
    from syzkaller_amd import cover as C

    lists, att = K.planted()
    exp = _planted_oracle()
    assert exp.tolist() == K.PLANTED_STATUS
    _check(ctx, lists, att, exp)
    # no attempts; one attempt; attempts without calls only
    assert C.minimize_pred_from_kcov([5], [0, 1], [], [], [], [0], [0], ctx=ctx).size == 0
    _check(ctx, lists, att[2:3], exp[2:3])
    _check(ctx, lists, [att[8], att[14]], exp[[8, 14]])


@pytest.mark.gpu
def test_random_batch(ctx):
    lists, att = K.random_batch()
    exp = _random_oracle()
    assert set(exp.tolist()) == {MP.OK, MP.NOT_EXECUTED, MP.LOST}
    _check(ctx, lists, att, exp)


@pytest.mark.gpu
def test_length_edges(ctx):
    lists, att, want = K.length_edges()
    exp = _edges_oracle()
    assert np.array_equal(exp, want)
    _check(ctx, lists, att, exp)


@pytest.mark.gpu
def test_sets(ctx):
    """With maxsig: rec_new and both sets as sg_triage_traces on the truncated PCs, the lists as sg_exec_signal's
    on the queued or selected calls and empty elsewhere; without: no set changes."""
    from syzkaller_amd import cover as C

    lists, att = K.random_batch()
    arrs = nv, no, cd, cl, pcs, co, po = MP.to_arrays(lists, att)
    pcs32 = (pcs & U64(S)).astype(U32)
    ncalls = co.size - 1
    xv, xo = C.exec_signal(pcs32, co, po, ctx=ctx)
    m0 = np.unique(xv)[::3].copy()                                       # a third of the batch's signal is known
    om, on = O.OSet(m0), O.OSet()
    e_st, e_rn, e_sv, e_so = MP.batch(lists, att, om, on)
    assert np.array_equal(e_st, _random_oracle()) and 0 < int(e_rn.sum()) < ncalls
    selected = np.zeros(ncalls, bool)
    for e, (_, c1, run) in enumerate(att):
        if c1 < len(run):
            selected[int(po[e]) + c1] = True
    assert (selected & (e_rn == 0)).any() and ((e_rn != 0) & ~selected).any()

    def fresh():
        ms, ns = C.SignalSet(ctx), C.SignalSet(ctx)
        C.SignalAdd(ms, m0)
        return ms, ns

    ts, tn = fresh()                                                     # the existing entry points
    t_rn = C.triage_traces(ts, tn, pcs32, co, ctx=ctx)
    t_max, t_new = ts.export(), tn.export()
    assert np.array_equal(t_rn, e_rn) and np.array_equal(t_max, om.export()) and np.array_equal(t_new, on.export())
    for c in range(ncalls):
        lst = xv[int(xo[c]):int(xo[c + 1])] if (e_rn[c] or selected[c]) else TR.EMPTY
        assert np.array_equal(e_sv[int(e_so[c]):int(e_so[c + 1])], lst), c

    def same(got, tag, ms, ns):
        for g, e, name in zip(got, (e_st, e_rn, e_sv, e_so), ("status", "rec_new", "sig_vals", "sig_off")):
            assert np.array_equal(g, e), (tag, name)
        assert np.array_equal(ms.export(), t_max) and np.array_equal(ns.export(), t_new), tag

    ms, ns = fresh()
    same(C.minimize_pred_from_kcov(*arrs, maxset=ms, newset=ns, ctx=ctx), "host", ms, ns)
    for shift in (0, 1):
        ms.clear()
        ns.clear()
        C.SignalAdd(ms, m0)
        same(_dev(ctx, arrs, sets=(ms, ns), shift=shift), ("dev", shift), ms, ns)
    # newsig NULL; a capacity one short: flags and offsets filled, no value written
    ms.clear()
    C.SignalAdd(ms, m0)
    st, rn, sv, so = _dev(ctx, arrs, sets=(ms, None), sig_cap=int(e_so[-1]) - 1)
    assert np.array_equal(st, e_st) and np.array_equal(rn, e_rn) and np.array_equal(so, e_so) and sv.size == 0
    assert np.array_equal(ms.export(), t_max)
    # without maxsig no set is read or written
    before = ms.export()
    assert np.array_equal(C.minimize_pred_from_kcov(*arrs, ctx=ctx), e_st)
    assert np.array_equal(ms.export(), before) and np.array_equal(ns.export(), t_new)
    for s in (ms, ns, ts, tn):
        s.close()


@pytest.mark.gpu
def test_fused_against_the_separate_entry_points(ctx):
    """Statuses equal sg_exec_signal on every call, sg_triage_subset and the not-executed rule chained by hand."""
    from syzkaller_amd import cover as C

    lists = list(K.planted()[0])
    att = list(K.planted()[1])
    rl, ra = K.random_batch()
    att += [(k + len(lists), c, r) for k, c, r in ra]
    lists += list(rl)
    arrs = nv, no, cd, cl, pcs, co, po = MP.to_arrays(lists, att)
    fused = C.minimize_pred_from_kcov(*arrs, ctx=ctx)
    xv, xo = C.exec_signal((pcs & U64(S)).astype(U32), co, po, ctx=ctx)
    news, sigs, executed = [], [], []
    for e, (k, c1, run) in enumerate(att):
        c = int(po[e]) + c1
        sig = xv[int(xo[c]):int(xo[c + 1])] if c1 < len(run) else TR.EMPTY
        executed.append(sig.size > 0)
        news.append(np.asarray(lists[k], U32))
        sigs.append(sig)
    a_vals, a_off = C.to_csr(news)
    r_vals, r_off = C.to_csr(sigs)
    ok = C.triage_subset(a_vals, a_off, r_vals, r_off, ctx=ctx)
    chain = np.where(np.array(executed), np.where(ok != 0, MP.OK, MP.LOST), MP.NOT_EXECUTED).astype(np.int32)
    assert np.array_equal(fused, chain), np.flatnonzero(fused != chain)
    assert set(chain.tolist()) == {MP.OK, MP.NOT_EXECUTED, MP.LOST}


def _remove_calls(calls, call_index0, pred):
    """prog/mutation.go:313-328 over a program given as the list of its calls."""
    p0 = list(calls)
    for i in range(len(p0) - 1, -1, -1):
        if i == call_index0:
            continue
        call_index = call_index0 - 1 if i < call_index0 else call_index0
        p = p0[:i] + p0[i + 1:]
        if not pred(p, call_index):
            continue
        p0, call_index0 = p, call_index
    return p0, call_index0


@pytest.mark.gpu
def test_end_to_end_call_removal(ctx):
    """TriageInput, then MinimizePred as the closure of prog.Minimize's call-removal loop: the same calls stay as
    with the oracle driving the same loop."""
    from syzkaller_amd import cover as C

    rng = np.random.default_rng(62)
    pool = K.TEXT + 16 * rng.choice(1 << 12, size=60, replace=False).astype(U64)
    full = [pool[rng.integers(0, 60, size=int(n))] for n in (40, 25, 0, 60, 35, 50, 20)]
    call = 4

    def execute(p):
        """The traces of the program made of calls p (ids into full).  Call 4 needs calls 3 and 1 before it:
        without 3 it does not run at all, without 1 it fails after five PCs.  Removing any other call only
        leaves the dedup table emptier, which never takes an edge away from a later call."""
        run = []
        for pos, cid in enumerate(p):
            t = full[cid]
            if cid == 4 and 3 not in p[:pos]:
                t = t[:0]
            elif cid == 4 and 1 not in p[:pos]:
                t = t[:5]
            run.append(t)
        return run

    prog = list(range(len(full)))
    signal = K.sig_of(execute(prog), call)
    assert signal.size > 10
    corpus_vals = signal[:2]
    corpus = C.SignalSet(ctx)
    C.SignalAdd(corpus, corpus_vals)
    runs = [execute(prog)] * 3
    status, new, _ = C.TriageInput(corpus, signal, call, runs)
    e_status, e_new, _ = TR.triage_input(O.OSet(corpus_vals), signal, call, runs, False)
    assert status == e_status == TR.OK and np.array_equal(new, e_new) and new.size > 5
    tried = []

    def oracle_pred(p, c1):
        tried.append(MP.predicate(e_new, execute(p), c1))
        return tried[-1] == MP.OK

    want, want_call = _remove_calls(prog, call, oracle_pred)
    assert (want, want_call) == ([1, 3, 4], 2) and set(tried) == {MP.OK, MP.NOT_EXECUTED, MP.LOST}
    pred = C.MinimizePred(new, ctx=ctx)
    assert _remove_calls(prog, call, lambda p, c1: pred(execute(p), c1)) == (want, want_call)
    # with the sets, every attempt also goes through execute()'s check
    ms, ns = C.SignalSet(ctx), C.SignalSet(ctx)
    pred = C.MinimizePred(new, ms, ns, ctx=ctx)
    assert _remove_calls(prog, call, lambda p, c1: pred(execute(p), c1)) == (want, want_call)
    assert len(ms) > 0 and np.array_equal(ms.export(), ns.export())
    for s in (corpus, ms, ns):
        s.close()
