"""Host-side mirror of syzkaller's pkg/cover API and the fuzzer/manager signal
loops, running on the MI355X through libsyzsig.so.

Names, argument meaning and results follow the reference
(pkg/cover/cover.go:11-182, syz-fuzzer/fuzzer.go:467-489 and :645-693,
syz-manager/manager.go:769-784, :907-912, :949-956) so the parity tests read
like pkg/cover/cover_test.go.  Arrays are numpy uint32 (PCs / signal).  A Go
`map[uint32]struct{}` is a SignalSet (a 2^32-bit bitmap in HBM).

Empty results are returned as empty arrays (Go returns nil; callers only use
len, and cover_test.go:54 treats two empty results as equal).
"""
import ctypes
from ctypes import byref, c_double, c_int, c_int64, c_size_t, c_uint64, c_void_p

import numpy as np

from . import _lib
from ._lib import call, lib

U32 = np.uint32
U64 = np.uint64


def _p32(a):
    return a.ctypes.data_as(_lib.P32)


def _p64(a):
    return a.ctypes.data_as(_lib.P64)


def _p8(a):
    return a.ctypes.data_as(_lib.P8)


def _u32(a):
    return np.ascontiguousarray(np.asarray(a, dtype=U32).reshape(-1))


def _u64(a):
    return np.ascontiguousarray(np.asarray(a, dtype=U64).reshape(-1))


class Context:
    """One HIP stream on one MI355X plus the device memory it owns."""

    def __init__(self, device=0):
        h = c_void_p()
        call("sg_ctx_create", device, byref(h))
        self.h = h
        self.device = device

    def close(self):
        if self.h:
            lib.sg_ctx_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def sync(self):
        call("sg_ctx_sync", self.h)

    def set_stream(self, hip_stream):
        """Queue on `hip_stream` (an int handle; 0 = the legacy default stream)."""
        call("sg_ctx_set_stream", self.h, c_void_p(hip_stream))

    def reset_stream(self):
        call("sg_ctx_reset_stream", self.h)

    def timing(self, enable):
        call("sg_ctx_timing", self.h, 1 if enable else 0)

    def counter(self, name):
        """sg_ctx_counter: one named 64-bit value of the context.  The names, what each one counts and where
        it lives (a host field, a device word read after a stream sync, a constant of the build) are the rows
        of kCounters in csrc/sg_ctx.hip; an unknown name is SG_EINVAL."""
        v = c_uint64()
        call("sg_ctx_counter", self.h, name.encode(), byref(v))
        return v.value

    def set_option(self, key, value):
        """sg_ctx_set_option: force a path for a test or a measurement (include/syzsig.h lists the keys)."""
        call("sg_ctx_set_option", self.h, key.encode(), int(value))

    def get_option(self, key):
        v = c_int64()
        call("sg_ctx_get_option", self.h, key.encode(), byref(v))
        return v.value

    def kernel_time(self, name):
        ms = c_double()
        n = c_uint64()
        call("sg_ctx_kernel_time", self.h, name.encode(), byref(ms), byref(n))
        return ms.value, n.value


_default = None


def default_context():
    global _default
    if _default is None:
        _default = Context(0)
    return _default


def _ctx(ctx):
    return ctx if ctx is not None else default_context()


class SignalSet:
    """map[uint32]struct{} (syz-fuzzer/fuzzer.go:65-68, syz-manager/manager.go:71-73)."""

    def __init__(self, ctx=None):
        self.ctx = _ctx(ctx)
        h = c_void_p()
        call("sg_set_create", self.ctx.h, byref(h))
        self.h = h

    def close(self):
        if self.h:
            lib.sg_set_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __len__(self):
        n = c_uint64()
        call("sg_set_count", self.h, byref(n))
        return n.value

    def clear(self):
        call("sg_set_clear", self.h)

    def export(self):
        n = c_size_t()
        call("sg_set_export", self.h, None, 0, byref(n))
        out = np.empty(n.value, dtype=U32)
        if n.value:
            call("sg_set_export", self.h, _p32(out), out.size, byref(n))
        return out

    def device_words(self):
        return lib.sg_set_device_words(self.h)

    def or_device(self, ptr):
        call("sg_set_or_dev", self.h, c_void_p(ptr))


# ---- pkg/cover/cover.go:160-182 -------------------------------------------------
def SignalNew(base, signal):
    s = _u32(signal)
    out = c_int()
    call("sg_set_new", base.h, _p32(s), s.size, byref(out))
    return bool(out.value)


def SignalDiff(base, signal):
    s = _u32(signal)
    out = np.empty(s.size, dtype=U32)
    n = c_size_t()
    call("sg_set_diff", base.h, _p32(s), s.size, _p32(out), byref(n))
    return out[: n.value]


def SignalAdd(base, signal):
    s = _u32(signal)
    call("sg_set_add", base.h, _p32(s), s.size)


# ---- pkg/cover/cover.go:28-117 --------------------------------------------------
def Canonicalize(cov, ctx=None):
    """In place on a uint32 numpy array (like Go's slice); returns cov[:n]."""
    if not (isinstance(cov, np.ndarray) and cov.dtype == U32 and cov.flags.c_contiguous):
        cov = _u32(cov)
    n = c_size_t()
    call("sg_canonicalize", _ctx(ctx).h, _p32(cov), cov.size, byref(n))
    return cov[: n.value]


def _merge(op, a, b, ctx):
    a, b = _u32(a), _u32(b)
    out = np.empty(a.size + b.size, dtype=U32)
    n = c_size_t()
    call("sg_merge", _ctx(ctx).h, op, _p32(a), a.size, _p32(b), b.size, _p32(out), byref(n))
    return out[: n.value]


def Difference(cov0, cov1, ctx=None):
    return _merge(_lib.OP_DIFFERENCE, cov0, cov1, ctx)


def SymmetricDifference(cov0, cov1, ctx=None):
    return _merge(_lib.OP_SYMDIFF, cov0, cov1, ctx)


def Union(cov0, cov1, ctx=None):
    return _merge(_lib.OP_UNION, cov0, cov1, ctx)


def Intersection(cov0, cov1, ctx=None):
    return _merge(_lib.OP_INTERSECT, cov0, cov1, ctx)


def union_fold(vals, off, group=None, ngroups=1, ctx=None):
    """The manager's cover.Union folds (syz-manager/html.go:84/:94/:184/:306,
    manager.go:916-917) for every group at once.  Returns (vals, off) with one
    fold per group."""
    vals, off = _u32(vals), _u64(off)
    n = off.size - 1
    g = _u32(group) if group is not None else None
    out = np.empty(max(vals.size, 1), dtype=U32)
    oo = np.zeros(ngroups + 1, dtype=U64)
    call("sg_union_fold", _ctx(ctx).h, _p32(vals), _p64(off), n, _p32(g) if g is not None else None, ngroups,
         _p32(out), out.size, _p64(oo))
    return out[: int(oo[-1])].copy(), oo


def HasDifference(cov0, cov1, ctx=None):
    a, b = _u32(cov0), _u32(cov1)
    out = c_int()
    call("sg_has_difference", _ctx(ctx).h, _p32(a), a.size, _p32(b), b.size, byref(out))
    return bool(out.value)


def has_difference_batch(a, a_beg, a_len, b, b_beg, b_len, ctx=None):
    """HasDifference (cover.go:106-117) of every pair, laid out as merge_batch's:
    a bool array."""
    a, b = _u32(a), _u32(b)
    ab, al, bb, bl = _u64(a_beg), _u64(a_len), _u64(b_beg), _u64(b_len)
    out = np.zeros(max(ab.size, 1), dtype=np.uint8)
    call("sg_has_difference_batch", _ctx(ctx).h, _p32(a), a.size, _p64(ab), _p64(al), _p32(b), b.size, _p64(bb),
         _p64(bl), ab.size, out.ctypes.data)
    return out[: ab.size].astype(bool)


def to_csr(lists):
    lens = np.array([len(x) for x in lists], dtype=U64)
    off = np.zeros(len(lists) + 1, dtype=U64)
    np.cumsum(lens, out=off[1:])
    vals = np.concatenate([_u32(x) for x in lists]) if lists else np.empty(0, dtype=U32)
    return _u32(vals), off


def minimize_order(off):
    off = _u64(off)
    n = off.size - 1
    order = np.empty(n, dtype=U32)
    call("sg_minimize_order", _p64(off), n, _p32(order))
    return order


def minimize_csr(vals, off, order=None, ctx=None):
    vals, off = _u32(vals), _u64(off)
    n = off.size - 1
    order = minimize_order(off) if order is None else _u32(order)
    out = np.empty(n, dtype=U32)
    m = c_size_t()
    call("sg_minimize", _ctx(ctx).h, _p32(vals), _p64(off), n, _p32(order), _p32(out), byref(m))
    return out[: m.value]


def Minimize(corpus, ctx=None):
    """pkg/cover/cover.go:120-146, including its sort.Sort order."""
    vals, off = to_csr(corpus)
    return [int(i) for i in minimize_csr(vals, off, None, ctx)]


# ---- batched hot path -------------------------------------------------------------
def triage_batch(maxset, newset, vals, rec_off, want_diff=True, ctx=None):
    """syz-fuzzer/fuzzer.go:645-693 over a batch of call records.

    Returns (rec_new uint8[nrec], diff_vals, diff_off) -- diff_* None if not
    requested."""
    vals, off = _u32(vals), _u64(rec_off)
    nrec = off.size - 1
    rec_new = np.zeros(nrec, dtype=np.uint8)
    c = maxset.ctx if ctx is None else ctx
    if want_diff:
        dv = np.empty(max(vals.size, 1), dtype=U32)
        do = np.empty(nrec + 1, dtype=U64)
        nd = c_uint64()
        call("sg_triage_batch", c.h, maxset.h, newset.h if newset is not None else None, _p32(vals), _p64(off), nrec,
             _p8(rec_new), _p32(dv), _p64(do), byref(nd))
        return rec_new, dv[: nd.value], do
    call("sg_triage_batch", c.h, maxset.h, newset.h if newset is not None else None, _p32(vals), _p64(off), nrec, _p8(rec_new),
         None, None, None)
    return rec_new, None, None


def triage_traces(maxset, newset, pcs, call_off, ctx=None):
    """fuzzer.go:645-693 over a batch given as raw per-call PC traces (set-exact
    edge signal, executor.h:389-401): the per-call flags, sets updated."""
    p, off = _u32(pcs), _u64(call_off)
    ncalls = off.size - 1
    rec_new = np.zeros(ncalls, dtype=np.uint8)
    c = maxset.ctx if ctx is None else ctx
    call("sg_triage_traces", c.h, maxset.h, newset.h if newset is not None else None, _p32(p), _p64(off), ncalls,
         _p8(rec_new))
    return rec_new


def triage_traces_queued(maxset, newset, pcs, call_off, prog_off, ctx=None):
    """The fuzzer's step from raw traces (sg_triage_traces_queued): the
    per-call flags of fuzzer.go:645-693 (sets updated, set-exact) and the
    executor-exact signal list of every queued call (fuzzer.go:678-683;
    executor.h:389-401), empty for the others.  Returns (rec_new, vals, off)."""
    p, co, po = _u32(pcs), _u64(call_off), _u64(prog_off)
    ncalls = co.size - 1
    rec_new = np.zeros(max(ncalls, 1), dtype=np.uint8)
    sv = np.empty(max(p.size, 1), dtype=U32)
    so = np.empty(ncalls + 1, dtype=U64)
    c = maxset.ctx if ctx is None else ctx
    call("sg_triage_traces_queued", c.h, maxset.h, newset.h if newset is not None else None, _p32(p), _p64(co),
         _p64(po), po.size - 1, _p8(rec_new), _p32(sv), _p64(so))
    return rec_new[:ncalls], sv[: int(so[-1])], so


def add_inputs(corpus, maxset, vals, off, ctx=None):
    """syz-fuzzer/fuzzer.go:467-489 addInput over a batch of inputs."""
    vals, off = _u32(vals), _u64(off)
    c = corpus.ctx if ctx is None else ctx
    call("sg_add_inputs", c.h, corpus.h, maxset.h, _p32(vals), _p64(off), off.size - 1)


def triage_newsig(corpus, vals, off, ctx=None):
    """syz-fuzzer/fuzzer.go:526-532 over a batch of triage inputs:
    new_k = Canonicalize(SignalDiff(corpusSignal, S_k)).  Returns (vals, off)."""
    vals, off = _u32(vals), _u64(off)
    n = off.size - 1
    nv = np.empty(max(vals.size, 1), dtype=U32)
    no = np.zeros(n + 1, dtype=U64)
    c = corpus.ctx if ctx is None else ctx
    call("sg_triage_newsig", c.h, corpus.h, _p32(vals), _p64(off), n, _p32(nv), _p64(no))
    return nv[: int(no[-1])], no


def triage_intersect(new_vals, new_off, r_vals, r_off, ctx=None):
    """fuzzer.go:567 over a batch: new_k = Intersection(new_k, Canonicalize(R_k)).
    Returns the packed (vals, off)."""
    nv, no = _u32(new_vals).copy(), _u64(new_off)
    rv, ro = _u32(r_vals), _u64(r_off)
    n = no.size - 1
    lens = np.zeros(n, dtype=U64)
    call("sg_triage_intersect", _ctx(ctx).h, _p32(nv), _p64(no), _p32(rv), _p64(ro), n, _p64(lens))
    out_off = np.concatenate([[0], np.cumsum(lens)]).astype(U64)
    out = np.concatenate([nv[int(no[k]): int(no[k]) + int(lens[k])] for k in range(n)]) if n else nv[:0]
    return out.astype(U32), out_off


def triage_subset(new_vals, new_off, r_vals, r_off, ctx=None):
    """fuzzer.go:584-587, the minimisation predicate over a batch:
    ok[k] = len(Intersection(new_k, Canonicalize(R_k))) == len(new_k)."""
    nv, no = _u32(new_vals), _u64(new_off)
    rv, ro = _u32(r_vals), _u64(r_off)
    n = no.size - 1
    ok = np.zeros(n, dtype=np.uint8)
    call("sg_triage_subset", _ctx(ctx).h, _p32(nv), _p64(no), _p32(rv), _p64(ro), n, _p8(ok))
    return ok


def accept_batch(corpus_sig, corpus_cov, sig_vals, sig_off, cov_vals=None, cov_off=None, ctx=None):
    """syz-manager/manager.go:907-912 NewInput acceptance over a batch."""
    sv, so = _u32(sig_vals), _u64(sig_off)
    n = so.size - 1
    acc = np.zeros(n, dtype=np.uint8)
    c = corpus_sig.ctx if ctx is None else ctx
    if corpus_cov is not None and cov_vals is not None:
        cv, co = _u32(cov_vals), _u64(cov_off)
        call("sg_accept_batch", c.h, corpus_sig.h, corpus_cov.h, _p32(sv), _p64(so), _p32(cv), _p64(co), n, _p8(acc))
    else:
        call("sg_accept_batch", c.h, corpus_sig.h, None, _p32(sv), _p64(so), None, None, n, _p8(acc))
    return acc


def merge_poll(mgr_max, a_vals, a_off, ctx=None):
    """syz-manager/manager.go:949-956 over polls in arrival order."""
    av, ao = _u32(a_vals), _u64(a_off)
    npoll = ao.size - 1
    nv = np.empty(max(av.size, 1), dtype=U32)
    no = np.empty(npoll + 1, dtype=U64)
    c = mgr_max.ctx if ctx is None else ctx
    call("sg_merge_poll", c.h, mgr_max.h, _p32(av), _p64(ao), npoll, _p32(nv), _p64(no))
    return nv[: int(no[-1])], no


# ---- RPC payloads (pkg/rpctype/rpctype.go:8-63) ------------------------------------
def delta_encode(vals, off, ctx=None):
    """Sorted lists -> their delta-varint payloads (bytes, byte offsets)."""
    vals, off = _u32(vals), _u64(off)
    n = off.size - 1
    bo = np.zeros(n + 1, dtype=U64)
    out = np.empty(max(5 * vals.size, 1), dtype=np.uint8)
    call("sg_delta_encode_batch", _ctx(ctx).h, _p32(vals), _p64(off), n, _p8(out), out.size, _p64(bo))
    return out[: int(bo[-1])].copy(), bo


def delta_decode(data, data_off, ctx=None):
    """Payloads -> the sorted lists (vals, off)."""
    data = np.ascontiguousarray(np.frombuffer(bytes(data), dtype=np.uint8) if isinstance(data, (bytes, bytearray))
                                else np.asarray(data, dtype=np.uint8))
    do = _u64(data_off)
    n = do.size - 1
    vals = np.empty(max(data.size, 1), dtype=U32)
    off = np.zeros(n + 1, dtype=U64)
    call("sg_delta_decode_batch", _ctx(ctx).h, _p8(data), _p64(do), n, _p32(vals), vals.size, _p64(off))
    return vals[: int(off[-1])].copy(), off


def set_encode(sset):
    """The set's members as one payload (PollArgs / ConnectRes / PollRes .MaxSignal)."""
    nb = c_size_t()
    call("sg_set_encode", sset.h, None, 0, byref(nb))
    out = np.empty(max(nb.value, 1), dtype=np.uint8)
    call("sg_set_encode", sset.h, _p8(out), out.size, byref(nb))
    return out[: nb.value].tobytes()


def set_decode_add(sset, payload):
    """SignalAdd of a payload (fuzzer.go:146-151, :392-398); returns its value count."""
    data = np.frombuffer(bytes(payload), dtype=np.uint8).copy()
    cnt = c_uint64()
    call("sg_set_decode_add", sset.h, _p8(data), data.size, byref(cnt))
    return cnt.value


def sancov(cov_vals, cov_off, ctx=None):
    """tools/syz-execprog/execprog.go:159-177 sancov files of a batch of calls (list of bytes)."""
    cv, co = _u32(cov_vals), _u64(cov_off)
    n = co.size - 1
    out = np.empty(max(8 * (n + cv.size), 1), dtype=np.uint8)
    call("sg_sancov_batch", _ctx(ctx).h, _p32(cv), _p64(co), n, _p8(out))
    return [out[8 * (k + int(co[k])): 8 * (k + 1 + int(co[k + 1]))].tobytes() for k in range(n)]


def canonicalize_batch(vals, off, ctx=None):
    """Batched Canonicalize in place; returns per-segment canonical lengths."""
    if not (isinstance(vals, np.ndarray) and vals.dtype == U32 and vals.flags.c_contiguous):
        raise TypeError("canonicalize_batch works in place on a contiguous uint32 array")
    off = _u64(off)
    n = off.size - 1
    lens = np.zeros(n, dtype=U64)
    call("sg_canonicalize_batch", _ctx(ctx).h, _p32(vals), _p64(off), n, _p64(lens))
    return lens


def merge_batch(op, a, a_beg, a_len, b, b_beg, b_len, ctx=None):
    a, b = _u32(a), _u32(b)
    ab, al, bb, bl = _u64(a_beg), _u64(a_len), _u64(b_beg), _u64(b_len)
    npair = ab.size
    ob = np.zeros(npair, dtype=U64)
    if npair > 1:
        np.cumsum(al[:-1] + bl[:-1], out=ob[1:])
    total = int((al + bl).sum())
    out = np.empty(max(total, 1), dtype=U32)
    ol = np.zeros(npair, dtype=U64)
    call("sg_merge_batch", _ctx(ctx).h, op, _p32(a), a.size, _p64(ab), _p64(al), _p32(b), b.size, _p64(bb),
         _p64(bl), npair, _p32(out), out.size, _p64(ob), _p64(ol))
    return [out[int(ob[k]): int(ob[k] + ol[k])] for k in range(npair)]


def exec_signal(pcs, call_off, prog_off, ctx=None):
    """executor/executor.h:389-401 + :497-526 over a batch of programs."""
    p, co, po = _u32(pcs), _u64(call_off), _u64(prog_off)
    ncalls = co.size - 1
    sv = np.empty(max(p.size, 1), dtype=U32)
    so = np.empty(ncalls + 1, dtype=U64)
    call("sg_exec_signal", _ctx(ctx).h, _p32(p), _p64(co), _p64(po), po.size - 1, _p32(sv), _p64(so))
    return sv[: int(so[-1])], so


EXEC_COVER_FAST_CAP = 8192  # include/syzsig.h SG_EXEC_COVER_FAST_CAP: a call's distinct PCs on the fast shape


def exec_cover(pcs, call_off, dedup=True, ctx=None):
    """handle_completion's flag_collect_cover branch (executor/executor.h:402-415)
    over a batch of raw KCOV buffers: pcs u64, call c's PCs
    pcs[call_off[c]:call_off[c + 1]].  Returns (cov u32, cov_off): call c's Cover
    is cov[cov_off[c]:cov_off[c + 1]] -- with dedup (flag_dedup_cover) its
    distinct PCs in u64 order, truncated after the unique (so PCs that differ
    only above bit 31 stay separate entries); without it every PC truncated, in
    trace order."""
    p, co = _u64(pcs), _u64(call_off)
    ncalls = co.size - 1
    npcs = int(co[-1])
    assert p.size == npcs
    cvo = np.empty(ncalls + 1, dtype=U64)
    cov = np.empty(max(npcs, 1), dtype=U32)
    call("sg_exec_cover", _ctx(ctx).h, _p64(p), _p64(co), ncalls, 1 if dedup else 0, _p64(cvo), _p32(cov), npcs)
    return cov[: int(cvo[-1])], cvo


def triage_runs_from_kcov(corpus, sig_vals, sig_off, call, minimized, nruns, pcs, call_off, prog_off, ctx=None):
    """triageInput's loop (syz-fuzzer/fuzzer.go:521-576) for n candidates from the
    raw KCOV buffers of their nruns re-executions each: candidate k's inp.signal
    is sig_vals[sig_off[k]:sig_off[k + 1]], its call call[k], its runs the
    executions k * nruns .. (k + 1) * nruns - 1, execution e's calls
    prog_off[e] .. prog_off[e + 1], call c's u64 PCs pcs[call_off[c]:call_off[c + 1]].
    Returns (status int32[n], new_vals, new_off, cov_vals, cov_off): newSignal
    and inputCover per candidate, both empty unless status is TIN_OK."""
    sv, so, cl, mn = _u32(sig_vals), _u64(sig_off), _u32(call), np.ascontiguousarray(np.asarray(minimized, np.uint8))
    p, co, po = _u64(pcs), _u64(call_off), _u64(prog_off)
    n = so.size - 1
    assert cl.size == n and mn.size == n and po.size == n * nruns + 1 and co.size == int(po[-1]) + 1
    status = np.empty(max(n, 1), dtype=np.int32)
    no, vo = np.empty(n + 1, dtype=U64), np.empty(n + 1, dtype=U64)
    nv, cv = np.empty(max(sv.size, 1), dtype=U32), np.empty(max(p.size, 1), dtype=U32)
    _lib.call("sg_triage_runs_from_kcov", corpus.ctx.h if ctx is None else ctx.h, corpus.h, _p32(sv), _p64(so), n,
              _p32(cl), _p8(mn), nruns, _p64(p), _p64(co), _p64(po),
              status.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), _p64(no), _p32(nv), sv.size, _p64(vo), _p32(cv), p.size)
    return status[:n], nv[: int(no[-1])], no, cv[: int(vo[-1])], vo


def TriageInput(corpus, signal, call, runs, minimized=False):
    """triageInput (fuzzer.go:521-576) up to prog.Minimize for one candidate:
    signal is inp.signal, call inp.call, runs the re-executions, each a list of
    per-call u64 PC arrays (an empty list: the execution returned no info).
    Returns (status, newSignal, inputCover)."""
    calls = [np.asarray(c, dtype=U64).reshape(-1) for r in runs for c in r]
    prog_off = np.concatenate([[0], np.cumsum([len(r) for r in runs])]).astype(U64)
    call_off = np.concatenate([[0], np.cumsum([c.size for c in calls])]).astype(U64)
    pcs = np.concatenate(calls) if calls else np.zeros(0, dtype=U64)
    sig = _u32(signal)
    status, nv, _, cv, _ = triage_runs_from_kcov(corpus, sig, [0, sig.size], [call], [1 if minimized else 0], len(runs),
                                                 pcs, call_off, prog_off)
    return int(status[0]), nv, cv


def minimize_pred_from_kcov(new_vals, new_off, cand, call, pcs, call_off, prog_off, maxset=None, newset=None, ctx=None):
    """The predicate triageInput hands to prog.Minimize (fuzzer.go:578-591) for n
    attempts from the raw KCOV buffers of their executions: attempt e tests the
    sorted list new_vals[new_off[cand[e]]:new_off[cand[e] + 1]] on call call[e]
    of execution e, whose calls are prog_off[e] .. prog_off[e + 1], call c's u64
    PCs pcs[call_off[c]:call_off[c + 1]].  Returns status int32[n] (MP_OK,
    MP_NOT_EXECUTED, MP_LOST) and, with maxset, also (rec_new, sig_vals,
    sig_off): execute()'s new-signal check of every call (both sets updated, as
    triage_traces) and the executor's lists of the queued or selected calls."""
    nv, no, cd, cl = _u32(new_vals), _u64(new_off), _u32(cand), _u32(call)
    p, co, po = _u64(pcs), _u64(call_off), _u64(prog_off)
    n, ncalls = po.size - 1, co.size - 1
    assert cd.size == n and cl.size == n and ncalls == int(po[-1]) and p.size == int(co[-1]) and nv.size == int(no[-1])
    if newset is not None and maxset is None:
        raise ValueError("newset only with maxset")
    c = ctx if ctx is not None else (maxset.ctx if maxset is not None else default_context())
    status = np.empty(max(n, 1), dtype=np.int32)
    rec_new = np.zeros(max(ncalls, 1), dtype=np.uint8)
    sv, so = np.empty(max(p.size, 1), dtype=U32), np.zeros(ncalls + 1, dtype=U64)
    _lib.call("sg_minimize_pred_from_kcov", c.h, maxset.h if maxset is not None else None,
              newset.h if newset is not None else None, _p32(nv), _p64(no), no.size - 1, _p32(cd), _p32(cl), n, _p64(p),
              _p64(co), _p64(po), status.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), _p8(rec_new), _p64(so),
              _p32(sv), p.size)
    if maxset is None:
        return status[:n]
    return status[:n], rec_new[:ncalls], sv[: int(so[-1])], so


class MinimizePred:
    """The closure of fuzzer.go:578-591 for one candidate: pred(run, call1) ->
    bool, where run is the shortened program's execution as a list of per-call
    u64 PC arrays (as in TriageInput) and new_signal is triageInput's newSignal.
    With maxset (and newset) every call also goes through execute()'s
    new-signal check, as the reference's execute() does."""

    def __init__(self, new_signal, maxset=None, newset=None, ctx=None):
        self.new = _u32(new_signal)
        self.maxset, self.newset, self.ctx = maxset, newset, ctx

    def __call__(self, run, call1):
        calls = [np.asarray(c, dtype=U64).reshape(-1) for c in run]
        call_off = np.concatenate([[0], np.cumsum([c.size for c in calls])]).astype(U64)
        pcs = np.concatenate(calls) if calls else np.zeros(0, dtype=U64)
        res = minimize_pred_from_kcov(self.new, [0, self.new.size], [0], [call1], pcs, call_off, [0, len(calls)],
                                      self.maxset, self.newset, self.ctx)
        status = res if self.maxset is None else res[0]
        return int(status[0]) == _lib.MP_OK


def cover_uncovered(cov, base, sym_start, sym_end, all_pcs, ctx=None):
    """syz-manager/cover.go:91-103 + uncoveredPcsInFuncs (:257-307); ascending."""
    c, ss, se, ap = _u32(cov), _u64(sym_start), _u64(sym_end), _u64(all_pcs)
    out = np.empty(max(ap.size, 1), dtype=U64)
    n = c_size_t()
    call("sg_cover_uncovered", _ctx(ctx).h, _p32(c), c.size, base, _p64(ss), _p64(se), ss.size, _p64(ap), ap.size,
         _p64(out), byref(n))
    return out[: n.value]


INGEST_MAX_LINE = 65536  # bufio.MaxScanTokenSize (include/syzsig.h SG_INGEST_MAX_LINE)


class LineTooLong(ValueError):
    """bufio.Scanner's ErrTooLong for a tool's output: `pos` is the byte offset of the first line whose content
    is INGEST_MAX_LINE bytes or more."""

    def __init__(self, fn, pos):
        super().__init__(f"{fn}: bufio.Scanner: token too long (the line at byte {pos})")
        self.pos = pos


def _text_u8(text):
    if isinstance(text, np.ndarray):
        return np.ascontiguousarray(text.astype(np.uint8, copy=False).reshape(-1))
    return np.frombuffer(text, dtype=np.uint8)


def objdump_pcs(text, call=b"callq ", func=b" <__sanitizer_cov_trace_pc>", ctx=None):
    """coveredPCs (syz-manager/cover.go:310-347) over the bytes of `objdump -d --no-show-raw-insn vmlinux`, and
    initAllCover's sort (:78): the call sites' PCs ascending, duplicates kept.  call / func are the two needles
    (newer binutils print b"call ").  Raises LineTooLong where the reference returns the scanner's error."""
    t = _text_u8(text)
    nc, nf = np.frombuffer(bytes(call), dtype=np.uint8), np.frombuffer(bytes(func), dtype=np.uint8)
    cap = t.size // 2 + 1  # (a kept line is at least a digit and ':': the needles may overlap the field)
    pcs = np.empty(cap, dtype=U64)
    n, st, pos = c_size_t(), ctypes.c_uint32(), c_uint64()
    _lib.call("sg_objdump_pcs", _ctx(ctx).h, _p8(t), t.size, _p8(nc), nc.size, _p8(nf), nf.size, _p64(pcs), cap,
              byref(n), byref(st), byref(pos))  # (`call` is the needle here)
    if st.value:
        raise LineTooLong("objdump_pcs", pos.value)
    return pcs[: n.value]


class NmSymbols:
    """nm_symbols' result.  Symbol k in text order: addr[k], size[k] (rounded up to 16 as ReadSymbols does) and
    name(k); sym_start / sym_end in the order cover_uncovered and CoverTable want (start, then text order), and
    order[j] the text-order index of sorted place j."""

    def __init__(self, text, addr, size, name_pos, name_len, sym_start, sym_end, order):
        self.text = text
        self.addr, self.size, self.name_pos, self.name_len = addr, size, name_pos, name_len
        self.sym_start, self.sym_end, self.order = sym_start, sym_end, order

    def __len__(self):
        return int(self.addr.size)

    def name(self, k):
        p = int(self.name_pos[k])
        return self.text[p:p + int(self.name_len[k])].tobytes()


def nm_symbols(text, ctx=None):
    """symbolizer.ReadSymbols (pkg/symbolizer/nm.go:19-69) over the bytes of `nm -nS vmlinux`, then the flatten and
    sort of uncoveredPcsInFuncs (cover.go:262-268).  Raises LineTooLong as objdump_pcs does."""
    t = _text_u8(text)
    cap = t.size // 6 + 1
    addr, npos, ss, se = (np.empty(cap, dtype=U64) for _ in range(4))
    size = np.empty(cap, dtype=np.int64)
    nlen, order = np.empty(cap, dtype=U32), np.empty(cap, dtype=U32)
    n, st, pos = c_size_t(), ctypes.c_uint32(), c_uint64()
    _lib.call("sg_nm_symbols", _ctx(ctx).h, _p8(t), t.size, _p64(addr), size.ctypes.data_as(ctypes.POINTER(c_int64)),
              _p64(npos), _p32(nlen), _p64(ss), _p64(se), _p32(order), cap, byref(n), byref(st), byref(pos))
    if st.value:
        raise LineTooLong("nm_symbols", pos.value)
    k = n.value
    return NmSymbols(t, addr[:k], size[:k], npos[:k], nlen[:k], ss[:k], se[:k], order[:k])


A2L_OK, A2L_EMPTY, A2L_BAD_PC, A2L_NO_COLON, A2L_NO_FILE_LINE, A2L_TOO_LONG, A2L_TOO_FEW = 0, 1, 2, 3, 4, 5, 6
_A2L_WHAT = {A2L_EMPTY: "EOF", A2L_BAD_PC: "failed to parse pc in addr2line output",
             A2L_NO_COLON: "failed to parse file:line in addr2line output",
             A2L_NO_FILE_LINE: "failed to read file:line from addr2line: EOF",
             A2L_TOO_LONG: "bufio.Scanner: token too long", A2L_TOO_FEW: "fewer records than PCs"}


class Addr2lineError(ValueError):
    """symbolize's error for a whole addr2line output: `status` (A2L_*, include/syzsig.h SG_A2L_*) and `pos`, the
    byte offset of the failing line."""

    def __init__(self, status, pos):
        super().__init__(f"addr2line_frames: {_A2L_WHAT.get(status, status)} (byte {pos})")
        self.status, self.pos = status, pos


class Addr2lineFrames:
    """addr2line_frames' result: rec_pc[r] and, for record r, frames frame_off[r]:frame_off[r+1] of frame_file /
    frame_line / frame_func; file id k is file(k), func id k is func(k), ids in order of first occurrence."""

    def __init__(self, text, rec_pc, frame_off, frame_file, frame_line, frame_func, spans, rounds):
        self.text, self.rec_pc, self.frame_off = text, rec_pc, frame_off
        self.frame_file, self.frame_line, self.frame_func = frame_file, frame_line, frame_func
        self.file_pos, self.file_len, self.func_pos, self.func_len = spans
        self.nfiles, self.nfuncs, self.rounds = int(self.file_pos.size), int(self.func_pos.size), rounds

    def _names(self, pos, ln):
        t = self.text.tobytes()
        return [t[p:p + n] for p, n in zip(pos.tolist(), ln.tolist())]

    def files(self):
        return self._names(self.file_pos, self.file_len)

    def funcs(self):
        return self._names(self.func_pos, self.func_len)


def addr2line_frames(text, nrec, hash_bits=64, ctx=None):
    """symbolize / parse (pkg/symbolizer/symbolizer.go:95-191) over the bytes `addr2line -afi` wrote for nrec PCs
    (and its sentinel), with File and Func interned on the device.  Raises Addr2lineError where the reference
    returns an error.  hash_bits below 64 only forces the interning's other rounds (tests)."""
    t = _text_u8(text)
    nrec = int(nrec)
    rec_pc, frame_off, info = np.zeros(max(nrec, 1), dtype=U64), np.zeros(nrec + 1, dtype=U64), np.zeros(6, dtype=U64)
    cap = t.size // 32 + 1  # a guess; the call is made again with the count when the frames outnumber it
    for _ in range(2):
        ff, fu, fl_len, fn_len = (np.empty(cap, dtype=U32) for _ in range(4))
        line = np.empty(cap, dtype=np.int64)
        fl_pos, fn_pos = np.empty(cap, dtype=U64), np.empty(cap, dtype=U64)
        _lib.call("sg_addr2line_frames", _ctx(ctx).h, _p8(t), t.size, nrec, _p64(rec_pc), _p64(frame_off), _p32(ff),
                  line.ctypes.data_as(ctypes.POINTER(c_int64)), _p32(fu), cap, _p64(fl_pos), _p32(fl_len), _p64(fn_pos),
                  _p32(fn_len), hash_bits, _p64(info))
        nfr, nfiles, nfuncs, status, pos, rounds = (int(x) for x in info)
        if nfr <= cap:
            break
        cap = nfr
    if status:
        raise Addr2lineError(status, pos)
    return Addr2lineFrames(t, rec_pc[:nrec], frame_off, ff[:nfr], line[:nfr], fu[:nfr],
                           (fl_pos[:nfiles], fl_len[:nfiles], fn_pos[:nfuncs], fn_len[:nfuncs]), rounds)


_GO_SPACE = ("\t\n\v\f\r \u0085\u00a0\u1680\u2000\u2001\u2002\u2003\u2004\u2005\u2006\u2007\u2008\u2009\u200a"
             "\u2028\u2029\u202f\u205f\u3000")  # unicode.IsSpace, which strings.Fields splits at


def _parse_uint_0x(digits):
    """strconv.ParseUint("0x" + digits, 0, 64), or None: base 0 lets '_' separate digits (and follow the prefix)."""
    last = "0"
    for c in digits:
        if c in "0123456789abcdefABCDEF":
            last = "0"
        elif c == "_" and last == "0":
            last = "_"
        else:
            return None
    digits = digits.replace("_", "")
    if last == "_" or not digits:
        return None
    v = int(digits, 16)
    return v if v < 1 << 64 else None


def vm_offset(readelf_text):
    """getVmOffset (syz-manager/cover.go:219-254) over the bytes of `readelf -SW vmlinux`: the upper 32 bits that
    every non-zero PROGBITS address shares.  Host only (a few KB of text).  ValueError where the reference returns
    an error, and also where it panics (PROGBITS as a line's last field: pieces[i+1] is out of range).  The
    reference never looks at its scanner's error, so a line of INGEST_MAX_LINE bytes or more ends the scan there
    and what came before it counts."""
    data = bytes(readelf_text)
    addr, s = 0, 0
    while s < len(data):
        e = data.find(b"\n", s)
        e = len(data) if e < 0 else e
        if e - s >= INGEST_MAX_LINE:
            break
        ln = data[s:e - 1] if e > s and data[e - 1:e] == b"\r" else data[s:e]
        s = e + 1
        pieces = [p for p in ln.decode("utf-8", "replace").translate({ord(c): " " for c in _GO_SPACE}).split(" ") if p]
        for i, p in enumerate(pieces):
            if p != "PROGBITS":
                continue
            if i + 1 >= len(pieces):
                raise ValueError("vm_offset: PROGBITS is the last field of a line (the reference panics)")
            v = _parse_uint_0x(pieces[i + 1])
            if v is None:
                raise ValueError(f"failed to parse addr in readelf output: {pieces[i + 1]!r}")
            if v == 0:
                continue
            v32 = v >> 32
            if addr == 0:
                addr = v32
            if addr != v32:
                raise ValueError("different section offsets in a single binary")
    return addr


class CoverTable:
    """sg_cover_table: the symbols, the call sites and the frames of every
    symbolised PC, on the device (include/syzsig.h).  The frames of tab_pcs[j]
    are entries frame_off[j] .. frame_off[j+1] of frame_file / frame_line /
    frame_func; the caller interns File and Func strings to ids (equal strings,
    equal ids).  Close it before its context."""

    def __init__(self, sym_start, sym_end, all_pcs, tab_pcs, frame_off, frame_file, frame_line, frame_func, nfiles,
                 nfuncs, ctx=None):
        self.ctx = _ctx(ctx)
        ss, se, ap, tp, fo = _u64(sym_start), _u64(sym_end), _u64(all_pcs), _u64(tab_pcs), _u64(frame_off)
        ff, fl, fn = _u32(frame_file), _u32(frame_line), _u32(frame_func)
        if ss.size != se.size or fo.size != tp.size + 1 or not ff.size == fl.size == fn.size == int(fo[-1]):
            raise ValueError("CoverTable: array lengths do not agree")
        self.nfiles, self.nfuncs = int(nfiles), int(nfuncs)
        h = c_void_p()
        call("sg_cover_table_create", self.ctx.h, _p64(ss), _p64(se), ss.size, _p64(ap), ap.size, _p64(tp), tp.size,
             _p64(fo), _p32(ff), _p32(fl), _p32(fn), self.nfiles, self.nfuncs, byref(h))
        self._adopt(h)

    def _adopt(self, h):
        self.h = h
        n = c_uint64()
        call("sg_cover_table_slots", self.h, byref(n))
        self.nslots = n.value

    @classmethod
    def from_text(cls, nm_text, all_pcs, addr2line_text, nrec=None, hash_bits=64, ctx=None):
        """The table from the tools' text in one call (sg_cover_table_from_text): `nm -nS` output, the call sites
        (objdump_pcs' result: ascending, distinct) and what `addr2line -afi` wrote for nrec PCs that include them
        (default: exactly the call sites).  The records' PCs and the frame arrays never leave the device.  Returns
        (table, files, funcs), the names as bytes by id, ids in order of first occurrence."""
        c = _ctx(ctx)
        nm, at, ap = _text_u8(nm_text), _text_u8(addr2line_text), _u64(all_pcs)
        nrec = ap.size if nrec is None else int(nrec)
        cap = at.size // 32 + 1  # a guess; the call is made again with the count when the frames outnumber it
        info, h = np.zeros(8, dtype=U64), c_void_p()
        for _ in range(2):
            fpos, upos = np.empty(cap, dtype=U64), np.empty(cap, dtype=U64)
            flen, ulen = np.empty(cap, dtype=U32), np.empty(cap, dtype=U32)
            call("sg_cover_table_from_text", c.h, _p8(nm), nm.size, _p64(ap), ap.size, _p8(at), at.size, nrec, hash_bits,
                 _p64(fpos), _p32(flen), _p64(upos), _p32(ulen), cap, _p64(info), byref(h))
            nfr, nfiles, nfuncs, status, pos, _, nm_status, nm_pos = (int(x) for x in info)
            if nm_status:
                raise LineTooLong("nm_symbols", nm_pos)
            if status:
                raise Addr2lineError(status, pos)
            if nfr <= cap:
                break
            cap = nfr
        self = cls.__new__(cls)
        self.ctx, self.nfiles, self.nfuncs = c, nfiles, nfuncs
        self._adopt(h)
        t = at.tobytes()
        files = [t[p:p + n] for p, n in zip(fpos[:nfiles].tolist(), flen[:nfiles].tolist())]
        funcs = [t[p:p + n] for p, n in zip(upos[:nfuncs].tolist(), ulen[:nfuncs].tolist())]
        return self, files, funcs

    def close(self):
        if self.h:
            lib.sg_cover_table_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def cover_lines(table, cov, base):
    """generateCoverHtml's set math and fileSet (syz-manager/cover.go:91-120, :165-196) on a CoverTable.  cov: an
    array of cover PCs (low 32 bits), or a SignalSet for the set form (its members, ascending; nothing uploaded).
    Returns (file_off, lines, covered, file_seen, ncovered_frames, missing): file f's lines are
    lines[file_off[f]:file_off[f+1]], ascending, covered[] alongside."""
    nf = table.nfiles
    file_off = np.zeros(nf + 1, dtype=U64)
    lines = np.empty(max(table.nslots, 1), dtype=U32)
    covered = np.empty(max(table.nslots, 1), dtype=np.uint8)
    seen = np.zeros(max(nf, 1), dtype=np.uint8)
    ncf, nm = c_uint64(), c_size_t()
    if isinstance(cov, SignalSet):
        missing = np.empty(max(len(cov), 1), dtype=U64)
        call("sg_cover_lines_set", table.h, cov.h, base, _p64(file_off), _p32(lines), _p8(covered), _p8(seen),
             byref(ncf), _p64(missing), byref(nm))
    else:
        c = _u32(cov)
        missing = np.empty(max(c.size, 1), dtype=U64)
        call("sg_cover_lines", table.h, _p32(c), c.size, base, _p64(file_off), _p32(lines), _p8(covered), _p8(seen),
             byref(ncf), _p64(missing), byref(nm))
    total = int(file_off[nf])
    return file_off, lines[:total], covered[:total], seen[:nf], ncf.value, missing[: nm.value]


class SourceTable:
    """sg_src_table: parseFile (syz-manager/cover.go:198-217) of every source file, once, on the device
    (include/syzsig.h).  File f is the CoverTable's file id f and its bytes are bytes[off[f]:off[f+1]]; have[f] == 0
    is a file that could not be read (its range empty).  Close it before its context."""

    def __init__(self, have, bytes, off, ctx=None):
        self.ctx = _ctx(ctx)
        hv = np.ascontiguousarray(np.asarray(have, dtype=np.uint8).reshape(-1))
        by = np.ascontiguousarray(np.asarray(bytes, dtype=np.uint8).reshape(-1) if isinstance(bytes, np.ndarray)
                                  else np.frombuffer(bytes, dtype=np.uint8))  # (else: bytes-like)
        of = _u64(off)
        if of.size != hv.size + 1 or int(of[-1]) != by.size:
            raise ValueError("SourceTable: array lengths do not agree")
        self.nfiles = int(hv.size)
        h = c_void_p()
        call("sg_src_table_create", self.ctx.h, _p8(hv), _p8(by), _p64(of), self.nfiles, byref(h))
        self.h = h

    def close(self):
        if self.h:
            lib.sg_src_table_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def counts(self):
        """(file_line_off, lines, stored bytes, raw bytes): file f's lines are file_line_off[f]:file_line_off[f+1]."""
        flo, tot = np.zeros(self.nfiles + 1, dtype=U64), np.zeros(3, dtype=U64)
        call("sg_src_table_counts", self.h, _p64(flo), _p64(tot))
        return flo, int(tot[0]), int(tot[1]), int(tot[2])

    def lines(self):
        """parseFile's result per file: [[line, ...], ...] as bytes, without the stored '\\n'."""
        flo, nlines, stored, _ = self.counts()
        lo, text = np.zeros(nlines + 1, dtype=U64), np.zeros(max(stored, 1), dtype=np.uint8)
        call("sg_src_table_export", self.h, _p64(lo), _p8(text))
        t, lo = text[:stored].tobytes(), lo.tolist()
        return [[t[lo[i]:lo[i + 1] - 1] for i in range(int(flo[f]), int(flo[f + 1]))] for f in range(self.nfiles)]


_pages_buf = [np.zeros(1 << 20, dtype=np.uint8)]  # cover_pages' grow-only host buffer for the bodies


def cover_pages(table, src, cov, base):
    """cover_lines, then generateCoverHtml's loop over fileSet's map (syz-manager/cover.go:122-156) on a SourceTable,
    in one call.  Returns cover_lines' tuple plus (body_off, bodies, coverage, bad_file): file f's Body is
    bodies[body_off[f]:body_off[f+1]] and its Coverage coverage[f]; bad_file is the lowest file of the report that
    could not be read (then nothing is rendered), else None.  The bodies land in a buffer that only grows (the
    library is called a second time only when they did not fit it); `bodies` is a view of it, good until the next
    call."""
    nf = table.nfiles
    file_off = np.zeros(nf + 1, dtype=U64)
    lines = np.empty(max(table.nslots, 1), dtype=U32)
    covered = np.empty(max(table.nslots, 1), dtype=np.uint8)
    seen = np.zeros(max(nf, 1), dtype=np.uint8)
    body_off, coverage = np.zeros(nf + 1, dtype=U64), np.zeros(max(nf, 1), dtype=U32)
    ncf, nm, nb, bad = c_uint64(), c_size_t(), c_size_t(), ctypes.c_uint32()
    is_set = isinstance(cov, SignalSet)
    c = None if is_set else _u32(cov)
    missing = np.empty(max(len(cov) if is_set else c.size, 1), dtype=U64)
    for _ in range(2):
        buf = _pages_buf[0]
        outs = (_p64(file_off), _p32(lines), _p8(covered), _p8(seen), byref(ncf), _p64(missing), byref(nm),
                _p64(body_off), _p32(coverage), _p8(buf), buf.size, byref(nb), byref(bad))
        if is_set:
            call("sg_cover_pages_set", table.h, src.h, cov.h, base, *outs)
        else:
            call("sg_cover_pages", table.h, src.h, _p32(c), c.size, base, *outs)
        if nb.value <= buf.size:
            break
        _pages_buf[0] = np.zeros(max(2 * buf.size, nb.value), dtype=np.uint8)
    total = int(file_off[nf])
    return (file_off, lines[:total], covered[:total], seen[:nf], ncf.value, missing[: nm.value], body_off,
            _pages_buf[0][: nb.value], coverage[:nf], None if bad.value == 0xFFFFFFFF else bad.value)


class CoverReport:
    """The string-level mirror of generateCoverHtml up to fileSet.  symbolize(pcs) -> [(pc, func, file, line), ...]
    is the caller's addr2line (symbolizer.go: a PC's frames in `-afi` order, "??" and line <= 0 already dropped).
    The constructor symbolises all_pcs (initAllCover's call sites, cover.go:64-89) and interns the names;
    file_set(cov, base) returns {file: [(line, covered), ...]} as fileSet does.  Covered PCs the table does not
    know are symbolised and the table rebuilt from the host copies, once per call.

    pages(cov, base) goes on to the sorted d.Files (cover.go:122-158): [(Name, Body, Coverage), ...].  read_file(name)
    returns a source file's bytes, or None for one that cannot be read (parseFile's error); every file the table
    names is read once, into a SourceTable built on first use and again whenever a rebuild added files.  Name is
    the file without the common prefix, only when it is longer than the prefix (cover.go:148-150); the prefix is
    the byte-wise common prefix of the files of the uncovered frames (file_seen bit 1: the second symbolize call's,
    cover.go:117 and :358-372), "" when there are none.  For names that share no first byte the reference's
    `prefix == ""` reset makes its result depend on frame order; the mirror's pinned choice is the true common
    prefix "".  Order is templateFileArray.Less (cover.go:391-404): names starting with '.' last, otherwise
    ascending; names are distinct, so the order is total."""

    def __init__(self, sym_start, sym_end, all_pcs, symbolize, ctx=None, read_file=None):
        self._init(sym_start, sym_end, all_pcs, ctx, read_file)
        self.symbolize = symbolize
        self.frames = {}                 # pc -> [(file id, line, func id), ...]
        self._add(self.all_pcs)
        self._build()

    def _init(self, sym_start, sym_end, all_pcs, ctx, read_file):
        self.ctx = _ctx(ctx)
        self.read_file = read_file
        self.src = None
        self.sym_start, self.sym_end, self.all_pcs = _u64(sym_start), _u64(sym_end), _u64(all_pcs)
        self.files, self.funcs = {}, {}  # name -> id
        self.table = None
        self._tools = None               # from_tools: (nm text, addr2line); then the table comes from text

    @classmethod
    def from_tools(cls, nm_text, objdump_text, addr2line, read_file=None, ctx=None):
        """The report from the tools' raw output: nm_text is `nm -nS vmlinux`'s, objdump_text `objdump -d
        --no-show-raw-insn vmlinux`'s, and addr2line(pcs) -> bytes what `addr2line -afi -e vmlinux` writes for
        those PCs and the sentinel 0xffffffffffffffff (symbolizer.go:122-131).  files, funcs, names and the table
        are what the constructor reaches from the same tools through a symbolize callable; names are str (UTF-8,
        undecodable bytes as surrogates).  Nothing here works per frame: the texts are parsed, the names interned
        and the table built on the device (CoverTable.from_text), and only the distinct names come back.  `frames`
        is made from the last addr2line output when somebody asks for it.  Covered PCs the table does not know
        join the table's PCs and addr2line is asked again, for all of them."""
        c = _ctx(ctx)
        syms = nm_symbols(nm_text, ctx=c)
        self = cls.__new__(cls)
        self._init(syms.sym_start, syms.sym_end, objdump_pcs(objdump_text, ctx=c), c, read_file)
        self.symbolize = None
        self._tools = (nm_text, addr2line)
        self._tab_pcs = self.all_pcs
        self._build()
        return self

    def __getattr__(self, name):
        if name == "frames" and self.__dict__.get("_tools"):  # pc -> [(file id, line, func id), ...], on demand
            fr = addr2line_frames(self._a2l_text, self._tab_pcs.size, ctx=self.ctx)
            off = fr.frame_off.tolist()
            rows = list(zip(fr.frame_file.tolist(), fr.frame_line.tolist(), fr.frame_func.tolist()))
            return {pc: rows[off[r]:off[r + 1]] for r, pc in enumerate(fr.rec_pc.tolist())}
        raise AttributeError(name)

    def _add(self, pcs):
        if self._tools:
            self._tab_pcs = np.union1d(self._tab_pcs, _u64(pcs))
            return
        pcs = [int(pc) for pc in pcs]
        for pc in pcs:
            self.frames.setdefault(pc, [])
        for pc, func, file, line in self.symbolize(pcs):
            fi = self.files.setdefault(file, len(self.files))
            fu = self.funcs.setdefault(func, len(self.funcs))
            self.frames[int(pc)].append((fi, int(line), fu))

    def _build(self):
        if self.table is not None:
            self.table.close()
        if self._tools:
            nm_text, addr2line = self._tools
            self._a2l_text = addr2line(self._tab_pcs.tolist())
            self.table, files, funcs = CoverTable.from_text(nm_text, self.all_pcs, self._a2l_text, self._tab_pcs.size,
                                                            ctx=self.ctx)
            self.names = [b.decode("utf-8", "surrogateescape") for b in files]
            self.files = {name: k for k, name in enumerate(self.names)}
            self.funcs = {b.decode("utf-8", "surrogateescape"): k for k, b in enumerate(funcs)}
            if self.src is not None:  # (a rebuild numbers the files again)
                self.src.close()
                self.src = None
            return
        tab = sorted(self.frames)
        off = np.zeros(len(tab) + 1, dtype=U64)
        off[1:] = np.cumsum([len(self.frames[pc]) for pc in tab])
        fr = np.array([f for pc in tab for f in self.frames[pc]], dtype=np.int64).reshape(-1, 3)
        self.table = CoverTable(self.sym_start, self.sym_end, self.all_pcs, tab, off, fr[:, 0], fr[:, 1], fr[:, 2],
                                len(self.files), len(self.funcs), ctx=self.ctx)
        self.names = sorted(self.files, key=self.files.get)
        if self.src is not None and self.src.nfiles != len(self.names):
            self.src.close()
            self.src = None

    def _sources(self):
        if self.src is None:
            data = [self.read_file(name) if self.read_file else None for name in self.names]
            off = np.zeros(len(data) + 1, dtype=U64)
            off[1:] = np.cumsum([len(d) if d is not None else 0 for d in data])
            self.src = SourceTable([d is not None for d in data], b"".join(d for d in data if d is not None), off,
                                   ctx=self.ctx)
        return self.src

    def close(self):
        if self.src is not None:
            self.src.close()
            self.src = None
        if self.table is not None:
            self.table.close()
            self.table = None

    def file_set(self, cov, base):
        if (len(cov) if isinstance(cov, SignalSet) else _u32(cov).size) == 0:
            raise ValueError("No coverage data available")  # html.go:183
        res = cover_lines(self.table, cov, base)
        if res[5].size:
            self._add(res[5])
            self._build()
            res = cover_lines(self.table, cov, base)
            assert res[5].size == 0
        file_off, lines, covered, _, ncf, _ = res
        if ncf == 0:
            raise ValueError("coverage doesn't match to vmlinux: no frames (does not have debug info?)")  # cover.go:113
        out = {}
        for f, name in enumerate(self.names):
            a, b = int(file_off[f]), int(file_off[f + 1])
            if b > a:
                out[name] = [(int(ln), bool(c)) for ln, c in zip(lines[a:b], covered[a:b])]
        return out

    def pages(self, cov, base):
        if (len(cov) if isinstance(cov, SignalSet) else _u32(cov).size) == 0:
            raise ValueError("No coverage data available")  # html.go:183
        res = cover_pages(self.table, self._sources(), cov, base)
        if res[5].size:
            self._add(res[5])
            self._build()
            res = cover_pages(self.table, self._sources(), cov, base)
            assert res[5].size == 0
        file_off, _, _, seen, ncf, _, body_off, bodies, coverage, bad = res
        if ncf == 0:
            raise ValueError("coverage doesn't match to vmlinux: no frames (does not have debug info?)")  # cover.go:113
        if bad is not None:
            raise OSError(2, "cannot read a source file of the report", self.names[bad])  # cover.go:124-127
        raw = [name.encode("utf-8", "surrogateescape") for name in self.names]
        prefix = None
        for f in np.flatnonzero(seen & 2).tolist():  # cover.go:358-372 over the uncovered frames
            if prefix is None:
                prefix = raw[f]
            else:
                i = 0
                while i < len(prefix) and i < len(raw[f]) and prefix[i] == raw[f][i]:
                    i += 1
                prefix = prefix[:i]
        prefix = prefix or b""
        out = []
        for f, name in enumerate(raw):
            if file_off[f + 1] > file_off[f]:
                if len(name) > len(prefix):  # cover.go:148-150
                    name = name[len(prefix):]
                out.append((name, bodies[int(body_off[f]):int(body_off[f + 1])].tobytes(), int(coverage[f])))
        out.sort(key=lambda t: (t[0][:1] == b".", t[0]))  # cover.go:391-404 (Go compares strings byte-wise)
        return [(name.decode("utf-8", "surrogateescape"), body, c) for name, body, c in out]


# pkg/ipc/ipc_linux.go:168-307 status codes (include/syzsig.h SG_IPC_*)
IPC_OK, IPC_NO_NCMD, IPC_SHORT_HEADER, IPC_BAD_INDEX, IPC_BAD_CALLNUM, IPC_DOUBLE = 0, 1, 2, 3, 4, 5
IPC_SIGNAL_SIZE, IPC_COVER_SIZE, IPC_COMPS_SHORT, IPC_COMPS_TYPE = 6, 7, 8, 9


def ipc_parse(out, out_off, call_off, call_nums=None, cover=True, ctx=None):
    """readOutCoverage (pkg/ipc/ipc_linux.go:168-307) over a batch of program
    output regions.  Returns (errno int64[nrec], fault u8[nrec], status
    int32[nprog], sig_vals, sig_off, cov_vals, cov_off); cov_* are None when
    cover=False."""
    w, oo, co = _u32(out), _u64(out_off), _u64(call_off)
    nprog = oo.size - 1
    assert co.size == nprog + 1
    nrec = int(co[-1])
    nums = None if call_nums is None else _u32(call_nums)
    assert nums is None or nums.size == nrec
    err = np.empty(max(nrec, 1), dtype=np.int64)
    fault = np.empty(max(nrec, 1), dtype=np.uint8)
    status = np.empty(max(nprog, 1), dtype=np.int32)
    sv = np.empty(max(w.size, 1), dtype=U32)
    so = np.empty(nrec + 1, dtype=U64)
    cv = np.empty(max(w.size, 1), dtype=U32) if cover else None
    cvo = np.empty(nrec + 1, dtype=U64) if cover else None
    call("sg_ipc_parse", _ctx(ctx).h, _p32(w), _p64(oo), _p64(co), _p32(nums) if nums is not None else None, nprog,
         err.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), _p8(fault),
         status.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), _p64(so), _p32(sv),
         _p64(cvo) if cover else None, _p32(cv) if cover else None)
    return (err[:nrec], fault[:nrec], status[:nprog], sv[: int(so[-1])], so,
            cv[: int(cvo[-1])] if cover else None, cvo)
