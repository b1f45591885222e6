"""Call-to-call priorities and the ChoiceTable (prog/prio.go:27-36, :133-247) on
the GPU: the pair counts of calcDynamicPrio kept exact and device-resident
(PrioTable), normalizePrio, the multiply by the static matrix and
BuildChoiceTable's running sums (include/syzsig.h, "call priorities").

The corpus is what the manager can keep next to each RpcInput: the call ids
(Call.Meta.ID) of every program.  The static matrix is an input: it depends
on the target alone.  Choose stays on the host and takes the caller's random
numbers.
"""
from ctypes import byref, c_void_p

import numpy as np

from . import _lib
from ._lib import call, lib
from .cover import _ctx, _p8, _p32, _p64

NO_CALL = 0xFFFFFFFF  # SG_NO_CALL: a target without an mmap call
MAX_CALLS = 8192      # SG_PRIO_MAX_CALLS

U8, U32, U64, I32, F32 = np.uint8, np.uint32, np.uint64, np.int32, np.float32


def _pf(a):
    return a.ctypes.data_as(_lib.PF)


def _pi(a):
    return a.ctypes.data_as(_lib.PI32)


def corpus_csr(corpus_calls=None, csr=None):
    """(call_ids, prog_off) of a corpus: from a sequence of per-program id sequences, or from csr = (call_ids,
    prog_off), the arrays themselves (program p owns call_ids[prog_off[p]:prog_off[p + 1]])."""
    if (corpus_calls is None) == (csr is None):
        raise ValueError("pass the programs or csr=(call_ids, prog_off)")
    if csr is not None:
        ids, off = csr
        ids, off = np.ascontiguousarray(ids, dtype=U32).reshape(-1), np.ascontiguousarray(off, dtype=U64).reshape(-1)
        if off.size == 0:
            raise ValueError("prog_off holds nprogs + 1 offsets")
        return ids, off
    progs = [np.asarray(p, dtype=U32).reshape(-1) for p in corpus_calls]
    off = np.zeros(len(progs) + 1, U64)
    if progs:
        off[1:] = np.cumsum([p.size for p in progs], dtype=U64)
    ids = np.concatenate(progs) if progs else np.zeros(0, U32)
    return np.ascontiguousarray(ids, dtype=U32), off


class PrioTable:
    """sg_prio_table: the static matrix, the enabled calls and the exact pair counts of one target."""

    def __init__(self, static, mmap_id=NO_CALL, enabled=None, ctx=None):
        self.ctx = _ctx(ctx)
        st = np.ascontiguousarray(static, dtype=F32)
        if st.ndim != 2 or st.shape[0] != st.shape[1]:
            raise ValueError("static is a square matrix, one row per call")
        self.ncalls = st.shape[0]
        en = None
        if enabled is not None:
            en = np.ascontiguousarray(np.asarray(enabled).astype(bool), dtype=U8).reshape(-1)
            if en.size != self.ncalls:
                raise ValueError("enabled holds one entry per call")
        self.enabled = None if en is None else en.astype(bool)
        self.mmap_id = NO_CALL if mmap_id is None else int(mmap_id)
        h = c_void_p()
        call("sg_prio_table_create", self.ctx.h, self.ncalls, self.mmap_id, _pf(st), None if en is None else _p8(en),
             byref(h))
        self.h = h

    def close(self):
        if self.h:
            lib.sg_prio_table_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def clear(self):
        call("sg_prio_table_clear", self.h)

    def add(self, corpus_calls=None, csr=None):
        """Adds the programs' pairs: two adds equal one add of the concatenation."""
        ids, off = corpus_csr(corpus_calls, csr)
        call("sg_prio_table_add", self.h, _p32(ids), _p64(off), off.size - 1)

    def counts(self):
        out = np.empty((self.ncalls, self.ncalls), U64)
        call("sg_prio_table_counts", self.h, _p64(out))
        return out

    def _outs(self, dynamic, prios, run):
        n = self.ncalls
        d = np.empty((n, n), F32) if dynamic else None
        p = np.empty((n, n), F32) if prios else None
        r = np.empty((n, n), I32) if run else None
        return d, p, r, [None if d is None else _pf(d), None if p is None else _pf(p), None if r is None else _pi(r)]

    def prios(self, dynamic=True, prios=True, run=True):
        """(dynamic, prios, run) from the counts, which stay as they are; None for an output not asked for."""
        d, p, r, ptrs = self._outs(dynamic, prios, run)
        call("sg_call_prios", self.h, *ptrs)
        return d, p, r

    def from_progs(self, corpus_calls=None, csr=None, dynamic=True, prios=True, run=True):
        """clear, add and prios in one call with one wait."""
        ids, off = corpus_csr(corpus_calls, csr)
        d, p, r, ptrs = self._outs(dynamic, prios, run)
        call("sg_call_prios_from_progs", self.h, _p32(ids), _p64(off), off.size - 1, *ptrs)
        return d, p, r


def CalculatePriorities(corpus_calls, static, mmap_id, ctx=None, csr=None):
    """target.CalculatePriorities(corpus) (prog/prio.go:27-36): the float32 matrix dynamic * static.  The corpus
    as per-program id sequences, or corpus_calls None and csr = (call_ids, prog_off)."""
    t = PrioTable(static, mmap_id, ctx=ctx)
    try:
        return t.from_progs(corpus_calls, csr, dynamic=False, run=False)[1]
    finally:
        t.close()


class ChoiceTable:
    """prog.ChoiceTable (prog/prio.go:196-247): run[i] is None for a disabled row.  enabledCalls is a Go map's
    iteration order in the reference; here it is ascending."""

    def __init__(self, run, enabled):
        self.enabled = np.asarray(enabled, dtype=bool)
        self.enabledCalls = np.flatnonzero(self.enabled)
        self.run = [np.asarray(run[i]) if self.enabled[i] else None for i in range(self.enabled.size)]

    def Choose(self, intn, call):
        """prio.go:231-247; intn(n) plays r.Intn: an integer in [0, n)."""
        run = self.run[call] if call >= 0 else None
        if run is None:
            return int(self.enabledCalls[intn(len(self.enabledCalls))])
        while True:
            x = intn(int(run[-1]))
            i = int(np.searchsorted(run, x, side="left"))  # sort.SearchInts
            if not self.enabled[i]:
                continue
            return i


def BuildChoiceTable(prios_or_table, enabled=None, ctx=None):
    """target.BuildChoiceTable (prog/prio.go:203-229) from a PrioTable (its counts, static matrix and enabled
    calls; `enabled` must be None) or from a prios matrix, whose running sums run through the same kernel: a
    table with no counts has dynamic == 1, so its prios are the static matrix it was given."""
    if isinstance(prios_or_table, PrioTable):
        if enabled is not None:
            raise ValueError("a PrioTable carries its own enabled calls")
        t = prios_or_table
        en = np.ones(t.ncalls, bool) if t.enabled is None else t.enabled
        return ChoiceTable(t.prios(dynamic=False, prios=False)[2], en)
    pr = np.ascontiguousarray(prios_or_table, dtype=F32)
    en = np.ones(pr.shape[0], bool) if enabled is None else np.asarray(enabled).astype(bool)
    t = PrioTable(pr, NO_CALL, en, ctx=ctx)
    try:
        return ChoiceTable(t.prios(dynamic=False, prios=False)[2], en)
    finally:
        t.close()
