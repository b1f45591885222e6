"""The hub's corpus on the GPU: prog.CallSet (prog/encoding.go:559-592), the name dictionary, and
syz-hub/state/state.go's addInputs, pendingInputs and purgeCorpus (include/syzsig.h, "the hub's corpus").

Programs are byte strings, as in syzkaller_amd.corpus: a sequence of bytes-like objects or csr=(bytes, off).
Names are bytes.  Keys are 20-byte identities (hash.Sig); the texts stay on the host.
"""
from ctypes import byref, c_size_t, c_uint64, c_void_p

import numpy as np

from ._lib import call, lib
from .corpus import SIG_BYTES, SigSet, _bytes_ptr, texts_csr
from .cover import _ctx, _p8, _p32, _p64

U8, U32, U64 = np.uint8, np.uint32, np.uint64

NAME_UNKNOWN = 0xFFFFFFFF     # SG_NAME_UNKNOWN
CALLSET_MAX_LINE = 262144     # SG_CALLSET_MAX_LINE
SEQ_LIMIT = 1 << 33           # SG_HUB_SEQ_LIMIT
CALLSET_ERRORS = {            # status -> the reference's error text
    1: "line does not contain opening bracket",
    2: "call name is empty",
    3: "bufio.Scanner: token too long",
    4: "program does not contain any calls",
}


class NameTable:
    """sg_nametab: call names interned to dense ids, in order of first insertion."""

    def __init__(self, ctx=None):
        self.ctx = _ctx(ctx)
        h = c_void_p()
        call("sg_nametab_create", self.ctx.h, byref(h))
        self.h = h
        self._names = []   # id -> name
        self._ids = {}     # name -> id (the host's view of what the library holds)

    def close(self):
        if self.h:
            lib.sg_nametab_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __len__(self):
        n = c_uint64()
        call("sg_nametab_count", self.h, byref(n))
        return n.value

    def add(self, names):
        """The ids of the names (bytes), an existing name keeping its id."""
        names = [bytes(x) for x in names]
        b, off = texts_csr(names)
        ids = np.zeros(len(names), U32)
        call("sg_nametab_add", self.h, _bytes_ptr(b), _p64(off), len(names), _p32(ids) if names else None)
        for name, i in zip(names, ids.tolist()):
            if i == len(self._names):
                self._names.append(name)
                self._ids[name] = i
        return ids

    def id(self, name):
        """The id of a name, or None."""
        return self._ids.get(bytes(name))

    def name(self, i):
        return self._names[i]

    def mask(self, names):
        """The bitmask (uint64 words over the table's ids) of the names that are in the table."""
        words = np.zeros((len(self._names) + 63) // 64, U64)
        for name in names:
            i = self._ids.get(bytes(name))
            if i is not None:
                words[i >> 6] |= U64(1 << (i & 63))
        return words


def call_sets(progs=None, csr=None, table=None, ctx=None):
    """prog.CallSet of every program, raw: (status, line_off, name_pos, name_len, name_id).  Program k owns call
    lines line_off[k]:line_off[k + 1], in text order with repeats; name_pos is an offset into the batch's bytes."""
    b, off = texts_csr(progs, csr)
    n = off.size - 1
    c = table.ctx if table is not None else _ctx(ctx)
    cap = int(np.count_nonzero(b == 0x28))
    status, line_off = np.zeros(n, U8), np.zeros(n + 1, U64)
    pos, ln, ids = np.zeros(cap, U64), np.zeros(cap, U32), np.full(cap, NAME_UNKNOWN, U32)
    nl = c_size_t()
    call("sg_call_sets", c.h, table.h if table is not None else None, _bytes_ptr(b), _p64(off), n,
         _p8(status) if n else None, _p64(line_off), _p64(pos) if cap else None, _p32(ln) if cap else None,
         _p32(ids) if cap else None, cap, byref(nl))
    assert nl.value <= cap
    return status, line_off, pos[:nl.value], ln[:nl.value], ids[:nl.value]


def CallSet(data, table=None, ctx=None):
    """prog.CallSet(data): the set of call names (bytes); ValueError with the reference's message otherwise
    ("bufio.Scanner: token too long" for a line of CALLSET_MAX_LINE bytes or more)."""
    data = bytes(data)
    status, _, pos, ln, _ = call_sets([data], table=table, ctx=ctx)
    if status[0]:
        raise ValueError(CALLSET_ERRORS[int(status[0])])
    return {data[p:p + n] for p, n in zip(pos.tolist(), ln.tolist())}


class HubCorpus:
    """sg_hubcorpus: st.Corpus as (key, seq, call ids) records in insertion order."""

    def __init__(self, table):
        self.table = table
        self.ctx = table.ctx
        h = c_void_p()
        call("sg_hubcorpus_create", self.ctx.h, table.h, byref(h))
        self.h = h

    def close(self):
        if self.h:
            lib.sg_hubcorpus_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def count(self):
        n = c_uint64()
        call("sg_hubcorpus_count", self.h, byref(n))
        return n.value

    __len__ = count

    def export(self):
        """(keys (n, 20), seqs, call_off, call_ids) of all records, in record order."""
        nr, ni = c_size_t(), c_size_t()
        one = np.zeros(1, U64)
        call("sg_hubcorpus_export", self.h, None, None, _p64(one), None, 0, 0, byref(nr), byref(ni))
        n, m = nr.value, ni.value
        sigs, seqs = np.zeros((n, SIG_BYTES), U8), np.zeros(n, U64)
        call_off, ids = np.zeros(n + 1, U64), np.zeros(m, U32)
        call("sg_hubcorpus_export", self.h, _p8(sigs) if n else None, _p64(seqs) if n else None, _p64(call_off),
             _p32(ids) if m else None, n, m, byref(nr), byref(ni))
        assert (nr.value, ni.value) == (n, m)
        return sigs, seqs, call_off, ids

    def add_raw(self, b, off, seqs, mgr=None, unk_cap=None):
        """One sg_hubcorpus_add: (status, is_new, sigs, unknown spans as (pos, len), nunk)."""
        n = off.size - 1
        seqs = np.ascontiguousarray(np.broadcast_to(np.asarray(seqs, U64), (n,)))
        cap = int(np.count_nonzero(b == 0x28)) if unk_cap is None else int(unk_cap)
        status, is_new, sigs = np.zeros(n, U8), np.zeros(n, U8), np.zeros((n, SIG_BYTES), U8)
        upos, ulen = np.zeros(cap, U64), np.zeros(cap, U32)
        nunk = c_size_t()
        call("sg_hubcorpus_add", self.h, mgr.h if mgr is not None else None, _bytes_ptr(b), _p64(off), n,
             _p64(seqs) if n else None, _p8(status) if n else None, _p8(is_new) if n else None, _p8(sigs) if n else None,
             _p64(upos) if cap else None, _p32(ulen) if cap else None, cap, byref(nunk))
        w = min(nunk.value, cap)
        return status, is_new.astype(bool), sigs, (upos[:w], ulen[:w]), nunk.value

    def add(self, progs=None, seqs=0, mgr=None, csr=None):
        """addInputs' loop over a batch: (status, is_new, sigs).  Names the dictionary does not hold yet are
        interned and the call repeated: nothing changes in a call that meets an unknown name."""
        b, off = texts_csr(progs, csr)
        while True:
            status, is_new, sigs, (upos, ulen), nunk = self.add_raw(b, off, seqs, mgr)
            if not nunk:
                return status, is_new, sigs
            view = b.tobytes()
            # (in order of first appearance in the batch: the ids' order is this project's pinned choice)
            self.table.add(list(dict.fromkeys(view[p:p + n] for p, n in zip(upos.tolist(), ulen.tolist()))))

    def pending(self, mgr, mgr_seq, hub_seq, mask, max_records=1000):
        """pendingInputs' selection: (keys, seqs, max_seq, more), keys in ascending (seq, record index) order."""
        mask = np.ascontiguousarray(mask, dtype=U64).reshape(-1)
        cap = self.count()
        sigs, seqs = np.zeros((cap, SIG_BYTES), U8), np.zeros(cap, U64)
        n, max_seq, more = c_size_t(), c_uint64(), c_uint64()
        call("sg_hubcorpus_pending", self.h, mgr.h, int(mgr_seq), int(hub_seq), _p64(mask) if mask.size else None,
             mask.size, int(max_records), _p8(sigs) if cap else None, _p64(seqs) if cap else None, cap, byref(n),
             byref(max_seq), byref(more))
        return sigs[:n.value], seqs[:n.value], max_seq.value, more.value

    def purge(self, mgrs):
        """purgeCorpus: deletes the records no manager set holds; the deleted keys, (n, 20), in record order."""
        mgrs = list(mgrs)
        cap = self.count()
        dels = np.zeros((cap, SIG_BYTES), U8)
        arr = (c_void_p * max(len(mgrs), 1))(*[m.h.value for m in mgrs])
        nd = c_size_t()
        call("sg_hubcorpus_purge", self.h, arr if mgrs else None, len(mgrs), _p8(dels) if cap else None, cap, byref(nd))
        return dels[:nd.value]


class _Manager:
    def __init__(self, name, ctx):
        self.name = name
        self.Corpus = SigSet(ctx=ctx)
        self.Calls = set()
        self.corpusSeq = 0
        self.Connected = False
        self.Added = self.Deleted = self.New = 0
        self._mask = None
        self._mask_names = -1


class HubState:
    """syz-hub/state/state.go's State over the device corpus: Connect, Sync, addInputs, purgeCorpus,
    pendingInputs.  Files, the databases, the seq files, repros and the RPC layer stay with the caller; the texts
    are kept in a host dict by key.  Sync returns the programs only: the reference's `make([][]byte,
    len(records))` followed by append (state.go:301-304) puts len(records) empty entries in front of them, and
    mgr.New counts those too (twice the records), which is kept here."""

    def __init__(self, ctx=None):
        self.ctx = _ctx(ctx)
        self.table = NameTable(self.ctx)
        self.Corpus = HubCorpus(self.table)
        self.corpusSeq = 0
        self.Managers = {}
        self.texts = {}

    def close(self):
        for m in self.Managers.values():
            m.Corpus.close()
        self.Managers = {}
        self.Corpus.close()
        self.table.close()

    def _mgr(self, name):
        mgr = self.Managers.get(name)
        if mgr is None or not mgr.Connected:
            raise ValueError(f"unconnected manager {name}")
        return mgr

    def _mask(self, mgr):
        if mgr._mask_names != len(self.table._names):
            mgr._mask = self.table.mask(mgr.Calls)
            mgr._mask_names = len(self.table._names)
        return mgr._mask

    def Connect(self, name, fresh, calls, corpus):
        mgr = self.Managers.get(name)
        if mgr is None:
            mgr = self.Managers[name] = _Manager(name, self.ctx)
        mgr.Connected = True
        if fresh:
            mgr.corpusSeq = 0
        mgr.Calls = {bytes(c) if not isinstance(c, str) else c.encode() for c in calls}
        mgr._mask_names = -1
        mgr.Corpus.clear()
        self.addInputs(mgr, corpus)
        self.purgeCorpus()

    def Sync(self, name, add, dels):
        """(progs, more) of state.go:175-195; dels are identities (hex strings or 20-byte strings)."""
        mgr = self._mgr(name)
        add, dels = list(add), list(dels)
        if dels:
            mgr.Corpus.remove(dels)
            self.purgeCorpus()
        self.addInputs(mgr, add)
        progs, more = self.pendingInputs(mgr)
        mgr.Added += len(add)
        mgr.Deleted += len(dels)
        mgr.New += 2 * len(progs)
        return progs, more

    def addInputs(self, mgr, inputs):
        inputs = [bytes(p) for p in inputs]
        if not inputs:
            return
        self.corpusSeq += 1
        _, is_new, sigs = self.Corpus.add(inputs, self.corpusSeq, mgr.Corpus)
        for k in np.flatnonzero(is_new).tolist():
            self.texts[sigs[k].tobytes()] = inputs[k]

    def purgeCorpus(self):
        for key in self.Corpus.purge([m.Corpus for m in self.Managers.values()]):
            self.texts.pop(key.tobytes(), None)

    def pendingInputs(self, mgr, max_records=1000):
        if not isinstance(mgr, _Manager):
            mgr = self._mgr(mgr)
        sigs, _, max_seq, more = self.Corpus.pending(mgr.Corpus, mgr.corpusSeq, self.corpusSeq, self._mask(mgr),
                                                     max_records)
        mgr.corpusSeq = max_seq
        return [self.texts[s.tobytes()] for s in sigs], more
