"""The corpus database on the GPU: pkg/db's Open (pkg/db/db.go:38-52, :167-249) and the hub's loadDB
(syz-hub/state/state.go:83-110) from the file's bytes, and its write side, Save, Delete, Flush and compact (:54-116,
:132-165) (include/syzsig.h, "the corpus database" and "the corpus database, written").

Every value of a database is its own raw DEFLATE stream; inflate_batch decodes a batch of them, a lane per stream,
and DB.Open leaves the live records' texts on the device, where prog_hashes and call_sets take them with no second
upload.  deflate_batch encodes a batch the same way (deflate_host: the same encoder on the host, byte for byte),
db_serialize writes records as serializeRecord does, and DB.compact of an unmodified database deflates the resident
texts with no upload.
"""
import os
from ctypes import byref, c_int, c_size_t, c_uint64, c_void_p

import numpy as np

from ._lib import call, lib
from .corpus import _bytes_ptr, texts_csr
from .cover import _ctx, _p8, _p32, _p64

U8, U32, U64 = np.uint8, np.uint32, np.uint64

INFLATE_OK, INFLATE_CORRUPT, INFLATE_TRUNCATED, INFLATE_TOO_LARGE = 0, 1, 2, 3   # SG_INFLATE_*
INFLATE_LONG = 65536                                                             # SG_INFLATE_LONG
DEFLATE_LONG = 65536                                                             # SG_DEFLATE_LONG
END_EOF, END_MAGIC, END_VERSION, END_RECORD, END_TRUNCATED, END_VALUE = range(6)  # SG_DB_END_*
SEQ_DELETED = (1 << 64) - 1                                                      # SG_DB_SEQ_DELETED


def inflate_batch(streams=None, csr=None, ctx=None, cap=None):
    """Raw DEFLATE of every stream: (status, consumed, out_off, out).  Stream k's output is out[out_off[k]:
    out_off[k + 1]]; a stream that is not OK owns none.  With cap below the total, out is None (the offsets still
    say what each stream needs)."""
    b, off = texts_csr(streams, csr)
    n = off.size - 1
    c = _ctx(ctx)
    status, consumed, out_off = np.zeros(n, U8), np.zeros(n, U64), np.zeros(n + 1, U64)
    nout = c_size_t()
    args = (c.h, _bytes_ptr(b), _p64(off), n, _p8(status) if n else None, _p64(consumed) if n else None, _p64(out_off))
    if cap is None:  # the count pass tells
        call("sg_inflate_batch", *args, None, 0, byref(nout))
        cap = nout.value
        if cap == 0:
            return status, consumed, out_off, np.zeros(0, U8)
    out = np.zeros(cap, U8)
    call("sg_inflate_batch", *args, _p8(out) if cap else None, cap, byref(nout))
    return status, consumed, out_off, out[:nout.value] if nout.value <= cap else None


def deflate_bound(n):
    """sg_deflate_bound: the stored form's length, which no stream of n input bytes exceeds."""
    return int(lib.sg_deflate_bound(n))


def _bound_total(off):
    """The sum of sg_deflate_bound over a CSR's lengths."""
    ln = np.diff(off.astype(np.int64))
    return int(ln.sum() + 5 * np.maximum(1, (ln + 65534) // 65535).sum())


def _deflate(fn, head, streams, csr, cap):
    b, off = texts_csr(streams, csr)
    n = off.size - 1
    out_off = np.zeros(n + 1, U64)
    nout = c_size_t()
    args = (*head, _bytes_ptr(b), _p64(off), n, _p64(out_off))
    if cap is None:  # no stream exceeds its stored form: one call
        cap = _bound_total(off)
    out = np.empty(cap, U8)
    call(fn, *args, _p8(out) if cap else None, cap, byref(nout))
    return out_off, out[:nout.value] if nout.value <= cap else None


def deflate_batch(streams=None, csr=None, ctx=None, cap=None):
    """Raw DEFLATE of every input, on the device: (out_off, out).  Input k's stream is out[out_off[k]:out_off[k + 1]].
    With cap below the total, out is None (the offsets still say what each stream needs)."""
    return _deflate("sg_deflate_batch", (_ctx(ctx).h,), streams, csr, cap)


def deflate_host(streams=None, csr=None, cap=None):
    """The same encoder on the host (no device, no context): the same bytes."""
    return _deflate("sg_deflate_host", (), streams, csr, cap)


def db_serialize(keys, seqs, texts, with_header=False, ctx=None, cap=None):
    """serializeHeader (with_header) and serializeRecord for the records in the given order, as bytes; a deletion is
    seq SEQ_DELETED with an empty (or None) text.  With cap below the length: None."""
    kb, koff = texts_csr([bytes(k) for k in keys])
    tb, toff = texts_csr([b"" if t is None else bytes(t) for t in texts])
    sq = np.ascontiguousarray(np.array([int(s) for s in seqs], dtype=U64))
    n = sq.size
    if koff.size - 1 != n or toff.size - 1 != n:
        raise ValueError("keys, seqs and texts are parallel")
    c = _ctx(ctx)
    nout = c_size_t()
    args = (c.h, _bytes_ptr(kb), _p64(koff), _p64(sq) if n else None, _bytes_ptr(tb), _p64(toff), n, int(bool(with_header)))
    if cap is None:  # the frames (24 bytes and the key at most) and every value's stored form: one call
        cap = 8 + 24 * n + kb.size + _bound_total(toff)
    out = np.empty(cap, U8)
    call("sg_db_serialize", *args, _p8(out) if cap else None, cap, byref(nout))
    return out[:nout.value].tobytes() if nout.value <= cap else None


def db_scan(data):
    """sg_db_scan: (key_pos, key_len, seq, val_pos, val_len, end) of the file's records, in file order."""
    b = np.frombuffer(bytes(data), dtype=U8)
    nrec, end = c_size_t(), c_int()
    call("sg_db_scan", _bytes_ptr(b), b.size, None, None, None, None, None, 0, byref(nrec), byref(end))
    n = nrec.value
    kp, kl, sq, vp, vl = np.zeros(n, U64), np.zeros(n, U32), np.zeros(n, U64), np.zeros(n, U64), np.zeros(n, U32)
    if n:
        call("sg_db_scan", _bytes_ptr(b), b.size, _p64(kp), _p32(kl), _p64(sq), _p64(vp), _p32(vl), n, byref(nrec),
             byref(end))
    return kp, kl, sq, vp, vl, end.value


class DB:
    """db.DB: Open without the compaction (Records, uncompacted, needs_compact; the texts stay on the device until
    close()), then Save, Delete, Flush and compact after the Go.  Save and Delete change Records, a pending list and
    uncompacted on the host only: device(), verify(), export(), nlive, text_bytes and key_bytes keep describing the
    database as it was opened.  A database that was not modified since Open compacts from its resident texts
    (sg_db_compact); a modified one through db_serialize over Records.  One built from bytes has no file name:
    Flush and compact raise ValueError on it, serialize_pending and serialize_compact still work."""

    def __init__(self, data, ctx=None, filename=None):
        self.ctx = _ctx(ctx)
        self.filename = None if filename is None else os.fspath(filename)
        self._pending = []       # (key, val or None, seq) since the last Flush (db.pending)
        self._modified = False   # Records no longer is what the device holds
        b = np.frombuffer(bytes(data), dtype=U8)
        h = c_void_p()
        call("sg_db_open", self.ctx.h, _bytes_ptr(b), b.size, byref(h))
        self.h = h
        counts = np.zeros(5, U64)
        call("sg_db_counts", self.h, _p64(counts))
        self.nlive, self.uncompacted, self.text_bytes, self.key_bytes, self.end = (int(x) for x in counts)
        self._records = None

    @classmethod
    def Open(cls, data_or_path, ctx=None):
        """db.Open: of a file's bytes, or of a path (a missing file is an empty database, as O_CREATE makes it)."""
        filename = None
        if isinstance(data_or_path, (str, os.PathLike)):
            filename = data_or_path
            try:
                with open(data_or_path, "rb") as f:
                    data_or_path = f.read()
            except FileNotFoundError:
                data_or_path = b""
        return cls(data_or_path, ctx, filename)

    def close(self):
        if self.h:
            lib.sg_db_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __len__(self):
        return len(self._records) if self._modified else self.nlive

    def export(self):
        """(keys, seqs, texts): the live records in file order of their winning write; keys and texts as bytes."""
        n = self.nlive
        key_off, text_off, seqs = np.zeros(n + 1, U64), np.zeros(n + 1, U64), np.zeros(n, U64)
        keys, texts = np.zeros(self.key_bytes, U8), np.zeros(self.text_bytes, U8)
        call("sg_db_export", self.h, _p64(key_off), _bytes_ptr(keys), _p64(seqs) if n else None, _p64(text_off),
             _bytes_ptr(texts))
        kb, tb, ko, to = keys.tobytes(), texts.tobytes(), key_off.tolist(), text_off.tolist()
        return ([kb[ko[k]:ko[k + 1]] for k in range(n)], seqs, [tb[to[k]:to[k + 1]] for k in range(n)])

    @property
    def Records(self):
        """key -> (val, seq), in the order of export()."""
        if self._records is None:
            keys, seqs, texts = self.export()
            self._records = {k: (v, int(s)) for k, s, v in zip(keys, seqs.tolist(), texts)}
        return self._records

    @property
    def needs_compact(self):
        """Open's test before db.compact() (db.go:48)."""
        return len(self) == 0 or self.uncompacted // 10 * 9 > len(self)

    # ---- the write side (db.go:54-116) ----
    def Save(self, key, val, seq):
        """db.Save (:54-64)."""
        key, val, seq = bytes(key), bytes(val), int(seq)
        if seq == SEQ_DELETED:
            raise ValueError("reserved seq")
        recs = self.Records
        if recs.get(key) == (val, seq):
            return
        recs.pop(key, None)   # (a rewritten key moves to the end: the order of the winning write, as Open has it)
        recs[key] = (val, seq)
        self._modified = True
        self._pending.append((key, val, seq))
        self.uncompacted += 1

    def Delete(self, key):
        """db.Delete (:66-73)."""
        key = bytes(key)
        recs = self.Records
        if key not in recs:
            return
        del recs[key]
        self._modified = True
        self._pending.append((key, None, SEQ_DELETED))
        self.uncompacted += 1

    def serialize_pending(self):
        """db.pending's bytes (:118-123): the records saved and deleted since the last Flush, in one db_serialize."""
        if not self._pending:
            return b""
        keys, vals, seqs = zip(*self._pending)
        return db_serialize(keys, seqs, vals, False, self.ctx)

    def serialize_compact(self):
        """compact()'s buffer (:96-100): the header and every live record."""
        if not self._modified:
            nout = c_size_t()   # (as db_serialize sizes it, from the counts: one call)
            cap = 8 + 29 * self.nlive + self.key_bytes + self.text_bytes + 5 * (self.text_bytes // 65535 + 1)
            out = np.empty(cap, U8)
            call("sg_db_compact", self.h, _p8(out), out.size, byref(nout))
            return out[:nout.value].tobytes()
        recs = self.Records
        return db_serialize(list(recs), [r[1] for r in recs.values()], [r[0] for r in recs.values()], True, self.ctx)

    def _need_file(self):
        if self.filename is None:
            raise ValueError("the database was opened from bytes: it has no file")

    def Flush(self):
        """db.Flush (:75-93).  (A file that is still empty gets its header first: Go's Open has compacted it by then.)"""
        self._need_file()
        if self.uncompacted // 10 * 9 > len(self):
            return self.compact()
        if not self._pending:
            return
        data = self.serialize_pending()
        with open(self.filename, "ab") as f:
            if f.tell() == 0:
                data = db_serialize([], [], [], True, self.ctx) + data
            f.write(data)
        self._pending = []

    def compact(self):
        """db.compact (:95-116): the buffer to filename + ".tmp", renamed over the file."""
        self._need_file()
        data = self.serialize_compact()
        tmp = self.filename + ".tmp"
        with open(tmp, "wb") as f:
            f.write(data)
        os.replace(tmp, self.filename)
        self.uncompacted = len(self)
        self._pending = []

    def device(self):
        """(texts, text_off) device pointers, as sg_prog_hashes_dev and sg_call_sets_dev take them."""
        t, o = c_void_p(), c_void_p()
        call("sg_db_device", self.h, byref(t), byref(o))
        return t.value, o.value

    def verify(self, table=None):
        """loadDB's loop over the resident texts: (bad, max_seq); bad[k] 1 CallSet fails, 2 the key is not the
        text's hash, 0 otherwise."""
        bad = np.zeros(self.nlive, U8)
        max_seq = c_uint64()
        call("sg_db_verify", self.h, table.h if table is not None else None, _p8(bad) if self.nlive else None,
             byref(max_seq))
        return bad, max_seq.value


def LoadDB(data, tab=None, ctx=None):
    """loadDB (state.go:83-110) up to its Flush: (db, maxSeq, the keys it would delete, in record order)."""
    db = DB.Open(data, ctx if ctx is not None else (tab.ctx if tab is not None else None))
    bad, max_seq = db.verify(tab)
    keys, _, _ = db.export() if bad.any() else ([], None, None)
    return db, max_seq, [keys[k] for k in np.flatnonzero(bad).tolist()]
