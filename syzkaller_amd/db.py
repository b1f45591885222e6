"""The corpus database's read side on the GPU: pkg/db's Open (pkg/db/db.go:38-52, :167-249) and the hub's loadDB
(syz-hub/state/state.go:83-110) from the file's bytes (include/syzsig.h, "the corpus database").

Every value of a database is its own raw DEFLATE stream; inflate_batch decodes a batch of them, a lane per stream,
and DB.Open leaves the live records' texts on the device, where prog_hashes and call_sets take them with no second
upload.  Save, Delete, Flush and compact are not here: they need a compressor.
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
    """db.DB after Open, without the compaction: Records, uncompacted, needs_compact; the texts stay on the device
    until close()."""

    def __init__(self, data, ctx=None):
        self.ctx = _ctx(ctx)
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
        if isinstance(data_or_path, (str, os.PathLike)):
            try:
                with open(data_or_path, "rb") as f:
                    data_or_path = f.read()
            except FileNotFoundError:
                data_or_path = b""
        return cls(data_or_path, ctx)

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
        return self.nlive

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
        return self.nlive == 0 or self.uncompacted // 10 * 9 > self.nlive

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
