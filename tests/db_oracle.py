"""The corpus database in Python, line by line: pkg/db/db.go:125-249 (deserializeDB, deserializeHeader,
deserializeRecord) over zlib, Open's compaction test (:48) and the hub's loadDB loop (syz-hub/state/state.go:91-105)
over hashlib and the CallSet oracle.  The inflate oracle is zlib.decompressobj(-15): OK exactly when it reaches eof,
CORRUPT when it raises, TRUNCATED when it returns without eof."""
import hashlib
import struct
import zlib

from tests import hub_state_oracle as HO

OK, CORRUPT, TRUNCATED = 0, 1, 2
DB_MAGIC, REC_MAGIC, CUR_VERSION, SEQ_DELETED = 0xBADDB, 0xFEE1BAD, 1, (1 << 64) - 1
END_EOF, END_MAGIC, END_VERSION, END_RECORD, END_TRUNCATED, END_VALUE = 0, 1, 2, 3, 4, 5


def inflate(stream):
    """(status, output, consumed) of one raw DEFLATE stream; output and consumed are b"" and 0 unless OK."""
    stream = bytes(stream)
    d = zlib.decompressobj(-15)
    try:
        out = d.decompress(stream)
    except zlib.error:
        return CORRUPT, b"", 0
    if not d.eof:
        return TRUNCATED, b"", 0
    return OK, out, len(stream) - len(d.unused_data)


def scan(data):
    """sg_db_scan: ([(key_pos, key_len, seq, val_pos, val_len)] in file order, end).  A record's framing advances by
    val_len whatever the stream inside consumes (the pinned choice)."""
    data = bytes(data)
    n = len(data)
    if n == 0:
        return [], END_EOF           # deserializeHeader: io.EOF is the current version (:196-198)
    if n < 4:
        return [], END_TRUNCATED
    if struct.unpack_from("<I", data, 0)[0] != DB_MAGIC:
        return [], END_MAGIC
    if n < 8:
        return [], END_TRUNCATED
    ver = struct.unpack_from("<I", data, 4)[0]
    if ver == 0 or ver > CUR_VERSION:
        return [], END_VERSION
    recs, pos = [], 8
    while True:
        if pos == n:
            return recs, END_EOF
        if n - pos < 4:
            return recs, END_TRUNCATED
        if struct.unpack_from("<I", data, pos)[0] != REC_MAGIC:
            return recs, END_RECORD
        if n - pos < 8:
            return recs, END_TRUNCATED
        key_len = struct.unpack_from("<I", data, pos + 4)[0]
        key_pos = pos + 8
        if n - key_pos < key_len + 8:
            return recs, END_TRUNCATED
        seq = struct.unpack_from("<Q", data, key_pos + key_len)[0]
        pos = key_pos + key_len + 8
        if seq == SEQ_DELETED:
            recs.append((key_pos, key_len, seq, 0, 0))
            continue
        if n - pos < 4:
            return recs, END_TRUNCATED
        val_len = struct.unpack_from("<I", data, pos)[0]
        pos += 4
        if n - pos < val_len:
            return recs, END_TRUNCATED
        recs.append((key_pos, key_len, seq, pos, val_len))
        pos += val_len


class ODB:
    """deserializeDB (:167-191): Records (key -> (val, seq), in order of the winning write), uncompacted, end."""

    def __init__(self, data):
        data = bytes(data)
        recs, end = scan(data)
        self.Records, self.uncompacted, self.end = {}, 0, end
        for key_pos, key_len, seq, val_pos, val_len in recs:
            key = data[key_pos:key_pos + key_len]
            val = b""
            if seq != SEQ_DELETED and val_len:
                status, val, _ = inflate(data[val_pos:val_pos + val_len])
                if status != OK:
                    self.end = END_VALUE
                    break
            self.uncompacted += 1
            self.Records.pop(key, None)   # (a rewritten key moves to the end: the order of the winning write)
            if seq != SEQ_DELETED:
                self.Records[key] = (val, seq)

    @property
    def needs_compact(self):
        return len(self.Records) == 0 or self.uncompacted // 10 * 9 > len(self.Records)


def LoadDB(data):
    """loadDB's loop: (db, maxSeq, the keys it deletes in record order, bad per record)."""
    db = ODB(data)
    max_seq, deleted, bad = 0, [], []
    for key, (val, seq) in db.Records.items():
        if HO.call_lines(val)[0] != 0:
            bad.append(1)
        elif hashlib.sha1(val).hexdigest().encode() != key:
            bad.append(2)
        else:
            bad.append(0)
            max_seq = max(max_seq, seq)
        if bad[-1]:
            deleted.append(key)
    return db, max_seq, deleted, bad
