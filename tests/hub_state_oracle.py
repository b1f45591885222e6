"""The test oracle of the hub's corpus, pure Python, one thread.  CallSet restates prog/encoding.go:559-592
over the bufio.Scanner / ScanLines rules the header pins; the corpus and the state restate the Go lines of
syz-hub/state/state.go over dicts, which keep insertion order -- the orders the product pins (the reference's
own are Go map iteration and an unstable sort)."""
import hashlib

import numpy as np

MAX_LINE = 256 << 10  # maxLineLen (encoding.go:382)
ERRORS = {
    1: "line does not contain opening bracket",
    2: "call name is empty",
    3: "bufio.Scanner: token too long",
    4: "program does not contain any calls",
}
FNV_OFFSET, FNV_PRIME = 0xCBF29CE484222325, 0x100000001B3


def fnv1a(name):
    h = FNV_OFFSET
    for c in bytes(name):
        h = ((h ^ c) * FNV_PRIME) & 0xFFFFFFFFFFFFFFFF
    return h


def scan_lines(data):
    """bufio.Scanner with ScanLines and a buffer of MAX_LINE: yields (start, end) of each line's content with the
    trailing '\\r' dropped, then raises ValueError(3) at a line whose content, '\\r' counted, is MAX_LINE bytes or
    more, whether a '\\n' or the end of the text ends it."""
    pos, n = 0, len(data)
    while pos < n:
        nl = data.find(b"\n", pos)
        end = n if nl < 0 else nl
        if end - pos >= MAX_LINE:
            raise ValueError(3)
        e = end - 1 if end > pos and data[end - 1] == 0x0D else end
        yield pos, e
        pos = end + 1


def call_lines(data):
    """(status, [(name_pos, name_len)] in text order with repeats); a failing program has no lines."""
    data = bytes(data)
    lines = []
    try:
        for s, e in scan_lines(data):
            ln = data[s:e]
            if len(ln) == 0 or ln[0] == 0x23:
                continue
            bracket = ln.find(b"(")
            if bracket == -1:
                return 1, []
            call = ln[:bracket]
            start = 0
            eq = call.find(b"=")
            if eq != -1:
                eq += 1
                while eq < len(call) and call[eq] == 0x20:
                    eq += 1
                start = eq
            if len(call) - start == 0:
                return 2, []
            lines.append((s + start, len(call) - start))
    except ValueError:
        return 3, []
    if not lines:
        return 4, []
    return 0, lines


def CallSet(data):
    data = bytes(data)
    status, lines = call_lines(data)
    if status:
        raise ValueError(ERRORS[status])
    return {data[p:p + n] for p, n in lines}


def call_sets(progs):
    """The raw arrays of sg_call_sets for a batch: (status, line_off, name_pos, name_len, names)."""
    status, line_off, pos, ln, names = [], [0], [], [], []
    base = 0
    for p in progs:
        p = bytes(p)
        st, lines = call_lines(p)
        status.append(st)
        for a, n in lines:
            pos.append(base + a)
            ln.append(n)
            names.append(p[a:a + n])
        line_off.append(len(pos))
        base += len(p)
    return (np.array(status, np.uint8), np.array(line_off, np.uint64), np.array(pos, np.uint64),
            np.array(ln, np.uint32), names)


def Hash(data):
    return hashlib.sha1(bytes(data)).digest()


class ONameTable:
    def __init__(self):
        self.ids = {}

    def add(self, names):
        return [self.ids.setdefault(bytes(x), len(self.ids)) for x in names]

    def mask(self, names):
        words = np.zeros((len(self.ids) + 63) // 64, np.uint64)
        for x in names:
            i = self.ids.get(bytes(x))
            if i is not None:
                words[i >> 6] |= np.uint64(1 << (i & 63))
        return words


class OSet:
    """A manager's corpus: map[hash.Sig]bool in insertion order."""

    def __init__(self):
        self.m = {}

    def remove(self, sigs):
        out = np.zeros(len(sigs), bool)
        for k, s in enumerate(sigs):
            out[k] = self.m.pop(bytes(s), None) is not None
        return out

    def export(self):
        return np.frombuffer(b"".join(self.m), np.uint8).reshape(-1, 20)


class OHubCorpus:
    """st.Corpus.Records as key -> [seq, ids], in insertion order."""

    def __init__(self, table):
        self.table = table
        self.recs = {}

    def unknown(self, progs):
        """The spans sg_hubcorpus_add reports: the call lines of status-0 programs whose name the table lacks."""
        _, _, pos, ln, names = call_sets(progs)
        return [(int(p), int(n)) for p, n, x in zip(pos, ln, names) if x not in self.table.ids]

    def add(self, progs, seqs, mgr=None):
        """state.go:326-336 per program, names interned first in order of first appearance: (status, is_new, keys)."""
        progs = [bytes(p) for p in progs]
        seqs = [seqs] * len(progs) if np.isscalar(seqs) else list(seqs)
        parsed = [call_lines(p) for p in progs]
        for p, (st, lines) in zip(progs, parsed):
            self.table.add(p[a:a + n] for a, n in lines)
        status, is_new, keys = [], [], []
        for p, seq, (st, lines) in zip(progs, seqs, parsed):
            key = Hash(p)
            status.append(st)
            keys.append(key)
            new = False
            if st == 0:
                if mgr is not None:
                    mgr.m[key] = True            # :332
                if key not in self.recs:         # :333-335
                    self.recs[key] = [int(seq), [self.table.ids[p[a:a + n]] for a, n in lines]]
                    new = True
            is_new.append(new)
        return np.array(status, np.uint8), np.array(is_new, bool), np.frombuffer(b"".join(keys), np.uint8).reshape(-1, 20)

    def export(self):
        keys = np.frombuffer(b"".join(self.recs), np.uint8).reshape(-1, 20)
        seqs = np.array([r[0] for r in self.recs.values()], np.uint64)
        off = np.zeros(len(self.recs) + 1, np.uint64)
        if self.recs:
            off[1:] = np.cumsum([len(r[1]) for r in self.recs.values()])
        ids = np.array([i for r in self.recs.values() for i in r[1]], np.uint32)
        return keys, seqs, off, ids

    def pending(self, mgr, mgr_seq, hub_seq, mask, max_records=1000):
        """state.go:265-300: (keys, seqs, max_seq, more), ascending (seq, record index)."""
        if mgr_seq == hub_seq:
            return [], [], hub_seq, 0
        mask = [int(w) for w in np.asarray(mask, np.uint64).reshape(-1)]

        def supported(i):
            return (i >> 6) < len(mask) and (mask[i >> 6] >> (i & 63)) & 1

        records = []
        for idx, (key, (seq, ids)) in enumerate(self.recs.items()):
            if mgr_seq >= seq:
                continue
            if key in mgr.m:
                continue
            if not all(supported(i) for i in ids):
                continue
            records.append((seq, idx, key))
        max_seq, more = hub_seq, 0
        records.sort()
        if len(records) > max_records:
            pos = max_records
            max_seq = records[pos][0]
            while pos + 1 < len(records) and records[pos + 1][0] == max_seq:
                pos += 1
            pos += 1
            more = len(records) - pos
            records = records[:pos]
        return [r[2] for r in records], [r[0] for r in records], max_seq, more

    def purge(self, mgrs):
        """state.go:338-354: the deleted keys in record order."""
        used = set()
        for m in mgrs:
            used.update(m.m)
        dels = [k for k in self.recs if k not in used]
        for k in dels:
            del self.recs[k]
        return dels


class _OManager:
    def __init__(self):
        self.Corpus = OSet()
        self.Calls = set()
        self.corpusSeq = 0
        self.Connected = False
        self.Added = self.Deleted = self.New = 0


class OHubState:
    """state.go's State: Connect (:141-173), Sync (:175-195), addInputs, purgeCorpus, pendingInputs."""

    def __init__(self):
        self.table = ONameTable()
        self.Corpus = OHubCorpus(self.table)
        self.corpusSeq = 0
        self.Managers = {}
        self.texts = {}

    def Connect(self, name, fresh, calls, corpus):
        mgr = self.Managers.setdefault(name, _OManager())
        mgr.Connected = True
        if fresh:
            mgr.corpusSeq = 0
        mgr.Calls = {bytes(c) for c in calls}
        mgr.Corpus = OSet()
        self.addInputs(mgr, corpus)
        self.purgeCorpus()

    def Sync(self, name, add, dels):
        mgr = self.Managers.get(name)
        if mgr is None or not mgr.Connected:
            raise ValueError(f"unconnected manager {name}")
        if len(dels) != 0:
            mgr.Corpus.remove([bytes.fromhex(d) if isinstance(d, str) else bytes(d) for d in dels])
            self.purgeCorpus()
        self.addInputs(mgr, add)
        progs, more = self.pendingInputs(mgr)
        mgr.Added += len(add)
        mgr.Deleted += len(dels)
        mgr.New += 2 * len(progs)  # len(progs) of :301-304: as many empty entries as programs in front of them
        return progs, more

    def addInputs(self, mgr, inputs):
        if len(inputs) == 0:
            return
        self.corpusSeq += 1
        _, is_new, keys = self.Corpus.add(inputs, self.corpusSeq, mgr.Corpus)
        for k in np.flatnonzero(is_new):
            self.texts[keys[k].tobytes()] = bytes(inputs[k])

    def purgeCorpus(self):
        for key in self.Corpus.purge([m.Corpus for m in self.Managers.values()]):
            del self.texts[key]

    def pendingInputs(self, mgr, max_records=1000):
        if not isinstance(mgr, _OManager):
            mgr = self.Managers[mgr]
        keys, _, max_seq, more = self.Corpus.pending(mgr.Corpus, mgr.corpusSeq, self.corpusSeq,
                                                     self.table.mask(mgr.Calls), max_records)
        mgr.corpusSeq = max_seq
        return [self.texts[k] for k in keys], more
