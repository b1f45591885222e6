"""Deterministic batches for the ordered-output sweep (sg_triage.hip
owned_outputs: k_own_pipe, k_own_wave, k_own_big), each built to sit on one of
the sweep's routing, capacity or probe-chain edges, with the facts it claims.

What is restated here from the kernels, and nothing else of them:
  own_home(s, bb) = (s * 0x9E3779B1 mod 2^32) >> (32 - bb)   the home bucket
  own_bits(n): the smallest bb >= 4 with 2^bb >= n            buckets of a set of n keys
  the set: 2^bb buckets of four slots, a key in the first bucket from its
      home with room; a lookup stops at the first bucket that is not full
  wave_triage: 0 < |O_r| <= 512 and c1 - c0 < 5 and c1 < nvals // 256
  wave_poll:   |O_r| <= 512
      (a record owning a signal that is not on the wave path is listed for
      k_own_big: the context counter "owned_big_records")

A case is (m0, vals, off) plus its claims; every case runs through both the
flags-and-diff form (sg_triage_batch[_dev], records) and the Poll form
(sg_merge_poll, the same records as polls), so it states the counter for
both.  The claims come from the construction; tests/test_owned_edges.py
checks them on the CPU against facts(), which derives the same numbers from
the oracle's diff lists and the predicates above, never from the library."""
import numpy as np

from oracle import pyoracle as O

SENT = 0xFFFFFFFF
M32 = 0xFFFFFFFF
MULT = 0x9E3779B1
INV = pow(MULT, -1, 1 << 32)
CHUNK = 256        # kChunk: elements per sweep chunk
WAVE_CAP = 512     # kOwnWave: the largest O_r of the wave path
SPAN_CAP = 5       # kOwnCB: chunks a wave-path record of k_own_pipe may span
PIECE = 4096       # kOwnBigCap: keys per piece of k_own_big
BIG_WAVES = 16     # kOwnBigT / 64: k_own_big's waves, chunk batches SPAN_CAP * BIG_WAVES apart
GROUP = 1 << 16    # records per group of the partitioned path


# ---- the restatement ---------------------------------------------------------
def own_home(s, bb):
    return ((int(s) * MULT) & M32) >> (32 - bb)


def own_bits(n):
    bb = 4
    while (1 << bb) < n:
        bb += 1
    return bb


def chain(bb, home, k, lows):
    """k distinct u32 values whose home at bb bits is `home`: the multiplier
    inverted over (home << (32 - bb)) | low for the first k of `lows`."""
    lows = [int(x) for x in lows][:k]
    assert len(lows) == k and len(set(lows)) == k and all(0 <= x < (1 << (32 - bb)) for x in lows)
    assert 0 <= home < (1 << bb)
    return [((((home << (32 - bb)) | low) * INV) & M32) for low in lows]


def wave_triage(n_owned, c0, c1, nvals):
    return 0 < n_owned <= WAVE_CAP and c1 - c0 < SPAN_CAP and c1 < nvals // CHUNK


def wave_poll(n_owned):
    return n_owned <= WAVE_CAP


class OwnedSet:
    """The LDS set on the CPU: insert by first bucket with room, lookup by the
    kernels' stopping rule; probe() also counts the buckets read."""

    def __init__(self, bb):
        self.bb, self.m = bb, (1 << bb) - 1
        self.b = [[] for _ in range(1 << bb)]

    def insert(self, s):
        assert s != SENT  # (held by a flag, never stored)
        h = own_home(s, self.bb)
        while len(self.b[h]) == 4:
            h = (h + 1) & self.m
        self.b[h].append(s)

    def probe(self, s):
        """(member, buckets read, buckets passed in order)"""
        h = own_home(s, self.bb)
        seen = [h]
        while True:
            if s in self.b[h]:
                return True, len(seen), seen
            if len(self.b[h]) < 4:
                return False, len(seen), seen
            h = (h + 1) & self.m
            seen.append(h)

    def counts(self):
        return [len(x) for x in self.b]


# ---- cases ---------------------------------------------------------------------
class Case:
    """name; m0 (maxSignal before), vals, off; owned {record: |O_r|} (every
    other record owns nothing); big_triage / big_poll (the predicted counter
    per form); slice_at (max_launch_records for the sliced rerun, or None);
    chainf (the probe-chain facts, or None); small (the pure-Python loop of
    tests/refmodel.py is run on it); notes {fact name: value} checked one by one."""

    def __init__(self, name, m0, recs, owned, big_triage, big_poll, slice_at=None, chainf=None, notes=None):
        self.name = name
        self.m0 = np.unique(np.asarray(m0, dtype=np.uint32))
        lens = [len(r) for r in recs]
        self.off = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
        self.vals = (np.concatenate([np.asarray(r, dtype=np.uint32) for r in recs]) if sum(lens)
                     else np.zeros(0, np.uint32))
        self.owned = dict(owned)
        self.big_triage, self.big_poll = big_triage, big_poll
        self.slice_at = slice_at
        self.chainf = chainf
        self.notes = notes or {}
        self.small = self.vals.size <= 20000 and len(recs) <= 1000

    def __repr__(self):
        return self.name


def facts(case):
    """The same numbers from the oracle's lists and the restated predicates:
    per-record |O_r| in both forms (the distinct values of the record's diff /
    new-signal list), the record's chunk span, and the counter per form."""
    vals, off = case.vals, case.off
    nvals = int(vals.size)
    _, dv, do = O.triage_batch(O.OSet(case.m0), O.OSet(), vals, off)
    pv, po = O.merge_poll(O.OSet(case.m0), vals, off)
    ot, op_, span = {}, {}, {}
    # only records with a non-empty list are visited (most of 131k records own nothing)
    for r in np.flatnonzero(np.diff(do.astype(np.int64))):
        ot[int(r)] = int(np.unique(dv[int(do[r]):int(do[r + 1])]).size)
    for r in np.flatnonzero(np.diff(po.astype(np.int64))):
        seg = pv[int(po[r]):int(po[r + 1])]
        assert np.unique(seg).size == seg.size  # (Poll lists each new signal once)
        op_[int(r)] = int(seg.size)
    big_t = 0
    for r, n in ot.items():
        c0, c1 = int(off[r]) // CHUNK, (int(off[r + 1]) - 1) // CHUNK
        span[r] = c1 - c0 + 1
        big_t += not wave_triage(n, c0, c1, nvals)
    big_p = sum(not wave_poll(n) for n in op_.values())
    return {"owned_triage": ot, "owned_poll": op_, "span": span, "big_triage": big_t, "big_poll": big_p,
            "np": int(np.unique(dv).size)}


class _Pool:
    """Values of one case: a fixed pool of known ones (maxSignal) and fresh,
    never repeated ones; claim() registers values built elsewhere."""

    def __init__(self, seed, nknown=1024):
        rng = np.random.default_rng(seed)
        v = np.unique(rng.integers(1, SENT, size=200000, dtype=np.uint64).astype(np.uint32))
        v = v[rng.permutation(v.size)]
        self.kn = v[:nknown]
        self.rest, self.at, self.kat = v[nknown:], 0, 0
        self.used = set(int(x) for x in self.kn)

    def known(self, n):
        idx = (self.kat + np.arange(n)) % self.kn.size
        self.kat += n
        return self.kn[idx]

    def fresh(self, n):
        out = []
        while len(out) < n:
            x = int(self.rest[self.at])
            self.at += 1
            if x not in self.used:
                self.used.add(x)
                out.append(x)
        return np.asarray(out, dtype=np.uint32)

    def claim(self, values):
        for x in values:
            assert int(x) != SENT and int(x) not in self.used, "constructed value collides"
            self.used.add(int(x))
        return list(values)


class _Batch:
    def __init__(self, seed):
        self.p = _Pool(seed)
        self.recs, self.owned, self.extra_m0 = [], {}, []

    @property
    def pos(self):
        return sum(len(r) for r in self.recs)

    def known(self, n):
        self.recs.append(self.p.known(n))
        return len(self.recs) - 1

    def start_at(self, mod):
        """a known-only record so that the next record starts at mod (mod 256)"""
        n = (mod - self.pos) % CHUNK
        return self.known(n if n else CHUNK)

    def own(self, length, n_owned, values=None):
        """A record of `length` entries owning `n_owned` signals: its first
        and last entries are owned (one owned: the last), the owned values are
        spread evenly, every third other entry repeats one of them and the
        rest are known."""
        assert 1 <= n_owned <= length
        ov = np.asarray(values, dtype=np.uint32) if values is not None else self.p.fresh(n_owned)
        assert ov.size == n_owned
        at = np.unique(np.round(np.linspace(0, length - 1, n_owned)).astype(np.int64)) if n_owned > 1 \
            else np.asarray([length - 1])
        assert at.size == n_owned
        rec = self.p.known(length).copy()
        rest = np.setdiff1d(np.arange(length), at)
        rep = rest[::3]
        rec[rep] = ov[(np.arange(rep.size) * 7) % n_owned]
        rec[at] = ov
        self.recs.append(rec)
        self.owned[len(self.recs) - 1] = n_owned
        return len(self.recs) - 1

    def raw(self, rec, n_owned):
        self.recs.append(np.asarray(rec, dtype=np.uint32))
        if n_owned:
            self.owned[len(self.recs) - 1] = n_owned
        return len(self.recs) - 1

    def tail(self, mod):
        """a known-only last record of >= 256 entries, the batch then ending at
        mod (mod 256): every earlier record's last chunk is a whole one"""
        n = CHUNK + (mod - self.pos) % CHUNK
        return self.known(n)

    def m0(self):
        return np.concatenate([self.p.kn, np.asarray(self.extra_m0, dtype=np.uint32)])

    def predict(self):
        """the counter per form from the construction: the stated |O_r| and
        the record bounds the builder laid down"""
        off = np.concatenate([[0], np.cumsum([len(r) for r in self.recs])])
        nvals = int(off[-1])
        bt = sum(not wave_triage(n, int(off[r]) // CHUNK, (int(off[r + 1]) - 1) // CHUNK, nvals)
                 for r, n in self.owned.items())
        bp = sum(not wave_poll(n) for n in self.owned.values())
        return bt, bp

    def case(self, name, big_triage, big_poll, **kw):
        # the count the case's author states must be the builder's own
        assert (big_triage, big_poll) == self.predict(), (name, self.predict())
        return Case(name, self.m0(), self.recs, self.owned, big_triage, big_poll, **kw)


def _first_unaligned(b):
    """an owning record (not the first record) whose first element is not at a
    multiple of 4: the sliced rerun starts its second slice there"""
    off = np.concatenate([[0], np.cumsum([len(r) for r in b.recs])])
    for r in sorted(b.owned):
        if r and off[r] % 4:
            return r
    raise AssertionError("no owning record at an element offset that is not a multiple of 4")


# ---- probe chains --------------------------------------------------------------
def chain_case(bb, n_owned, k_home, k_mid, last, seed):
    """One record owning n_owned signals (own_bits(n_owned) == bb), of which
    (a) k_home have the last bucket as home: they fill it and wrap through
        buckets 0, 1, ...;
    (d) k_mid have bucket 0 as home, inside that chain, so that many keys
        are displaced along it;
    the others lie two to a bucket far from it.  The record also holds
    (b) members of m0 with the last bucket as home, and with bucket 0;
    (c) values with the last bucket as home that record 0 owns,
    all misses that walk the whole chain, a known value homed on a half-full
    bucket, and every chain value a second time.  last: the record is the
    batch's last and ends in its partial chunk (k_own_big in the triage form)."""
    assert own_bits(n_owned) == bb and (k_home + k_mid) % 4 == 0
    nb = 1 << bb
    H = nb - 1
    b = _Batch(seed)
    a = b.p.claim(chain(bb, H, k_home, range(k_home)))
    d = b.p.claim(chain(bb, 0, k_mid, range(100, 100 + k_mid)))
    nfill = n_owned - k_home - k_mid
    assert nfill % 2 == 0 and nb // 4 + nfill // 2 <= 3 * nb // 4 and (k_home + k_mid) // 4 <= nb // 4
    fill = []
    for j in range(nfill // 2):
        fill += chain(bb, nb // 4 + j, 2, (200 + j, 300000 + j))
    fill = b.p.claim(fill)
    mb = b.p.claim(chain(bb, H, 6, range(1000, 1006)) + chain(bb, 0, 3, range(1100, 1103)))
    half = b.p.claim(chain(bb, nb // 4, 1, (1200,))) if nfill else []
    mc = b.p.claim(chain(bb, H, 5, range(2000, 2005)))
    b.extra_m0 += mb + half
    # record 0 owns the (c) values; then known padding up to 1 mod 256
    b.raw(np.concatenate([b.p.known(3), mc, b.p.known(2)]), len(mc))
    b.start_at(1)
    body = a + mb + d + mc + fill + half
    n = len(body)
    step = next(s for s in (89, 97, 101, 103) if np.gcd(s, n) == 1)
    body = [body[(i * step) % n] for i in range(n)]
    body += a[::-1] + d  # every chain value again
    rec = b.raw(body, n_owned)
    if not last:
        b.tail(7)
    elif b.pos % CHUNK == 0:
        b.recs[rec] = np.concatenate([b.recs[rec], b.p.known(3)])
    full = (k_home + k_mid) // 4
    # buckets H, 0, .., full - 2 are full and bucket full - 1 is empty: a miss
    # homed on H reads full + 1 buckets, one homed on bucket 0 reads full
    cf = {"bb": bb, "home": H, "rec": rec, "full_run": full, "miss_reads": full + 1, "miss_mid_reads": full,
          "chain": a, "mid": d, "miss_home": mb[:6] + mc, "miss_mid": mb[6:], "half": half}
    return b.case(f"chain_bb{bb}_{'last' if last else 'mid'}", int(last or n_owned > WAVE_CAP),
                  int(n_owned > WAVE_CAP), slice_at=rec, chainf=cf)


def chain_cases():
    out = []
    for last in (False, True):
        out.append(chain_case(4, 16, 9, 3, last, 11))       # buckets 15, 0, 1 full of 16
        out.append(chain_case(6, 64, 64, 0, last, 12))      # every key homed on bucket 63: 63, 0 .. 14 full
        out.append(chain_case(9, 512, 40, 8, last, 13))     # the wave path's largest set
        out.append(chain_case(12, 4096, 100, 12, last, 14))  # one whole piece of k_own_big
    return out


# ---- routing -------------------------------------------------------------------
OWNED_EDGES = (1, 16, 17, 256, 257, 511, 512, 513)


def span_len(start_mod, span, longest):
    """the shortest / longest record starting at start_mod (mod 256) that spans `span` chunks"""
    return CHUNK * span - start_mod if longest else CHUNK * (span - 1) - start_mod + 1


def routing_span_case(span, longest):
    """Owning records starting at 0, 1 and 255 (mod 256), each spanning
    exactly `span` chunks, with |O_r| at every edge of OWNED_EDGES; a
    known-only record of 6 chunks between them; whole chunks to the end."""
    b = _Batch(100 + span * 2 + longest)
    for sm in (0, 1, 255):
        for n in OWNED_EDGES:
            b.start_at(sm)
            b.own(span_len(sm, span, longest), n)
        b.known(6 * CHUNK)
    b.tail(0 if span == 4 else 77)
    nbig = 3 * len(OWNED_EDGES) if span > SPAN_CAP else 3  # span <= 5: only the 513s
    return b.case(f"route_span{span}_{'max' if longest else 'min'}", nbig, 3, slice_at=_first_unaligned(b),
                  notes={"span": span})


def routing_last_case(end_mod, n_owned):
    """the owning record is the batch's last, the batch ending at end_mod (mod 256)"""
    b = _Batch(200 + end_mod + n_owned)
    b.start_at(1)
    b.own(600, 3)
    b.start_at(255)
    length = 2 * CHUNK + (end_mod - (b.pos + 2 * CHUNK)) % CHUNK
    r = b.own(length, n_owned)
    assert b.pos % CHUNK == end_mod
    return b.case(f"route_last_mod{end_mod}_own{n_owned}", 0 if end_mod == 0 else 1, 0, slice_at=r,
                  notes={"end_mod": end_mod})


def routing_lanes_case(nrec, owners, bigs=(), empty=()):
    """nrec short records; `owners` own two signals each, `bigs` own 513,
    `empty` have no entries; record 1 (or 2) is padded so that the batch ends
    on a chunk boundary: no record meets a partial chunk."""
    b = _Batch(300 + nrec + len(owners))
    padrec = next(r for r in range(1, nrec) if r not in owners and r not in bigs and r not in empty)
    for r in range(nrec):
        if r in bigs:
            b.own(700, 513)
        elif r in owners:
            b.own(5, 2)
        elif r in empty:
            b.raw([], 0)
        else:
            b.known(3)
    b.recs[padrec] = b.p.known(3 + (-b.pos) % CHUNK)
    assert b.pos % CHUNK == 0 and len(b.recs) == nrec
    return b.case(f"route_lanes_{nrec}_{len(owners)}own_{len(bigs)}big", len(bigs), len(bigs),
                  slice_at=_first_unaligned(b), notes={"nrec": nrec})


def bb_steps_case():
    """|O_r| on both sides of every bucket-count step below the wave cap"""
    b = _Batch(400)
    for n in (2, 15, 16, 17, 32, 33, 64, 65, 128, 129, 256, 257):
        b.start_at(3)
        b.own(n + 40, n)
    b.tail(5)
    return b.case("bb_steps", 0, 0, slice_at=_first_unaligned(b))


def routing_cases():
    out = [routing_span_case(4, True), routing_span_case(5, False), routing_span_case(5, True),
           routing_span_case(6, False)]
    for end_mod in (0, 1, 255):
        for n in (1, 512):
            out.append(routing_last_case(end_mod, n))
    out.append(routing_lanes_case(63, {0, 62}))
    out.append(routing_lanes_case(64, {0, 63}))
    out.append(routing_lanes_case(65, {0, 63, 64}))                                   # block 1: exactly one
    # a block of 64 wave-path records; then one with none (a known-only record, empty ones, one for k_own_big)
    out.append(routing_lanes_case(128, set(range(64)), bigs={127}, empty=set(range(65, 127))))
    out.append(routing_lanes_case(129, {0, 63, 128} | set(range(64, 128))))              # two, 64, one
    out.append(bb_steps_case())
    return out


# ---- pieces --------------------------------------------------------------------
def piece_case(n_owned, sent):
    """One record owning n_owned signals, every one of them twice, the two
    occurrences in different chunks (>= 256 entries apart).  sent: 0xFFFFFFFF
    is one of them (its key lies in the highest partition bucket; which piece
    of the record's keys holds it is the bucket stage's emit order)."""
    b = _Batch(500 + n_owned)
    b.start_at(9)
    ov = b.p.fresh(n_owned)
    if sent:
        ov[n_owned // 2] = SENT
    rec = np.concatenate([ov, b.p.known(CHUNK + 5), ov[::-1]])
    r = b.raw(rec, n_owned)
    b.tail(100)
    return b.case(f"piece_{n_owned}{'_ff' if sent else ''}", 1, 1, slice_at=r,
                  notes={"pieces": -(-n_owned // PIECE), "twice_apart": CHUNK + 6})


def piece_cases():
    return [piece_case(4095, False), piece_case(4096, False), piece_case(4097, True), piece_case(8192, False),
            piece_case(8193, True)]


# ---- totals ----------------------------------------------------------------------
def totals_cases():
    """batches whose whole new signal is 0, 1 and 2 values (the sort is skipped,
    one 8-byte copy, run)"""
    out = []
    b = _Batch(600)
    for n in (5, 300, 0, 7):
        b.known(n)
    out.append(b.case("total_0", 0, 0, notes={"np": 0}))
    for name, v in (("ord", 0x12345678), ("zero", 0), ("ff", SENT)):
        b = _Batch(601)
        b.known(5)
        b.start_at(2)
        b.p.used.discard(v)
        b.raw(np.concatenate([b.p.known(2), [v], b.p.known(3), [v]]), 1)
        b.tail(0)
        out.append(b.case(f"total_1_{name}", 0, 0, notes={"np": 1}))
    b = _Batch(602)
    b.known(4)
    b.raw(np.concatenate([[0x0BADF00D], b.p.known(2)]), 1)
    b.known(9)
    b.raw(np.concatenate([b.p.known(2), [0x0BADF00D, SENT]]), 1)  # (the first value again: not owned here)
    out.append(b.case("total_2", 2, 0, notes={"np": 2}))  # 20 entries: one partial chunk, both records to k_own_big
    return out


# ---- record groups ---------------------------------------------------------------
GROUP_OWNERS = (0, 65535, 65536, 65537, 131071, 131072, 131073)


def groups_case(whole):
    """131,074 records, nearly all without entries; GROUP_OWNERS own one
    signal each, r and r + 65536 neighbours of one partition bucket.  whole:
    the batch ends on a chunk boundary (every owner on the wave path), else
    all of it lies in one partial chunk (every owner to k_own_big)."""
    b = _Batch(700)
    nrec = 2 * GROUP + 2
    recs = [np.zeros(0, np.uint32)] * nrec
    base = 0x5EED0000
    for j, r in enumerate(GROUP_OWNERS):
        s = base + (r % GROUP) * 2 + (r // GROUP)
        recs[r] = np.concatenate([b.p.known(1), [s], b.p.known(1)]).astype(np.uint32)
        b.owned[r] = 1
    if whole:
        n = sum(len(x) for x in recs)
        recs[70000] = b.p.known((-n) % CHUNK)
    b.recs = recs
    nb = 0 if whole else len(GROUP_OWNERS)
    return b.case(f"groups_{'whole' if whole else 'partial'}", nb, 0, slice_at=65537, notes={"nrec": nrec})


# ---- Poll forms --------------------------------------------------------------------
def poll_boundary_case(n_extra):
    """A record from a chunk boundary, 7 chunks long: the last element of
    chunk j and the first of chunk j + 1 are the same new value; n_extra more
    new values in between (0: the wave path of the Poll form; 600: k_own_big)."""
    b = _Batch(800 + n_extra)
    b.start_at(0)
    nch = 7
    rec = b.p.known(nch * CHUNK + 1).copy()
    v = b.p.fresh(nch)
    for j in range(nch):
        rec[CHUNK * j + CHUNK - 1] = v[j]
        rec[CHUNK * (j + 1)] = v[j]
    if n_extra:
        x = b.p.fresh(n_extra)
        at = 2 + 2 * np.arange(n_extra)
        at = at[(at % CHUNK != 0) & (at % CHUNK != CHUNK - 1)][:n_extra]
        x = x[:at.size]
        rec[at] = x
        n_extra = at.size
    r = b.raw(rec, nch + n_extra)
    b.tail(3)
    big = int(nch + n_extra > WAVE_CAP)
    return b.case(f"poll_boundary_{nch + n_extra}", 1, big, slice_at=None, notes={"rec": r, "pairs": nch})


def poll_waves_case():
    """A record of k_own_big whose 600 new values come three times: at p, p +
    5 chunks (another wave's chunk batch) and p + 80 chunks (the same wave's
    next one)."""
    b = _Batch(900)
    b.start_at(0)
    step1, step2 = SPAN_CAP * CHUNK, SPAN_CAP * BIG_WAVES * CHUNK
    v = b.p.fresh(600)
    rec = b.p.known(step2 + 600).copy()
    for s in (0, step1, step2):
        rec[s:s + 600] = v
    b.raw(rec, 600)
    b.tail(0)
    return b.case("poll_waves", 1, 1, notes={"steps": (step1, step2)})


def poll_ff_case(n_extra):
    """0xFFFFFFFF three times across a chunk boundary (elements 254, 255, 256
    of the record), n_extra other new values around it"""
    b = _Batch(950 + n_extra)
    b.start_at(0)
    rec = b.p.known(2 * CHUNK).copy()
    if n_extra:
        rec = np.concatenate([rec, b.p.fresh(n_extra)])
    rec[[CHUNK - 2, CHUNK - 1, CHUNK]] = SENT
    b.raw(rec, 1 + n_extra)
    b.tail(0)
    big = int(1 + n_extra > WAVE_CAP)
    return b.case(f"poll_ff_{1 + n_extra}", big, big)


def poll_cases():
    return [poll_boundary_case(0), poll_boundary_case(600), poll_waves_case(), poll_ff_case(0), poll_ff_case(511),
            poll_ff_case(512)]


_ALL = None


def all_cases():
    global _ALL
    if _ALL is None:
        _ALL = (chain_cases() + routing_cases() + piece_cases() + totals_cases()
                + [groups_case(True), groups_case(False)] + poll_cases())
        names = [c.name for c in _ALL]
        assert len(set(names)) == len(names)
    return _ALL
