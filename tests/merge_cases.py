"""Deterministic cases for the pkg/cover slice algebra (sg_merge.hip): every
merge path -- generic (k_merge_keep / scan / k_merge_scatter / k_merge_len),
k_diff_small, and k_merge_small's gap and tile forms -- HasDifference and the
big Canonicalize path, each case built to sit on one of the kernels' constants,
with the facts it claims.

What is restated here from sg_merge.hip, and nothing else of it:
  merge_dev's routing: Union / SymmetricDifference take k_merge_small iff every
      pair has min(a_len, b_len) <= 4096 (kMS), Difference / Intersection take
      k_diff_small iff every pair has a_len <= 4096, both only while every pair
      has a_len + b_len < 2^32; otherwise the whole batch is generic.  A
      k_merge_small pair is a gap pair iff nl >= 32 ns (kGapRatio), else a tile
      pair (tiles of 8192 = kMTile values of the large side L).
  canonicalize_dev's routing: no segment above 4096 (kTile) values -> one pass,
      a wave per list of <= 1024 (kWaveList) values, a workgroup per longer
      one; else the big path: 4096-value sorted runs and one rank-merge pass
      per doubling of the run width below the longest segment, a segment's
      result in buffer (its own passes & 1).
  the element rule of the file's header, as a positional model per path
      (model()), with named mistakes a kernel could make.

A merge case is a list of pairs, each declared with the k_merge_small form its
lengths select ("gap" / "tile", or "big" when neither side fits) and which of
its sides fit ("a", "b", "ab", ""); the counters the case claims per op follow
from the declarations alone, and tests/test_merge_edges.py checks them against
route() on the lengths.  Every case also exists with its sides swapped, so
each edge is met with either side the small one."""
import numpy as np

SENT = 0xFFFFFFFF
TOP = 0xFFFFFFFE   # the largest value that is not the sentinel
DIFF, SYMDIFF, UNION, INTER = 0, 1, 2, 3
OPS = (DIFF, SYMDIFF, UNION, INTER)
OPNAME = {DIFF: "Difference", SYMDIFF: "SymmetricDifference", UNION: "Union", INTER: "Intersection"}
KMS = 4096         # kMS: the largest small side
GAP_RATIO = 32     # kGapRatio
MTILE = 8192       # kMTile: L values per tile of the tile form
TILE = 4096        # kTile: a sorted run of Canonicalize
CHUNK = 256        # kChunk: elements per ballot chunk of the generic path
WAVE_LIST = 1024   # kWaveList
HD_GRID = 4096 * 256  # k_has_difference's threads (single-pair form)
HD_BLOCK = 256     # k_has_difference_batch's threads per pair


def u32(x):
    return np.ascontiguousarray(np.asarray(x, dtype=np.uint64).astype(np.uint32))


def srt(*parts):
    return np.sort(np.concatenate([u32(p).reshape(-1) for p in parts])) if parts else u32([])


def rep(v, n):
    return np.full(n, v, dtype=np.uint32)


# ---- the restatement -----------------------------------------------------------
def is_gap(ns, nl):
    return nl >= GAP_RATIO * ns


def route(op, alen, blen):
    """(generic, diff_small, gap, tile) pairs of one merge_dev call"""
    alen, blen = [int(x) for x in alen], [int(x) for x in blen]
    n = len(alen)
    fits = all(x + y < (1 << 32) for x, y in zip(alen, blen))
    if op in (UNION, SYMDIFF):
        if fits and all(min(x, y) <= KMS for x, y in zip(alen, blen)):
            g = sum(1 for x, y in zip(alen, blen) if is_gap(min(x, y), max(x, y)))
            return (0, 0, g, n - g)
    elif fits and all(x <= KMS for x in alen):
        return (0, n, 0, 0)
    return (n, 0, 0, 0)


def pair_path(op, alen, blen, k):
    """the path pair k of the batch takes"""
    r = route(op, alen, blen)
    if r[0]:
        return "generic"
    if r[1]:
        return "diff_small"
    return "gap" if is_gap(min(int(alen[k]), int(blen[k])), max(int(alen[k]), int(blen[k]))) else "tile"


def canon_passes(n):
    p, w = 0, TILE
    while w < n:
        p, w = p + 1, w * 2
    return p


def canon_route(lens):
    """(wave lists, block lists, big segments, merge passes) of one canonicalize_dev call"""
    lens = [int(x) for x in lens]
    big = [x for x in lens if x > TILE]
    if not big:
        return (sum(1 for x in lens if 0 < x <= WAVE_LIST), sum(1 for x in lens if WAVE_LIST < x <= TILE), 0, 0)
    return (0, 0, len(big), canon_passes(max(big)))


# ---- the positional model --------------------------------------------------------
MISTAKES = {
    # name: (paths it can be made on, what it is)
    "t_from_tile": (("tile",), "L's copy index t counted from the tile start, not the list start"),
    "lost_at_nl": (("tile",), "S elements with insertion point nl lost when nl % 8192 == 0"),
    "dense_cap16": (("tile",), "a 64-value window's S range read 16 values deep only"),
    "no_sentinel_clamp": (("gap",), "gap copies not clamped at L's first sentinel"),
    "drops_cl": (("gap",), "gap drops taken as cl instead of min(cl, cS)"),
    "q_eq_nb_match": (("diff_small",), "k_diff_small treating q == nb as a match"),
    "sentinel_kept": (("generic", "diff_small", "gap", "tile"), "a sentinel kept when the other side lacks it"),
    "keep_off_by_one": (("generic",), "copy t kept iff t > c (t <= c) instead of t >= c (t < c)"),
    "ties_wrong_bound": (("generic",), "cov0's position counts cov1's kept copies of its own value"),
}


def _ss(lst, x, side):
    return np.searchsorted(lst, x, side).astype(np.int64)


def _copy_index(lst):
    return np.arange(lst.size, dtype=np.int64) - _ss(lst, lst, "left")


def _excl(flags):
    out = np.zeros(flags.size + 1, dtype=np.int64)
    np.cumsum(flags, out=out[1:])
    return out


def _keep(op, side, t, c, slack=0):
    if op == DIFF:
        return t >= c + slack if side == 0 else np.zeros(t.size, bool)
    if op == INTER:
        return t < c + slack if side == 0 else np.zeros(t.size, bool)
    if op == UNION:
        return np.ones(t.size, bool) if side == 0 else t >= c + slack
    return t >= c + slack


def _scatter(n, parts):
    """the writes of a model; None when one lands outside [0, n) or two collide,
    unwritten positions -1"""
    out = np.full(int(n), -1, dtype=np.int64)
    for pos, vals in parts:
        if pos.size == 0:
            continue
        if pos.min() < 0 or pos.max() >= n or (out[pos] != -1).any() or np.unique(pos).size != pos.size:
            return None
        out[pos] = vals
    return out


def _model_generic(op, a, b, mk):
    ta, tb = _copy_index(a), _copy_index(b)
    la, ua = _ss(b, a, "left"), _ss(b, a, "right")
    lb, ub = _ss(a, b, "left"), _ss(a, b, "right")
    slack = 1 if mk == "keep_off_by_one" else 0
    ka, kb = _keep(op, 0, ta, ua - la, slack), _keep(op, 1, tb, ub - lb, slack)
    if mk != "sentinel_kept":
        ka, kb = ka & (a != SENT), kb & (b != SENT)
    pa, pb = _excl(ka), _excl(kb)
    pos_a = pa[:-1][ka] + pb[(ua if mk == "ties_wrong_bound" else la)[ka]]
    pos_b = pb[:-1][kb] + pa[ub[kb]]
    return _scatter(pa[-1] + pb[-1], [(pos_a, a[ka]), (pos_b, b[kb])])


def _small_sides(a, b):
    sS = 0 if a.size <= b.size else 1
    return (sS, a, b) if sS == 0 else (sS, b, a)


def _model_tile(op, a, b, mk):
    sS, S, L = _small_sides(a, b)
    sL, ns, nl = 1 - sS, S.size, L.size
    lbL, ubL = _ss(L, S, "left"), _ss(L, S, "right")
    kS = _keep(op, sS, _copy_index(S), ubL - lbL)
    if mk != "sentinel_kept":
        kS = kS & (S != SENT)
    sidx = lbL if sS == 0 else ubL
    skp = _excl(kS)
    i = np.arange(nl, dtype=np.int64)
    first = _ss(L, L, "left")
    if mk == "t_from_tile":
        first = np.maximum(first, (i // MTILE) * MTILE)
    lbs, ubs = _ss(S, L, "left"), _ss(S, L, "right")
    if mk == "dense_cap16":
        for w0 in range(0, nl, 64):
            w1 = min(w0 + 64, nl)
            jA, jB = int(_ss(S, L[w0], "left")), int(_ss(S, L[w1 - 1], "right"))
            if jB - jA > 16:
                win = S[jA:jA + 16]
                lbs[w0:w1] = jA + _ss(win, L[w0:w1], "left")
                ubs[w0:w1] = jA + _ss(win, L[w0:w1], "right")
    kL = _keep(op, sL, i - first, ubs - lbs)
    if mk != "sentinel_kept":
        kL = kL & (L != SENT)
    rank = _excl(kL)
    pos_L = rank[:-1][kL] + skp[(lbs if sL == 0 else ubs)[kL]]
    wS = kS & (sidx != nl) if mk == "lost_at_nl" and nl % MTILE == 0 else kS
    pos_S = skp[:-1][wS] + rank[sidx[wS]]
    return _scatter(skp[-1] + rank[-1], [(pos_L, L[kL]), (pos_S, S[wS])])


def _model_gap(op, a, b, mk):
    sS, S, L = _small_sides(a, b)
    sL, nl = 1 - sS, L.size
    ldrop = op == SYMDIFF or sL == 1
    lbL, ubL = _ss(L, S, "left"), _ss(L, S, "right")
    kS = _keep(op, sS, _copy_index(S), ubL - lbL)
    if mk != "sentinel_kept":
        kS = kS & (S != SENT)
    skp = _excl(kS)
    nle = nl if mk == "no_sentinel_clamp" else int(_ss(L, SENT, "left"))
    i = np.arange(nl, dtype=np.int64)
    tL = i - _ss(L, L, "left")
    cl = _ss(L, L, "right") - _ss(L, L, "left")
    lbs, ubs = _ss(S, L, "left"), _ss(S, L, "right")
    cS = ubs - lbs
    d = np.where(cS > 0, cl, 0) if mk == "drops_cl" else np.minimum(cl, cS)
    dropped = (tL < d) & (L != SENT) if ldrop else np.zeros(nl, bool)
    D = _excl(dropped)
    kL = ~dropped & (i < nle)
    pos_L = i[kL] - D[:-1][kL] + skp[ubs[kL]]
    pos_S = lbL[kS] - D[lbL[kS]] + skp[:-1][kS]
    return _scatter(skp[-1] + nle - D[-1], [(pos_L, L[kL]), (pos_S, S[kS])])


def _model_diff(op, a, b, mk):
    t, lo = _copy_index(a), _ss(b, a, "left")
    q = lo + t
    inb = q < b.size
    more = np.zeros(a.size, bool)
    more[inb] = b[q[inb]] == a[inb]
    if mk == "q_eq_nb_match":
        more |= q == b.size
    keep = ~more if op == DIFF else more
    if mk != "sentinel_kept":
        keep = keep & (a != SENT)
    return a[keep].astype(np.int64)


def model(op, a, b, path, mistake=None):
    """The result of `op` on one pair as the kernels of `path` place it, element
    by element; None (or -1 entries) where a mistaken form writes outside the
    result or twice to one place."""
    a, b = np.asarray(a, dtype=np.int64), np.asarray(b, dtype=np.int64)
    assert mistake is None or path in MISTAKES[mistake][0]
    f = {"generic": _model_generic, "tile": _model_tile, "gap": _model_gap, "diff_small": _model_diff}[path]
    return f(op, a, b, mistake)


def same(m, want):
    return m is not None and m.size == want.size and np.array_equal(m, want.astype(np.int64))


# ---- the generic path over a whole batch --------------------------------------------
# Its kernels work in the virtual element space of all pairs' lists laid end to
# end: an element finds its pair by a search of the offsets (seg_search: the
# last pair whose offset is <= u, so empty pairs before it are passed over),
# and "kept elements before" is a difference of two global prefixes, taken at
# the element and at its pair's start.  The prefix past the last chunk (only
# the total itself, when it is a multiple of 4096) is the grand total.
BATCH_MISTAKES = {
    "seg_first_repeat": "k_merge_scatter's pair search stops at the first of equal offsets (an empty pair)",
    "no_pair_base": "the kept count before the pair's start not subtracted",
    "prefix_end_zero": "the prefix past the last chunk taken as 0, not the total",
}


def model_generic_batch(op, layout, mistake=None):
    """Every pair's result as the generic path places it in the batch's output
    (out_beg = the running sum of a_len + b_len); None where a mistaken form
    reads or writes outside the buffers, writes twice to one place or gives a
    length outside its range."""
    A, ab, al, B, bb, bl = [np.asarray(x).astype(np.int64) for x in layout]
    npair = al.size
    obeg = _excl(al + bl)
    sides = []
    for s in (0, 1):
        v, beg, ln = (A, ab, al) if s == 0 else (B, bb, bl)
        ov, obg, oln = (B, bb, bl) if s == 0 else (A, ab, al)
        off = _excl(ln)
        n = int(off[-1])
        keep = np.zeros(n, bool)
        if s == 0 or op in (UNION, SYMDIFF):
            for k in range(npair):
                mine, other = v[beg[k]:beg[k] + ln[k]], ov[obg[k]:obg[k] + oln[k]]
                c = _ss(other, mine, "right") - _ss(other, mine, "left")
                keep[off[k]:off[k + 1]] = _keep(op, s, _copy_index(mine), c) & (mine != SENT)
            live = n > 0
        else:
            live = False  # Difference / Intersection: cov1 has no masks (nchunks[1] == 0)
        sides.append({"v": v, "beg": beg, "len": ln, "off": off, "n": n, "keep": keep, "P": _excl(keep),
                      "cap": -(-n // TILE) * TILE, "live": live})

    def pre(sd, p):
        end = 0 if mistake == "prefix_end_zero" else sd["P"][-1]
        return np.where(p >= sd["cap"], end, sd["P"][np.minimum(p, sd["n"])])

    out = np.full(int(obeg[-1]), -1, dtype=np.int64)
    for s in (0, 1):
        me, ot = sides[s], sides[1 - s]
        if not me["live"]:
            continue
        u = np.flatnonzero(me["keep"])
        k = _ss(me["off"], u, "right") - 1
        if mistake == "seg_first_repeat":
            k = _ss(me["off"], me["off"][k], "left")
        src = me["beg"][k] + (u - me["off"][k])
        if src.size and src.max() >= me["v"].size:
            return None
        x = me["v"][src]
        pos = pre(me, u) - (0 if mistake == "no_pair_base" else pre(me, me["off"][k]))
        if ot["live"]:
            j = np.zeros(u.size, np.int64)
            for kk in np.unique(k):
                sel = k == kk
                other = ot["v"][ot["beg"][kk]:ot["beg"][kk] + ot["len"][kk]]
                j[sel] = _ss(other, x[sel], "left" if s == 0 else "right")
            pos = pos + pre(ot, ot["off"][k] + j) - pre(ot, ot["off"][k])
        dest = obeg[k] + pos
        if dest.size and (dest.min() < 0 or dest.max() >= out.size or (out[dest] != -1).any()
                          or np.unique(dest).size != dest.size):
            return None
        out[dest] = x
    res = []
    for k in range(npair):
        n = sum(int(pre(sd, sd["off"][k + 1]) - pre(sd, sd["off"][k])) for sd in sides if sd["live"])
        if n < 0 or n > al[k] + bl[k]:
            return None
        res.append(out[obeg[k]:obeg[k] + n])
    return res


# ---- merge cases -----------------------------------------------------------------
class MergeCase:
    """name, family; pairs [(a, b)] with kinds ["gap" | "tile" | "big"] and fits
    ["a" | "b" | "ab" | ""]; the layout (a, a_beg, a_len, b, b_beg, b_len) the
    batch call gets (the pairs laid end to end unless the case gives one);
    notes {fact: value} checked one by one on the CPU."""

    def __init__(self, name, family, notes=None):
        self.name, self.family = name, family
        self.pairs, self.kinds, self.fits = [], [], []
        self.layout = None
        self.notes = notes or {}

    def add(self, a, b, kind, fits):
        a, b = u32(a), u32(b)
        assert np.all(a[:-1] <= a[1:]) and np.all(b[:-1] <= b[1:]), self.name
        assert kind in ("gap", "tile", "big") and fits in ("a", "b", "ab", "")
        a.setflags(write=False)
        b.setflags(write=False)
        self.pairs.append((a, b))
        self.kinds.append(kind)
        self.fits.append(fits)
        return self

    def claim(self, op):
        """(generic, diff_small, gap, tile) from the declarations"""
        n = len(self.pairs)
        if op in (UNION, SYMDIFF):
            if "big" in self.kinds:
                return (n, 0, 0, 0)
            return (0, 0, self.kinds.count("gap"), self.kinds.count("tile"))
        return (0, n, 0, 0) if all("a" in f for f in self.fits) else (n, 0, 0, 0)

    def claim_pair(self, op, k):
        """... of pair k run on its own"""
        if op in (UNION, SYMDIFF):
            kd = self.kinds[k]
            return (1, 0, 0, 0) if kd == "big" else (0, 0, int(kd == "gap"), int(kd == "tile"))
        return (0, 1, 0, 0) if "a" in self.fits[k] else (1, 0, 0, 0)

    def lens(self):
        return [a.size for a, _ in self.pairs], [b.size for _, b in self.pairs]

    def batch(self):
        if self.layout is not None:
            return self.layout
        al, bl = self.lens()
        a = np.concatenate([x for x, _ in self.pairs]) if self.pairs else u32([])
        b = np.concatenate([y for _, y in self.pairs]) if self.pairs else u32([])
        ab = np.concatenate([[0], np.cumsum(al)[:-1]]).astype(np.uint64)
        bb = np.concatenate([[0], np.cumsum(bl)[:-1]]).astype(np.uint64)
        return u32(a), ab, np.array(al, np.uint64), u32(b), bb, np.array(bl, np.uint64)

    def swapped(self):
        c = MergeCase(self.name + "_sw", self.family, self.notes)
        for (a, b), kd, f in zip(self.pairs, self.kinds, self.fits):
            c.add(b, a, kd, {"a": "b", "b": "a"}.get(f, f))
        if self.layout is not None:
            a, ab, al, b, bb, bl = self.layout
            c.layout = (b, bb, bl, a, ab, al)
        return c

    def __repr__(self):
        return self.name


def _fill(n, lo, step, odd=0):
    return u32(lo + step * np.arange(n, dtype=np.int64) + odd)


def _routing():
    out = []
    A = _fill(4096, 0, 3)
    big_l = srt(_fill(131071, 0, 2), [TOP])           # 131072 = 32 * 4096
    base = [
        (A, _fill(4096, 1, 2), "tile", "ab"),           # na == nb == 4096
        (A, _fill(5000, 0, 5), "tile", "a"),
        (_fill(5000, 0, 5), A, "tile", "b"),
        (A, big_l, "gap", "a"),                         # nl == 32 ns
        (A, big_l[:-1], "tile", "a"),                   # nl == 32 ns - 1
        ([], [], "gap", "ab"),                          # ns == 0, nl == 0
        ([], [7], "gap", "ab"),                         # ns == 0, nl == 1
        (_fill(300, 0, 1), [], "gap", "ab"),            # ns == 0, nl == 300
        ([0, 5, TOP], _fill(96, 0, 1), "gap", "ab"),    # nl == 32 ns
        ([0, 5, TOP], _fill(95, 0, 1), "tile", "ab"),   # nl == 32 ns - 1
        ([4, 4, 9], [4, 9, 9], "tile", "ab"),           # na == nb
        ([], [], "gap", "ab"),
    ]
    c = MergeCase("route_min4096", "routing")
    for p in base:
        c.add(*p)
    out.append(c)
    c = MergeCase("route_min4097", "routing")           # one pair with no small side: all generic
    for p in base[:6]:
        c.add(*p)
    c.add(_fill(4097, 0, 3), _fill(4097, 1, 2), "big", "")
    for p in base[6:]:
        c.add(*p)
    out.append(c)
    # Difference / Intersection: a_len at 4096 everywhere, then one at 4097
    basea = [
        (A, _fill(100000, 0, 2), "tile", "a"),
        (A, A, "tile", "ab"),
        ([], _fill(5000, 0, 1), "gap", "a"),
        ([], [], "gap", "ab"),
        (_fill(4096, 5, 1), _fill(4097, 0, 2), "tile", "a"),
        ([0], [], "gap", "ab"),
    ]
    c = MergeCase("route_a4096", "routing")
    for p in basea:
        c.add(*p)
    out.append(c)
    c = MergeCase("route_a4097", "routing")
    for p in basea[:3]:
        c.add(*p)
    c.add(_fill(4097, 0, 3), [1, 3, 6], "gap", "b")     # a_len 4097: Difference / Intersection go generic
    for p in basea[3:]:
        c.add(*p)
    out.append(c)
    return out


def _tile():
    out = []
    c = MergeCase("tile_nl_edges", "tile")
    for nl in (8191, 8192, 8193, 16384, 16385):
        ns = nl // 32 + 1
        L = _fill(nl, 0, 3)
        idx = np.linspace(0, nl - 1, ns).astype(np.int64)
        S = u32(L[idx].astype(np.int64) + (np.arange(ns) % 2))  # every other one present in L
        S[-1] = TOP
        c.add(S, L, "tile", "a")
    out.append(c)
    # insertion points 0, 8191, 8192 (a tile end) and nl; nl a multiple of 8192 and not
    c = MergeCase("tile_ins_points", "tile", {"ins": (0, 8191, 8192)})
    for nl in (16384, 16385, 8192, 12000):
        L = _fill(nl, 10, 2)
        v = lambda i: int(L[i])  # noqa: E731
        edge = [0, 5, v(8191) - 1, v(8191), v(8191), v(nl - 1), v(nl - 1) + 1, TOP]
        if nl > 8192:
            edge += [v(8192) - 1, v(8192)]
        fillers = [v(100 + 16 * k) + 1 for k in range(nl // 32 + 10) if 100 + 16 * k < nl]
        c.add(srt(edge, fillers), L, "tile", "a")
    out.append(c)
    # a run of one L value across the 8192 boundary, S's count of it 1, run - 1, run, run + 1
    run, X = 400, 20000
    c = MergeCase("tile_run_cross", "tile", {"run": (8000, run)})
    L = srt(_fill(8000, 0, 2), rep(X, run), _fill(3600, 20001, 3))
    for cnt in (1, run - 1, run, run + 1):
        c.add(srt(rep(X, cnt), _fill(400, 1, 75)), L, "tile", "a")
    out.append(c)
    # 16 and 17 S values inside one 64-value window of L
    c = MergeCase("tile_dense_16_17", "tile", {"dense": (16, 17)})
    L = _fill(2048, 0, 1000)
    for cnt in (16, 17):
        inside = [int(L[64]) + 1 + 3000 * q for q in range(cnt)]   # L[64] < .. < L[127]
        inside[3] = int(L[67])                                     # some of them equal to L values
        inside[9] = int(L[96])
        fillers = [int(L[64 * w + 10 * h]) + 7 for w in range(32) if w != 1 for h in (1, 3)]
        c.add(srt(inside, fillers), L, "tile", "ab")
    out.append(c)
    # ballot_count's steps: all of S below all of L, and above
    c = MergeCase("tile_ballot_steps", "tile")
    for ns, nl in ((63, 2000), (64, 2000), (65, 2000), (4096, 9000)):
        fits = "ab" if nl <= KMS else "a"
        c.add(_fill(ns, 0, 1), _fill(nl, 10000, 2), "tile", fits)
        c.add(_fill(ns, TOP - ns + 1, 1), _fill(nl, 0, 2), "tile", fits)
    out.append(c)
    # S of 4096 equal values against L runs that are shorter, equal and longer
    c = MergeCase("tile_s4096_equal", "tile")
    for r in (100, 4096, 5000):
        c.add(rep(77777, 4096), srt(_fill(6000, 0, 3), rep(77777, r), _fill(3000, 80000, 1)), "tile", "a")
    out.append(c)
    # L's sentinel tail crossing the last tile's start; S all sentinels
    c = MergeCase("tile_sentinels", "tile", {"sent_tail": (8100, 8292)})
    L = srt(_fill(8100, 0, 2), rep(SENT, 192))
    c.add(srt(_fill(300, 1, 50), [8000, 8000, TOP, SENT, SENT]), L, "tile", "a")
    c.add(rep(SENT, 300), _fill(5000, 0, 1), "tile", "a")
    c.add(rep(SENT, 300), srt(_fill(4000, 0, 1), rep(SENT, 1000)), "tile", "a")
    out.append(c)
    return out


def _gap():
    out = []
    c = MergeCase("gap_4096_runs", "gap", {"runs": 4096})
    S = u32(64 * np.arange(4096, dtype=np.int64) + (np.arange(4096) % 2))  # every other one absent from L
    S[-1] = TOP
    c.add(S, _fill(131072, 0, 2), "gap", "a")
    out.append(c)
    c = MergeCase("gap_4096_equal", "gap", {"runs": 1})
    for r in (4095, 4096, 4097):
        c.add(rep(99999, 4096), srt(_fill(131072 - r - 1000, 0, 2), rep(99999, r), _fill(1000, 200000, 7)), "gap", "a")
    out.append(c)
    # S's count of a value below, equal to and above L's count; the first gap empty / the last gap empty
    c = MergeCase("gap_counts", "gap")
    S = [5, 5, 9, 9, 9, 12, 40, 40, 40, 40, 300, 300]
    c.add(S, srt(rep(5, 3), rep(9, 3), rep(40, 2), _fill(400, 0, 1)), "gap", "ab")          # 3+1, 3+1, 0+1, 2+1, 1
    c.add(S, srt(rep(5, 30), rep(9, 3), rep(300, 2), _fill(400, 5, 1)), "gap", "ab")        # first gap empty
    c.add(S, srt(rep(5, 1), rep(300, 300), _fill(290, 0, 1), rep(300, 100)), "gap", "ab")   # last gap empty
    out.append(c)
    # gaps of 0, 1, 63, 64, 65, 255, 256 and 257 values between S's values, present in L and absent
    glen = (0, 1, 63, 64, 65, 255, 256, 257)
    c = MergeCase("gap_lengths", "gap", {"gaps": glen})
    for present in (False, True):
        L, S = [], []
        for k, g in enumerate(glen):
            s = 1000 * (k + 1)
            S.append(s)
            if present:
                L.append(s)
            L.extend(range(s + 1, s + 1 + g))
        S.append(9500)                                   # the last gap: empty
        if present:
            L.append(9500)
        c.add(S, sorted(L), "gap", "ab")
        c.add(S, srt([0], L), "gap", "ab")               # a first gap of one value
    out.append(c)
    # more than 16 runs (the per-wave gap loop) and more than 64
    c = MergeCase("gap_many_runs", "gap", {"runs": (17, 100)})
    c.add(_fill(17, 3, 50), _fill(1000, 0, 1), "gap", "ab")
    c.add(srt(_fill(100, 0, 40), _fill(30, 0, 80)), _fill(4200, 0, 1), "gap", "a")    # 100 runs, 30 of them pairs
    out.append(c)
    c = MergeCase("gap_sentinels", "gap")
    c.add([5000, 5001, TOP], _fill(1000, 0, 1), "gap", "ab")              # S entirely beyond L's last value
    c.add([0, 7, 7, SENT], rep(SENT, 200), "gap", "ab")                   # L all sentinels: nle == 0
    c.add([3, 3, 600, SENT, SENT], srt(_fill(500, 0, 1), rep(SENT, 20)), "gap", "ab")
    c.add([], rep(SENT, 5), "gap", "ab")
    out.append(c)
    return out


def _diff_small():
    out = []
    c = MergeCase("diff_sizes", "diff_small")
    kinds = {(1, 1): "tile", (4095, 100000): "tile", (4096, 100000): "tile"}  # the other nine: nl >= 32 ns
    for na in (0, 1, 4095, 4096):
        for nb in (0, 1, 100000):
            a = _fill(na, 0, 3) if na != 1 else u32([TOP])
            b = _fill(nb, 0, 2) if nb != 1 else u32([TOP])
            c.add(a, b, kinds.get((na, nb), "gap"), "ab" if nb <= 4096 else "a")
    out.append(c)
    # 4096 equal values in a against a run of that value at the very end of b: q == nb
    c = MergeCase("diff_4096_equal_tail", "diff_small", {"tail": (0, 1, 4095, 4096, 4097)})
    for r in (0, 1, 4095, 4096, 4097):
        c.add(rep(50000, 4096), srt(_fill(5000, 0, 2), rep(50000, r)), "tile", "a")
    out.append(c)
    # a thread's four elements straddling value runs
    c = MergeCase("diff_straddle", "diff_small")
    vals = 10 * np.arange(900, dtype=np.int64)
    a = np.repeat(vals, np.arange(900) % 7 + 1)          # runs of 1..7: 3600 values
    b = np.repeat(vals, np.arange(900) % 5)              # counts 0..4
    c.add(a, b, "tile", "ab")
    c.add(srt(a[:3000], [TOP, TOP, TOP]), srt(b, [TOP, TOP]), "tile", "ab")
    out.append(c)
    c = MergeCase("diff_sentinels", "diff_small")
    c.add(srt(_fill(50, 0, 2), rep(SENT, 3)), srt(_fill(70, 0, 3), rep(SENT, 2)), "tile", "ab")
    c.add(srt(_fill(50, 0, 2), rep(SENT, 3)), _fill(70, 0, 3), "tile", "ab")
    c.add(rep(SENT, 4096), rep(SENT, 4096), "tile", "ab")
    out.append(c)
    return out


def _rand_sorted(rng, n, hi):
    return np.sort(rng.integers(0, hi, size=n, dtype=np.uint64)).astype(np.uint32)


def _generic():
    out = []
    rng = np.random.default_rng(20260)
    # cumulative a and b offsets on multiples of 256 and 4096, and one either side of them
    A = [255, 256, 257, 511, 512, 513, 4095, 4096, 4097, 8191, 8192, 8193, 8193, 8193, 12287, 12288, 12289, 16386,
         20479, 20480, 20481, 20735, 20736, 20737, 24575, 24576, 24577, 24577, 28671, 28672, 28673, 32767, 32768,
         32769, 33023, 33024, 33025, 36863, 36864, 36865, 40962]
    B = [1, 255, 256, 257, 257, 4095, 4096, 4097, 4351, 4352, 4353, 8191, 8192, 8193, 8193, 12290, 12543, 12544,
         12545, 16383, 16384, 16385, 16385, 16385, 20479, 20480, 20481, 24575, 24576, 24577, 24831, 24832, 24833,
         28671, 28672, 28673, 28673, 32767, 32768, 32769, 36866]
    c = MergeCase("gen_offsets", "generic", {"a_off": A, "b_off": B})
    pa = pb = 0
    for k, (ea, eb) in enumerate(zip(A, B)):
        na, nb = ea - pa, eb - pb
        hi = (8, 300, 1 << 20, 1 << 32)[k % 4]
        kind = "big" if min(na, nb) > KMS else ("gap" if max(na, nb) >= 32 * min(na, nb) else "tile")
        c.add(_rand_sorted(rng, na, hi), _rand_sorted(rng, nb, hi), kind,
              ("a" if na <= KMS else "") + ("b" if nb <= KMS else ""))
        pa, pb = ea, eb
    out.append(c)
    # empty sides and fully empty pairs at the start, in the middle (consecutive) and at the end
    c = MergeCase("gen_empties", "generic")
    e, x, y = u32([]), _fill(700, 0, 3), _fill(900, 0, 2)
    for a, b in ((e, e), (e, y), (x, e), (x, y), (e, e), (e, e), (e, x), (e, y), (y, e), (x, e)):
        c.add(a, b, "gap" if min(a.size, b.size) == 0 else "tile", "ab")
    c.add(_fill(4097, 0, 3), _fill(4097, 1, 2), "big", "")
    for a, b in ((x, x), (e, e), (y, e), (e, x), (e, e)):
        c.add(a, b, "gap" if min(a.size, b.size) == 0 else "tile", "ab")
    out.append(c)
    # the total length a multiple of 4096, and one more than that
    for nm, extra in (("gen_total_m0", 0), ("gen_total_m1", 1)):
        c = MergeCase(nm, "generic", {"total_mod": extra})
        c.add(srt(_fill(4097, 0, 3), rep(SENT, 2)), srt(_fill(4100, 1, 2), [SENT]), "big", "")
        c.add(_fill(1000, 0, 2), _fill(1003, 0, 3), "tile", "ab")
        c.add(srt(_fill(3092 + extra, 5, 2), [TOP]), srt(_fill(3087 + extra, 5, 3), [TOP]), "tile", "ab")
        out.append(c)                                   # a: 4099 + 1000 + 3093 = 8192; b: 4101 + 1003 + 3088 = 8192
    # a run of 5,000 equal values crossing chunks against counts 0, 4999, 5000 and 5001 in the other list
    c = MergeCase("gen_run5000", "generic", {"run": 5000})
    a = srt(_fill(100, 0, 7), rep(1234, 5000), _fill(50, 2000, 3))
    for cnt in (0, 4999, 5000, 5001):
        c.add(a, srt(_fill(90, 0, 14), rep(1234, cnt), [TOP]), "big" if cnt else "gap", "" if cnt else "b")
    out.append(c)
    # a shared b range, overlapping a ranges and the ranges out of order
    c = MergeCase("gen_shared", "generic")
    abuf = srt(_rand_sorted(rng, 11990, 3000), rep(SENT, 10))
    bbuf = srt(_rand_sorted(rng, 6000, 3000))
    ab, al = [5000, 0, 3000, 7000, 100], [5000, 4097, 4000, 5000, 0]
    bb, bl = [0, 0, 0, 1000, 5999], [6000, 6000, 6000, 4097, 1]
    for k in range(5):
        a, b = abuf[ab[k]:ab[k] + al[k]], bbuf[bb[k]:bb[k] + bl[k]]
        kind = "big" if min(al[k], bl[k]) > KMS else ("gap" if max(al[k], bl[k]) >= 32 * min(al[k], bl[k]) else "tile")
        c.add(a, b, kind, ("a" if al[k] <= KMS else "") + ("b" if bl[k] <= KMS else ""))
    c.layout = (abuf, np.array(ab, np.uint64), np.array(al, np.uint64), bbuf, np.array(bb, np.uint64),
                np.array(bl, np.uint64))
    out.append(c)
    # 3,000 pairs of 0 to 3 values beside one 4097 / 4097 pair
    c = MergeCase("gen_3000_tiny", "generic", {"npair": 3001})
    for k in range(3000):
        na, nb = k % 4, (k // 4) % 4
        a, b = _rand_sorted(rng, na, 6), _rand_sorted(rng, nb, 6)
        if k % 50 == 0 and na:
            a = srt(a[:-1], [SENT])
        if k == 1500:
            c.add(_fill(4097, 0, 3), srt(_fill(4096, 1, 2), [TOP]), "big", "")
        c.add(a, b, "gap" if min(na, nb) == 0 else "tile", "ab")
    out.append(c)
    return out


_merge_cases = None


def merge_cases():
    global _merge_cases
    if _merge_cases is None:
        base = _routing() + _tile() + _gap() + _diff_small() + _generic()
        _merge_cases = [x for c in base for x in (c, c.swapped())]
    return _merge_cases


# ---- HasDifference -----------------------------------------------------------------
class HdCase:
    """name; pairs [(a, b)]; expect [bool]; at [index in a of the sole element
    that b lacks, or None] per pair; single: also run through the one-pair call"""

    def __init__(self, name, pairs, at, single):
        self.name, self.single = name, single
        self.pairs = [(u32(a), u32(b)) for a, b in pairs]
        self.at = list(at)
        self.expect = [x is not None for x in at]

    def __repr__(self):
        return self.name


def _without(a, i, repl):
    """b: a with a[i] replaced by a value a lacks (sorted again)"""
    b = a.astype(np.int64)
    b[i] = repl
    return u32(np.sort(b))


_hd_cases = None


def hd_cases():
    global _hd_cases
    if _hd_cases is None:
        n = HD_GRID + 1                                   # the grid-stride loop's second round: one element
        a = _fill(n, 2, 2)                                # evens from 2; a[-1] = 2n
        a[-1] = TOP
        small = _fill(1000, 2, 2)
        out = [
            HdCase("hd_single_last", [(a, _without(a, n - 1, 1))], [n - 1], True),
            HdCase("hd_single_first", [(a, _without(a, 0, 1))], [0], True),
            HdCase("hd_single_equal", [(a, a)], [None], True),
            HdCase("hd_batch_positions",
                   [(small, _without(small, i, 1)) for i in (0, 255, 256, 999)] + [(small, small)],
                   [0, 255, 256, 999, None], True),
            HdCase("hd_batch_one_differs",
                   [(small, small)] * 3 + [([], small), (srt(small, [TOP]), srt(small, [SENT]))] + [(small, small)] * 2
                   + [([], [])],
                   [None] * 4 + [1000] + [None] * 3, False),
        ]
        _hd_cases = out
    return _hd_cases


# ---- Canonicalize, the big path -------------------------------------------------------
class CanonCase:
    """name; segs [unsorted uint32 arrays]; claim (wave, block, big, passes);
    notes"""

    def __init__(self, name, segs, claim, notes=None):
        self.name = name
        self.segs = [u32(s) for s in segs]
        lens = [s.size for s in self.segs]
        self.off = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
        self.vals = np.concatenate(self.segs) if sum(lens) else u32([])
        self.vals.setflags(write=False)
        self.claim = claim
        self.notes = notes or {}

    def __repr__(self):
        return self.name


CANON_M = (1, 2, 3, 4, 5, 7, 8)
CANON_D = (-1, 0, 1)

_canon_cases = None


def canon_cases():
    global _canon_cases
    if _canon_cases is None:
        rng = np.random.default_rng(4096)
        uni = u32([0, 7, 1 << 20, TOP, SENT])             # a universe of 5: equal keys on every run boundary
        lens = [TILE * m + d for m in CANON_M for d in CANON_D]
        order = rng.permutation(len(lens))
        tiny = (3, 0, 1, 0, 0, 37, 5, 0, 65, 1, 7, 0, 129, 11, 1, 0, 3, 5, 9, 2, 1)
        segs = []
        for q, i in enumerate(order):
            segs.append(uni[rng.integers(0, 5, size=tiny[q])])
            segs.append(uni[rng.integers(0, 5, size=lens[i])])
        segs.append(u32([]))
        # 19 segments above 4096 (4095 and 4096 are not), the longest 32769: 4 passes
        mixed = CanonCase("canon_runs_mixed", segs, (0, 0, 19, 4), {"lens": sorted(lens)})
        full = rng.integers(0, 1 << 32, size=20000, dtype=np.uint64)
        full[:4] = [0, TOP, SENT, SENT]
        _canon_cases = [
            mixed,
            CanonCase("canon_8193_sentinels", [rep(SENT, 8193)], (0, 0, 1, 2)),
            CanonCase("canon_one_value", [rep(TOP, 12289), [5, 5], rep(0, 4097)], (0, 0, 2, 2)),
            CanonCase("canon_full_range", [[9, 1], full, rep(SENT, 3)], (0, 0, 1, 3)),
            # the one-pass path beside them, at its own list sizes
            CanonCase("canon_small_lists", [rng.integers(0, 50, size=n) for n in (0, 1, 1024, 1025, 4096, 64, 0, 4095)],
                      (3, 3, 0, 0)),
        ]
    return _canon_cases


def canon_expected(seg):
    """pkg/cover/cover.go:28-40 in plain numpy: (the whole slice after the
    in-place loop, the canonical length)"""
    s = np.sort(u32(seg))
    prev = np.concatenate([[SENT], s[:-1]]).astype(np.uint32)
    kept = s[s != prev]
    out = s.copy()
    out[:kept.size] = kept
    return out, int(kept.size)
