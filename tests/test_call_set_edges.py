"""The CallSet scan (sg_call_set.hip, over the walk of sg_linewalk.h) at the edges of its walk: tiles dense
enough for the 64-lines-a-store groups, every byte class on both sides of a tile boundary, lines longer than a
tile, a batch of more tiles than waves, the wide tiles the device form takes for overlapping programs, and the
long-line limit at the places of a 64-byte step.

tests/call_set_cases.py builds each family and restates the few constants a case sits on.  The CPU tests below
assert on each case the property it relies on (lines per tile, positions met, tile totals and a wave's share,
the shift taken), so a case that drifts off its edge fails without a GPU.  The GPU tests compare status,
line_off, name_pos, name_len and name_id with the oracle (tests/hub_state_oracle.py), element by element; no
tolerance anywhere."""
import os
import re

import numpy as np
import pytest

from tests import call_set_cases as S
from tests import hub_state_cases as K
from tests import hub_state_checks as C
from tests import hub_state_oracle as OR
from tests.conftest import ROOT

U64 = np.uint64
UNK = C.UNK
_memo = {}


def memo(fn):
    """a family's cases, built once and shared by its CPU and GPU tests"""
    if fn.__name__ not in _memo:
        _memo[fn.__name__] = fn()
    return _memo[fn.__name__]


def _names_of(progs, k, lo, pos, ln):
    view, base = progs[k], sum(len(p) for p in progs[:k])
    return [view[p - base:p - base + n] for p, n in zip(pos[lo[k]:lo[k + 1]].tolist(), ln[lo[k]:lo[k + 1]].tolist())]


# ---- CPU: the restatement and what each family relies on -------------------------------------
def test_restated_constants_are_the_kernel_file_s():
    src = open(os.path.join(ROOT, "syzkaller_amd", "csrc", "sg_call_set.hip")).read()
    assert re.search(r"kCsTileLog = (\d+);", src).group(1) == str(S.TILE.bit_length() - 1)
    assert "kCsMaxWaves = 1u << %d;" % (S.MAX_WAVES.bit_length() - 1) in src
    assert "return nbytes / kCsTile + 1 + nprogs;" in src                       # tile_bound
    assert "std::min<uint64_t>((pl.bound + 3) & ~3ull, kCsMaxWaves)" in src      # nwaves
    assert "(total + a.nwaves - 1) / a.nwaves" in src                            # per
    walk = open(os.path.join(ROOT, "syzkaller_amd", "csrc", "sg_linewalk.h")).read()   # the store group is the walk's
    assert "sgd::LineGroup<CsName> calls;" in src and "kLineGroup = %d;" % S.GROUP in walk
    assert "(n & (kLineGroup - 1)) == kLineGroup - 1" in walk and S.GROUP == 64
    assert "while (k + 1 < kCsShifts && sums[k] + nprogs > bound) k++;" in src   # pick_shift
    assert S.MAX_LINE == OR.MAX_LINE
    # the helper: call lines by the tile they start in, a name behind `rN = ` counted where its line starts
    assert S.tile_profile([b"a()\n" + b"#" * 251 + b"\nr0 = b()\nc()", b"", b"x", b"#" * 300]) == [[1, 2], [], [0], [0, 0]]
    assert S.tile_profile([b"#" * 251 + b"\nr0 = b()\n"]) == [[1, 0]] and S.tile_profile([b"a()\n" * 3], 8) == [[2, 1]]
    assert S.pick_shift([256, 0, 255], 511) == 0 and S.pick_shift([512] * 4, 512) == 1 and S.pick_shift([1 << 20] * 9, 1 << 20) == 4


def test_dense_conditions():
    cases = memo(S.dense_progs)
    prof = S.tile_profile([t for t, _, _ in cases])
    for (text, tile, n), pr in zip(cases, prof):
        assert OR.call_lines(text)[0] == 0 and pr[tile] == n, (tile, n)
    assert sorted(n for _, tile, n in cases[:-1] if tile == 0) == sorted(n for _, tile, n in cases[:-1] if tile == 1) == list(S.DENSE_COUNTS)
    assert {pr[0] for pr in prof} >= set(S.DENSE_COUNTS) and {pr[1] for pr in prof if len(pr) > 1} >= set(S.DENSE_COUNTS)
    row = prof[-1]
    assert len(row) == 12 and all(x >= S.GROUP for x in row[:11]) and set(row[:11]) == {85, 86}
    assert S.TILE // 3 + 1 == 86 == max(max(pr) for pr in prof)     # no tile of three-byte lines holds more
    progs, at = memo(S.dense_batch)
    assert [progs[i] for i in at] == [t for t, _, _ in cases]
    assert any(progs[i - 1] == b"" for i in at) and any(0 < len(progs[i + 1]) < 200 for i in at[:-1])
    names = OR.call_sets(progs)[4]
    tab = set(S.TABLE_LETTERS)
    assert any(x in tab for x in names) and any(x not in tab for x in names)


def test_boundary_conditions():
    for offsets, window in zip(S.BOUNDARY_OFFSETS, S.BOUNDARY_WINDOWS):
        progs, marks = K.offset_batch(offsets)
        assert sorted({(a, o) for _, a, o, _ in marks}) == [(a, o) for a in range(4) for o in offsets]
        starts = np.concatenate([[0], np.cumsum([len(p) for p in progs])])
        seen = {c: set() for c in b"s=(\n"}
        for i, a, o, name in marks:
            line = b"r%d = " % (o % 10) + name + b"("
            assert starts[i] % 4 == a and progs[i][o:o + len(line)] == line and progs[i][o - 1] == 10
            assert OR.call_lines(progs[i]) == (0, [(o + 5, len(name)), (o + len(line) + 5, 1)])
            seen[ord("s")].add((a, o))
            for c in b"=(\n":
                seen[c].add((a, progs[i].index(bytes([c]), o)))
        for c, got in seen.items():   # the line start and each class on every place of the window, at every misalignment
            assert got >= {(a, x) for a in range(4) for x in window}, chr(c)
    cases = memo(S.length_progs)
    assert {len(t) for t, _, _ in cases} == set(S.PROGRAM_LENGTHS)
    for text, status, note in cases:
        assert OR.call_lines(text)[0] == status, note
    last = {(len(t), t[S.TILE * ((len(t) - 1) // S.TILE):]) for t, _, _ in cases}
    for n in (257, 513):
        assert {(n, b"x"), (n, b"\n"), (n, b"\r"), (n, b"(")} <= last
    assert all(any(len(t) == n and t.endswith(b"()\n") for t, _, _ in cases) for n in S.PROGRAM_LENGTHS)


def test_span_conditions():
    cases = memo(S.span_progs)
    met = set()
    for text, status, names, (o, length, paren, eq, cr) in cases:
        st, lines = OR.call_lines(text)
        assert st == status and [text[p:p + n] for p, n in lines] == names, (o, length, paren, eq, cr)
        end = text.index(b"\n", o)
        assert (o == 0 or text[o - 1] == 10) and end - o == length and text[:o].count(b"(") == 0
        b = text.find(b"(", o, end)
        nxt = (o // S.TILE + 1) * S.TILE
        assert b == {"near": o + 9, "last": nxt - 1, "next": nxt, "two_on": nxt + S.TILE + 7, "absent": -1}[paren]
        q = text.find(b"=", o, end)
        if eq == "other_side" and paren != "absent":
            assert q >= 0 and (q < nxt) != (b < nxt)            # the '=' and the '(' on different sides
        if cr:
            assert text[end - 1] == 13 and end % S.TILE == 0    # the '\r' is a tile's last byte
        if not cr:
            met.add((o, length, paren))
    assert {o for o, _, _ in met} == set(S.SPAN_STARTS) and {n for _, n, _ in met} == set(S.SPAN_LENGTHS)
    for paren in S.PAREN_PLACES:   # every place with every start; "two_on" only where the line is long enough
        assert {o for o, _, p in met if p == paren} == set(S.SPAN_STARTS), paren
    assert {0, 1, 2} == {st for _, st, _, _ in cases}
    assert any(eq == "other_side" and 0 <= t.find(b"(", m[0]) < t.find(b"=", m[0]) for t, _, _, m in cases for eq in [m[3]])
    assert any(cr for _, _, _, (_, _, _, _, cr) in cases)
    assert any(b"\n" not in t[k:k + S.TILE] for t, _, _, _ in cases for k in range(0, len(t) - S.TILE + 1, S.TILE))
    # two failing lines in tiles two apart: the first by position decides
    (a, sa), (b, sb) = S.failure_order_progs()
    for text, status, first, second in ((a, sa, b"r1 = (x", b"no bracket"), (b, sb, b"no bracket", b"r1 = (x")):
        assert OR.call_lines(text)[0] == status == (2 if first.startswith(b"r1") else 1)
        assert text.index(first) // S.TILE == 1 and text.index(second) // S.TILE == 3
        assert OR.call_lines(text.replace(first, b"#" * len(first)))[0] == 3 - status   # the other one alone


def test_wide_conditions():
    progs = memo(S.wide_batch)
    lengths = [len(p) for p in progs]
    tile_off, per, nw = S.shares(lengths)
    total = int(tile_off[-1])
    assert len(progs) == S.WIDE_PROGRAMS == 70000 and nw == S.MAX_WAVES and total > S.MAX_WAVES and per == 2
    assert total <= S.tile_bound(len(progs), sum(lengths))
    first = np.arange(0, total, per)                              # the first tile of each wave's share
    owner = np.searchsorted(tile_off, first, side="right") - 1    # its program
    assert (first > tile_off[owner]).any()                        # a share that starts inside a program
    last = np.minimum(first + per, total) - 1
    jump = np.searchsorted(tile_off, last, side="right") - 1 - owner
    assert jump.max() > 300 and (jump == 2).any()                 # shares that hold a run of empty programs
    runs = re.findall(r"0+", "".join("1" if x else "0" for x in lengths))
    assert {len(r) for r in runs} >= set(S.EMPTY_RUNS)
    st = OR.call_sets(progs)[0]
    assert {0, 1, 2, 4} <= set(st.tolist()) and (st[7::97] != 0).all()
    # a failing program and a valid one inside one share, in both orders
    a, b = owner, np.searchsorted(tile_off, last, side="right") - 1
    assert ((st[a] != 0) & (st[b] == 0)).any() and ((st[a] == 0) & (st[b] != 0)).any()
    ntile = np.diff(tile_off)
    assert (ntile == 2).sum() >= 5 and (ntile == 3).sum() >= 5 and (ntile == 12).sum() == 1
    for text, _ in S.failure_order_progs():
        assert text in progs


def test_high_shift_conditions():
    text, offs, line_starts = memo(S.high_shift_case)
    nbytes = len(text)
    ranges = C.clamp_ranges(offs, nbytes)
    live = [(a0, a1) for a0, a1 in ranges if a1 > a0]
    assert nbytes == S.HIGH_SHIFT_BYTES and len(live) == S.HIGH_SHIFT_STARTS and all(a1 == nbytes for _, a1 in live)
    assert len(ranges) == 2 * len(live) - 1 and len({a0 for a0, _ in live}) == len(live)
    at_line = [a0 in set(line_starts.tolist()) for a0, _ in live]
    assert at_line.count(True) >= 100 and at_line.count(False) >= 100
    k = S.pick_shift([a1 - a0 for a0, a1 in ranges], nbytes)
    assert k == 5
    assert sum(S.ntiles(a1 - a0) for a0, a1 in ranges) > S.tile_bound(len(ranges), nbytes)   # shift 0 does not fit
    assert any(S.ntiles(a1 - a0, S.TILE << k) == 2 for a0, a1 in live)
    prof = S.tile_profile([text[a0:a1] for a0, a1 in live], S.TILE << k)
    assert max(max(pr) for pr in prof) >= 2 * S.GROUP + 1        # two full store groups and a tail
    st = [OR.call_lines(text[a0:a1])[0] for a0, a1 in live]
    assert st.count(0) >= 200 and {1, 2} <= set(st)


def test_long_step_conditions():
    cases = memo(S.long_step_cases)
    assert sum(len(t) for t, _, _ in cases) < 7 << 20
    seen = set()
    for text, status, names in cases:
        st, lines = OR.call_lines(text)
        assert st == status and [text[p:p + n] for p, n in lines] == names
        o = text.index(b"r0 = big(")
        end = text.find(b"\n", o)
        length = (len(text) if end < 0 else end) - o
        assert (o == 0 or text[o - 1] == 10) and length == (S.MAX_LINE - 1 if status == 0 else S.MAX_LINE)
        seen.add((o, status, end < 0))
    assert seen == {(o, s, e) for o in S.LONG_STARTS for s in (0, 3) for e in (False, True)}
    assert {o % S.STEP for o in S.LONG_STARTS} == {0, 1, 62, 63} and 255 in S.LONG_STARTS


# ---- GPU -------------------------------------------------------------------------------
@pytest.fixture
def letters(ctx):
    from syzkaller_amd import hub as H

    table = H.NameTable(ctx)
    table.add(S.TABLE_LETTERS + K.NAMES)
    yield table, {x: i for i, x in enumerate(S.TABLE_LETTERS + K.NAMES)}
    table.close()


@pytest.mark.gpu
def test_dense_tiles(ctx, letters):
    table, otab = letters
    progs, at = memo(S.dense_batch)
    st, lo, pos, ln, ids = C.check_sets(ctx, progs, table, otab)
    for i, (_, _, n) in zip(at, memo(S.dense_progs)):
        assert st[i] == 0 and lo[i + 1] - lo[i] >= n
    assert (ids != UNK).any() and (ids == UNK).any()
    for text, _, _ in memo(S.dense_progs):     # and each alone: its tiles are the batch's first
        C.check_sets(ctx, [text], table, otab)
        C.check_sets(ctx, [b"", text, b""], table, otab)


@pytest.mark.gpu
@pytest.mark.parametrize("which", (0, 1), ids=("tile1", "tile2"))
def test_every_offset_about_a_tile_boundary(ctx, which):
    progs, marks = K.offset_batch(S.BOUNDARY_OFFSETS[which])
    st, lo, pos, ln, _ = C.check_sets(ctx, progs)
    view = b"".join(progs)
    for i, a, o, name in marks:
        assert st[i] == 0 and lo[i + 1] - lo[i] == 2, (a, o)
        p, n = int(pos[lo[i]]), int(ln[lo[i]])
        assert view[p:p + n] == name, (a, o)


@pytest.mark.gpu
def test_program_lengths_about_a_tile(ctx, letters):
    table, otab = letters
    cases = memo(S.length_progs)
    st = C.check_sets(ctx, [t for t, _, _ in cases], table, otab)[0]
    assert st.tolist() == [s for _, s, _ in cases]
    for text, status, note in cases:
        assert C.check_sets(ctx, [text])[0].tolist() == [status], note


@pytest.mark.gpu
def test_lines_that_span_tiles(ctx):
    cases = memo(S.span_progs)
    progs = [t for t, _, _, _ in cases]
    st, lo, pos, ln, _ = C.check_sets(ctx, progs)
    assert st.tolist() == [s for _, s, _, _ in cases]
    view = b"".join(progs)
    names = [view[p:p + n] for p, n in zip(pos.tolist(), ln.tolist())]
    assert names == [x for _, _, ns, _ in cases for x in ns]
    for text, status, _, what in cases:        # and each alone
        assert C.check_sets(ctx, [text])[0].tolist() == [status], what


@pytest.mark.gpu
def test_failing_lines_in_different_tiles(ctx):
    cases = S.failure_order_progs()
    for text, status in cases:
        assert C.check_sets(ctx, [text])[0].tolist() == [status]
    assert C.check_sets(ctx, [t for t, _ in cases] * 2)[0].tolist() == [s for _, s in cases] * 2


@pytest.mark.gpu
def test_more_tiles_than_waves(ctx, letters):
    table, otab = letters
    progs = memo(S.wide_batch)
    st, lo, pos, ln, ids = C.check_sets(ctx, progs, table, otab)
    for text, status in S.failure_order_progs():
        assert st[progs.index(text)] == status
    assert (ids != UNK).sum() > 60000


@pytest.mark.gpu
def test_more_tiles_than_waves_through_hubcorpus_add(ctx):
    from syzkaller_amd import hub as H

    progs = memo(S.wide_batch)
    t = H.NameTable(ctx)
    c, o = H.HubCorpus(t), OR.OHubCorpus(OR.ONameTable())
    got, exp = c.add(progs, 3), o.add(progs, 3)
    for g, e in zip(got, exp):
        assert np.array_equal(g, e)
    C.same_corpus(c, o)
    assert len(t) == len(o.table.ids) and all(t.id(x) == i for x, i in o.table.ids.items())
    assert c.count() > 60000
    c.close()
    t.close()


@pytest.mark.gpu
def test_device_form_at_a_high_shift(ctx, letters):
    table, otab = letters
    text, offs, _ = memo(S.high_shift_case)
    nbytes, n = len(text), offs.size - 1
    exp = C.dev_expect(text, C.clamp_ranges(offs, nbytes), otab)
    total = exp[1][-1]
    assert total > int(text.count(b"("))
    d_b = C.to_dev(np.frombuffer(text, np.uint8))
    got = C.dev_run(ctx, table, d_b.data_ptr(), nbytes, offs, n, total)
    for g, e, what in zip(got, exp, ("status", "line_off", "name_pos", "name_len", "name_id")):
        assert g == e, what
    # a cap one too small: the statuses and the offsets, nothing else (dev_run checks the untouched bytes)
    got = C.dev_run(ctx, table, d_b.data_ptr(), nbytes, offs, n, total - 1)
    assert got[:2] == exp[:2] and got[2:] == ([], [], [])


@pytest.mark.gpu
def test_long_line_limit_at_step_positions(ctx):
    cases = memo(S.long_step_cases)
    progs = [t for t, _, _ in cases]
    st, lo, pos, ln, _ = C.check_sets(ctx, progs)
    assert st.tolist() == [s for _, s, _ in cases]
    for k, (_, _, names) in enumerate(cases):
        assert _names_of(progs, k, lo, pos, ln) == names, k
