"""pkg/report on the GPU (csrc/sg_crash_report.hip, syzkaller_amd/report.py): sg_crash_scan, sg_crash_parse and
sg_console_output against tests/crash_report_oracle.py, a sequential restatement of report.go.

CPU: the oracle against hand-derived results, the parallel reading (the one the kernels follow) against the oracle
on random fragment sequences, and the entry points' argument checks.  GPU: every output of every call, byte for byte
and element for element, on logs cut to the kernels' tile (SG_CRASH_TILE) and halo (SG_CRASH_MAX_LITERAL)."""
import ctypes
import os
import random
import re

import numpy as np
import pytest

from tests import crash_report_cases as K
from tests import crash_report_oracle as OR
from tests.conftest import ROOT

U8, U32, U64, I32 = np.uint8, np.uint32, np.uint64, np.int32
P = K.P


def _define(name):
    head = open(os.path.join(ROOT, "include", "syzsig.h")).read()
    return int(re.search(r"^#define %s (\d+)$" % name, head, flags=re.M).group(1))


T = _define("SG_CRASH_TILE")
MAXLIT = _define("SG_CRASH_MAX_LITERAL")


# ---- CPU ---------------------------------------------------------------------------------------------------------
def test_header_states_the_table():
    assert _define("SG_CRASH_OOPSES") == len(OR.HEADERS) == 13
    lits = OR.HEADERS + [OR.MODULI, OR.TAINT, OR.PANIC, OR.NMI_A, OR.NMI_B, OR.EOI, b"Boot_DEBUG:", b"_INFO::",
                         b"INFO: lockdep is turned off", b"INFO: Stall ended before state dump start"]
    assert max(len(x) for x in lits) == len(OR.MODULI) == MAXLIT
    assert T % 256 == 0 and T > 2 * MAXLIT


def test_oracle_against_hand_derived_results():
    for name, log, desc, oops, start, end, text in K.hand_cases():
        o, s, e, dp, dl, t = OR.parse_bounds(log)
        assert (o, s, e, log[dp:dp + dl], t) == (oops, start, end, desc, text), name
        assert OR.contains_crash(log) == (oops != -1), name
    # the window of five, the cut at rank 41 and the taint lines, counted by hand
    pre = b"".join(K.con(b"p%d" % i) for i in range(7))
    body = [b"BUG: first"] + [b"l%d" % i for i in range(2, 41)] + [OR.PANIC + b": x", b"after"]
    body[5] = OR.TAINT
    log = pre + b"".join(K.con(b) for b in body)
    o, s, e, dp, dl, t = OR.parse_bounds(log)
    want = [b"p%d" % i for i in range(2, 7)] + [b for b in body[:40] if b != OR.TAINT]
    assert (o, s, t) == (0, len(pre), b"".join(w + b"\n" for w in want))
    assert e == len(log) - len(K.con(b"after")) - 1            # the panic line is a record line too
    log = pre + b"".join(K.con(b) for b in body[:39] + body[40:])  # the panic line at rank 40 stays
    assert OR.parse_bounds(log)[5].endswith(OR.PANIC + b": x\nafter\n")
    assert OR.console_output(b"x\n" + K.con(b"a\r", end=b"\n") + b"[ 1.] b\n" + K.con(b" ? f+0x1/0x2")) == b"a\n"
    assert OR.parse_bounds(b"BUG: x\n" + K.con(b"y"), ignores=[re.compile(rb"BUG: x")])[0] == -1


def test_parallel_reading_equals_the_oracle():
    logs = K.random_logs(7, 2500)
    rng = random.Random(8)
    nrec = ntext = ncut = 0
    for log in logs:
        want = OR.parse_bounds(log)
        assert OR.model_parse(log) == want, log
        assert OR.model_scan(log) == OR.scan(log), log
        assert OR.model_console(log) == OR.console_output(log), log
        ign = K.random_ignored(rng, log)
        assert OR.model_parse(log, ign) == OR.parse_bounds(log, ignored=ign), (log, ign)
        nrec += want[0] != -1
        ntext += bool(want[5])
        ncut += want[5].count(b"\n") >= 40
    assert nrec > 1000 and ntext > 500 and ncut > 50           # the generator reaches what it is for


def test_host_description_steps():
    from syzkaller_amd import report as R

    d = R.finish_description(b"BUG: unable to handle kernel paging request at ffff880012345678 in syz-executor3:1234\r")
    assert d == b"BUG: unable to handle kernel paging request at ADDR in syz-executor"
    assert R.finish_description(b"WARNING in foo+0x12/0x340 at a.c:12:3 CPU#3 123456") == b"WARNING in foo at a.c:LINE CPU NUM"
    assert len(R.finish_description(b"x" * 500)) == 180
    log = b"BUG: KASAN: use-after-free in ip6_send+0x1/0x2\nRead of size 8 by task a\n"
    assert R.extract_description(log, 0, b"fallback") == b"KASAN: use-after-free Read in ip6_send"
    assert R.extract_description(b"BUG: other\n", 0, b"BUG: other") == b"BUG: other"
    assert R.extract_description(b"x Kernel panic - not syncing: Fatal y\n", 5, b"") == b"kernel panic: Fatal y"


def test_argument_checks_come_before_the_context():
    """The handle is a block of zeros: SG_EINVAL comes before it is touched, and a well-formed call reaches the
    device check, which fails here without a device."""
    from syzkaller_amd import _lib
    from syzkaller_amd._lib import SG_EINVAL as E
    from syzkaller_amd._lib import lib

    blk = np.zeros(1 << 13, U64)
    fake = blk.ctypes.data_as(ctypes.c_void_p)
    p8, p64, p32 = (lambda a: a.ctypes.data_as(_lib.P8)), (lambda a: a.ctypes.data_as(_lib.P64)), (lambda a: a.ctypes.data_as(_lib.P32))
    text = np.frombuffer(b"BUG: x\n[1.2] y\n", U8).copy()
    off = np.array([0, 7, text.size], U64)
    bad_off, bad_first = np.array([0, 9, 7], U64), np.array([1, 7, text.size], U64)
    a8, a32, a64, i32 = np.zeros(64, U8), np.zeros(64, U32), np.zeros(64, U64), np.zeros(64, I32)
    n = ctypes.c_size_t(77)
    ref = ctypes.byref

    def bad(fn, a, i, v):
        b = list(a)
        b[i] = v
        assert getattr(lib, fn)(*b) == E, (fn, i)
        assert lib.sg_last_error()

    scan = [fake, p8(text), p64(off), 2, p8(a8), p32(a32), p64(a64), p64(a64), p32(a32), p64(a64), 4, ref(n), None]
    for i in (0, 1, 2, 4, 5, 6, 7, 8, 9, 11):
        bad("sg_crash_scan", scan, i, None)
    bad("sg_crash_scan", scan, 2, p64(bad_off))
    bad("sg_crash_scan", scan, 2, p64(bad_first))
    big = np.array([0, 1 << 32], U64)
    bad("sg_crash_scan", scan[:2] + [p64(big), 1] + scan[4:], 0, fake)
    assert b"2^32" in lib.sg_last_error()
    sdev = [fake, fake, fake, 2, text.size] + [fake] * 6 + [4, fake, None]
    for i in (0, 1, 2, 5, 6, 7, 8, 9, 10, 12):
        bad("sg_crash_scan_dev", sdev, i, None)
    bad("sg_crash_scan_dev", sdev, 4, 1 << 32)
    bad("sg_crash_scan_dev", sdev, 3, 1 << 32)
    pi = i32.ctypes.data_as(_lib.PI32)
    ioff, ipos = np.array([0, 1, 1], U64), np.array([0], U64)
    parse = [fake, p8(text), p64(off), 2, p64(ioff), p64(ipos), pi, p64(a64), p64(a64), p64(a64), p64(a64), p64(a64),
             p8(a8), 8, ref(n), None]
    for i in (0, 1, 2, 5, 6, 7, 8, 9, 10, 11, 12, 14):
        bad("sg_crash_parse", parse, i, None)
    bad("sg_crash_parse", parse, 4, p64(np.array([0, 2, 1], U64)))           # no CSR
    bad("sg_crash_parse", parse, 5, p64(np.array([7], U64)))                 # outside its log
    two = parse[:4] + [p64(np.array([0, 2, 2], U64)), p64(np.array([3, 3], U64))] + parse[6:]
    bad("sg_crash_parse", two, 0, fake)                                       # not ascending
    pdev = [fake, fake, fake, 2, text.size, fake, fake, 1] + [fake] * 7 + [8, None]
    for i in (0, 1, 2, 5, 6, 8, 9, 10, 11, 12, 13, 14):
        bad("sg_crash_parse_dev", pdev, i, None)
    bad("sg_crash_parse_dev", pdev, 4, 1 << 32)
    cons = [fake, p8(text), p64(off), 2, p64(a64), p8(a8), 8, ref(n), None]
    for i in (0, 1, 2, 4, 5, 7):
        bad("sg_console_output", cons, i, None)
    cdev = [fake, fake, fake, 2, text.size, fake, fake, 8, None]
    for i in (0, 1, 2, 5, 6):
        bad("sg_console_output_dev", cdev, i, None)
    bad("sg_console_output_dev", cdev, 4, 1 << 32)
    assert n.value == 77 and not a8.any() and not a64.any() and not a32.any()


def _has_gpu():
    try:
        import torch

        return torch.cuda.device_count() > 0
    except Exception:
        return False


@pytest.mark.skipif(_has_gpu(), reason="checks the no-GPU failure path")
def test_well_formed_calls_fail_loudly_without_a_device():
    from syzkaller_amd import _lib
    from syzkaller_amd._lib import SG_ENODEV, lib

    blk = np.zeros(1 << 13, U64)
    fake = blk.ctypes.data_as(ctypes.c_void_p)
    text = np.frombuffer(b"BUG: x\n", U8).copy()
    off = np.array([0, text.size], U64)
    a8, a32, a64, i32 = np.zeros(64, U8), np.zeros(64, U32), np.zeros(64, U64), np.zeros(64, I32)
    p8, p64, p32 = (lambda a: a.ctypes.data_as(_lib.P8)), (lambda a: a.ctypes.data_as(_lib.P64)), (lambda a: a.ctypes.data_as(_lib.P32))
    n = ctypes.c_size_t(77)
    ref = ctypes.byref
    assert lib.sg_crash_scan(fake, p8(text), p64(off), 1, p8(a8), p32(a32), p64(a64), p64(a64), p32(a32), p64(a64), 4,
                             ref(n), None) == SG_ENODEV
    assert lib.sg_crash_parse(fake, p8(text), p64(off), 1, None, None, i32.ctypes.data_as(_lib.PI32), p64(a64), p64(a64),
                              p64(a64), p64(a64), p64(a64), p8(a8), 8, ref(n), None) == SG_ENODEV
    assert lib.sg_console_output(fake, p8(text), p64(off), 1, p64(a64), p8(a8), 8, ref(n), None) == SG_ENODEV
    assert lib.sg_crash_scan_dev(fake, fake, fake, 1, 7, fake, fake, fake, fake, fake, fake, 4, fake, None) == SG_ENODEV
    assert lib.sg_crash_parse_dev(fake, fake, fake, 1, 7, None, None, 0, fake, fake, fake, fake, fake, fake, fake, 8,
                                  None) == SG_ENODEV
    assert lib.sg_console_output_dev(fake, fake, fake, 1, 7, fake, fake, 8, None) == SG_ENODEV
    assert n.value == 77


# ---- GPU ---------------------------------------------------------------------------------------------------------
def _check(ctx, logs, ignored=None):
    """Every output of the three host forms over `logs` against the oracle; returns (records, bounds)."""
    from syzkaller_amd import report as R

    recs = R.crash_scan(logs, ctx)
    want = [(l,) + r for l, log in enumerate(logs) for r in OR.scan(log)]
    got = list(zip(recs.log.tolist(), recs.line_start.tolist(), recs.line_end.tolist(), recs.oops.tolist(),
                   recs.match.tolist()))
    assert got == want
    assert recs.contains.tolist() == [int(OR.contains_crash(log)) for log in logs]
    b = R.parse_bounds_batch(logs, ignored, ctx)
    for l, log in enumerate(logs):
        o, s, e, dp, dl, t = OR.parse_bounds(log, ignored=None if ignored is None else set(ignored[l]))
        assert (int(b.oops[l]), int(b.start[l]), int(b.end[l]), int(b.desc_pos[l]), int(b.desc_len[l])) == (o, s, e, dp, dl), l
        assert b.text(l) == t, l
    assert R.console_output_batch(logs, ctx) == [OR.console_output(log) for log in logs]
    nlines = sum(len(OR.lines(log)) for log in logs)
    assert int(recs.stats[0]) == int(b.stats[0]) == nlines and int(recs.stats[2]) == len(want)
    assert int(b.stats[1]) == sum(OR.is_console(log[p:n]) for log in logs for p, n in OR.lines(log))
    return recs, b


@pytest.mark.gpu
def test_gpu_hand_cases_and_public_interface(ctx):
    from syzkaller_amd import report as R

    cases = K.hand_cases()
    logs = [c[1] for c in cases]
    _check(ctx, logs)
    out = R.parse_batch(logs, ctx=ctx)
    for (name, log, desc, oops, start, end, text), got in zip(cases, out):
        assert got[1:] == (text, start, end), name
        assert (got[0] != b"") == (oops != -1), name
    log = P + b"BUG: KASAN: use-after-free in ip6_send+0x1/0x2\n" + P + b"Read of size 8 by task syz-executor7/123\n"
    assert R.Parse(log, ctx=ctx)[0] == b"KASAN: use-after-free Read in ip6_send"
    assert R.Parse(b"x general protection fault: 0000 [#1] SMP\n", ctx=ctx)[0] == b"general protection fault: 0000 [#1] SMP"
    assert R.ContainsCrash(log, ctx=ctx) and not R.ContainsCrash(b"all quiet\n", ctx=ctx)
    assert R.ExtractConsoleOutput(b"junk\n" + P + b"kept\r\n", ctx=ctx) == b"kept\n"
    assert R.contains_crash_batch([], ctx=ctx) == [] and R.parse_batch([], ctx=ctx) == []
    assert R.console_output_batch([], ctx=ctx) == []


@pytest.mark.gpu
def test_gpu_literals_at_tile_edges(ctx):
    b = K.Batch()
    for h in OR.HEADERS:                                         # every header at every split of its length
        for k in range(1, len(h)):
            b.add_at(T, k, P, h, b" at the edge\n")
    nmi = OR.NMI_A + b"(perf)" + OR.NMI_B
    for k in (1, len(OR.NMI_A), len(OR.NMI_A) + 3, len(nmi) - 1):   # the two halves in different tiles
        b.add_at(T, k, P, nmi, b": 1 msecs\n")
    b.add_at(T, len(OR.NMI_A), P, OR.NMI_A[:-1] + OR.NMI_B, b"\n")  # the second half exactly at the first's end
    b.add(P + OR.NMI_A[:-1] + OR.NMI_B[1:] + b"\n")                 # ... and one byte too early: the blank is shared
    b.add(P + OR.NMI_B + b" " + OR.NMI_A + b"\n")                  # the halves the wrong way round
    b.add(P + OR.NMI_A + OR.NMI_A + OR.NMI_B + b"\n")              # the leftmost first half counts
    for lit in (OR.MODULI, OR.TAINT, OR.PANIC, OR.EOI):
        for k in (1, len(lit) // 2, len(lit) - 1):
            b.add_at(T, k, P + b"BUG: WARNING: ? f+0x1/0x2 ", lit, b"\n")
    for k in (1, 2, 3, 5, 9):                                      # the questionable walk across a tile's end
        b.add_at(T, k, P, b" ? func_name+0x12/0x34", b"\n" + P + b"BUG: here\n")
    recs, _ = _check(ctx, b.logs)
    assert len(recs) >= sum(len(h) - 1 for h in OR.HEADERS)


@pytest.mark.gpu
def test_gpu_log_boundaries(ctx):
    logs = []
    for h in OR.HEADERS[:4]:                                       # split between two logs: matches in neither
        logs += [P + b"x " + h[:2], h[2:] + b" y\n"]
    logs += [b"", b"", P + b"tail Kernel BUG", b"", b"\n", b"no newline at all", b"\n\n", b"BUG: in the last bytes", b""]
    logs += [b"INFO: NMI handler ", b" took too long to run INFO: x\n"]
    _check(ctx, logs)
    for one in ([], [b""], [b"\n"], [b"UBSAN: alone"], [b"", b"", b""]):  # nlogs of 0 and 1, nothing but empty logs
        _check(ctx, one)


@pytest.mark.gpu
def test_gpu_long_lines(ctx):
    logs = [
        P + b"y" * (3 * T - len(P) - 12) + b"kernel BUG x\n" + K.con(b"after"),   # 3 T bytes, the header in the last
        b"z" * 70000 + b"UBSAN: far\n",                                        # nothing caps a line
        P + b"w" * 70000 + b" WARNING: w\r\n" + P + b"body\r\n",
        b"[" + b" " * 5000 + b"1" * 5000 + b"." + b"2" * 5000 + b"] long prefix BUG: x\n",
        P + b" ? " + b"a" * 9000 + b"+0x1/0x2\n" + P + b"BUG: b\n",
        K.con(b"BUG: a\r", end=b"\n") + K.con(b"b", end=b"\r\n") + b"\r\n" + K.con(b"", end=b"\r\n"),
    ]
    _check(ctx, logs)


@pytest.mark.gpu
def test_gpu_records_on_one_line(ctx):
    logs = [
        K.con(b"UBSAN: then WARNING: then BUG: all three"),            # table order, not text order
        K.con(b"x BUG: one BUG: two BUG: three"),                        # the leftmost match
        K.con(b"Boot_DEBUG: WARNING: alive"),                           # a suppressed BUG: beside a live WARNING:
        K.con(b"kernel BUG at x.c:1!"), K.con(b"Kernel BUG: y"), K.con(b"BUG kmalloc-64: z"), K.con(b"kernel BUG: both"),
        K.con(b"INFO: lockdep is turned off BUG: still"), K.con(OR.MODULI + b" INFO: live"),
        b"".join(K.con(h + b" " + g) for h in OR.HEADERS for g in OR.HEADERS[:3]),
    ]
    recs, _ = _check(ctx, logs)
    assert recs.oops[:3].tolist() == [0, 1, 12] and int(recs.match[3]) == len(P) + 2


@pytest.mark.gpu
def test_gpu_console_line_classification(ctx):
    bodies = [b"<6>[    1.000000] ok", b"[1.2] ok", b"[ 1.] no", b"[1.2]x no", b"<>[1.2] no", b"< 6>[1.2] no",
              b"x [1.2] not at the start", b"<12>[  3.4] ok", b"[1.2]", b"[1.2] ", b"[.2] no", b"<6[1.2] no", b"[1 .2] no",
              b"[1.2] a ? f+0x1/0x2", b"[1.2] a ? f+0x1/0x2 <EOI>", b"[1.2] a ? f+0x1/2", b"[1.2] a ?f+0x1/0x2",
              b"[1.2] a ?  f.g_h+0xab/0xcd", b"[1.2] a ? f+0x/0x2", b"[1.2] a ? f+0x1/", b"[1.2] a ? +0x1/0x2",
              b"[1.2] a ? ? f+0x1/0x2", b"[1.2] [<ffffffff81234567>] ? f+0x1/0x2", b"[1.2] a ? F+0X1/0x2",
              b"[1.2] a ? f+0x1/g", b"[1.2] a ? f+0x1g/2", b"[1.2] a ? f+0x1/0x2\r"]
    logs = [b"".join(x + b"\n" for x in bodies), b"BUG: x\n" + b"".join(x + b"\r\n" for x in bodies), bodies[-2]]
    _check(ctx, logs)


def _oops_log(before, l0_console=True, after=3, interleave=False):
    pre = b""
    for i in range(before):
        pre += K.con(b"before %d" % i) + (b"plain %d\n" % i if interleave else b"")
    l0 = (P if l0_console else b"") + b"BUG: the report\n"
    return pre + l0 + b"".join(K.con(b"trace %d" % i) for i in range(after))


@pytest.mark.gpu
def test_gpu_five_line_prefix(ctx):
    logs = [_oops_log(n) for n in (0, 4, 5, 6)] + [_oops_log(6, interleave=True), _oops_log(7, l0_console=False)]
    logs += [_oops_log(3, l0_console=False, after=0),               # no console line at or after L0: no text
             _oops_log(3, l0_console=False, after=0) + b"plain\n[ 1.] no\n",
             K.con(OR.TAINT) * 3 + _oops_log(2),                    # taint lines in the window stay
             _oops_log(2, after=0)[:-1]]
    _, b = _check(ctx, logs)
    assert b.text(6) == b"" and b.oops[6] == 0 and b.text(5).startswith(b"before 2\n")


@pytest.mark.gpu
def test_gpu_the_cut(ctx):
    def log(rank, line, tail=(b"after 1", OR.TAINT, b"after 2")):
        body = [b"BUG: first"] + [b"l%d" % i for i in range(2, rank)] + [line] + list(tail)
        return K.con(b"p") + b"".join(K.con(x) for x in body)

    panic = OR.PANIC + b": panic_on_warn set"
    logs = [log(40, panic), log(41, panic), log(41, OR.TAINT + b" " + panic), log(41, panic, ()), log(60, panic),
            log(41, panic).replace(K.con(b"l7"), K.con(OR.TAINT)),       # a taint line before the cut is a rank
            log(41, panic).replace(K.con(b"l7"), b"l7 no console\n"),   # ... a plain line is not
            log(41, OR.TAINT + b" " + panic) + K.con(panic) + K.con(b"gone")]
    _, b = _check(ctx, logs)
    assert b.text(0).endswith(b"after 1\nafter 2\n") and b.text(1).endswith(b"l40\n")


@pytest.mark.gpu
def test_gpu_ignores(ctx):
    from syzkaller_amd import report as R

    mid = b"".join(K.con(b"m%d" % i) for i in range(7))
    log = K.con(b"p0") + K.con(b"BUG: first") + mid + K.con(b"WARNING: second") + K.con(b"x") + K.con(b"UBSAN: third") + K.con(b"y")
    starts = sorted({r[0] for r in OR.scan(log)})
    assert len(starts) == 3
    ign = [[], [starts[0]], [starts[2]], starts, [starts[0], starts[1]], [starts[1]]]
    _, b = _check(ctx, [log] * len(ign), ign)
    assert b.oops.tolist() == [0, 1, 0, -1, 12, 0]
    assert int(b.start[1]) == starts[1] and b.text(1).startswith(b"m2\n") and int(b.end[2]) < starts[2]
    # the public form: regexps over the record lines, then the parse
    igs = [re.compile(rb"BUG: first"), re.compile(rb"UBSAN")]
    got = R.parse_batch([log, b"quiet\n", log], igs, ctx)
    o = OR.parse_bounds(log, ignores=igs)
    assert got[0] == got[2] == (b"WARNING: second", o[5], o[1], o[2]) and got[1] == (b"", b"", 0, 0)
    assert R.contains_crash_batch([log, K.con(b"BUG: first")], igs, ctx) == [True, False]
    rng = random.Random(5)
    logs = K.random_logs(21, 40)
    _check(ctx, logs, [sorted(K.random_ignored(rng, x)) for x in logs])


@pytest.mark.gpu
def test_gpu_random_logs(ctx):
    _check(ctx, K.random_logs(3, 300))


@pytest.mark.gpu
def test_gpu_device_forms_and_cap(ctx):
    import torch

    from syzkaller_amd import report as R
    from syzkaller_amd._lib import call

    logs = K.random_logs(4, 60) + [b"", b"BUG: last"]
    rng = random.Random(6)
    ignored = [sorted(K.random_ignored(rng, x)) for x in logs]
    data, off = R.to_batch(logs)
    nlogs = len(logs)
    recs = R.crash_scan(logs, ctx)
    hb = R.parse_bounds_batch(logs, ignored, ctx)
    hc = R.console_output_batch(logs, ctx)
    k = len(recs)
    FILL = 0xA5
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(U8).copy()).to("cuda")  # noqa: E731
    buf = lambda nbytes: torch.full((nbytes + 16,), FILL, dtype=torch.uint8, device="cuda")  # noqa: E731
    host = lambda t, dt, n: t.cpu().numpy()[: n * np.dtype(dt).itemsize].view(dt)  # noqa: E731
    d_data, d_off = dev(data), dev(off)
    for cap in (k, k + 3, k - 1, 0):
        d_cont, d_n, d_st = buf(nlogs), buf(8), buf(24)
        r = [buf(cap * 4), buf(cap * 8), buf(cap * 8), buf(cap * 4), buf(cap * 8)]
        call("sg_crash_scan_dev", ctx.h, d_data.data_ptr(), d_off.data_ptr(), nlogs, data.size, d_cont.data_ptr(),
             *[x.data_ptr() for x in r], cap, d_n.data_ptr(), d_st.data_ptr())
        ctx.sync()
        assert int(host(d_n, U64, 1)[0]) == k and host(d_cont, U8, nlogs).tolist() == recs.contains.tolist()
        assert host(d_st, U64, 3).tolist() == recs.stats.tolist()
        if cap >= k:
            got = [host(x, dt, k) for x, dt in zip(r, (U32, U64, U64, U32, U64))]
            for g, w in zip(got, (recs.log, recs.line_start, recs.line_end, recs.oops, recs.match)):
                assert np.array_equal(g, w)
            assert all((x.cpu().numpy()[k * s:] == FILL).all() for x, s in zip(r, (4, 8, 8, 4, 8)))
        else:                                                        # above cap: the count and nothing else
            assert all((x.cpu().numpy() == FILL).all() for x in r)
        assert (d_cont.cpu().numpy()[nlogs:] == FILL).all() and (d_n.cpu().numpy()[8:] == FILL).all()
    ign_off = np.concatenate([[0], np.cumsum([len(s) for s in ignored])]).astype(U64)
    ign_pos = np.array([p for s in ignored for p in s] + [0], U64)
    d_ioff, d_ipos = dev(ign_off), dev(ign_pos)
    ntext = int(hb.text_off[nlogs])
    for cap in (ntext, ntext + 5, ntext - 1):
        outs = [buf(nlogs * 4)] + [buf(nlogs * 8) for _ in range(4)] + [buf((nlogs + 1) * 8), buf(cap)]
        call("sg_crash_parse_dev", ctx.h, d_data.data_ptr(), d_off.data_ptr(), nlogs, data.size, d_ioff.data_ptr(),
             d_ipos.data_ptr(), int(ign_off[-1]), *[x.data_ptr() for x in outs], cap, None)
        ctx.sync()
        assert np.array_equal(host(outs[0], I32, nlogs), hb.oops)
        for x, w in zip(outs[1:5], (hb.start, hb.end, hb.desc_pos, hb.desc_len)):
            assert np.array_equal(host(x, U64, nlogs), w)
        assert np.array_equal(host(outs[5], U64, nlogs + 1), hb.text_off)
        t = outs[6].cpu().numpy()
        if cap >= ntext:
            assert np.array_equal(t[:ntext], hb.text_bytes) and (t[ntext:] == FILL).all()
        else:
            assert (t == FILL).all()
    assert ntext > 0 and k > 0
    want = np.frombuffer(b"".join(hc), U8)
    for cap in (want.size, want.size - 1):
        d_ooff, d_out = buf((nlogs + 1) * 8), buf(cap)
        call("sg_console_output_dev", ctx.h, d_data.data_ptr(), d_off.data_ptr(), nlogs, data.size, d_ooff.data_ptr(),
             d_out.data_ptr(), cap, None)
        ctx.sync()
        assert host(d_ooff, U64, nlogs + 1).tolist() == np.concatenate([[0], np.cumsum([len(x) for x in hc])]).tolist()
        t = d_out.cpu().numpy()
        assert np.array_equal(t[:cap], want) and (t[cap:] == FILL).all() if cap >= want.size else (t == FILL).all()
    # the host form above its cap: the count, and no record written
    few = R.crash_scan(logs, ctx, cap=max(k - 1, 0))
    assert len(few) == k and np.array_equal(few.oops, recs.oops)      # (crash_scan asks again with the count)
