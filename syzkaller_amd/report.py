"""pkg/report over batches of console logs: the mirror of the reference's interface (pkg/report/report.go).

The per-line work -- the header searches of matchOops, consoleOutputRe, questionableRe and the report text -- runs on
the GPU over a whole batch of logs in one call (csrc/sg_crash_report.hip).  What stays here is what the reference
does once per crash, over the oops alone: the caller's `ignores` (Go regular expressions; here `re` patterns over
bytes) on the few lines that have records, extractDescription's format expressions over output[start:], the '\\r'
strip, the six replacements of report.go:471-483 and the cut at 180 bytes.  Everything works on bytes."""
import re
from ctypes import byref, c_size_t

import numpy as np

from . import _lib
from .cover import _ctx, _p8, _p32, _p64

U8, U32, U64, I32 = np.uint8, np.uint32, np.uint64, np.int32

HEADERS = [
    b"BUG:", b"WARNING:", b"INFO:", b"Unable to handle kernel paging request", b"general protection fault:",
    b"Kernel panic", b"kernel BUG", b"Kernel BUG", b"BUG kmalloc-", b"divide error:", b"invalid opcode:",
    b"unreferenced object", b"UBSAN:",
]


def _compile(p):
    """report.go's compile(): the four placeholders, then the pattern as it stands."""
    p = p.replace(rb"{{ADDR}}", rb"0x[0-9a-f]+")
    p = p.replace(rb"{{PC}}", rb"\[\<[0-9a-f]+\>\]")
    p = p.replace(rb"{{FUNC}}", rb"([a-zA-Z0-9_]+)(?:\.|\+)")
    p = p.replace(rb"{{SRC}}", rb"([a-zA-Z0-9-_/.]+\.[a-z]+:[0-9]+)")
    return re.compile(p)


_LOCK = rb"(?:.*\n)+?.*is trying to acquire lock(?:.*\n)+?.*at: {{PC}} +{{FUNC}}"
_STALL = rb"(?:.*\n)+?.*</IRQ>.*\n(?:.* \? .*\n)+?(?:.*rcu.*\n)+?.*\]  {{FUNC}}"
_RIP2, _RIP1 = rb"(?:.*\n)+?.*RIP: [0-9]+:{{PC}} +{{PC}} +{{FUNC}}", rb"(?:.*\n)+?.*RIP: [0-9]+:{{FUNC}}"
# oops -> [(pattern, format)]: the formats of the oops table (report.go:32-343), in its order
_FORMATS = {
    0: [
        (rb"BUG: KASAN: ([a-z\-]+) in {{FUNC}}(?:.*\n)+?.*(Read|Write) of size ([0-9]+)", b"KASAN: %[1]v %[3]v in %[2]v"),
        (rb"BUG: KASAN: ([a-z\-]+) on address(?:.*\n)+?.*(Read|Write) of size ([0-9]+)", b"KASAN: %[1]v %[2]v of size %[3]v"),
        (rb"BUG: KASAN: (.*)", b"KASAN: %[1]v"),
        (rb"BUG: unable to handle kernel paging request(?:.*\n)+?.*IP: (?:{{PC}} +)?{{FUNC}}",
         b"BUG: unable to handle kernel paging request in %[1]v"),
        (rb"BUG: unable to handle kernel paging request", b"BUG: unable to handle kernel paging request"),
        (rb"BUG: unable to handle kernel NULL pointer dereference(?:.*\n)+?.*IP: (?:{{PC}} +)?{{FUNC}}",
         b"BUG: unable to handle kernel NULL pointer dereference in %[1]v"),
        (rb"BUG: spinlock lockup suspected", b"BUG: spinlock lockup suspected"),
        (rb"BUG: spinlock recursion", b"BUG: spinlock recursion"),
        (rb"BUG: soft lockup", b"BUG: soft lockup"),
        (rb"BUG: .*still has locks held!(?:.*\n)+?.*{{PC}} +{{FUNC}}", b"BUG: still has locks held in %[1]v"),
        (rb"BUG: bad unlock balance detected!(?:.*\n)+?.*{{PC}} +{{FUNC}}", b"BUG: bad unlock balance in %[1]v"),
        (rb"BUG: held lock freed!(?:.*\n)+?.*{{PC}} +{{FUNC}}", b"BUG: held lock freed in %[1]v"),
        (rb"BUG: Bad rss-counter state", b"BUG: Bad rss-counter state"),
        (rb"BUG: non-zero nr_ptes on freeing mm", b"BUG: non-zero nr_ptes on freeing mm"),
        (rb"BUG: non-zero nr_pmds on freeing mm", b"BUG: non-zero nr_pmds on freeing mm"),
        (rb"BUG: Dentry .* still in use \([0-9]+\) \[unmount of ([^\]]+)\]", b"BUG: Dentry still in use [unmount of %[1]v]"),
        (rb"BUG: Bad page state .*", b"BUG: Bad page state"),
        (rb"BUG: spinlock bad magic .*", b"BUG: spinlock bad magic"),
    ],
    1: [
        (rb"WARNING: .* at {{SRC}} {{FUNC}}", b"WARNING in %[2]v"),
        (rb"WARNING: possible circular locking dependency detected" + _LOCK, b"possible deadlock in %[1]v"),
        (rb"WARNING: possible irq lock inversion dependency detected(?:.*\n)+?.*just changed the state of lock"
         rb"(?:.*\n)+?.*at: {{PC}} +{{FUNC}}", b"possible deadlock in %[1]v"),
        (rb"WARNING: SOFTIRQ-safe -> SOFTIRQ-unsafe lock order detected(?:.*\n)+?.*is trying to acquire"
         rb"(?:.*\n)+?.*at: {{PC}} +{{FUNC}}", b"possible deadlock in %[1]v"),
        (rb"WARNING: possible recursive locking detected" + _LOCK, b"possible deadlock in %[1]v"),
        (rb"WARNING: inconsistent lock state(?:.*\n)+?.*takes(?:.*\n)+?.*at: {{PC}} +{{FUNC}}",
         b"inconsistent lock state in %[1]v"),
        (rb"WARNING: suspicious RCU usage(?:.*\n)+?.*?{{SRC}}", b"suspicious RCU usage at %[1]v"),
        (rb"WARNING: kernel stack regs at [0-9a-f]+ in [^ ]* has bad '([^']+)' value",
         b"WARNING: kernel stack regs has bad '%[1]v' value"),
        (rb"WARNING: kernel stack frame pointer at [0-9a-f]+ in [^ ]* has bad value",
         b"WARNING: kernel stack frame pointer has bad value"),
    ],
    2: [
        (rb"INFO: possible circular locking dependency detected \]" + _LOCK, b"possible deadlock in %[1]v"),
        (rb"INFO: possible irq lock inversion dependency detected \](?:.*\n)+?.*just changed the state of lock"
         rb"(?:.*\n)+?.*at: {{PC}} +{{FUNC}}", b"possible deadlock in %[1]v"),
        (rb"INFO: SOFTIRQ-safe -> SOFTIRQ-unsafe lock order detected \](?:.*\n)+?.*is trying to acquire"
         rb"(?:.*\n)+?.*at: {{PC}} +{{FUNC}}", b"possible deadlock in %[1]v"),
        (rb"INFO: possible recursive locking detected \]" + _LOCK, b"possible deadlock in %[1]v"),
        (rb"INFO: inconsistent lock state \](?:.*\n)+?.*takes(?:.*\n)+?.*at: {{PC}} +{{FUNC}}",
         b"inconsistent lock state in %[1]v"),
        (rb"INFO: rcu_preempt detected stalls" + _STALL, b"INFO: rcu detected stall in %[1]v"),
        (rb"INFO: rcu_preempt detected stalls", b"INFO: rcu detected stall"),
        (rb"INFO: rcu_sched detected(?: expedited)? stalls" + _STALL, b"INFO: rcu detected stall in %[1]v"),
        (rb"INFO: rcu_sched detected(?: expedited)? stalls", b"INFO: rcu detected stall"),
        (rb"INFO: rcu_preempt self-detected stall on CPU" + _STALL, b"INFO: rcu detected stall in %[1]v"),
        (rb"INFO: rcu_preempt self-detected stall on CPU", b"INFO: rcu detected stall"),
        (rb"INFO: rcu_sched self-detected stall on CPU" + _STALL, b"INFO: rcu detected stall in %[1]v"),
        (rb"INFO: rcu_sched self-detected stall on CPU", b"INFO: rcu detected stall"),
        (rb"INFO: rcu_bh detected stalls on CPU", b"INFO: rcu detected stall"),
        (rb"INFO: suspicious RCU usage(?:.*\n)+?.*?{{SRC}}", b"suspicious RCU usage at %[1]v"),
        (rb"INFO: task .* blocked for more than [0-9]+ seconds", b"INFO: task hung"),
    ],
    3: [(rb"Unable to handle kernel paging request(?:.*\n)+?.*PC is at {{FUNC}}",
         b"unable to handle kernel paging request in %[1]v")],
    4: [(rb"general protection fault:" + _RIP2, b"general protection fault in %[1]v"),
        (rb"general protection fault:" + _RIP1, b"general protection fault in %[1]v")],
    5: [
        (rb"Kernel panic - not syncing: Attempted to kill init!", b"kernel panic: Attempted to kill init!"),
        (rb"Kernel panic - not syncing: Couldn't open N_TTY ldisc for [^ ]+ --- error -[0-9]+",
         b"kernel panic: Couldn't open N_TTY ldisc"),
        (rb"Kernel panic - not syncing: (.*)", b"kernel panic: %[1]v"),
    ],
    6: [(rb"kernel BUG (.*)", b"kernel BUG %[1]v")],
    7: [(rb"Kernel BUG (.*)", b"kernel BUG %[1]v")],
    8: [(rb"BUG kmalloc-.*: Object already free", b"BUG: Object already free")],
    9: [(rb"divide error: " + _RIP2, b"divide error in %[1]v"), (rb"divide error: " + _RIP1, b"divide error in %[1]v")],
    10: [(rb"invalid opcode: " + _RIP2, b"invalid opcode in %[1]v"), (rb"invalid opcode: " + _RIP1, b"invalid opcode in %[1]v")],
    11: [(rb"unreferenced object {{ADDR}} \(size ([0-9]+)\):(?:.*\n.*)+backtrace:.*\n.*{{PC}}.*\n.*{{PC}}.*\n.*{{PC}} {{FUNC}}",
          b"memory leak in %[2]v (size %[1]v)")],
    12: [],
}
FORMATS = {i: [(_compile(p), f) for p, f in v] for i, v in _FORMATS.items()}

_EXECUTOR = re.compile(rb"syz-executor[0-9]+((/|:)[0-9]+)?")
_ADDR = re.compile(rb"[0-9a-f]{8,}")
_DECNUM = re.compile(rb"[0-9]{5,}")
_LINENUM = re.compile(rb"(:[0-9]+)+")
_FUNC = re.compile(rb"([a-zA-Z][a-zA-Z0-9_.]+)\+0x[0-9a-z]+/0x[0-9a-z]+")
_CPU = re.compile(rb"CPU#[0-9]+")
MAX_DESC_LEN = 180


def extract_description(output, oops, fallback):
    """extractDescription (report.go:533-565) over output = the log from `start` on; `fallback` is the header's line
    rest, which the device found."""
    result, start_pos = b"", -1
    for rx, fmt in FORMATS[oops]:
        m = rx.search(output)
        if m is None or (start_pos != -1 and start_pos <= m.start()):
            continue
        start_pos = m.start()
        result = re.sub(rb"%\[([0-9]+)\]v", lambda a: m.group(int(a.group(1))), fmt)
    return result if result else fallback


def finish_description(desc):
    """report.go:467-488."""
    if desc.endswith(b"\r"):
        desc = desc[:-1]
    desc = _EXECUTOR.sub(b"syz-executor", desc)
    desc = _ADDR.sub(b"ADDR", desc)
    desc = _DECNUM.sub(b"NUM", desc)
    desc = _LINENUM.sub(b":LINE", desc)
    desc = _FUNC.sub(rb"\1", desc)
    desc = _CPU.sub(b"CPU", desc)
    return desc[:MAX_DESC_LEN]


def to_batch(logs):
    """A list of bytes as the calls' CSR: (bytes as u8, off)."""
    off = np.zeros(len(logs) + 1, dtype=U64)
    if logs:
        off[1:] = np.cumsum([len(b) for b in logs], dtype=U64)
    data = np.frombuffer(b"".join(bytes(b) for b in logs), dtype=U8)
    return data, off


class CrashRecords:
    """sg_crash_scan's result: contains[nlogs], and of record k its log, its line's start and end in the log, its
    oops (an index into HEADERS) and the header's offset in the line; ordered by (log, line, table order)."""

    def __init__(self, contains, log, line_start, line_end, oops, match, stats):
        self.contains, self.log, self.line_start, self.line_end = contains, log, line_start, line_end
        self.oops, self.match, self.stats = oops, match, stats

    def __len__(self):
        return int(self.log.size)


def crash_scan(logs, ctx=None, cap=None):
    data, off = to_batch(logs)
    nlogs = len(logs)
    cap = 1024 + 4 * nlogs if cap is None else cap
    contains, stats, n = np.zeros(nlogs, dtype=U8), np.zeros(3, dtype=U64), c_size_t()
    while True:
        r32 = [np.empty(cap, dtype=U32) for _ in range(2)]
        r64 = [np.empty(cap, dtype=U64) for _ in range(3)]
        _lib.call("sg_crash_scan", _ctx(ctx).h, _p8(data), _p64(off), nlogs, _p8(contains), _p32(r32[0]), _p64(r64[0]),
                  _p64(r64[1]), _p32(r32[1]), _p64(r64[2]), cap, byref(n), _p64(stats))
        if n.value <= cap:
            break
        cap = n.value
    k = n.value
    return CrashRecords(contains, r32[0][:k], r64[0][:k], r64[1][:k], r32[1][:k], r64[2][:k], stats)


def contains_crash_batch(logs, ignores=None, ctx=None):
    """ContainsCrash of every log: a list of bool."""
    recs = crash_scan(logs, ctx)
    if not ignores:
        return [bool(c) for c in recs.contains]
    out = [False] * len(logs)
    ignored = _ignored_lines(logs, recs, ignores)
    for k in range(len(recs)):
        if int(recs.line_start[k]) not in ignored[int(recs.log[k])]:
            out[int(recs.log[k])] = True
    return out


def ContainsCrash(output, ignores=None, ctx=None):
    return contains_crash_batch([output], ignores, ctx)[0]


def _ignored_lines(logs, recs, ignores):
    """Per log, the starts of the record lines that one of `ignores` matches (each distinct line asked once)."""
    out = [set() for _ in logs]
    seen = set()
    for k in range(len(recs)):
        key = (int(recs.log[k]), int(recs.line_start[k]))
        if key in seen:
            continue
        seen.add(key)
        line = bytes(logs[key[0]][key[1]:int(recs.line_end[k])])
        if any(rx.search(line) for rx in ignores):
            out[key[0]].add(key[1])
    return out


class ParseBounds:
    """sg_crash_parse's result: per log oops (-1: none), start, end, desc_pos, desc_len, and text(l)."""

    def __init__(self, oops, start, end, desc_pos, desc_len, text_off, text_bytes, stats):
        self.oops, self.start, self.end, self.desc_pos, self.desc_len = oops, start, end, desc_pos, desc_len
        self.text_off, self.text_bytes, self.stats = text_off, text_bytes, stats

    def text(self, l):
        return self.text_bytes[int(self.text_off[l]):int(self.text_off[l + 1])].tobytes()


def parse_bounds_batch(logs, ignored=None, ctx=None, cap=None):
    """sg_crash_parse over `logs`; ignored: per log, an iterable of the ignored lines' starts (None: none)."""
    data, off = to_batch(logs)
    nlogs = len(logs)
    ign_off = ign_pos = None
    if ignored is not None:
        lists = [sorted(int(p) for p in s) for s in ignored]
        ign_off = np.zeros(nlogs + 1, dtype=U64)
        if nlogs:
            ign_off[1:] = np.cumsum([len(s) for s in lists], dtype=U64)
        ign_pos = np.array([p for s in lists for p in s] + [0], dtype=U64)
    oops = np.empty(nlogs, dtype=I32)
    start, end, dpos, dlen = (np.empty(nlogs, dtype=U64) for _ in range(4))
    text_off, stats, n = np.zeros(nlogs + 1, dtype=U64), np.zeros(3, dtype=U64), c_size_t()
    cap = int(data.size) if cap is None else cap
    text = np.empty(cap, dtype=U8)
    _lib.call("sg_crash_parse", _ctx(ctx).h, _p8(data), _p64(off), nlogs, None if ign_off is None else _p64(ign_off),
              None if ign_pos is None else _p64(ign_pos), oops.ctypes.data_as(_lib.PI32), _p64(start), _p64(end),
              _p64(dpos), _p64(dlen), _p64(text_off), _p8(text), cap, byref(n), _p64(stats))
    return ParseBounds(oops, start, end, dpos, dlen, text_off, text[:min(n.value, cap)], stats)


def parse_batch(logs, ignores=None, ctx=None):
    """report.Parse of every log: a list of (desc, text, start, end), desc and text bytes.  With ignores: the scan,
    the regexps over the distinct record lines, then the parse with the ignored lines; without: the parse alone."""
    ignored = None
    if ignores:
        ignored = _ignored_lines(logs, crash_scan(logs, ctx), ignores)
    b = parse_bounds_batch(logs, ignored, ctx)
    out = []
    for l, log in enumerate(logs):
        if b.oops[l] < 0:
            out.append((b"", b"", 0, 0))
            continue
        start, dp = int(b.start[l]), int(b.desc_pos[l])
        log = bytes(log)
        desc = extract_description(log[start:], int(b.oops[l]), log[dp:dp + int(b.desc_len[l])])
        out.append((finish_description(desc), b.text(l), start, int(b.end[l])))
    return out


def Parse(output, ignores=None, ctx=None):
    return parse_batch([output], ignores, ctx)[0]


def console_output_batch(logs, ctx=None):
    """ExtractConsoleOutput of every log: a list of bytes."""
    data, off = to_batch(logs)
    nlogs = len(logs)
    out_off, stats, n = np.zeros(nlogs + 1, dtype=U64), np.zeros(3, dtype=U64), c_size_t()
    cap = int(data.size)
    out = np.empty(cap, dtype=U8)
    _lib.call("sg_console_output", _ctx(ctx).h, _p8(data), _p64(off), nlogs, _p64(out_off), _p8(out), cap, byref(n),
              _p64(stats))
    return [out[int(out_off[l]):int(out_off[l + 1])].tobytes() for l in range(nlogs)]


def ExtractConsoleOutput(output, ctx=None):
    return console_output_batch([output], ctx)[0]
