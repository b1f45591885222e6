"""Logs for the crash-report tests, written for this project in the shape of kernel messages: hand-derived cases
for the oracle, the fragment generator that the parallel model is held against, and builders that put a literal at
a chosen place of a batch (a tile boundary of the kernels)."""
import random

from tests import crash_report_oracle as OR

P = b"[   12.345678] "          # a console prefix
P6 = b"<6>[    1.000000] "


def con(body, p=P, end=b"\n"):
    return p + body + end


# (name, log, desc of the fallback = output[desc_pos : desc_pos + desc_len], oops, start, end, text): derived by hand
def hand_cases():
    out = []
    for i, h in enumerate(OR.HEADERS):
        lead = con(b"booting") + con(b"still booting")
        line = P + b"x " + h + b" something broke"
        log = lead + line + b"\n" + con(b"Call Trace:") + b"plain fuzzer output\n"
        out.append(("header %d" % i, log, h + b" something broke", i, len(lead), len(lead) + len(line),
                    b"booting\nstill booting\nx " + h + b" something broke\nCall Trace:\n"))
    supp = [
        (b"Boot_DEBUG: BUG: x", 0), (OR.MODULI + b" and more", 1), (b"INFO: lockdep is turned off", 2),
        (b"INFO: Stall ended before state dump start", 2), (b"a_INFO:: INFO: x", 2),
        (b"INFO: NMI handler (perf) took too long to run: 1.2 msecs", 2),
    ]
    for body, _ in supp:
        out.append(("suppressed " + body[:12].decode(), con(b"a") + con(body) + con(b"b"), b"", -1, 0, 0, b""))
    # a suppression removes only its own oops
    log = con(b"Boot_DEBUG: WARNING: x")
    out.append(("own oops only", log, b"WARNING: x", 1, 0, len(log) - 1, b"Boot_DEBUG: WARNING: x\n"))
    return out


# ---- random fragment sequences ----------------------------------------------------------------------------------
PREFIXES = [P, P6, b"[1.2] ", b"", b"", b"[ 1.] ", b"< 6>[1.2] ", b"x[1.2] "]
BODIES = (
    [h + b" boom" for h in OR.HEADERS] +
    [b"Boot_DEBUG: BUG: x", b"Boot_DEBUG: WARNING: y", OR.MODULI, b"INFO: lockdep is turned off", b"my_INFO:: INFO: z",
     b"INFO: Stall ended before state dump start", b"INFO: NMI handler (x) took too long to run: 9",
     b" took too long to run INFO: NMI handler x", b"INFO: NMI handler took too long to run",
     b"INFO: NMI handler  took too long to run",
     b" [<ffffffff81000000>] ? f+0x1/0x2", b" ? f+0x1/0x2", b" ? f+0x1/0x2 <EOI>", b" ?f+0x1/0x2", b" ? f+0x1/2",
     b" ?  g.part.3+0xab/0x100", b" ? h+0x/0x2", b" [<ffffffff81000000>] f+0x1/0x2",
     OR.TAINT, OR.PANIC + b": Fatal", OR.PANIC + b" " + OR.TAINT, b"Call Trace:", b"", b"executing program 3",
     b"kernel BUG at fs/x.c:1!", b"Kernel BUG: BUG kmalloc-64: bad"]
)
ENDS = [b"\n", b"\n", b"\n", b"\r\n"]


def random_log(rng, nmax=70):
    n = rng.randrange(0, nmax)
    calm = rng.random() < 0.5       # mostly plain console lines, so that runs pass 40 lines
    parts = []
    for _ in range(n):
        if calm and rng.random() < 0.85:
            parts.append(P + rng.choice([b"Call Trace:", b" [<ffffffff81000000>] f+0x1/0x2", OR.TAINT, b"x"]) + b"\n")
        else:
            parts.append(rng.choice(PREFIXES) + rng.choice(BODIES) + rng.choice(ENDS))
    log = b"".join(parts)
    if log and rng.random() < 0.3:
        log = log[:-1]              # no '\n' at the end
    return log


def random_logs(seed, count, nmax=70):
    rng = random.Random(seed)
    return [random_log(rng, nmax) for _ in range(count)]


def random_ignored(rng, log):
    """A subset of the record lines of `log`."""
    starts = sorted({r[0] for r in OR.scan(log)})
    return {s for s in starts if rng.random() < 0.4}


# ---- placing bytes in a batch -----------------------------------------------------------------------------------
def filler(n):
    """n bytes of plain lines without any literal, ending in '\\n' (n == 0: nothing)."""
    out = b""
    while n > 200:
        out += b"f" * 199 + b"\n"
        n -= 200
    return out + (b"f" * (n - 1) + b"\n" if n else b"")


class Batch:
    """Logs laid one behind the other, as the calls take them; `at` is the batch position of the next log's byte 0."""

    def __init__(self):
        self.logs, self.at = [], 0

    def add(self, log):
        self.logs.append(log)
        self.at += len(log)
        return len(self.logs) - 1

    def add_at(self, tile, back, lead, lit, tail):
        """A log whose line lead + lit + tail has lit start `back` bytes before the next multiple of `tile`."""
        pad = (-(self.at + len(lead)) - back) % tile
        return self.add(filler(pad) + lead + lit + tail)
