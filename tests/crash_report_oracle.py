"""Oracle of the crash-report calls: pkg/report/report.go restated in Python, line for line and on one thread.

`scan`, `parse_bounds` and `console_output` are the Go loops of ContainsCrash (:369-387), Parse up to
extractDescription (:393-465) and ExtractConsoleOutput (:492-513) with matchOops (:515-531); the regular
expressions are the reference's, run by `re` over bytes.  `model_parse` is the other reading, the one the kernels
follow: per-line facts first, then the text stated by ranks with no running state.  The CPU tests hold the two
against each other.  No Go toolchain is needed."""
import re

HEADERS = [
    b"BUG:", b"WARNING:", b"INFO:", b"Unable to handle kernel paging request", b"general protection fault:",
    b"Kernel panic", b"kernel BUG", b"Kernel BUG", b"BUG kmalloc-", b"divide error:", b"invalid opcode:",
    b"unreferenced object", b"UBSAN:",
]
MODULI = b"WARNING: /etc/ssh/moduli does not exist, using fixed modulus"
SUPPRESSIONS = {
    0: [rb"Boot_DEBUG:"],
    1: [re.escape(MODULI)],
    2: [rb"INFO: lockdep is turned off", rb"INFO: Stall ended before state dump start",
        rb"INFO: NMI handler .* took too long to run", rb"_INFO::"],
}
_SUPP = {i: [re.compile(p) for p in ps] for i, ps in SUPPRESSIONS.items()}
CONSOLE_RE = re.compile(rb"^(?:\<[0-9]+\>)?\[ *[0-9]+\.[0-9]+\] ")
QUESTIONABLE_RE = re.compile(rb"(?:\[\<[0-9a-f]+\>\])? \? +[a-zA-Z0-9_.]+\+0x[0-9a-f]+/[0-9a-f]+")
EOI = b"<EOI>"
TAINT = b"Disabling lock debugging due to kernel taint"
PANIC = b"Kernel panic - not syncing"
NMI_A, NMI_B = b"INFO: NMI handler ", b" took too long to run"


def lines(output):
    """The (pos, next) of the loop of :370-376."""
    pos, out = 0, []
    while pos < len(output):
        nxt = output.find(b"\n", pos)
        if nxt == -1:
            nxt = len(output)
        out.append((pos, nxt))
        pos = nxt + 1
    return out


def match_oops(line, i, ignores=()):
    m = line.find(HEADERS[i])
    if m == -1:
        return -1
    for s in _SUPP.get(i, ()):
        if s.search(line):
            return -1
    for ig in ignores:
        if ig.search(line):
            return -1
    return m


def scan(output, ignores=()):
    """[(line_start, line_end, oops, match)] in (line, table) order."""
    recs = []
    for pos, nxt in lines(output):
        for i in range(len(HEADERS)):
            m = match_oops(output[pos:nxt], i, ignores)
            if m != -1:
                recs.append((pos, nxt, i, m))
    return recs


def contains_crash(output, ignores=()):
    return bool(scan(output, ignores))


def is_console(line):
    return bool(CONSOLE_RE.match(line)) and (not QUESTIONABLE_RE.search(line) or EOI in line)


def parse_bounds(output, ignores=(), ignored=None):
    """Parse up to :465: (oops, start, end, desc_pos, desc_len, text); oops -1 and zeros without one.  `ignored`, a
    set of line starts, stands for ignores that match exactly those lines."""
    oops, start, end, dpos, dlen = -1, 0, 0, 0, 0
    prefix, text, text_lines, skip_text = [], bytearray(), 0, False
    for pos, nxt in lines(output):
        ln = output[pos:nxt]
        for i in range(len(HEADERS)):
            m = match_oops(ln, i, ignores)
            if m == -1 or (ignored is not None and pos in ignored):
                continue
            if oops == -1:
                oops, start, dpos, dlen = i, pos, pos + m, nxt - (pos + m)
            end = nxt
        if is_console(ln):
            ls = ln.find(b"] ") + pos + 2
            le = nxt
            if le != 0 and output[le - 1:le] == b"\r":
                le -= 1
            if oops == -1:
                prefix.append(output[ls:le])
                if len(prefix) > 5:
                    prefix = prefix[1:]
            else:
                for p in prefix:
                    text += p + b"\n"
                prefix = []
                text_lines += 1
                body = output[ls:le]
                skip_line = skip_text
                if TAINT in body:
                    skip_line = True
                elif text_lines > 40 and PANIC in body:
                    skip_text = True
                    skip_line = True
                if not skip_line:
                    text += body + b"\n"
    return oops, start, end, dpos, dlen, bytes(text)


def console_output(output):
    out = bytearray()
    for pos, nxt in lines(output):
        ln = output[pos:nxt]
        if is_console(ln):
            ls = ln.find(b"] ") + pos + 2
            le = nxt
            if le != 0 and output[le - 1:le] == b"\r":
                le -= 1
            out += output[ls:le] + b"\n"
    return bytes(out)


# ---- the parallel reading ---------------------------------------------------------------------------------------
def _prefix_len(ln):
    """consoleOutputRe by hand, as the kernel reads it: the prefix's length, or -1."""
    q, e = 0, len(ln)
    dig = lambda c: 48 <= c <= 57  # noqa: E731
    if q < e and ln[q] == ord("<"):
        d = q + 1
        while d < e and dig(ln[d]):
            d += 1
        if d == q + 1 or d >= e or ln[d] != ord(">"):
            return -1
        q = d + 1
    if q >= e or ln[q] != ord("["):
        return -1
    q += 1
    while q < e and ln[q] == 32:
        q += 1
    d = q
    while q < e and dig(ln[q]):
        q += 1
    if q == d or q >= e or ln[q] != ord("."):
        return -1
    q += 1
    d = q
    while q < e and dig(ln[q]):
        q += 1
    if q == d or e - q < 2 or ln[q] != ord("]") or ln[q + 1] != 32:
        return -1
    return q + 2


def _questionable(ln):
    """questionableRe from each " ? ", every run closed by the first byte outside its class."""
    word = set(b"abcdefghijklmnopqrstuvwxyzABCDEFGHIJKLMNOPQRSTUVWXYZ0123456789_.")
    hexd = set(b"0123456789abcdef")
    p = ln.find(b" ? ")
    while p != -1:
        q, e = p + 2, len(ln)
        while q < e and ln[q] == 32:
            q += 1
        w0 = q
        while q < e and ln[q] in word:
            q += 1
        if q > w0 and ln[q:q + 3] == b"+0x":
            q += 3
            h0 = q
            while q < e and ln[q] in hexd:
                q += 1
            if q > h0 and e - q >= 2 and ln[q] == ord("/") and ln[q + 1] in hexd:
                return True
        p = ln.find(b" ? ", p + 1)
    return False


def line_facts(ln):
    """(live oops mask, prefix length or -1 when no console line, taint, panic) of one line, from literal finds."""
    live = 0
    for i, h in enumerate(HEADERS):
        if h in ln:
            live |= 1 << i
    if b"Boot_DEBUG:" in ln:
        live &= ~1
    if MODULI in ln:
        live &= ~2
    if b"INFO: lockdep is turned off" in ln or b"INFO: Stall ended before state dump start" in ln or b"_INFO::" in ln:
        live &= ~4
    a = ln.find(NMI_A)
    if a != -1 and ln.find(NMI_B, a + len(NMI_A)) != -1:
        live &= ~4
    pfx = _prefix_len(ln)
    if pfx != -1 and _questionable(ln) and EOI not in ln:
        pfx = -1
    return live, pfx, TAINT in ln, PANIC in ln


def model_parse(output, ignored=None):
    """parse_bounds' result from per-line facts and ranks, as include/syzsig.h states it."""
    L = lines(output)
    facts = [line_facts(output[p:n]) for p, n in L]
    live = [0 if (ignored is not None and L[k][0] in ignored) else f[0] for k, f in enumerate(facts)]
    rec = [k for k in range(len(L)) if live[k]]
    if not rec:
        return -1, 0, 0, 0, 0, b""
    l0, l1 = rec[0], rec[-1]
    pos, nxt = L[l0]
    oops = (live[l0] & -live[l0]).bit_length() - 1
    m = output[pos:nxt].find(HEADERS[oops])
    cons = [k for k in range(len(L)) if facts[k][1] != -1]
    after = [k for k in cons if k >= l0]
    text = bytearray()
    if after:
        cut = next((k for r, k in enumerate(after, 1) if r > 40 and facts[k][3] and not facts[k][2]), len(L))
        keep = [k for k in cons if k < l0][-5:] + [k for k in after if k < cut and not facts[k][2]]
        for k in keep:
            p, n = L[k]
            e = n - 1 if output[n - 1:n] == b"\r" and n > p else n
            text += output[p + facts[k][1]:e] + b"\n"
    return oops, pos, L[l1][1], pos + m, nxt - (pos + m), bytes(text)


def model_scan(output):
    out = []
    for p, n in lines(output):
        live = line_facts(output[p:n])[0]
        for i in range(len(HEADERS)):
            if live >> i & 1:
                out.append((p, n, i, output[p:n].find(HEADERS[i])))
    return out


def model_console(output):
    out = bytearray()
    for p, n in lines(output):
        pfx = line_facts(output[p:n])[1]
        if pfx != -1:
            e = n - 1 if output[n - 1:n] == b"\r" and n > p else n
            out += output[p + pfx:e] + b"\n"
    return bytes(out)
