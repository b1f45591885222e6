"""A sequential restatement of the Go lines the cover ingest replaces: bufio.Scanner / ScanLines with its token
limit, strconv.ParseUint, coveredPCs (syz-manager/cover.go:310-347) with the sort of :78, symbolizer.ReadSymbols
(pkg/symbolizer/nm.go:19-69) with the flatten-and-sort of cover.go:262-268, and getVmOffset (cover.go:219-254).
One line at a time, one byte test at a time: nothing here is shared with the library."""

MAX_LINE = 65536  # bufio.MaxScanTokenSize
U64 = (1 << 64) - 1


class TooLong(Exception):
    def __init__(self, pos):
        super().__init__(f"bufio.Scanner: token too long at byte {pos}")
        self.pos = pos


def scan_lines(text):
    """[(start, line bytes)] as bufio.Scanner with ScanLines hands them out; TooLong(start) for the first line whose
    content, the '\\r' counted, is MAX_LINE bytes or more (the buffer is full before a '\\n' is seen)."""
    out, s, n = [], 0, len(text)
    while s < n:
        e = text.find(b"\n", s)
        if e < 0:
            e = n
        if e - s >= MAX_LINE:
            raise TooLong(s)
        ln = text[s:e]
        if ln.endswith(b"\r"):
            ln = ln[:-1]
        out.append((s, ln))
        s = e + 1
    return out


def parse_uint16(b):
    """strconv.ParseUint(string(b), 16, 64): the value, or None for its error."""
    if len(b) == 0:
        return None
    v = 0
    for c in b:
        if 0x30 <= c <= 0x39:
            d = c - 0x30
        elif 0x61 <= c <= 0x66:
            d = c - 0x61 + 10
        elif 0x41 <= c <= 0x46:
            d = c - 0x41 + 10
        else:
            return None
        v = v * 16 + d
        if v > U64:
            return None  # ErrRange
    return v


def objdump_pcs(text, call=b"callq ", func=b" <__sanitizer_cov_trace_pc>"):
    pcs = []
    for _, ln in scan_lines(text):
        pos = ln.find(call)
        if pos == -1:
            continue
        if ln[pos:].find(func) == -1:
            continue
        colon = ln.find(b":")
        if colon == -1:
            continue
        pc = parse_uint16(ln[:colon])
        if pc is None:
            continue
        pcs.append(pc)
    return sorted(pcs)


def go_int_size(size):
    """int(size+15) / 16 * 16 with a 64-bit int: the add wraps, the division truncates toward zero."""
    v = (size + 15) & U64
    if v >= 1 << 63:
        v -= 1 << 64
    q = abs(v) // 16
    return (q if v >= 0 else -q) * 16


def nm_symbols(text):
    """[(addr, Size, name_pos, name bytes)] in text order."""
    syms = []
    for start, ln in scan_lines(text):
        if ln.find(b" t ") == -1 and ln.find(b" T ") == -1:
            continue
        sp1 = ln.find(b" ")
        if sp1 == -1:
            continue
        sp2 = ln[sp1 + 1:].find(b" ")
        if sp2 == -1:
            continue
        sp2 += sp1 + 1
        if not ln[sp2:].startswith(b" t ") and not ln[sp2:].startswith(b" T "):
            continue
        addr = parse_uint16(ln[:sp1])
        if addr is None:
            continue
        size = parse_uint16(ln[sp1 + 1:sp2])
        if size is None:
            continue
        syms.append((addr, go_int_size(size), start + sp2 + 3, ln[sp2 + 3:]))
    return syms


def nm_sorted(syms):
    """(sym_start, sym_end, order): cover.go:262-268 with the tie order pinned as (start, text order)."""
    order = sorted(range(len(syms)), key=lambda k: (syms[k][0], k))
    return ([syms[k][0] for k in order], [(syms[k][0] + syms[k][1]) & U64 for k in order], order)


# unicode.IsSpace
_GO_SPACE = set("\t\n\v\f\r \u0085\u00a0\u1680\u2028\u2029\u202f\u205f\u3000") | {chr(c) for c in range(0x2000, 0x200b)}


def fields(s):
    out, cur = [], ""
    for ch in s:
        if ch in _GO_SPACE:
            if cur:
                out.append(cur)
            cur = ""
        else:
            cur += ch
    if cur:
        out.append(cur)
    return out


def parse_uint_base0_hex(s):
    """strconv.ParseUint(s, 0, 64) for an s that starts with "0x": digits and, between them or behind the prefix,
    single underscores."""
    assert s[:2] == "0x"
    body = s[2:]
    if not body:
        return None
    last = "0"  # underscoreOK: the prefix counts as a digit
    v = 0
    seen = False
    for ch in body:
        if ch == "_":
            if last != "0":
                return None
            last = "_"
            continue
        if ch not in "0123456789abcdefABCDEF":
            return None
        last = "0"
        seen = True
        v = v * 16 + int(ch, 16)
        if v > U64:
            return None
    if last == "_" or not seen:
        return None
    return v


def vm_offset(text):
    """getVmOffset; ValueError for its errors and for its index panic.  s.Err() is never looked at there."""
    try:
        lines = scan_lines(text)
    except TooLong as e:
        lines = scan_lines(text[:e.pos])
    addr = 0
    for _, ln in lines:
        pieces = fields(ln.decode("utf-8", "replace"))
        for i in range(len(pieces)):
            if pieces[i] != "PROGBITS":
                continue
            if i + 1 >= len(pieces):
                raise ValueError("index out of range")
            v = parse_uint_base0_hex("0x" + pieces[i + 1])
            if v is None:
                raise ValueError("failed to parse addr in readelf output")
            if v == 0:
                continue
            v32 = v >> 32
            if addr == 0:
                addr = v32
            if addr != v32:
                raise ValueError("different section offsets in a single binary")
    return addr


# ---- addr2line: symbolize + parse (pkg/symbolizer/symbolizer.go:95-191) ------------------------------
A2L_OK, A2L_EMPTY, A2L_BAD_PC, A2L_NO_COLON, A2L_NO_FILE_LINE, A2L_TOO_LONG, A2L_TOO_FEW = 0, 1, 2, 3, 4, 5, 6
INT_MAX = (1 << 63) - 1


def _underscore_ok(s):
    """strconv.underscoreOK"""
    i = "^"
    if s[:1] in ("-", "+"):
        s = s[1:]
    hexa = False
    if len(s) >= 2 and s[0] == "0" and s[1].lower() in "box":
        i = "0"
        hexa = s[1].lower() == "x"
        s = s[2:]
    for ch in s:
        if "0" <= ch <= "9" or (hexa and "a" <= ch.lower() <= "f"):
            i = "0"
            continue
        if ch == "_":
            if i != "0":
                return False
            i = "_"
            continue
        if i == "_":
            return False
        i = "!"
    return i != "_"


def parse_uint0(b):
    """strconv.ParseUint(string(b), 0, 64): the value, or None for its error (syntax or range)."""
    s = b.decode("latin-1")
    if s == "":
        return None
    s0, base = s, 10
    if s[0] == "0":
        if len(s) >= 3 and s[1].lower() == "b":
            base, s = 2, s[2:]
        elif len(s) >= 3 and s[1].lower() == "o":
            base, s = 8, s[2:]
        elif len(s) >= 3 and s[1].lower() == "x":
            base, s = 16, s[2:]
        else:
            base, s = 8, s[1:]
    n, underscores = 0, False
    for ch in s:
        if ch == "_":
            underscores = True
            continue
        if "0" <= ch <= "9":
            d = ord(ch) - 48
        elif "a" <= ch.lower() <= "z" and ch.isascii():
            d = ord(ch.lower()) - 97 + 10
        else:
            return None
        if d >= base:
            return None
        n = n * base + d
        if n > U64:
            return None
    if underscores and not _underscore_ok(s0):
        return None
    return n


class _Scanner:
    """bufio.Scanner over a byte string: scan() / text() / err as symbolize and parse use them"""

    def __init__(self, text):
        self.t, self.p, self.tok, self.start, self.err = text, 0, b"", 0, None

    def scan(self):
        if self.err is not None or self.p >= len(self.t):
            self.tok = b""
            return False
        e = self.t.find(b"\n", self.p)
        if e < 0:
            e = len(self.t)
        if e - self.p >= MAX_LINE:
            self.err, self.tok, self.start = TooLong(self.p), b"", self.p
            return False
        ln = self.t[self.p:e]
        self.start, self.p = self.p, e + 1
        self.tok = ln[:-1] if ln.endswith(b"\r") else ln
        return True


class A2LError(Exception):
    def __init__(self, status, pos):
        super().__init__("addr2line status %d at byte %d" % (status, pos))
        self.status, self.pos = status, pos


def addr2line_frames(text, nrec):
    """symbolize's goroutine over `text` for len(pcs) == nrec: [(pc, [(func, file, line, func_pos, file_pos)])] per
    record, or A2LError(status, byte position).  Positions: the failing line's start; a function line that the
    text ends behind: that line's start; too few records: len(text)."""
    s = _Scanner(text)
    if not s.scan():
        if s.err is not None:
            raise A2LError(A2L_TOO_LONG, s.err.pos)
        raise A2LError(A2L_EMPTY, 0)
    out = []
    for _ in range(nrec):
        if out and out[-1][2]:
            raise A2LError(A2L_TOO_FEW, len(text))          # the last Scan returned false: Text() is "", no PC
        pc = parse_uint0(s.tok)
        if pc is None:
            raise A2LError(A2L_BAD_PC, s.start)
        frames, at_end = [], False
        while True:
            if not s.scan():
                at_end = True
                break
            ln = s.tok
            if len(ln) > 3 and ln[0:1] == b"0" and ln[1:2] == b"x":
                break
            fn, fn_pos = ln, s.start
            if not s.scan():
                if s.err is not None:
                    raise A2LError(A2L_TOO_LONG, s.err.pos)
                raise A2LError(A2L_NO_FILE_LINE, fn_pos)
            ln = s.tok
            colon = ln.rfind(b":")
            if colon == -1:
                raise A2LError(A2L_NO_COLON, s.start)
            end = colon + 1
            while end < len(ln) and 0x30 <= ln[end] <= 0x39:
                end += 1
            file, digits = ln[:colon], ln[colon + 1:end]
            line = int(digits) if digits else None
            if line is None or line > INT_MAX or fn in (b"", b"??") or file in (b"", b"??") or line <= 0:
                continue
            frames.append((fn, file, line, fn_pos, s.start))
        if s.err is not None:
            raise A2LError(A2L_TOO_LONG, s.err.pos)
        out.append((pc, frames, at_end))
    return [(pc, frames) for pc, frames, _ in out]


def intern(records):
    """CoverReport's setdefault(name, len(dict)) over the kept frames in order: (files, funcs) name -> id"""
    files, funcs = {}, {}
    for _, frames in records:
        for fn, file, _, _, _ in frames:
            files.setdefault(file, len(files))
            funcs.setdefault(fn, len(funcs))
    return files, funcs
