"""Oracle of the cover report's file bodies: parseFile (syz-manager/cover.go:198-217)
and the render loop of generateCoverHtml (cover.go:123-147) restated literally
over Python bytes and the fileSet dict of tests/cover_lines_oracle.py
({file: [(line, covered), ...]}).  Pinned by restatement only: no Go toolchain
is at hand to run the reference's own loop."""
import functools

REPLACER = {ord(">"): b"&gt;", ord("<"): b"&lt;", ord("&"): b"&amp;", ord("\t"): b"        "}  # cover.go:203
COVERED = (b"<span id='covered'>", b"</span> /*covered*/\n")   # cover.go:133, :135
UNCOVERED = (b"<span id='uncovered'>", b"</span>\n")           # cover.go:138, :140


def replace(line):
    """strings.Replacer over single-byte patterns: one pass, byte by byte, nothing it wrote is looked at again."""
    return b"".join(REPLACER.get(b, bytes([b])) for b in line)


def parse_file(data):
    """cover.go:198-217 after ReadFile."""
    lines = []
    while True:
        idx = data.find(b"\n")
        if idx == -1:
            break
        lines.append(replace(data[:idx]))
        data = data[idx + 1:]
    if len(data) != 0:
        lines.append(data)  # :213-215: the raw bytes
    return lines


def render(lines, covered):
    """cover.go:128-147: (buf, coverage)."""
    covered = list(covered)
    coverage = 0
    buf = bytearray()
    for i, ln in enumerate(lines):
        if len(covered) > 0 and covered[0][0] == i + 1:
            if covered[0][1]:
                buf += COVERED[0] + ln + COVERED[1]
                coverage += 1
            else:
                buf += UNCOVERED[0] + ln + UNCOVERED[1]
            covered = covered[1:]
        else:
            buf += ln + b"\n"
    return bytes(buf), coverage


def pages(file_set, names, sources):
    """cover.go:123-147 over fileSet's result, the files taken in id order (`names` lists them by id; the reference
    walks its map in no order).  sources: {name: bytes, or None for a file that cannot be read}.  Returns (body_off,
    bodies, coverage, bad_file) in the form sg_cover_pages returns them: the lowest unreadable file of the report
    stops everything (the reference returns parseFile's error at the first one it meets)."""
    bad = [f for f, name in enumerate(names) if name in file_set and sources.get(name) is None]
    body_off, coverage, bodies = [0], [], bytearray()
    for name in names:
        cov = 0
        if name in file_set and not bad:
            body, cov = render(parse_file(sources[name]), file_set[name])
            bodies += body
        body_off.append(len(bodies))
        coverage.append(cov)
    return body_off, bytes(bodies), coverage, (bad[0] if bad else None)


def common_prefix(files):
    """symbolize's prefix (cover.go:358-372) over the frames' files in frame order, for files that share their first
    byte (else the `prefix == ""` reset makes the reference's result depend on that order)."""
    prefix = ""
    for file in files:
        if prefix == "":
            prefix = file
        else:
            i = 0
            while i < len(prefix) and i < len(file):
                if prefix[i] != file[i]:
                    break
                i += 1
            prefix = prefix[:i]
    return prefix


def less(n1, n2):
    """templateFileArray.Less (cover.go:391-404)."""
    if len(n1) != 0 and len(n2) != 0:
        if n1[0] != "." and n2[0] == ".":
            return True
        if n1[0] == "." and n2[0] != ".":
            return False
    return n1 < n2


def files(file_set, prefix, sources):
    """cover.go:122-158: the sorted d.Files as [(Name, Body, Coverage), ...]; OSError for a file that cannot be
    read."""
    out = []
    for f, covered in file_set.items():
        if sources.get(f) is None:
            raise OSError(2, "open", f)  # :124-127
        body, coverage = render(parse_file(sources[f]), covered)
        if len(f) > len(prefix):
            f = f[len(prefix):]
        out.append((f, body, coverage))
    return sorted(out, key=functools.cmp_to_key(lambda a, b: -1 if less(a[0], b[0]) else 1 if less(b[0], a[0]) else 0))
