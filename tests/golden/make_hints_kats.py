"""Regenerate tests/golden/hints_kats.json from the reference.

Run where a checkout of the reference exists:
    python tests/golden/make_hints_kats.py REFERENCE_CHECKOUT

The known-answer tables of prog/hints_test.go -- TestHintsCheckConstArg
(:28-64, 3 cases), TestHintsCheckDataArg (:68-179, 5 cases) and
TestHintsShrinkExpand (:181-338, 9 cases) -- and the specialInts of
prog/rand.go:59-67, extracted from the Go source text as data.  Numbers are
kept as hex strings (they are u64), byte strings as hex.  The reference
itself never travels; only the JSON does.
"""
import json
import os
import re
import sys

HERE = os.path.dirname(os.path.abspath(__file__))


def _strip_comments(src):
    return re.sub(r"//[^\n]*", "", src)


def _blocks(s):
    """The top-level {...} blocks of s (their insides), quotes respected."""
    out, depth, start, i, n = [], 0, 0, 0, len(s)
    while i < n:
        c = s[i]
        if c == '"':
            i += 1
            while s[i] != '"':
                i += 2 if s[i] == "\\" else 1
        elif c == "{":
            if depth == 0:
                start = i + 1
            depth += 1
        elif c == "}":
            depth -= 1
            if depth == 0:
                out.append(s[start:i])
        i += 1
    return out


def _gobytes(lit):
    """A Go interpreted string literal of \\xHH escapes and plain ASCII."""
    out, i = bytearray(), 0
    while i < len(lit):
        if lit[i] == "\\":
            assert lit[i + 1] == "x", lit
            out.append(int(lit[i + 2:i + 4], 16))
            i += 4
        else:
            out.append(ord(lit[i]))
            i += 1
    return bytes(out)


def _num(x):
    return "0x%x" % int(x, 0)


def _compmap(body):
    """CompMap{k: uint64Set{v: true, ...}, ...} -> [[k, [v, ...]], ...]."""
    return [[_num(k), [_num(v) for v in re.findall(r"(0x[0-9a-fA-F]+|\d+)\s*:\s*true", vs)]]
            for k, vs in re.findall(r"(0x[0-9a-fA-F]+|\d+)\s*:\s*uint64Set\{([^}]*)\}", body)]


def parse_tables(ref):
    src = _strip_comments(open(os.path.join(ref, "prog/hints_test.go")).read())
    tests = {}
    for body in re.split(r"\nfunc ", src):
        m = re.match(r"(TestHints\w+)\(", body)
        if not m:
            continue
        table = body[body.index("var tests = "):]
        table = _blocks(table[table.index("{"):])[0]
        cases = []
        for e in _blocks(table):
            name = re.match(r'\s*"([^"]*)"\s*,', e)
            rest = e[name.end():]
            cm = re.search(r"CompMap\{", rest)
            comps_body = _blocks(rest[cm.start():])[0]
            after = rest[cm.end() + len(comps_body) + 1:]
            case = {"name": name.group(1), "comps": _compmap(comps_body)}
            sm = re.match(r'\s*"((?:[^"\\]|\\.)*)"\s*,', rest)
            if sm:  # a DataArgTest: in and res are byte strings
                case["in"] = _gobytes(sm.group(1)).hex()
                case["res"] = sorted(_gobytes(x).hex() for x in re.findall(r'"((?:[^"\\]|\\.)*)"\s*:\s*true', after))
            else:
                case["in"] = _num(re.match(r"\s*(0x[0-9a-fA-F]+|\d+)\s*,", rest).group(1))
                res = _blocks(after[after.index("uint64Set"):])[0]
                case["res"] = [_num(v) for v in re.findall(r"(0x[0-9a-fA-F]+|\d+)\s*:\s*true", res)]
            cases.append(case)
        tests[m.group(1)] = cases
    return tests


def parse_special_ints(ref):
    src = _strip_comments(open(os.path.join(ref, "prog/rand.go")).read())
    body = re.search(r"var specialInts = \[\]uint64\{(.*?)\n\}", src, re.S).group(1)
    vals = []
    for term in body.split(","):
        term = term.strip()
        if not term:
            continue
        m = re.fullmatch(r"\(1 << (\d+)\)(?: ([+-]) (\d+))?", term)
        if m:
            v = 1 << int(m.group(1))
            if m.group(2):
                v += int(m.group(3)) if m.group(2) == "+" else -int(m.group(3))
        else:
            v = int(term, 0)
        vals.append(v)
    return vals


def main():
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    ref = sys.argv[1]
    tests = parse_tables(ref)
    assert [len(tests[k]) for k in ("TestHintsCheckConstArg", "TestHintsCheckDataArg", "TestHintsShrinkExpand")] == [
        3, 5, 9], {k: len(v) for k, v in tests.items()}
    special = parse_special_ints(ref)
    assert len(special) == 33
    with open(os.path.join(HERE, "hints_kats.json"), "w") as f:
        f.write('{"source": "prog/hints_test.go, prog/rand.go:59-67",\n "special_ints": %s,\n "tests": {\n' %
                json.dumps(["0x%x" % v for v in special]))
        names = list(tests)
        for i, name in enumerate(names):
            f.write(" %s: [\n" % json.dumps(name))
            f.write(",\n".join("  " + json.dumps(c) for c in tests[name]))
            f.write("]" + ("," if i < len(names) - 1 else "") + "\n")
        f.write("}}\n")


if __name__ == "__main__":
    main()
