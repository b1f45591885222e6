"""Regenerate tests/golden/symbolizer_kats.json from the reference.

Run where the reference checkout exists:
    python tests/golden/make_symbolizer_kats.py [/root/reference]

The table of TestParse (pkg/symbolizer/symbolizer_test.go:15-103): for each PC the text the stubbed addr2line
answers with and the frames symbolize must return, extracted from the Go source text as data.  The reference itself
never travels; only this data file does."""
import json
import os
import re
import sys

HERE = os.path.dirname(os.path.abspath(__file__))


def main():
    ref = sys.argv[1] if len(sys.argv) > 1 else "/root/reference"
    src = open(os.path.join(ref, "pkg", "symbolizer", "symbolizer_test.go")).read()
    table = src[src.index("addresses := []struct"):src.index("// Stub addr2line.")]
    tests = []
    # an entry: `{ 0x<pc>, "<line>\n" + ... , []Frame{...} | nil, },`
    for m in re.finditer(r"\{\s*(0x[0-9a-fA-F]+),\s*((?:\"(?:[^\"\\]|\\.)*\"\s*\+?\s*)+),\s*(nil|\[\]Frame\{.*?\n\t\t\t\}),\n\t\t\}",
                         table, flags=re.S):
        pc = int(m.group(1), 16)
        resp = "".join(json.loads(s) for s in re.findall(r"\"(?:[^\"\\]|\\.)*\"", m.group(2)))
        frames = []
        if m.group(3) != "nil":
            for f in re.finditer(r"Frame\{\s*PC:\s*(0x[0-9a-fA-F]+),\s*Func:\s*\"([^\"]*)\",\s*File:\s*\"([^\"]*)\",\s*"
                                 r"Line:\s*(\d+),\s*Inline:\s*(true|false),\s*\}", m.group(3)):
                frames.append({"pc": int(f.group(1), 16), "func": f.group(2), "file": f.group(3), "line": int(f.group(4)),
                               "inline": f.group(5) == "true"})
        tests.append({"pc": pc, "resp": resp, "frames": frames})
    assert len(tests) == 6 and sum(len(t["frames"]) for t in tests) == 5, len(tests)
    out = {"source": "pkg/symbolizer/symbolizer_test.go TestParse", "tests": tests}
    with open(os.path.join(HERE, "symbolizer_kats.json"), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
