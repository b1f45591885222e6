#!/usr/bin/env python3
"""Where the encoder's bytes go, on the host (no device): --programs texts of scripts/exp/db_compact_rate.py's corpus
through sg_deflate_host, against C zlib at levels 9 and 1 with and without Go's framing (a sync flush and the final
empty stored block: 9 bytes a record), and for the dynamic streams the split into header and payload, with the
payload priced again under true Huffman lengths over the same tokens.  Sizes only: nothing here is a time.  One
JSON line."""
import argparse
import heapq
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from hub_state_rate import make_corpus, make_names  # noqa: E402
from syzkaller_amd import db as D  # noqa: E402
from tests import db_cases as K  # noqa: E402
from tests import db_write_cases as W  # noqa: E402


def huffman_bits(freqs):
    """The payload bits of an optimal prefix code (not length-limited: a lower bound for DEFLATE's 15)."""
    h = [f for f in freqs if f]
    if len(h) < 2:
        return sum(h)
    heapq.heapify(h)
    total = 0
    while len(h) > 1:
        a, b = heapq.heappop(h), heapq.heappop(h)
        total += a + b
        heapq.heappush(h, a + b)
    return total


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--programs", type=int, default=3000)
    ap.add_argument("--median", type=float, default=512.0)
    ap.add_argument("--sigma", type=float, default=1.0)
    a = ap.parse_args()
    progs = make_corpus(a.programs, make_names(), a.median, a.sigma, 7)
    off, out = D.deflate_host(progs)
    blob, o = out.tobytes(), off.tolist()
    res = {"metric": "db_deflate_split", "programs": a.programs, "text_bytes": sum(map(len, progs)), "ours": o[-1]}
    for level in (9, 1):
        res["go_framing_level%d" % level] = sum(len(K.go_stream(p, level)) for p in progs)
        res["raw_level%d" % level] = sum(len(K.raw_stream(p, level)) for p in progs)
    forms, bits, header, payload, optimal = [0, 0, 0], 0, 0, 0, 0
    for k in range(len(progs)):
        s = blob[o[k]:o[k + 1]]
        forms[W.form_of(s)] += 1
        if W.form_of(s) != W.DYNAMIC:
            continue
        blocks, toks, end = W.read_stream(s)
        _, ll, dl = blocks[0]
        lf, df, extra = [0] * 286, [0] * 30, 0
        for t in toks:
            if isinstance(t, tuple):
                ls, _, le = K.length_symbol(t[0])
                ds, _, de = K.dist_symbol(t[1])
                lf[ls] += 1
                df[ds] += 1
                extra += le + de
            else:
                lf[t] += 1
        lf[256] += 1
        pay = sum(f * ln for f, ln in zip(lf, ll)) + sum(f * ln for f, ln in zip(df, dl)) + extra
        bits += 8 * len(s)
        payload += pay
        header += end - pay
        optimal += huffman_bits(lf) + huffman_bits(df) + extra
    res.update({"forms": {"stored": forms[0], "fixed": forms[1], "dynamic": forms[2]}, "dynamic_bits": bits,
                "dynamic_header_bits": header, "dynamic_payload_bits": payload,
                "dynamic_payload_bits_huffman_lengths": optimal})
    print(json.dumps(res))


if __name__ == "__main__":
    main()
