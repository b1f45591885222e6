"""TEST INFRASTRUCTURE ONLY (the checker of sg_ipc_comps / sg_hints_replacers;
the product never imports it).

Pure-Python restatement, one Go statement per step, of
 - the comparison half of the executor output reader,
   pkg/ipc/ipc_linux.go:257-304, on a walk equivalent to
   oracle.ipc_oracle.read_out_coverage (:168-256);
 - prog/hints.go: shrinkExpand (:150-177), checkConstArg (:95-99),
   checkDataArg (:101-118), sliceToUint64 / pad (:188-205).
Pinned by the reference's own tables (tests/golden/hints_kats.json, from
prog/hints_test.go) and by ipc_oracle's statuses.
"""
from oracle.ipc_oracle import (BAD_CALLNUM, BAD_INDEX, COMP_CONST_MASK, COMP_SIZE8, COMP_SIZE_MASK, COMPS_SHORT,
                               COMPS_TYPE, COVER_SIZE, DOUBLE, NO_NCMD, OK, SHORT_HEADER, SIGNAL_SIZE)

M64 = (1 << 64) - 1
MAX_DATA_LENGTH = 100  # hints.go:36

# prog/rand.go:59-67
SPECIAL_INTS = [0, 1, 31, 32, 63, 64, 127, 128, 129, 255, 256, 257, 511, 512, 1023, 1024, 1025, 2047, 2048, 4095, 4096,
                (1 << 15) - 1, (1 << 15), (1 << 15) + 1, (1 << 16) - 1, (1 << 16), (1 << 16) + 1, (1 << 31) - 1,
                (1 << 31), (1 << 31) + 1, (1 << 32) - 1, (1 << 32), (1 << 32) + 1]
SPECIAL_INTS_SET = set(SPECIAL_INTS)  # hints.go:179-184


def read_comps(out, ncalls, call_nums=None):
    """ipc_linux.go:168-307 over one program's output words, keeping the
    comparisons.  Returns (status, comps) with comps[i] the list of the
    reader's AddComp(key, value) calls for call i, in its order; None while
    Go's Comps is nil (the call did not execute, or the reader returned
    before :304)."""
    out = [int(x) & 0xFFFFFFFF for x in out]
    pos = 0

    def read():  # readOut (:170-177)
        nonlocal pos
        if pos >= len(out):
            return None
        v = out[pos]
        pos += 1
        return v

    comps = [None] * ncalls
    seen = [False] * ncalls  # Signal != nil
    ncmd = read()
    if ncmd is None:  # :197-200
        return NO_NCMD, comps
    for _ in range(ncmd):
        hdr = [read() for _ in range(7)]  # :219
        if any(v is None for v in hdr):
            return SHORT_HEADER, comps
        idx, num, _errno, _fi, nsig, ncov, ncomps = hdr
        if idx >= ncalls:  # :223
            return BAD_INDEX, comps
        if call_nums is not None and int(call_nums[idx]) != num:  # :229
            return BAD_CALLNUM, comps
        if seen[idx]:  # :234
            return DOUBLE, comps
        if nsig > len(out) - pos:  # :241
            return SIGNAL_SIZE, comps
        seen[idx] = True  # :247
        pos += nsig
        if ncov > len(out) - pos:  # :250
            return COVER_SIZE, comps
        pos += ncov
        added = []  # :258 compMap, as its AddComp sequence
        for _ in range(ncomps):  # :259
            typ = read()  # :262
            if typ is None:
                return COMPS_SHORT, comps
            if typ > COMP_CONST_MASK | COMP_SIZE_MASK:  # :266
                return COMPS_TYPE, comps
            is_size8 = (typ & COMP_SIZE_MASK) == COMP_SIZE8  # :272
            is_const = (typ & COMP_CONST_MASK) != 0  # :273
            if is_size8:  # :276-283
                tmp1 = read()
                if tmp1 is None:
                    return COMPS_SHORT, comps
                tmp2 = read()
                if tmp2 is None:
                    return COMPS_SHORT, comps
                op1, op2 = tmp1, tmp2
            else:  # :285-288, readOut64 (:188-195)
                ws = []
                for _ in range(4):
                    x = read()
                    if x is None:
                        return COMPS_SHORT, comps
                    ws.append(x)
                op1 = ws[0] + (ws[1] << 32)
                op2 = ws[2] + (ws[3] << 32)
            if op1 == op2:  # :290
                continue
            added.append((op2, op1))  # :294
            if is_const:  # :295
                continue
            added.append((op1, op2))  # :302
        comps[idx] = added  # :304
    return OK, comps


def comps_batch(out, out_off, call_off, call_nums=None):
    """The batch contract of sg_ipc_comps: (status[], pair_lists[]) in record
    order; a program whose read failed contributes empty lists."""
    status, lists = [], []
    for p in range(len(out_off) - 1):
        r0, r1 = int(call_off[p]), int(call_off[p + 1])
        nums = None if call_nums is None else list(call_nums[r0:r1])
        st, comps = read_comps(out[int(out_off[p]):int(out_off[p + 1])], r1 - r0, nums)
        status.append(st)
        for c in comps:
            lists.append((c or []) if st == OK else [])
    return status, lists


def comp_map(added):
    """CompMap.AddComp (hints.go:41-46) over a sequence of calls."""
    m = {}
    for a1, a2 in added:
        m.setdefault(a1, set()).add(a2)
    return m


def shrink_expand(v, comp_map_, on_match=None):
    """hints.go:150-177.  on_match(mutant, new_v) sees every match that
    reaches :170, before the replacers set deduplicates them."""
    replacers = set()
    res = {}
    for size in (8, 16, 32):  # :155
        res[v & ((1 << size) - 1)] = size
        if v & (1 << (size - 1)) != 0:
            res[(v | ~((1 << size) - 1)) & M64] = size
    res[v] = 64  # :161
    for mutant, size in res.items():  # :163
        for new_v in comp_map_.get(mutant, ()):  # :164
            mask = ((1 << size) - 1) & M64  # :165
            new_hi = new_v & ~mask & M64  # :166
            if new_hi == 0 or (new_hi ^ (~mask & M64)) == 0:
                if (new_v & mask) not in SPECIAL_INTS_SET:  # :167
                    replacer = (v & ~mask & M64) | (new_v & mask)  # :170
                    replacers.add(replacer)
                    if on_match is not None:
                        on_match(mutant, new_v)
    return replacers


def check_const_arg(v, comp_map_):
    """hints.go:95-99: the set of the new ConstArg values."""
    return set(shrink_expand(v, comp_map_))


def slice_to_uint64(s):
    """hints.go:188-205."""
    padded = bytes(s[:8]) + b"\x00" * max(0, 8 - len(s))
    return int.from_bytes(padded, "little")


def check_data_arg(data, comp_map_):
    """hints.go:101-118 (for a DirIn argument): the set of the data strings
    the callback sees."""
    data = bytearray(data)
    res = set()
    for i in range(min(len(data), MAX_DATA_LENGTH)):  # :108
        original = bytes(data[i:i + 8])  # :109
        val = slice_to_uint64(data[i:])  # :110
        for replacer in shrink_expand(val, comp_map_):  # :111
            b = replacer.to_bytes(8, "little")  # :112
            n = min(8, len(data) - i)
            data[i:i + n] = b[:n]  # :113 copy() stops at the shorter slice
            res.add(bytes(data))  # :114
            data[i:i + n] = original[:n]  # :115
    return res
