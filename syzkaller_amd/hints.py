"""Comparison hints on the GPU: the executor's own comparison branch over raw
KCOV_TRACE_CMP buffers (executor/executor.h:379-387), the executor's
comparisons into per-call CompMaps (pkg/ipc/ipc_linux.go:257-304) and the
matching of argument values against them (prog/hints.go:95-177), over batches.

comps_pairs joins the two ends at full operand width, and hints_from_kcov /
HintSeed run all three stages in one call for a hint seed's raw buffers.

A CompMap travels as the reader's AddComp sequence: an array of {key, value}
pairs with one offset per call.  Cloning the program, replaceArg and validate
stay with the caller; what comes back is, per argument value, the replacers
that shrinkExpand yields, ascending.
"""
import ctypes

import numpy as np

from ._lib import call
from .cover import U64, _ctx, _p32, _p64, _u32, _u64

MAX_DATA_LENGTH = 100  # hints.go:36
EXEC_COMPS_FAST_CAP = 4096  # include/syzsig.h SG_EXEC_COMPS_FAST_CAP: a call's distinct records on the fast shape


def exec_comps(recs, call_off, ctx=None, words=True):
    """handle_completion's flag_collect_comps branch (executor.h:379-387) over a
    batch of raw KCOV_TRACE_CMP buffers: recs u64[n, 4] {type, arg1, arg2, pc},
    call c's records recs[call_off[c]:call_off[c + 1]].  Returns (comp_off,
    comps u64[m, 3], word_off, words): call c's sorted, deduplicated
    comparisons {type, arg1', arg2'} (operands as write() extends them) are
    comps[comp_off[c]:comp_off[c + 1]], the u32 words write() emits for them
    words[word_off[c]:word_off[c + 1]] (the writer's widths); word_off and
    words are None with words=False."""
    r, co = _u64(recs), _u64(call_off)
    ncalls = co.size - 1
    nrecs = int(co[-1])
    assert r.size == 4 * nrecs
    cpo = np.empty(ncalls + 1, dtype=U64)
    comps = np.empty((max(nrecs, 1), 3), dtype=U64)
    wo = np.empty(ncalls + 1, dtype=U64) if words else None
    w = np.empty(max(5 * nrecs, 1), dtype=np.uint32) if words else None
    call("sg_exec_comps", _ctx(ctx).h, _p64(r), _p64(co), ncalls, _p64(cpo), _p64(comps), nrecs,
         _p64(wo) if words else None, _p32(w) if words else None, 5 * nrecs if words else 0)
    if not words:
        return cpo, comps[: int(cpo[-1])], None, None
    return cpo, comps[: int(cpo[-1])], wo, w[: int(wo[-1])]


def ipc_comps(out, out_off, call_off, call_nums=None, ctx=None):
    """The comparison half of readOutCoverage over a batch of program output
    regions (arguments as cover.ipc_parse).  Returns (status int32[nprog],
    pairs u64[n, 2], pair_off u64[nrec + 1]): call r's AddComp(key, value)
    calls, in the reader's order, are pairs[pair_off[r]:pair_off[r + 1]]."""
    w, oo, co = _u32(out), _u64(out_off), _u64(call_off)
    nprog = oo.size - 1
    assert co.size == nprog + 1
    nrec = int(co[-1])
    nums = None if call_nums is None else _u32(call_nums)
    assert nums is None or nums.size == nrec
    status = np.empty(max(nprog, 1), dtype=np.int32)
    po = np.empty(nrec + 1, dtype=U64)
    cap = 2 * ((w.size + 2) // 3)  # a comparison is >= 3 words and yields <= 2 pairs
    pairs = np.empty((max(cap, 1), 2), dtype=U64)
    call("sg_ipc_comps", _ctx(ctx).h, _p32(w), _p64(oo), _p64(co), _p32(nums) if nums is not None else None, nprog,
         status.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), _p64(po), _p64(pairs), cap)
    return status[:nprog], pairs[: int(po[-1])], po


def comp_maps(pairs, pair_off):
    """ipc.GetCompMaps: one CompMap (dict key -> set of values) per call."""
    pairs = _u64(pairs)
    pairs = pairs.reshape(pairs.size // 2, 2)
    maps = []
    for r in range(len(pair_off) - 1):
        m = {}
        for k, v in pairs[int(pair_off[r]):int(pair_off[r + 1])].tolist():
            m.setdefault(k, set()).add(v)
        maps.append(m)
    return maps


def shrink_expand_batch(pairs, pair_off, vals, val_off, ctx=None, cap=None):
    """shrinkExpand over a batch: record r's CompMap is its pairs, its argument
    values vals[val_off[r]:val_off[r + 1]].  Returns (reps, rep_off): value
    slot i's distinct replacers, ascending, are reps[rep_off[i]:rep_off[i + 1]]."""
    p, po, v, vo = _u64(pairs), _u64(pair_off), _u64(vals), _u64(val_off)
    nrec = po.size - 1
    assert vo.size == nrec + 1 and p.size == 2 * int(po[-1]) and v.size == int(vo[-1])
    ro = np.empty(v.size + 1, dtype=U64)
    cap = max(1024, 4 * v.size) if cap is None else int(cap)
    for _ in range(2):  # a second call when the first capacity was short
        reps = np.empty(max(cap, 1), dtype=U64)
        call("sg_hints_replacers", _ctx(ctx).h, _p64(po), _p64(p), nrec, _p64(vo), _p64(v), _p64(ro), _p64(reps), cap)
        if int(ro[-1]) <= cap:
            break
        cap = int(ro[-1])
    return reps[: int(ro[-1])], ro


def _pi32(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))


def comps_pairs(comp_off, comps, ctx=None):
    """The reader's loop body (ipc_linux.go:290-302) at full operand width over
    the triples exec_comps returns.  Returns (status int32[ncalls], pairs
    u64[n, 2], pair_off u64[ncalls + 1]): call c's AddComp(key, value) calls, in
    the reader's order, are pairs[pair_off[c]:pair_off[c + 1]]; a call holding
    a type above 7 has status SG_IPC_COMPS_TYPE and no pairs."""
    co, c = _u64(comp_off), _u64(comps)
    ncalls = co.size - 1
    ncomps = int(co[-1])
    assert c.size == 3 * ncomps
    status = np.empty(max(ncalls, 1), dtype=np.int32)
    po = np.empty(ncalls + 1, dtype=U64)
    cap = 2 * ncomps  # a comparison yields at most 2 pairs
    pairs = np.empty((max(cap, 1), 2), dtype=U64)
    call("sg_comps_pairs", _ctx(ctx).h, _p64(co), _p64(c), ncalls, _pi32(status), _p64(po), _p64(pairs), cap)
    return status[:ncalls], pairs[: int(po[-1])], po


def hints_from_kcov(recs, call_off, vals, val_off, ctx=None, cap=None):
    """Raw KCOV_TRACE_CMP buffers and argument values to replacers in one call:
    exec_comps, comps_pairs and shrink_expand_batch with call c as record c,
    the triples and pairs staying on the device.  Returns (status int32[ncalls],
    reps, rep_off): value slot i's distinct replacers, ascending, are
    reps[rep_off[i]:rep_off[i + 1]]; a call whose status is SG_IPC_COMPS_TYPE
    has an empty CompMap."""
    r, co, v, vo = _u64(recs), _u64(call_off), _u64(vals), _u64(val_off)
    ncalls = co.size - 1
    assert vo.size == ncalls + 1 and r.size == 4 * int(co[-1]) and v.size == int(vo[-1])
    status = np.empty(max(ncalls, 1), dtype=np.int32)
    ro = np.empty(v.size + 1, dtype=U64)
    cap = max(1024, 4 * v.size) if cap is None else int(cap)
    for _ in range(2):  # a second call when the first capacity was short
        reps = np.empty(max(cap, 1), dtype=U64)
        call("sg_hints_from_kcov", _ctx(ctx).h, _p64(r), _p64(co), ncalls, _p64(vo), _p64(v), _pi32(status), _p64(ro),
             _p64(reps), cap)
        if int(ro[-1]) <= cap:
            break
        cap = int(ro[-1])
    return status[:ncalls], reps[: int(ro[-1])], ro


def HintSeed(calls, ctx=None):
    """The data half of MutateWithHints (prog/hints.go:50-59) for one hint seed
    (syz-fuzzer/fuzzer.go:627-643).  calls: one (recs u64[n, 4], args) per call,
    the call's raw KCOV_TRACE_CMP records and its arguments, each an int (a
    ConstArg.Val) or bytes (the Data of a DirIn / DirInOut DataArg).  One
    hints_from_kcov call.  Returns per call a list with, per argument, the set
    of replacer ints (checkConstArg) or of mutated data strings (checkDataArg)."""
    recs, call_off, vals, val_off = [], [0], [], [0]
    for r, args in calls:
        r = _u64(r)
        assert r.size % 4 == 0
        recs.append(r)
        call_off.append(call_off[-1] + r.size // 4)
        for a in args:
            if isinstance(a, (bytes, bytearray, memoryview)):
                data = bytes(a)
                vals += [slice_to_uint64(data[i:]) for i in range(min(len(data), MAX_DATA_LENGTH))]
            else:
                vals.append(int(a))
        val_off.append(len(vals))
    recs = np.concatenate(recs) if recs else np.zeros(0, dtype=U64)
    _, reps, ro = hints_from_kcov(recs, call_off, np.array(vals, dtype=U64), val_off, ctx=ctx)
    res, slot = [], 0
    for _, args in calls:
        out = []
        for a in args:
            if isinstance(a, (bytes, bytearray, memoryview)):
                data = bytes(a)
                got = set()
                for i in range(min(len(data), MAX_DATA_LENGTH)):
                    k = min(8, len(data) - i)
                    for rep in reps[int(ro[slot]):int(ro[slot + 1])].tolist():
                        got.add(data[:i] + rep.to_bytes(8, "little")[:k] + data[i + k:])
                    slot += 1
            else:
                got = set(reps[int(ro[slot]):int(ro[slot + 1])].tolist())
                slot += 1
            out.append(got)
        res.append(out)
    return res


def _pairs_of(compmap):
    """A CompMap given as a dict, laid out as its sorted (key, value) items."""
    items = sorted((int(k), int(v)) for k, vs in compmap.items() for v in vs)
    return np.array(items, dtype=U64).reshape(len(items), 2)


def _one(vals, compmap, ctx):
    pairs = _pairs_of(compmap)
    vals = _u64(vals)
    reps, ro = shrink_expand_batch(pairs, [0, pairs.shape[0]], vals, [0, vals.size], ctx=ctx)
    return reps, ro


def ShrinkExpand(v, compmap, ctx=None):
    """prog/hints.go:150-177 shrinkExpand: the set of replacers of v."""
    reps, _ = _one([v], compmap, ctx)
    return set(reps.tolist())


def CheckConstArg(v, compmap, ctx=None):
    """prog/hints.go:95-99 checkConstArg: the values of the new ConstArgs."""
    return ShrinkExpand(v, compmap, ctx)


def slice_to_uint64(s):
    """prog/hints.go:188-205 sliceToUint64: little endian, zero padded."""
    return int.from_bytes(bytes(s[:8]).ljust(8, b"\x00"), "little")


def CheckDataArg(data, compmap, ctx=None):
    """prog/hints.go:101-118 checkDataArg for a userspace -> kernel argument:
    the set of data strings its callback sees.  One value slot per window
    Data[i:], i < min(len, 100); each replacer goes back little endian,
    truncated to the remaining length."""
    data = bytes(data)
    n = min(len(data), MAX_DATA_LENGTH)
    if n == 0:
        return set()
    reps, ro = _one([slice_to_uint64(data[i:]) for i in range(n)], compmap, ctx)
    res = set()
    for i in range(n):
        k = min(8, len(data) - i)
        for rep in reps[int(ro[i]):int(ro[i + 1])].tolist():
            res.add(data[:i] + rep.to_bytes(8, "little")[:k] + data[i + k:])
    return res
