"""TEST INFRASTRUCTURE ONLY: the checker of sg_exec_cover.

The flag_collect_cover branch of handle_completion (executor/executor.h:402-415)
restated, one statement per reference step.  The branch is inline in
handle_completion, so no compiled-reference fixture pins it: the parity rests
on this restatement alone.
"""
import numpy as np

U32, U64 = np.uint32, np.uint64


def call_cover(pcs, dedup=True):
    """One call's Cover words from its KCOV buffer (th->cover_data, u64 PCs)."""
    data = np.asarray(pcs, dtype=U64).reshape(-1).copy()
    cover_size = data.size                                      # :404
    if dedup:                                                   # :405 flag_dedup_cover
        data = np.sort(data, kind="stable")                     # :408 std::sort, unsigned 64-bit
        keep = np.ones(cover_size, dtype=bool)
        keep[1:] = data[1:] != data[:-1]                        # :409 std::unique: one of every run of equals
        data = data[keep]
        cover_size = data.size
    return (data[:cover_size] & U64(0xFFFFFFFF)).astype(U32)    # :411-414 (uint32_t)th->cover_data[i]


def batch(pcs, call_off, dedup=True):
    """The batch contract of sg_exec_cover: (cov u32, cov_off u64[ncalls + 1])."""
    pcs = np.asarray(pcs, dtype=U64).reshape(-1)
    off = np.asarray(call_off, dtype=U64).reshape(-1)
    lists = [call_cover(pcs[int(off[c]):int(off[c + 1])], dedup) for c in range(off.size - 1)]
    cov_off = np.zeros(off.size, dtype=U64)
    if lists:
        cov_off[1:] = np.cumsum([x.size for x in lists])
    cov = np.concatenate(lists) if lists else np.zeros(0, dtype=U32)
    return cov.astype(U32), cov_off


def to_arrays(calls):
    """A list of per-call PC sequences -> (pcs u64, call_off u64)."""
    off = np.zeros(len(calls) + 1, dtype=U64)
    if calls:
        off[1:] = np.cumsum([len(c) for c in calls])
    flat = [np.asarray(c, dtype=U64).reshape(-1) for c in calls if len(c)]
    return (np.concatenate(flat) if flat else np.zeros(0, dtype=U64)), off
