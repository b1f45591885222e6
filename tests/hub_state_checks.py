"""What tests/test_hub_state.py and tests/test_call_set_edges.py both check a GPU result with: the raw arrays of
sg_call_sets against the oracle's, a corpus against the oracle's, and the device form (sg_call_sets_dev) run
over guarded buffers with the values expected of clamped ranges."""
import numpy as np

from tests import hub_state_oracle as OR

U8, U32, U64 = np.uint8, np.uint32, np.uint64
FILL = 0xA5
UNK = 0xFFFFFFFF


def check_sets(ctx, progs, table=None, otable=None):
    from syzkaller_amd import hub as H

    st, lo, pos, ln, ids = H.call_sets(progs, table=table, ctx=ctx)
    est, elo, epos, eln, names = OR.call_sets(progs)
    assert np.array_equal(st, est) and np.array_equal(lo, elo)
    assert np.array_equal(pos, epos) and np.array_equal(ln, eln)
    eids = [UNK if otable is None else otable.get(x, UNK) for x in names]
    assert ids.tolist() == eids
    return st, lo, pos, ln, ids


def same_corpus(c, o):
    for g, e in zip(c.export(), o.export()):
        assert np.array_equal(g, e)
    assert c.count() == len(o.recs)


def to_dev(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).copy()).to("cuda")


def dev_run(ctx, tab, d_bytes_ptr, nbytes, offs, count, cap):
    """sg_call_sets_dev's five outputs, each with 16 guard bytes behind it that must stay as they were."""
    import torch

    from syzkaller_amd._lib import call

    sizes = (count, 8 * (count + 1), 8 * cap, 4 * cap, 4 * cap)
    bufs = [torch.full((m + 16,), FILL, dtype=torch.uint8, device="cuda") for m in sizes]
    torch.cuda.synchronize()
    call("sg_call_sets_dev", ctx.h, tab.h if tab else None, d_bytes_ptr, to_dev(offs).data_ptr(), count, nbytes,
         *[t.data_ptr() for t in bufs], cap)
    ctx.sync()
    outs = [t.cpu().numpy() for t in bufs]
    for o, m in zip(outs, sizes):
        assert (o[m:] == FILL).all()
    lo = outs[1][:sizes[1]].view(U64)
    nl = int(lo[-1])
    written = nl if nl <= cap else 0
    for o, w in zip(outs[2:], (8, 4, 4)):
        assert (o[w * written:] == FILL).all()
    return (outs[0][:count].tolist(), lo.tolist(), outs[2][:8 * written].view(U64).tolist(),
            outs[3][:4 * written].view(U32).tolist(), outs[4][:4 * written].view(U32).tolist())


def clamp_ranges(offs, nbytes):
    """The [start, end) the device form gives each program of garbage offsets: clamped to [start, nbytes]."""
    out = []
    for k in range(len(offs) - 1):
        a0 = min(int(offs[k]), nbytes)
        out.append((a0, min(max(int(offs[k + 1]), a0), nbytes)))
    return out


def dev_expect(view, ranges, tab):
    st, lo, pos, ln, ids = [], [0], [], [], []
    for a0, a1 in ranges:
        s, lines = OR.call_lines(view[a0:a1])
        st.append(s)
        for p, m in lines:
            pos.append(a0 + p)
            ln.append(m)
            ids.append(tab.get(view[a0 + p:a0 + p + m], UNK))
        lo.append(len(pos))
    return st, lo, pos, ln, ids
