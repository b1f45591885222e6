"""What tests/test_call_prios.py and tests/test_call_prios_edges.py share: the bit-exact comparison of the three
outputs with the oracle's, and arrays on the device."""
import numpy as np

U32, U64, I32, F32 = np.uint32, np.uint64, np.int32, np.float32


def has_gpu():
    try:
        import torch

        return torch.cuda.device_count() > 0
    except Exception:
        return False


def bits(a):
    return np.ascontiguousarray(a, F32).view(U32)


def same(got, exp, what):
    cnt, dyn, pr, run = exp
    gd, gp, gr = got
    assert np.array_equal(bits(gd), bits(dyn)), (what, "dynamic", int((bits(gd) != bits(dyn)).sum()))
    assert np.array_equal(bits(gp), bits(pr)), (what, "prios")
    assert gr.dtype == I32 and np.array_equal(gr, run), (what, "run")


def to_dev(a):
    import torch

    a = np.ascontiguousarray(a)
    if a.dtype == U64:
        return torch.from_numpy(a.view(np.int64).copy()).to("cuda")
    return torch.from_numpy(a.view(np.int32).copy()).to("cuda")
