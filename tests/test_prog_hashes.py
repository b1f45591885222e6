"""Program identities (pkg/hash; syz-manager/manager.go:777-793, :913, :994-1069; syz-fuzzer/fuzzer.go:480-484;
syz-hub/state/state.go:91-101): sg_prog_hashes*, sg_sigset_*, sg_hub_sync.  On the CPU the boundary, every
rejected argument, the no-device result, the oracle against the FIPS vectors and the conditions the cases
rely on.  On the GPU every hash, flag, export and diff bit-exact against the oracle
(tests/prog_hashes_oracle.py: hashlib.sha1 and the Go lines over a dict)."""
import os
import re
import subprocess

import numpy as np
import pytest

from tests import prog_hashes_cases as K
from tests import prog_hashes_oracle as OR
from tests.conftest import ROOT

U8, U64 = np.uint8, np.uint64
NAMES = ("sg_prog_hashes", "sg_prog_hashes_dev", "sg_sigset_create", "sg_sigset_destroy", "sg_sigset_clear",
         "sg_sigset_count", "sg_sigset_export", "sg_sigset_contains", "sg_sigset_add_new", "sg_sigset_add_progs",
         "sg_hub_sync")
FILL = 0xA5
LONG = K.SHA1_LONG


def _has_gpu():
    try:
        import torch

        return torch.cuda.device_count() > 0
    except Exception:
        return False


# ---- CPU: the boundary ---------------------------------------------------------
def test_header_binding_and_library():
    import syzkaller_amd
    from syzkaller_amd import _lib
    from syzkaller_amd import corpus as P

    text = open(os.path.join(ROOT, "include", "syzsig.h")).read()
    for cite in ("manager.go:994-1069", ":1021-1025", ":1053-1056", ":1057-1069", ":777-781", ":788-793", ":913",
                 "fuzzer.go:480-484", "manager.go:1053-1069", ":1057-1061", ":1063-1069", "state.go:91-101"):
        assert cite in text, cite
    assert "not a parity claim" in text and "no tombstones" in text and "64-bit bit count" in text
    assert re.search(r"#define SG_SIG_BYTES 20\b", text) and re.search(r"#define SG_SHA1_LONG %d\b" % LONG, text)
    src = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r" T (sg_[a-z0-9_]+)$", out, flags=re.M))
    for name in NAMES:
        assert re.search(r"\b(int|void) %s\s*\(" % name, src), name
        assert name in _lib.SIGNATURES and name in exported, name
    for name in ("Hash", "String", "prog_hashes", "SigSet", "HubSync", "VerifyKeys"):
        assert callable(getattr(P, name)) and getattr(syzkaller_amd, name) is getattr(P, name)
    for m in ("add_new", "add_progs", "contains", "count", "export", "clear", "__len__"):
        assert callable(getattr(P.SigSet, m)), m
    assert P.SIG_BYTES == 20 and P.SHA1_LONG == LONG
    # the hash kernels use no float and no atomics
    unit = open(os.path.join(ROOT, "syzkaller_amd", "csrc", "sg_prog_hash.hip")).read().split("#include", 1)[1]
    assert "atomic" not in unit and "float" not in unit and "double" not in unit


def _fake_set(count):
    """A readable block that passes for an sg_sigset up to the checks: a null context and a count (the set's
    second field: sg_sigset.hip asserts the offset)."""
    block = np.zeros(1 << 12, U64)
    block[1] = count
    return block


def test_invalid_arguments_are_einval():
    """Every check the calls make before they touch the context: a context, or a set, that is only a readable
    block of memory is enough."""
    from syzkaller_amd import _lib
    from syzkaller_amd.cover import _p8, _p64

    lib, E = _lib.lib, _lib.SG_EINVAL
    block = np.zeros(1 << 16, U8)
    fake = block.ctypes.data_as(_lib.c_void_p)  # never used: each case below returns first
    data = np.arange(40, dtype=U8)
    off = np.array([0, 10, 10, 40], U64)
    bad0, dec = off.copy(), off.copy()
    bad0[0] = 1
    dec[2] = 9
    sigs, hexs, flags = np.full(60, FILL, U8), np.full(120, FILL, U8), np.full(3, FILL, U8)
    nd = _lib.c_size_t(77)
    ref = _lib.ctypes.byref(nd)
    assert lib.sg_prog_hashes(None, _p8(data), _p64(off), 3, _p8(sigs), _p8(hexs)) == E
    assert lib.sg_prog_hashes(fake, _p8(data), None, 3, _p8(sigs), _p8(hexs)) == E
    assert lib.sg_prog_hashes(fake, None, _p64(off), 3, _p8(sigs), _p8(hexs)) == E
    assert lib.sg_prog_hashes(fake, _p8(data), _p64(bad0), 3, _p8(sigs), _p8(hexs)) == E
    assert lib.sg_prog_hashes(fake, _p8(data), _p64(dec), 3, _p8(sigs), _p8(hexs)) == E
    assert lib.sg_last_error()
    assert lib.sg_prog_hashes_dev(None, fake, fake, 1, 1, fake) == E
    assert lib.sg_prog_hashes_dev(fake, fake, None, 1, 1, fake) == E
    assert lib.sg_prog_hashes_dev(fake, None, fake, 1, 1, fake) == E
    assert lib.sg_prog_hashes_dev(fake, fake, fake, 1, 1, None) == E
    assert lib.sg_prog_hashes_dev(fake, fake, fake, 1 << 32, 1, fake) == E
    out = _lib.c_void_p()
    assert lib.sg_sigset_create(None, 0, _lib.ctypes.byref(out)) == E
    assert lib.sg_sigset_create(fake, 0, None) == E
    assert lib.sg_sigset_create(fake, 1 << 31, _lib.ctypes.byref(out)) == E and not out.value
    assert lib.sg_sigset_clear(None) == E
    assert lib.sg_sigset_count(None, _p64(np.zeros(1, U64))) == E and lib.sg_sigset_count(fake, None) == E
    assert lib.sg_sigset_export(None, _p8(sigs), 3, ref) == E
    assert lib.sg_sigset_export(fake, _p8(sigs), 3, None) == E
    assert lib.sg_sigset_export(fake, None, 3, ref) == E
    for fn in (lib.sg_sigset_contains, lib.sg_sigset_add_new):
        assert fn(None, _p8(sigs), 3, _p8(flags)) == E
        assert fn(fake, None, 3, _p8(flags)) == E
        assert fn(fake, _p8(sigs), 3, None) == E
        assert fn(fake, _p8(sigs), 1 << 31, _p8(flags)) == E
    full = _fake_set((1 << 31) - 2).ctypes.data_as(_lib.c_void_p)
    assert lib.sg_sigset_add_new(full, _p8(sigs), 3, _p8(flags)) == E               # the set would reach 2^31
    assert lib.sg_sigset_add_progs(full, _p8(data), _p64(off), 3, _p8(sigs), _p8(flags)) == E
    assert lib.sg_sigset_add_progs(None, _p8(data), _p64(off), 3, _p8(sigs), _p8(flags)) == E
    assert lib.sg_sigset_add_progs(fake, _p8(data), None, 3, _p8(sigs), _p8(flags)) == E
    assert lib.sg_sigset_add_progs(fake, None, _p64(off), 3, _p8(sigs), _p8(flags)) == E
    assert lib.sg_sigset_add_progs(fake, _p8(data), _p64(off), 3, _p8(sigs), None) == E
    assert lib.sg_sigset_add_progs(fake, _p8(data), _p64(bad0), 3, _p8(sigs), _p8(flags)) == E
    assert lib.sg_sigset_add_progs(fake, _p8(data), _p64(dec), 3, _p8(sigs), _p8(flags)) == E
    dels = np.full(100, FILL, U8)
    args = (_p8(data), _p64(off), 3, _p8(sigs), _p8(flags), _p8(dels), 5, ref)
    assert lib.sg_hub_sync(None, *args) == E
    assert lib.sg_hub_sync(fake, None, *args[1:]) == E
    assert lib.sg_hub_sync(fake, args[0], None, *args[2:]) == E
    assert lib.sg_hub_sync(fake, args[0], _p64(bad0), *args[2:]) == E
    assert lib.sg_hub_sync(fake, args[0], _p64(dec), *args[2:]) == E
    assert lib.sg_hub_sync(fake, *args[:4], None, *args[5:]) == E                   # add
    assert lib.sg_hub_sync(fake, *args[:5], None, 5, ref) == E                      # del_sigs with del_cap > 0
    assert lib.sg_hub_sync(fake, *args[:7], None) == E                              # ndel
    held = _fake_set(6).ctypes.data_as(_lib.c_void_p)
    assert lib.sg_hub_sync(held, *args) == E                                        # del_cap 5 below the count 6
    assert b"del_cap" in lib.sg_last_error()
    lib.sg_sigset_destroy(None)
    assert (sigs == FILL).all() and (hexs == FILL).all() and (flags == FILL).all() and (dels == FILL).all()
    assert nd.value == 77


@pytest.mark.skipif(_has_gpu(), reason="checks the no-GPU failure path")
def test_no_device_is_enodev():
    """Valid arguments and no device: the first thing the call asks of the context fails."""
    from syzkaller_amd import _lib
    from syzkaller_amd.cover import _p8, _p64

    block = np.zeros(1 << 16, U8)  # a zeroed sg_ctx: device 0, an unlocked mutex
    fake = block.ctypes.data_as(_lib.c_void_p)
    data, off, sigs = np.arange(40, dtype=U8), np.array([0, 10, 40], U64), np.zeros(40, U8)
    assert _lib.lib.sg_prog_hashes(fake, _p8(data), _p64(off), 2, _p8(sigs), None) == _lib.SG_ENODEV
    assert _lib.lib.sg_prog_hashes_dev(fake, fake, fake, 2, 40, fake) == _lib.SG_ENODEV
    out = _lib.c_void_p()
    assert _lib.lib.sg_sigset_create(fake, 0, _lib.ctypes.byref(out)) == _lib.SG_ENODEV and not out.value


# ---- CPU: the oracle and the cases ---------------------------------------------
def test_oracle_fips_vectors():
    for msg, digest in OR.VECTORS:
        assert OR.String(msg) == digest and OR.Hash(msg).hex() == digest
    assert len(OR.VECTORS[2][0]) == 56 and len(OR.VECTORS[3][0]) == 10 ** 6
    assert OR.Hash(b"ab", b"", b"c") == OR.Hash(b"abc") and OR.Hash(b"a", b"b") == OR.Hash(b"a" + b"b")


def test_oracle_sets():
    s = OR.OSigSet()
    a, b, c = (bytes([k]) * 20 for k in (1, 2, 3))
    assert s.add_new([a, b, a]).tolist() == [True, True, False] and s.count() == 2
    assert s.add_new([c, a]).tolist() == [True, False] and s.export().tobytes() == a + b + c
    assert s.contains([c, bytes(20)]).tolist() == [True, False]
    hub = OR.OSigSet()
    progs = [b"x", b"y", b"x", b"z"]
    add, dels = OR.hub_sync(hub, progs)
    assert add.tolist() == [0, 1, 3] and dels == [] and hub.count() == 3
    add, dels = OR.hub_sync(hub, [b"z", b"w"])
    assert add.tolist() == [1] and dels == [OR.String(b"x"), OR.String(b"y")]
    assert hub.export().tobytes() == OR.Hash(b"z") + OR.Hash(b"w")
    add, dels = OR.hub_sync(hub, [])
    assert add.size == 0 and len(dels) == 2 and hub.count() == 0


def test_case_conditions():
    progs, marks = K.padding_batch()
    starts = np.concatenate([[0], np.cumsum([len(p) for p in progs])])
    assert sorted({(a, n) for _, a, n in marks}) == [(a, n) for a in range(4) for n in range(131)]
    for i, a, n in marks:
        assert starts[i] % 4 == a and len(progs[i]) == n and len(progs[i - 1]) >= 1
    for n in (55, 56, 63, 64, 65, 119, 120, 127, 128):
        assert n in K.PAD_LENGTHS
    for n in K.WAVE_SIZES:
        lens = [len(p) for p in K.mixed(n, n)]
        assert len(lens) == n and max(lens) <= 300
        if n >= 63:
            assert any(lens[k:k + 3] == [0, 0, 0] for k in range(n)) and max(lens) > 128
    lp, nlong = K.long_batch()
    assert [len(p) for p in lp[:3]] == [LONG - 1, LONG, LONG + 1] and nlong == 2
    assert sum(len(p) <= 300 for p in lp) == 200
    for nshared in (8, 19):
        s = K.shared_prefix(nshared, 40, nshared)
        assert len({r.tobytes() for r in s}) == 40 and len({r[:nshared].tobytes() for r in s}) == 1
        assert len({r[:nshared + 1].tobytes() for r in s}) > 1
    h = K.one_home(300, 5)
    assert len({r.tobytes() for r in h}) == 300 and len({r[:4].tobytes() for r in h}) == 300
    for bits in range(6, 17):
        assert len({K.home_slot(r, 1 << bits) for r in h}) == 1, bits
    assert 300 > 64  # a probe chain longer than a wave
    fixed = K.hub_steps_fixed()
    assert fixed[1] == fixed[0] and fixed[3] == []
    assert set(fixed[0]) - set(fixed[2]) and set(fixed[2]) - set(fixed[0]) and len(set(fixed[2])) < len(fixed[2])
    steps = K.hub_steps_random()
    assert len(steps) == 20 and [] in steps
    assert any(len(set(s)) < len(s) for s in steps)
    assert all(set(a) - set(b) for a, b in zip(steps, steps[1:]) if a)  # every step removes something


# ---- GPU ----------------------------------------------------------------------
def _hashes(ctx, progs):
    from syzkaller_amd import corpus as P

    return P.prog_hashes(progs, ctx=ctx)


@pytest.mark.gpu
def test_padding_edges_at_every_misalignment(ctx):
    progs, marks = K.padding_batch()
    got, exp = _hashes(ctx, progs), OR.hashes(progs)
    for i, a, n in marks:
        assert got[i].tobytes() == exp[i].tobytes(), (a, n)
    assert np.array_equal(got, exp)


@pytest.mark.gpu
def test_fips_vectors_and_hash_pieces(ctx):
    from syzkaller_amd import corpus as P

    before = ctx.counter("sha1_long_progs")
    got = P.prog_hashes([m for m, _ in OR.VECTORS], hex=True, ctx=ctx)
    assert got == [d for _, d in OR.VECTORS]
    assert ctx.counter("sha1_long_progs") == before + 1  # the million-byte vector
    assert P.Hash(b"ab", b"", b"c", ctx=ctx) == OR.Hash(b"abc") == P.Hash(b"abc", ctx=ctx)
    assert P.String(b"abc", ctx=ctx) == OR.VECTORS[1][1]
    keys = [OR.String(p) for p in K.POOL[:50]]
    keys[7], keys[31] = keys[8], keys[31].upper()
    assert np.flatnonzero(P.VerifyKeys(K.POOL[:50], keys, ctx=ctx)).tolist() == [7, 31]


@pytest.mark.gpu
@pytest.mark.parametrize("nprogs", (0,) + K.WAVE_SIZES)
def test_wave_edges(ctx, nprogs):
    progs = K.mixed(nprogs, nprogs) if nprogs else []
    got = _hashes(ctx, progs)
    assert got.shape == (nprogs, 20) and np.array_equal(got, OR.hashes(progs))


@pytest.mark.gpu
def test_long_threshold_and_counter(ctx):
    assert ctx.counter("sha1_long_len") == LONG
    progs, nlong = K.long_batch()
    before = ctx.counter("sha1_long_progs")
    assert np.array_equal(_hashes(ctx, progs), OR.hashes(progs))
    assert ctx.counter("sha1_long_progs") == before + nlong
    big = [K.text(17, 8), K.text((1 << 20) + 3, 9), K.text(100, 10)]
    assert np.array_equal(_hashes(ctx, big), OR.hashes(big))
    assert ctx.counter("sha1_long_progs") == before + nlong + 1
    short = K.mixed(65, 12)
    assert np.array_equal(_hashes(ctx, short), OR.hashes(short))
    assert ctx.counter("sha1_long_progs") == before + nlong + 1


@pytest.mark.gpu
def test_hex_null_outputs_and_tails(ctx):
    from syzkaller_amd import _lib
    from syzkaller_amd.corpus import texts_csr
    from syzkaller_amd.cover import _p8, _p64

    progs = K.mixed(70, 21)
    b, off = texts_csr(progs)
    n = len(progs)
    exp = OR.hashes(progs)
    exphex = "".join(OR.String(p) for p in progs).encode()
    assert exphex == exphex.lower()
    for want_sigs, want_hex in ((1, 1), (1, 0), (0, 1), (0, 0)):
        sigs, hexs = np.full(20 * n + 32, FILL, U8), np.full(40 * n + 32, FILL, U8)
        _lib.call("sg_prog_hashes", ctx.h, _p8(b), _p64(off), n, _p8(sigs) if want_sigs else None,
                  _p8(hexs) if want_hex else None)
        assert (sigs[20 * n:] == FILL).all() and (hexs[40 * n:] == FILL).all()
        assert sigs[:20 * n].tobytes() == (exp.tobytes() if want_sigs else bytes([FILL]) * (20 * n))
        assert hexs[:40 * n].tobytes() == (exphex if want_hex else bytes([FILL]) * (40 * n))
    # nprogs == 0 writes nothing
    sigs = np.full(40, FILL, U8)
    _lib.call("sg_prog_hashes", ctx.h, None, _p64(np.zeros(1, U64)), 0, _p8(sigs), _p8(sigs))
    assert (sigs == FILL).all()


def _to_dev(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).copy()).to("cuda")


@pytest.mark.gpu
def test_device_form_clamps_garbage_offsets(ctx):
    import torch

    from syzkaller_amd._lib import call
    from syzkaller_amd.corpus import texts_csr

    progs = K.mixed(130, 31)
    b, off = texts_csr(progs)
    n, nbytes = len(progs), int(off[-1])
    d_b = _to_dev(b)
    for shift in (0, 1, 3):  # the byte buffer at a misaligned device address too
        d_bs = torch.empty(nbytes + 8, dtype=torch.uint8, device="cuda")
        d_bs[shift:shift + nbytes] = d_b
        d_sigs = torch.full((20 * n + 32,), FILL, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        call("sg_prog_hashes_dev", ctx.h, d_bs.data_ptr() + shift, _to_dev(off).data_ptr(), n, nbytes, d_sigs.data_ptr())
        ctx.sync()
        got = d_sigs.cpu().numpy()
        assert got[:20 * n].tobytes() == OR.hashes(progs).tobytes() and (got[20 * n:] == FILL).all(), shift
    # offsets past nbytes, and an end below its start: clamped to [start, nbytes]
    bad = np.array([0, 50, 20, nbytes + 1000, 1 << 63, 7, nbytes], U64)
    view = bytes(b)
    exp = []
    for k in range(bad.size - 1):
        a0 = min(int(bad[k]), nbytes)
        a1 = min(max(int(bad[k + 1]), a0), nbytes)
        exp.append(view[a0:a1])
    assert [len(e) for e in exp[:2]] == [50, 0] and len(exp[2]) == nbytes - 20 and len(exp[3]) == 0
    d_sigs = torch.full((20 * 6 + 32,), FILL, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    call("sg_prog_hashes_dev", ctx.h, d_b.data_ptr(), _to_dev(bad).data_ptr(), 6, nbytes, d_sigs.data_ptr())
    ctx.sync()
    got = d_sigs.cpu().numpy()
    assert got[:120].tobytes() == OR.hashes(exp).tobytes() and (got[120:] == FILL).all()
    # and later calls still give right answers
    assert np.array_equal(_hashes(ctx, progs), OR.hashes(progs))


def _check(s, o):
    assert s.count() == o.count() == len(s)
    assert np.array_equal(s.export(), o.export())


@pytest.mark.gpu
def test_add_new_repeats_crafted_identities_and_chains(ctx):
    from syzkaller_amd.corpus import SigSet

    s, o = SigSet(ctx=ctx), OR.OSigSet()
    pre = K.random_sigs(100, 41)
    assert s.add_new(pre).all() and o.add_new(pre).all()
    _check(s, o)
    # repeats inside a batch (only the first flagged), against the preloaded set
    fresh = K.random_sigs(50, 42)
    batch = np.concatenate([fresh[:10], pre[5:15], fresh[:10], fresh[10:], pre[:3], fresh[49:50]])
    exp = o.add_new(batch)
    assert exp.sum() == 50 and np.array_equal(s.add_new(batch), exp)
    _check(s, o)
    # equal in the first 8 and in the first 19 bytes; the all-zero and the all-0xff identity
    for batch in (K.shared_prefix(8, 40, 8), K.shared_prefix(19, 40, 19),
                  np.stack([K.ZERO_SIG, K.FF_SIG, K.ZERO_SIG, K.FF_SIG])):
        exp = o.add_new(batch)
        assert np.array_equal(s.add_new(batch), exp)
        _check(s, o)
        assert s.contains(batch).all() and not s.add_new(batch).any()
    assert s.contains([bytes(20), b"\xff" * 20]).all() and not s.contains([b"\xff" * 19 + b"\xfe"]).any()
    # 300 identities with one home slot: a probe chain longer than a wave, in one batch and across batches
    chain = K.one_home(300, 5)
    for part in (chain[:200], chain[150:]):
        exp = o.add_new(part)
        assert np.array_equal(s.add_new(part), exp)
        _check(s, o)
    assert s.contains(chain).all()
    # clear, then reuse
    s.clear()
    o.clear()
    _check(s, o)
    assert not s.contains(chain[:5]).any()
    exp = o.add_new(chain[::-1])
    assert exp.all() and np.array_equal(s.add_new(chain[::-1]), exp)
    _check(s, o)
    s.close()


@pytest.mark.gpu
def test_growth_from_a_hint_of_one(ctx):
    from syzkaller_amd.corpus import SigSet

    s, o = SigSet(1, ctx=ctx), OR.OSigSet()
    sigs = K.random_sigs(10000, 51)
    sigs[6000:6050] = sigs[100:150]  # known ones among the later batches
    assert np.array_equal(s.add_new(sigs[:5000]), o.add_new(sigs[:5000]))
    _check(s, o)
    for k in range(100):
        part = sigs[5000 + 50 * k: 5050 + 50 * k]
        assert np.array_equal(s.add_new(part), o.add_new(part)), k
        _check(s, o)
    assert s.count() == 9950 and s.contains(sigs).all()
    s.close()


@pytest.mark.gpu
def test_sigset_growth_across_swaps(ctx):
    """remove and hub_sync build the new set in the second {store, table} pair and swap it in: the pair that
    grows next is the one swapped in, at its own capacity, and it must keep the keys it holds."""
    from syzkaller_amd.corpus import SigSet

    s, o = SigSet(1, ctx=ctx), OR.OSigSet()
    sigs = K.random_sigs(4505, 52)
    ever = [sigs]

    def same(what):
        assert s.count() == o.count() == len(s), what
        assert np.array_equal(s.export(), o.export()), what
        for e in ever:
            assert np.array_equal(s.contains(e), o.contains(e)), what

    def remove(batch):
        exp = np.array([o.m.pop(bytes(x), None) is not None for x in batch], dtype=bool)
        assert np.array_equal(s.remove(batch), exp)

    assert np.array_equal(s.add_new(sigs[:1500]), o.add_new(sigs[:1500]))  # the store passes 1024 keys, the table grows
    same("1500 added")
    remove(sigs[10:1500])                                                    # rebuilt in the second pair, swapped
    assert s.count() == 10
    same("all but 10 removed")
    fresh = sigs[1500:4500]
    assert np.array_equal(s.add_new(fresh), o.add_new(fresh))                # the swapped-in pair grows, keeping 10
    same("3000 added")
    corpus = K.POOL + [K.text(40 + k % 90, 8000 + k) for k in range(800)]
    assert len(corpus) == 1200
    ever.append(OR.hashes(corpus))
    _sync(s, o, corpus, "a corpus of 1200")                                  # the second swap: back to the first pair
    same("synced")
    more = [K.text(30 + k % 120, 9000 + k) for k in range(2000)]
    ever.append(OR.hashes(more))
    assert np.array_equal(s.add_progs(more), o.add_new(ever[-1]))
    same("2000 programs added")
    remove(s.export())
    assert s.count() == 0
    same("everything removed")
    assert np.array_equal(s.add_new(sigs[4500:]), o.add_new(sigs[4500:]))
    assert s.count() == 5
    same("5 added")
    s.close()


@pytest.mark.gpu
def test_contains(ctx):
    from syzkaller_amd.corpus import SigSet

    s = SigSet(ctx=ctx)
    have, absent = K.random_sigs(500, 61), K.random_sigs(300, 62)
    assert not s.contains(have[:10]).any()  # an empty set
    s.add_new(have)
    q = np.concatenate([have[::7], absent, have[::7], absent[:5], have[:1]])
    exp = np.concatenate([np.ones(len(have[::7]), bool), np.zeros(300, bool), np.ones(len(have[::7]), bool),
                          np.zeros(5, bool), np.ones(1, bool)])
    assert np.array_equal(s.contains(q), exp)
    assert s.contains([r.tobytes().hex() for r in have[:3]]).all() and s.count() == 500  # reads only
    assert s.contains(np.zeros((0, 20), U8)).size == 0
    s.close()


@pytest.mark.gpu
def test_add_progs_is_hashes_then_add_new(ctx):
    from syzkaller_amd.corpus import SigSet

    a, b = SigSet(ctx=ctx), SigSet(ctx=ctx)
    o = OR.OSigSet()
    for step, progs in enumerate((K.POOL[:200], K.POOL[150:300] + K.POOL[:20] + [K.text(LONG + 5, 71)], [],
                                  K.mixed(300, 72))):
        new_a, sig_a = a.add_progs(progs, sigs=True)
        h = _hashes(ctx, progs)
        new_b = b.add_new(h)
        exp = o.add_new(OR.hashes(progs))
        assert np.array_equal(sig_a, h) and np.array_equal(new_a, new_b) and np.array_equal(new_a, exp), step
        assert np.array_equal(a.add_progs(progs), np.zeros(len(progs), bool))  # sigs NULL; nothing is new twice
        _check(a, o)
        _check(b, o)
    a.close()
    b.close()


def _sync(s, o, progs, what):
    from syzkaller_amd.corpus import HubSync

    add, dels, sigs = HubSync(s, progs, sigs=True)
    eadd, edels = OR.hub_sync(o, progs)
    assert np.array_equal(add, eadd) and dels == edels, what
    assert np.array_equal(sigs, OR.hashes(progs)), what
    _check(s, o)
    return add, dels


@pytest.mark.gpu
def test_hub_sync_fixed_steps(ctx):
    from syzkaller_amd import _lib
    from syzkaller_amd.corpus import SigSet, texts_csr
    from syzkaller_amd.cover import _p8, _p64

    s, o = SigSet(ctx=ctx), OR.OSigSet()
    first, again, third, empty = K.hub_steps_fixed()
    add, dels = _sync(s, o, first, "into an empty set")
    assert add.tolist() == list(range(60)) and dels == []
    add, dels = _sync(s, o, again, "the same corpus")
    assert add.size == 0 and dels == []
    # del_cap one too small: SG_EINVAL before any work, the set untouched
    b, off = texts_csr(third)
    flags, dsig, nd = np.full(len(third), FILL, U8), np.full(20 * 60, FILL, U8), _lib.c_size_t(77)
    rc = _lib.lib.sg_hub_sync(s.h, _p8(b), _p64(off), len(third), None, _p8(flags), _p8(dsig), 59, _lib.ctypes.byref(nd))
    assert rc == _lib.SG_EINVAL and nd.value == 77 and (flags == FILL).all() and (dsig == FILL).all()
    _check(s, o)
    add, dels = _sync(s, o, third, "removes, adds and repeats")
    assert len(add) == 25 and len(dels) == 20 and s.count() == 65
    add, dels = _sync(s, o, empty, "an empty corpus")
    assert add.size == 0 and len(dels) == 65 and s.count() == 0
    add, dels = _sync(s, o, empty, "an empty corpus into an empty set")
    assert add.size == 0 and dels == []
    # the set goes on as an ordinary one
    assert np.array_equal(s.add_progs(first), o.add_new(OR.hashes(first)))
    _check(s, o)
    s.close()


@pytest.mark.gpu
def test_hub_sync_random_steps(ctx):
    from syzkaller_amd.corpus import SigSet

    s, o = SigSet(4, ctx=ctx), OR.OSigSet()
    for k, progs in enumerate(K.hub_steps_random()):
        _sync(s, o, progs, k)
    s.close()


@pytest.mark.gpu
def test_minimize_unchanged_around_the_identities(ctx, kats):
    from syzkaller_amd import cover as C
    from syzkaller_amd.corpus import SigSet

    def kat():
        for case in kats["TestMinimize"]["cases"]:
            assert C.Minimize([np.array(c, np.uint32) for c in case["inp"]], ctx=ctx) == case["out"]

    kat()
    s, o = SigSet(ctx=ctx), OR.OSigSet()
    _sync(s, o, K.POOL[:100], "around")
    assert np.array_equal(_hashes(ctx, K.POOL), OR.hashes(K.POOL))
    kat()
    s.close()
    kat()
