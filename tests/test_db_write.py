"""The corpus database's write side (pkg/db/db.go:54-116 Save, Delete, Flush, compact; :132-165 serializeHeader and
serializeRecord): sg_deflate_bound, sg_deflate_host, sg_deflate_batch*, sg_db_serialize, sg_db_compact and DB's
methods.  On the CPU the boundary, every rejected argument, the no-device result, the encoder itself
(syzkaller_amd/csrc/sg_deflate.h) as a stand-alone program under the address and undefined-behaviour sanitizers over
the case file (tests/db_write_cases.py), what each case promises read from its stream bit by bit, and the Go
semantics of DB over the host encoder.  On the GPU the device against the host byte for byte, the wave, class and
long-path edges, determinism, the reference's own tests through files, and compaction's round trips.  A stream is
valid when zlib.decompressobj(-15) (tests/db_oracle.inflate) reaches its end, gives the input back and has consumed
exactly the stream."""
import functools
import os
import re
import struct
import subprocess

import numpy as np
import pytest

from tests import db_cases as K
from tests import db_oracle as OR
from tests import db_write_cases as W
from tests.conftest import ROOT

U8, U32, U64 = np.uint8, np.uint32, np.uint64
NAMES = ("sg_deflate_bound", "sg_deflate_host", "sg_deflate_batch", "sg_deflate_batch_dev", "sg_db_serialize",
         "sg_db_compact")
FILL = 0xA5


def _has_gpu():
    try:
        import torch

        return torch.cuda.device_count() > 0
    except Exception:
        return False


@functools.lru_cache(maxsize=None)
def _cases():
    return tuple(W.cases())


@functools.lru_cache(maxsize=None)
def _host_streams():
    """The case file through sg_deflate_host, once: {name: stream} (the reference every other test compares with)."""
    from syzkaller_amd.db import deflate_host

    off, out = deflate_host([d for _, d in _cases()])
    blob, off = out.tobytes(), off.tolist()
    return {name: blob[off[k]:off[k + 1]] for k, (name, _) in enumerate(_cases())}


def _valid(stream, data):
    return OR.inflate(stream) == (K.OK, bytes(data), len(stream))


# ---- CPU: the boundary ---------------------------------------------------------
def test_header_binding_and_library():
    import syzkaller_amd
    from syzkaller_amd import _lib
    from syzkaller_amd import db as D

    text = open(os.path.join(ROOT, "include", "syzsig.h")).read()
    for cite in ("db.go:137-165", ":95-116", ":75-93", "manager.go:786-795", "state.go:106", ":349-351", ":48-50",
                 "state.go:310-336", "manager.go:921-922", ":132-165", ":96-100", ":242", ":143-145", ":148-149"):
        assert cite in text, cite
    assert "unpinned" in text and "need a compressor" not in text
    assert re.search(r"#define SG_DEFLATE_LONG %d\b" % W.DEFLATE_LONG, text)
    src = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r" T (sg_[a-z0-9_]+)$", out, flags=re.M))
    for name in NAMES:
        assert re.search(r"\b(int|size_t) %s\s*\(" % name, src), name
        assert name in _lib.SIGNATURES and name in exported, name
    for name in ("deflate_batch", "deflate_host", "deflate_bound", "db_serialize"):
        assert callable(getattr(D, name)) and getattr(syzkaller_amd, name) is getattr(D, name)
    for name in ("Save", "Delete", "Flush", "compact", "serialize_pending", "serialize_compact"):
        assert callable(getattr(D.DB, name)), name
    assert D.DEFLATE_LONG == W.DEFLATE_LONG and "needs a compressor" not in D.__doc__ and "as it was opened" in D.DB.__doc__
    # the encoder and its kernels: the three properties are stated; no floating point, no read-modify-write primitives
    csrc = os.path.join(ROOT, "syzkaller_amd", "csrc")
    head = open(os.path.join(csrc, "sg_deflate.h")).read()
    assert "TERMINATION." in head and "BOUNDS." in head and "DETERMINISM." in head
    for f in ("sg_deflate.h", "sg_deflate.hip"):
        unit = open(os.path.join(csrc, f)).read().split("#include", 1)[1]
        assert "atomic" not in unit and "float" not in unit and "double" not in unit, f
    # the counters are rows of the context's table; the options' table is untouched
    ctx_src = open(os.path.join(csrc, "sg_ctx.hip")).read()
    for name in ("deflate_long_streams", "deflate_long_len", "deflate_stored_streams", "deflate_fixed_streams",
                 "deflate_dynamic_streams"):
        assert '{"%s",' % name in ctx_src and '"%s"' % name in text, name
    assert "deflate" not in open(os.path.join(csrc, "sg_opts.h")).read()
    # the bound, host only
    for n in (0, 1, 65534, 65535, 65536, 131070, 131071, 1 << 20):
        assert D.deflate_bound(n) == W.bound(n) == n + 5 * max(1, (n + 65534) // 65535)


def test_invalid_arguments_are_einval():
    """Every check the calls make before they touch the context: a context that is only a readable block of memory
    is enough.  No output is written."""
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
    oo, out = np.full(4, 7, U64), np.full(128, FILL, U8)
    nout = _lib.c_size_t(77)
    ref = _lib.ctypes.byref(nout)
    args = (_p8(data), _p64(off), 3, _p64(oo), _p8(out), 128, ref)
    for head, fn in (((), lib.sg_deflate_host), ((fake,), lib.sg_deflate_batch)):
        assert fn(*head, None, *args[1:]) == E                      # in with bytes to read
        assert fn(*head, args[0], None, *args[2:]) == E             # in_off
        assert fn(*head, args[0], _p64(bad0), *args[2:]) == E
        assert fn(*head, args[0], _p64(dec), *args[2:]) == E
        assert fn(*head, *args[:3], None, *args[4:]) == E           # out_off
        assert fn(*head, *args[:4], None, 128, ref) == E            # out with cap > 0
        assert fn(*head, *args[:6], None) == E                      # nout
        assert fn(*head, args[0], _p64(off), 1 << 32, *args[3:]) == E and b"2^32" in lib.sg_last_error()
    assert lib.sg_deflate_batch(None, *args) == E
    dev = (fake, fake, 3, 40, fake, fake, 128)
    assert lib.sg_deflate_batch_dev(None, *dev) == E
    assert lib.sg_deflate_batch_dev(fake, None, *dev[1:]) == E
    assert lib.sg_deflate_batch_dev(fake, fake, None, *dev[2:]) == E
    assert lib.sg_deflate_batch_dev(fake, *dev[:4], None, *dev[5:]) == E    # d_out_off
    assert lib.sg_deflate_batch_dev(fake, *dev[:5], None, 128) == E         # d_out with cap > 0
    assert lib.sg_deflate_batch_dev(fake, fake, fake, 1 << 32, *dev[3:]) == E
    # sg_db_serialize: three records, the second a deletion
    keys, koff = np.frombuffer(b"k0k1k2", U8), np.array([0, 2, 4, 6], U64)
    seqs = np.array([1, K.SEQ_DELETED, 3], U64)
    toff = np.array([0, 10, 10, 40], U64)
    ser = (_p8(keys), _p64(koff), _p64(seqs), _p8(data), _p64(toff), 3, 1, _p8(out), 128, ref)
    assert lib.sg_db_serialize(None, *ser) == E
    assert lib.sg_db_serialize(fake, None, *ser[1:]) == E                   # keys with bytes to read
    assert lib.sg_db_serialize(fake, ser[0], None, *ser[2:]) == E           # key_off
    assert lib.sg_db_serialize(fake, ser[0], _p64(bad0), *ser[2:]) == E
    assert lib.sg_db_serialize(fake, *ser[:2], None, *ser[3:]) == E         # seqs
    assert lib.sg_db_serialize(fake, *ser[:3], None, *ser[4:]) == E         # texts with bytes to read
    assert lib.sg_db_serialize(fake, *ser[:4], None, *ser[5:]) == E         # text_off
    assert lib.sg_db_serialize(fake, *ser[:4], _p64(dec), *ser[5:]) == E
    assert lib.sg_db_serialize(fake, *ser[:7], None, 128, ref) == E         # out with cap > 0
    assert lib.sg_db_serialize(fake, *ser[:9], None) == E                   # nout
    assert lib.sg_db_serialize(fake, *ser[:5], 1 << 32, *ser[6:]) == E
    with_val = np.array([0, 10, 11, 40], U64)                               # the deletion has a value: Go panics
    assert lib.sg_db_serialize(fake, *ser[:4], _p64(with_val), *ser[5:]) == E and b"deletion" in lib.sg_last_error()
    reserved = np.array([1, K.SEQ_DELETED, K.SEQ_DELETED], U64)
    assert lib.sg_db_serialize(fake, *ser[:2], _p64(reserved), *ser[3:]) == E
    assert lib.sg_db_compact(None, _p8(out), 128, ref) == E
    assert lib.sg_db_compact(fake, None, 128, ref) == E
    assert lib.sg_db_compact(fake, _p8(out), 128, None) == E
    assert (oo == 7).all() and (out == FILL).all() and nout.value == 77


@pytest.mark.skipif(_has_gpu(), reason="checks the no-GPU failure path")
def test_no_device_is_enodev():
    from syzkaller_amd import _lib
    from syzkaller_amd.cover import _p8, _p64

    block = np.zeros(1 << 16, U8)  # a zeroed sg_ctx: device 0, an unlocked mutex
    fake = block.ctypes.data_as(_lib.c_void_p)
    data, off = np.frombuffer(b"some text " * 4, U8), np.array([0, 10, 40], U64)
    oo = np.zeros(3, U64)
    nout = _lib.c_size_t()
    ref = _lib.ctypes.byref(nout)
    N = _lib.SG_ENODEV
    assert _lib.lib.sg_deflate_batch(fake, _p8(data), _p64(off), 2, _p64(oo), None, 0, ref) == N
    assert _lib.lib.sg_deflate_batch_dev(fake, fake, fake, 2, 40, fake, None, 0) == N
    keys, koff, seqs = np.frombuffer(b"ab", U8), np.array([0, 1, 2], U64), np.array([1, 2], U64)
    assert _lib.lib.sg_db_serialize(fake, _p8(keys), _p64(koff), _p64(seqs), _p8(data), _p64(off), 2, 1, None, 0, ref) == N
    # ... and the two that need none
    assert _lib.lib.sg_deflate_host(_p8(data), _p64(off), 2, _p64(oo), None, 0, ref) == 0 and nout.value == int(oo[2]) > 0
    assert _lib.lib.sg_deflate_bound(40) == 45


# ---- CPU: the encoder under sanitizers --------------------------------------------
@pytest.fixture(scope="module")
def deflate_exe(tmp_path_factory):
    """tests/cpp/deflate_test.cc built once with the host compiler under ASan and UBSan."""
    exe = str(tmp_path_factory.mktemp("deflate") / "deflate_test")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "syzkaller_amd", "csrc"), "-o", exe,
                    os.path.join(ROOT, "tests", "cpp", "deflate_test.cc")], check=True)
    return exe


def test_deflate_cpp_under_sanitizers(deflate_exe, tmp_path):
    """tests/cpp/deflate_test.cc over the case file and seeded random inputs.  The program itself checks the count
    phase against both sinks, the clamped prefix, the least of the three forced forms and the bound; here every
    stream, the forced ones too, against zlib, and the chosen one against sg_deflate_host: the library's host build
    of the same source gives the same bytes."""
    from syzkaller_amd.db import deflate_host

    inputs = [d for _, d in _cases()] + W.random_inputs()
    inp, outp = str(tmp_path / "inputs.bin"), str(tmp_path / "streams.bin")
    with open(inp, "wb") as f:
        f.write(struct.pack("<I", len(inputs)))
        for d in inputs:
            f.write(struct.pack("<I", len(d)) + d)
    r = subprocess.run([deflate_exe, inp, outp], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "PASS %d" % len(inputs) in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
    off, out = deflate_host(inputs)
    host, off = out.tobytes(), off.tolist()
    blob, at = open(outp, "rb").read(), 0
    for k, d in enumerate(inputs):
        form, n = struct.unpack_from("<BQ", blob, at)
        at += 9
        stream = blob[at:at + n]
        at += n
        assert _valid(stream, d) and W.form_of(stream) == form, k
        assert stream == host[off[k]:off[k + 1]], k
        lens = []
        for f in range(3):
            (m,) = struct.unpack_from("<Q", blob, at)
            at += 8
            forced = blob[at:at + m]
            at += m
            assert _valid(forced, d) and W.form_of(forced) == f, (k, f)
            lens.append(m)
        assert n == min(lens) and form == lens.index(n) and lens[0] == W.bound(len(d)), k
    assert at == len(blob)


# ---- CPU: what the cases promise ---------------------------------------------------
def test_reader_against_zlib():
    """tests/db_write_cases.read_stream, the reader the checks below rely on: zlib's own streams give their input
    back through it, and end where zlib says they do."""
    for data, level in ((K.prog_text(1, 3000), 9), (b"fixed fixed text", 9), (bytes(range(256)) * 3, 0), (b"", 9)):
        s = K.raw_stream(data, level)
        blocks, toks, end_bit = W.read_stream(s)
        out = bytearray()
        for t in toks:
            if isinstance(t, tuple):
                for _ in range(t[0]):
                    out.append(out[-t[1]])
            else:
                out.append(t)
        assert bytes(out) == data and (end_bit + 7) // 8 == OR.inflate(s)[2] == len(s)


def test_case_file():
    by, data = _host_streams(), dict(_cases())
    assert len(by) == len(_cases())                      # the names are distinct
    for name, s in by.items():
        assert _valid(s, data[name]), name
        assert len(s) <= W.bound(len(data[name])), name
    read = {name: W.read_stream(s) for name, s in by.items() if len(s) < 40000 or W.form_of(s) == W.STORED}
    matches = {name: [t for t in r[1] if isinstance(t, tuple)] for name, r in read.items()}
    # every stream is one block, or a chain of stored blocks of at most 65,535 bytes that ends in a short one
    for name, (blocks, _, end_bit) in read.items():
        assert (end_bit + 7) // 8 == len(by[name]), name
        if blocks[0][0] == W.STORED:
            n = len(data[name])
            assert [b[1] for b in blocks] == [65535] * (n // 65535) + ([n % 65535] if n % 65535 or n == 0 else []), name
        else:
            assert len(blocks) == 1, name
    # short inputs and runs
    assert by["len_0"] == b"\x03\x00"
    assert all(W.form_of(by["len_%d" % n]) == W.FIXED and not matches["len_%d" % n] for n in range(4))
    assert matches["run_3"] == [] and matches["run_4"] == [(3, 1)] and matches["run_257"] == [(256, 1)]
    assert matches["run_258"] == [(257, 1)] and matches["run_259"] == [(258, 1)]
    assert matches["run_260"] == [(258, 1)] and read["run_260"][1][-1] == ord("z")      # one byte is left: a literal
    # (no position inside a match is entered: at 259 the slot still holds 1, where the first match began)
    assert matches["run_517"] == [(258, 1), (258, 258)]
    # every length code and every distance code, at both ends of its extra bits
    for sym, length in W.length_ends():
        assert (length, 300) in matches["length_code_%d_len_%d" % (sym, length)], (sym, length)
        assert K.length_symbol(length)[0] == sym
    for sym, dist in W.dist_ends():
        assert (10, dist) in matches["dist_code_%d_dist_%d" % (sym, dist)], (sym, dist)
        assert K.dist_symbol(dist)[0] == sym
    assert len(W.length_ends()) == 8 + 1 + 2 * 20 and len(W.dist_ends()) == 4 + 2 * 26
    # the window's edge, and 16-bit positions
    assert (20, 32768) in matches["repeat_at_32768"]
    assert all(d <= 32768 for _, d in matches["repeat_at_32769"])
    assert not any(ln == 20 for ln, _ in matches["repeat_at_32769"])                    # the only source is out of reach
    assert W.form_of(by["block_65536_twice"]) == W.STORED and len(by["block_65536_twice"]) == 131072 + 15
    across = W.read_stream(by["repeat_across_65536"])
    pos, spans = 0, []
    for t in across[1]:
        n = t[0] if isinstance(t, tuple) else 1
        if isinstance(t, tuple):
            spans.append((pos, pos + n))
        pos += n
    assert across[0][0][0] == W.DYNAMIC and pos == 65539 and any(a <= 65536 < b for a, b in spans) and spans[-1][1] == pos
    # incompressible bytes are stored, split at 65,535 (checked above) -- from the size on at which the stored form
    # is the least of the three: one random byte is 3 bytes as a fixed block and 6 stored
    for n in (100, 65535, 65536, 131071):
        assert W.form_of(by["random_%d" % n]) == W.STORED and len(by["random_%d" % n]) == W.bound(n), n
    assert W.form_of(by["random_1"]) == W.FIXED and len(by["random_1"]) == 3 < W.bound(1)
    # literals and codes
    assert W.form_of(by["literals_above_143"]) == W.FIXED and len(by["literals_above_143"]) == (3 + 12 * 9 + 7 + 7) // 8
    assert W.form_of(by["literals_above_143_long"]) == W.FIXED and matches["literals_above_143_long"]
    assert [t for t in read["literals_above_143_long"][1] if not isinstance(t, tuple)] == list(data["literals_above_143_long"][:16])
    for name in ("two_symbols", "one_symbol", "one_distance"):
        assert W.form_of(by[name]) == W.DYNAMIC, name
    assert W.kraft(read["one_distance"][0][0][2]) == (1, 1 << 14)                      # one distance code, of length 1
    assert set(matches["one_distance"]) == {(258, 258)}
    assert {d for _, d in matches["one_symbol"]} == {1, 258} and W.kraft(read["one_symbol"][0][0][2]) == (2, 1 << 15)
    for name, (blocks, _, _) in list(read.items()) + [("repeat_across_65536", across)]:
        for typ, ll, dl in blocks:
            if typ != W.DYNAMIC:
                continue
            assert len(ll) >= 257 and ll[256] and max(ll) <= 15 and W.kraft(ll)[1] == 1 << 15, name   # complete
            nd, kd = W.kraft(dl)
            assert (nd, kd) in ((0, 0), (1, 1 << 14)) or kd == 1 << 15, name
    assert W.form_of(by["no_repeats_8_symbols"]) == W.DYNAMIC and not matches["no_repeats_8_symbols"]
    assert W.kraft(read["no_repeats_8_symbols"][0][0][2]) == (0, 0)                    # no distance code at all
    assert W.kraft(read["two_symbols"][0][0][2])[0] >= 2                               # and a complete one
    # sizes: 2 KiB and more is dynamic, 40 bytes is not; the streams end on every bit phase
    for size in W.PROG_SIZES:
        s = by["prog_%d" % size]
        assert (s[0] & 6 == 4) == (W.form_of(s) == W.DYNAMIC)
        if size >= 2048:
            assert s[0] & 6 == 4, size
    assert by["prog_40"][0] & 6 != 4
    phases = {read["phase_%d" % size][2] % 8 for size in W.PHASE_SIZES}
    assert phases == set(range(8)), phases
    # the matcher finds something: zlib level 9 needs 272 bytes for this, a 512-entry greedy fixed-code parse 829
    assert len(data["line40_65536"]) == 65536 and len(by["line40_65536"]) < 8192


# ---- CPU: the Go semantics over the host encoder -------------------------------------
def _host_serialize(keys, seqs, texts, with_header=False, ctx=None):
    """db_serialize restated over sg_deflate_host and tests/db_cases.db_record: no device."""
    from syzkaller_amd.db import deflate_host

    texts = [b"" if t is None else bytes(t) for t in texts]
    off, out = deflate_host(texts) if texts else (np.zeros(1, U64), np.zeros(0, U8))
    blob, off = out.tobytes(), off.tolist()
    recs = [W.record_bytes(bytes(k), None if int(s) == K.SEQ_DELETED else t, int(s), blob[off[i]:off[i + 1]])
            for i, (k, s, t) in enumerate(zip(keys, seqs, texts))]
    return (K.db_header() if with_header else b"") + b"".join(recs)


def _bare_db(records, uncompacted, filename):
    """A DB as Open leaves it, built by hand: no device."""
    from syzkaller_amd.db import DB

    db = object.__new__(DB)
    db.ctx, db.h, db.filename = None, None, filename
    db._records, db._pending, db._modified = dict(records), [], True
    db.uncompacted, db.nlive = uncompacted, len(records)
    return db


def test_go_semantics_on_the_host(tmp_path, monkeypatch):
    from syzkaller_amd import db as D

    monkeypatch.setattr(D, "db_serialize", _host_serialize)
    path = str(tmp_path / "corpus.db")
    db = _bare_db({}, 0, path)
    with pytest.raises(ValueError):
        db.Save(b"k", b"v", K.SEQ_DELETED)                      # the reserved seq
    assert db.uncompacted == 0 and not db._pending
    v = [K.prog_text(s, 50 + 40 * s) for s in range(4)]
    db.Save(b"a", v[0], 1)
    db.Save(b"a", v[0], 1)                                      # same seq, same bytes: nothing (:58-60)
    assert db.uncompacted == 1 and len(db._pending) == 1
    db.Save(b"a", v[0], 2)                                      # another seq: a write
    db.Save(b"a", v[1], 2)                                      # other bytes: a write
    db.Save(b"e", b"", 7)                                       # an empty value
    db.Save(b"e", b"", 7)
    db.Delete(b"absent")                                        # (:67-69)
    db.Save(b"d", v[2], 3)
    db.Delete(b"d")
    assert db.uncompacted == 6 and db.Records == {b"a": (v[1], 2), b"e": (b"", 7)} and len(db) == 2
    pending = db.serialize_pending()
    recs, end = OR.scan(K.db_header() + pending)
    assert end == 0 and len(recs) == 6 and [r[2] for r in recs] == [1, 2, 2, 7, 3, K.SEQ_DELETED]
    assert recs[3][4] == 0 and recs[5][3:] == (0, 0)            # the empty value has no stream, the deletion no field
    db.Flush()                                                  # 6 // 10 * 9 = 0: appended, behind a header
    assert not db._pending and db.uncompacted == 6
    data = open(path, "rb").read()
    assert data == K.db_header() + pending
    o = OR.ODB(data)
    assert o.Records == db.Records and o.uncompacted == 6 and o.end == 0
    db.Save(b"b", v[3], 9)
    db.Flush()                                                  # appended: no second header
    assert open(path, "rb").read() == data + _host_serialize([b"b"], [9], [v[3]])
    # Flush's decision (:76) on both sides: 9 live records, uncompacted 19 (9 > 9 is false) and 20 (18 > 9)
    for unc, compacts in ((19, False), (20, True)):
        p2 = str(tmp_path / ("edge%d.db" % unc))
        live = {b"key%d" % k: (v[k % 4], k) for k in range(9)}
        open(p2, "wb").write(K.db_header() + b"old bytes that only a compaction removes")
        db = _bare_db(live, unc - 1, p2)
        db.Save(b"key0", v[1], 100)
        assert db.uncompacted == unc and (unc // 10 * 9 > len(db)) == compacts
        db.Flush()
        got = open(p2, "rb").read()
        assert not os.path.exists(p2 + ".tmp") and not db._pending
        if compacts:
            o = OR.ODB(got)
            assert o.Records == db.Records and list(o.Records) == list(db.Records)
            assert o.uncompacted == 9 == db.uncompacted and o.end == 0 and got == db.serialize_compact()
        else:
            assert got.endswith(_host_serialize([b"key0"], [100], [v[1]])) and b"old bytes" in got and db.uncompacted == unc
    # a database from bytes has no file
    db = _bare_db({b"a": (v[0], 1)}, 1, None)
    with pytest.raises(ValueError):
        db.Flush()
    with pytest.raises(ValueError):
        db.compact()
    assert OR.ODB(db.serialize_compact()).Records == {b"a": (v[0], 1)} and db.serialize_pending() == b""


# ---- GPU -------------------------------------------------------------------------
def _to_dev(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).copy()).to("cuda")


def _host(inputs):
    from syzkaller_amd.db import deflate_host

    off, out = deflate_host(list(inputs))
    return off, out.tobytes()


def _check_batch(ctx, inputs):
    """One device call against the host encoder, byte for byte, and every stream against zlib."""
    from syzkaller_amd.db import deflate_batch

    hoff, hout = _host(inputs)
    off, out = deflate_batch(list(inputs), ctx=ctx, cap=len(hout))
    assert off.tolist() == hoff.tolist() and out.tobytes() == hout
    o = off.tolist()
    streams = [hout[o[k]:o[k + 1]] for k in range(len(inputs))]
    assert all(_valid(s, d) for s, d in zip(streams, inputs))
    return streams


def _form_counts(streams):
    return [sum(W.form_of(s) == f for s in streams) for f in range(3)]


def _counters(ctx):
    return [ctx.counter("deflate_%s_streams" % f) for f in ("stored", "fixed", "dynamic")]


@pytest.mark.gpu
def test_host_and_device_agree(ctx):
    """The whole case file in one batch: the host form, the count form and the device form give sg_deflate_host's
    offsets and bytes; a cap one below the total leaves out untouched."""
    import torch

    from syzkaller_amd import _lib
    from syzkaller_amd.corpus import texts_csr
    from syzkaller_amd.cover import _p8, _p64
    from syzkaller_amd.db import deflate_batch

    inputs = [d for _, d in _cases()]
    want = _host_streams()
    assert ctx.counter("deflate_long_len") == W.DEFLATE_LONG
    n_long = sum(len(d) > W.DEFLATE_LONG for d in inputs)
    before = ctx.counter("deflate_long_streams")
    streams = _check_batch(ctx, inputs)
    assert ctx.counter("deflate_long_streams") == before + n_long and n_long >= 3
    assert streams == [want[name] for name, _ in _cases()]
    assert _counters(ctx) == _form_counts(streams) and min(_counters(ctx)) > 0
    hoff, hout = _host(inputs)
    total = len(hout)
    off, out = deflate_batch(inputs, ctx=ctx, cap=0)             # the count form
    assert out is None and off.tolist() == hoff.tolist()
    b, off_in = texts_csr(inputs)
    n = len(inputs)
    for cap in (total - 1, total):
        oo, out = np.zeros(n + 1, U64), np.full(total + 16, FILL, U8)
        nout = _lib.c_size_t()
        _lib.call("sg_deflate_batch", ctx.h, _p8(b), _p64(off_in), n, _p64(oo), _p8(out), cap, _lib.ctypes.byref(nout))
        assert nout.value == total and oo.tolist() == hoff.tolist()
        if cap < total:
            assert (out == FILL).all()
        else:
            assert out[:total].tobytes() == hout and (out[total:] == FILL).all()
    d_b, d_off = _to_dev(b), _to_dev(off_in)
    for cap in (total, total - 1, 0):
        d_oo = torch.zeros(n + 3, dtype=torch.int64, device="cuda")
        d_out = torch.full((total + 16,), FILL, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        _lib.call("sg_deflate_batch_dev", ctx.h, d_b.data_ptr(), d_off.data_ptr(), n, b.size, d_oo.data_ptr(),
                  d_out.data_ptr() if cap else None, cap)
        ctx.sync()
        got_off, got = d_oo.cpu().numpy().view(U64), d_out.cpu().numpy()
        assert got_off[:n + 1].tolist() == hoff.tolist() and not got_off[n + 1:].any()
        if cap == total:
            assert got[:total].tobytes() == hout and (got[total:] == FILL).all()
        else:
            assert (got == FILL).all()


@pytest.mark.gpu
def test_device_form_clamps_garbage_offsets(ctx):
    """Offsets past nbytes and an end below its start are clamped to [start, nbytes]: garbage streams, no error, and
    nothing outside the buffers."""
    import torch

    from syzkaller_amd._lib import call
    from syzkaller_amd.corpus import texts_csr

    inputs = [K.prog_text(s, 60 + 7 * s) for s in range(9)]
    b, off = texts_csr(inputs)
    nbytes = int(off[-1])
    bad = np.array([0, int(off[1]), 20, nbytes + 1000, 1 << 63, 7, int(off[2]), nbytes], U64)
    view, pieces = bytes(b), []
    for k in range(bad.size - 1):
        a0 = min(int(bad[k]), nbytes)
        pieces.append(view[a0:min(max(int(bad[k + 1]), a0), nbytes)])
    hoff, hout = _host(pieces)
    m, total = bad.size - 1, len(hout)
    d_oo = torch.zeros(m + 1, dtype=torch.int64, device="cuda")
    d_out = torch.full((total + 64,), FILL, dtype=torch.uint8, device="cuda")
    d_b, d_bad = _to_dev(b), _to_dev(bad)
    torch.cuda.synchronize()
    call("sg_deflate_batch_dev", ctx.h, d_b.data_ptr(), d_bad.data_ptr(), m, nbytes, d_oo.data_ptr(), d_out.data_ptr(),
         total + 64)
    ctx.sync()
    got = d_out.cpu().numpy()
    assert d_oo.cpu().numpy().view(U64).tolist() == hoff.tolist()
    assert got[:total].tobytes() == hout and (got[total:] == FILL).all()


@pytest.mark.gpu
def test_wave_and_class_edges(ctx):
    """Batches around the wave size, every length 0 to 199, and a byte either side of the boundaries of the length
    classes the kernels sort by.  The class is input length >> 6, one rule for all 1,024 of them: every boundary
    up to 1,024 bytes is here, then 4,096, 32,768, the last one below SG_DEFLATE_LONG, and SG_DEFLATE_LONG itself,
    where the stream leaves the lane path.  Empty streams lie in between."""
    texts = [K.prog_text(s, 30 + 11 * (s % 23)) for s in range(129)]
    for n in (1, 63, 64, 65, 129):
        before = ctx.counter("deflate_long_streams")
        streams = _check_batch(ctx, texts[:n])
        assert ctx.counter("deflate_long_streams") == before and _counters(ctx) == _form_counts(streams)
    big = K.prog_text(199, 70000)
    _check_batch(ctx, [big[:n] for n in range(200)])
    edges = [W.CLASS_BYTES * k for k in range(1, 17)] + [4096, 32768, W.DEFLATE_LONG - W.CLASS_BYTES]
    batch = []
    for e in edges:
        batch += [big[:e - 1], b"", big[:e], big[:e + 1]]
    before = ctx.counter("deflate_long_streams")
    _check_batch(ctx, batch)
    assert ctx.counter("deflate_long_streams") == before
    rng = np.random.default_rng(65536)
    noise = rng.integers(0, 256, W.DEFLATE_LONG + 1, dtype=U8).tobytes()
    L = W.DEFLATE_LONG
    batch = [big[:L - 1], b"", big[:L], big[:L + 1], b"", noise[:L - 1], noise[:L], noise, b"", texts[0]]
    before = ctx.counter("deflate_long_streams")
    streams = _check_batch(ctx, batch)
    assert ctx.counter("deflate_long_streams") == before + 2      # the two of L + 1 bytes: the lane path ends at L
    assert _counters(ctx) == _form_counts(streams) and W.form_of(streams[7]) == W.STORED


@pytest.mark.gpu
def test_determinism(ctx):
    """A stream's bytes depend on its input alone: the same inputs reversed, and split over two calls, give each
    stream the same bytes; the last call's form counters are the counts read off the streams' first bytes."""
    named = [(n, d) for n, d in _cases() if len(d) <= 70000]
    want = _host_streams()
    inputs = [d for _, d in named]
    rev = _check_batch(ctx, inputs[::-1])[::-1]
    assert rev == [want[n] for n, _ in named]
    assert _counters(ctx) == _form_counts(rev)
    cut = len(inputs) // 3
    first = _check_batch(ctx, inputs[:cut])
    assert _counters(ctx) == _form_counts(first)
    second = _check_batch(ctx, inputs[cut:])
    assert _counters(ctx) == _form_counts(second) and first + second == rev


@pytest.mark.gpu
def test_serialize_layout(ctx):
    """sg_db_serialize against tests/db_cases.db_record with this library's stream swapped in, and sg_db_scan reads
    back exactly the fields that were written."""
    from syzkaller_amd.db import db_scan, db_serialize

    v = [K.prog_text(s, 50 + 90 * s) for s in range(6)]
    recs = [(b"k0", v[0], 1), (b"", v[1], 2), (b"gone", None, K.SEQ_DELETED), (b"empty", b"", 4),
            (b"k" * 300, v[2], (1 << 64) - 2), (b"k0", v[3], 0), (b"also gone", None, K.SEQ_DELETED), (b"last", v[5], 9)]
    keys, vals, seqs = zip(*recs)
    hoff, hout = _host([b"" if t is None else t for t in vals])
    o = hoff.tolist()
    want = b"".join(W.record_bytes(k, t, s, hout[o[i]:o[i + 1]]) for i, (k, t, s) in enumerate(recs))
    assert db_serialize(keys, seqs, vals, False, ctx) == want
    data = db_serialize(keys, seqs, vals, True, ctx)
    assert data == K.db_header() + want
    assert db_serialize(keys, seqs, vals, True, ctx, cap=len(data) - 1) is None
    kp, kl, sq, vp, vl, end = db_scan(data)
    assert end == 0 and sq.tolist() == list(seqs) and kl.tolist() == [len(k) for k in keys]
    assert [data[p:p + n] for p, n in zip(kp.tolist(), kl.tolist())] == list(keys)
    for i, (k, t, s) in enumerate(recs):
        stream = data[int(vp[i]):int(vp[i]) + int(vl[i])]
        if t:
            assert stream == hout[o[i]:o[i + 1]] and _valid(stream, t), i
        else:
            assert (int(vp[i]) == 0 or t == b"") and int(vl[i]) == 0, i
    assert OR.ODB(data).Records == {b"": (v[1], 2), b"empty": (b"", 4), b"k" * 300: (v[2], (1 << 64) - 2), b"k0": (v[3], 0),
                                    b"last": (v[5], 9)}
    assert db_serialize([], [], [], True, ctx) == K.db_header() and db_serialize([], [], [], False, ctx) == b""
    assert db_serialize([b"only"], [K.SEQ_DELETED], [None], False, ctx) == K.db_record(b"only", None, 0)


def _go_open(path, ctx):
    """db.Open (:38-52) with its compaction, as a caller of this library writes it."""
    from syzkaller_amd.db import DB

    db = DB.Open(path, ctx)
    if db.needs_compact:
        db.compact()
    return db


@pytest.mark.gpu
def test_reference_db_tests_end_to_end(ctx, tmp_path):
    """pkg/db/db_test.go's TestBasic, TestModify and TestLarge (tests/db_cases.py has them as data) through files."""
    from syzkaller_amd.db import DB

    for name, writes, want in (("basic", K.DB_TEST_BASIC, K.DB_TEST_BASIC_WANT),
                               ("modify", K.DB_TEST_MODIFY, K.DB_TEST_MODIFY_WANT)):
        path = str(tmp_path / (name + ".db"))
        db = _go_open(path, ctx)
        assert len(db.Records) == 0 and open(path, "rb").read() == K.db_header() and db.uncompacted == 0
        for key, val, seq in writes:
            if val is None:
                db.Delete(key)
            else:
                db.Save(key, val, seq)
        assert db.Records == want and db.uncompacted == len(writes)
        compacts = len(writes) // 10 * 9 > len(want)
        assert compacts == (name == "modify")
        db.Flush()
        assert db.Records == want and db.uncompacted == (len(want) if compacts else len(writes))
        db.close()
        data = open(path, "rb").read()
        o = OR.ODB(data)                                           # zlib reads what was written
        assert o.Records == want and o.end == 0 and o.uncompacted == (len(want) if compacts else len(writes))
        db = DB.Open(path, ctx)
        assert db.Records == want and db.end == 0 and db.uncompacted == o.uncompacted
        db.close()
    # TestLarge: 1000 records of one random 1000-byte value
    val = np.random.default_rng(1000).integers(0, 256, 1000, dtype=U8).tobytes()
    path = str(tmp_path / "large.db")
    db = _go_open(path, ctx)
    for k in range(K.DB_TEST_LARGE_RECORDS):
        db.Save(b"%d" % k, val, 0)
    assert db.uncompacted == K.DB_TEST_LARGE_RECORDS
    db.Flush()
    db.close()
    db = _go_open(path, ctx)
    assert len(db.Records) == K.DB_TEST_LARGE_RECORDS and all(r == (val, 0) for r in db.Records.values())
    assert db.uncompacted == K.DB_TEST_LARGE_RECORDS and not db.needs_compact
    for k in range(K.DB_TEST_LARGE_RECORDS):
        db.Save(b"%d" % k, val, 0)                                 # the same seq and bytes: nothing
    assert db.uncompacted == K.DB_TEST_LARGE_RECORDS and not db._pending and db.serialize_pending() == b""
    size = os.path.getsize(path)
    db.Flush()
    assert os.path.getsize(path) == size
    db.close()


@pytest.mark.gpu
def test_compact_round_trips(ctx, tmp_path):
    """A file of about 300 writes with overwrites, deletions, empty values and one value past SG_DEFLATE_LONG:
    sg_db_compact of the opened database is db_serialize of its export with the header; the result reopens to the
    same Records, compacted; and a modified database compacts to what zlib reads back as its Records."""
    from syzkaller_amd.db import DB, db_serialize

    recs = W.history_records()
    assert 290 <= len(recs) <= 310
    path = str(tmp_path / "history.db")
    open(path, "wb").write(K.db_file(recs))
    db = DB.Open(path, ctx)
    o = OR.ODB(K.db_file(recs))
    assert list(db.Records.items()) == list(o.Records.items()) and db.uncompacted == len(recs)
    assert any(len(v) > W.DEFLATE_LONG for v, _ in db.Records.values())
    assert any(v == b"" for v, _ in db.Records.values())
    keys, seqs, texts = db.export()
    before = ctx.counter("deflate_long_streams")
    data = db.serialize_compact()
    assert ctx.counter("deflate_long_streams") == before + 1
    assert data == db_serialize(keys, seqs.tolist(), texts, True, ctx)
    assert OR.ODB(data).Records == o.Records
    nlive = len(db)
    db.compact()
    assert open(path, "rb").read() == data and db.uncompacted == nlive and not os.path.exists(path + ".tmp")
    db.close()
    db = DB.Open(path, ctx)
    assert list(db.Records.items()) == list(o.Records.items())
    assert db.uncompacted == nlive == len(db) and not db.needs_compact and db.end == OR.END_EOF
    bad, _ = db.verify()
    assert bad.tolist() == [1 if v == b"" else 0 for v, _ in db.Records.values()]   # (an empty text has no call)
    # modified: Records on the host are what is written; device() still describes the file as opened
    first = next(iter(db.Records))
    db.Delete(first)
    db.Save(b"new key", K.prog_text(5, 500), 77)
    assert len(db) == nlive and db.nlive == nlive and db.uncompacted == nlive + 2
    data2 = db.serialize_compact()
    o2 = OR.ODB(data2)
    assert o2.Records == db.Records and list(o2.Records) == list(db.Records) and first not in o2.Records
    assert len(db.export()[0]) == nlive and db.export()[0][0] == first
    db.close()


@pytest.mark.gpu
def test_empty_database(ctx, tmp_path):
    from syzkaller_amd.db import DB

    path = str(tmp_path / "empty.db")
    db = DB.Open(path, ctx)
    assert len(db) == 0 and db.needs_compact and db.serialize_compact() == K.db_header()
    db.compact()
    assert open(path, "rb").read() == K.db_header() and db.uncompacted == 0
    db.close()
    db = DB.Open(path, ctx)
    assert len(db) == 0 and db.Records == {} and db.end == OR.END_EOF
    db.close()
    db = DB.Open(K.db_header(), ctx)                              # from bytes: no file
    with pytest.raises(ValueError):
        db.compact()
    with pytest.raises(ValueError):
        db.Flush()
    assert db.serialize_compact() == K.db_header() and db.serialize_pending() == b""
    db.close()
