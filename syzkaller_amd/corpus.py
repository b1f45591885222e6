"""The corpus' identities on the GPU: pkg/hash (SHA-1 of the serialized program), the identity sets
(map[hash.Sig]bool: the fuzzer's corpusHashes, the manager's hubCorpus) and hubSync's Add / Del
(include/syzsig.h, "program identities").

Programs are byte strings.  Every batch call takes them as a sequence of bytes-like objects or as
csr=(bytes, off): program k owns bytes[off[k]:off[k + 1]].
"""
from ctypes import byref, c_size_t, c_uint64, c_void_p

import numpy as np

from ._lib import call, lib
from .cover import _ctx, _p8, _p64

SIG_BYTES = 20     # SG_SIG_BYTES
SHA1_LONG = 65536  # SG_SHA1_LONG

U8, U64 = np.uint8, np.uint64


def texts_csr(progs=None, csr=None):
    """(bytes, off) of a batch of programs."""
    if (progs is None) == (csr is None):
        raise ValueError("pass the programs or csr=(bytes, off)")
    if csr is not None:
        b, off = csr
        b, off = np.ascontiguousarray(b, dtype=U8).reshape(-1), np.ascontiguousarray(off, dtype=U64).reshape(-1)
        if off.size == 0:
            raise ValueError("off holds nprogs + 1 offsets")
        return b, off
    parts = [np.frombuffer(bytes(p), dtype=U8) for p in progs]
    off = np.zeros(len(parts) + 1, U64)
    if parts:
        off[1:] = np.cumsum([p.size for p in parts], dtype=U64)
    b = np.concatenate(parts) if parts else np.zeros(0, U8)
    return np.ascontiguousarray(b, dtype=U8), off


def _bytes_ptr(b):
    return _p8(b) if b.size else None


def _sigs(sigs):
    """Identities as an (n, 20) uint8 array: from such an array, or from a sequence of 20-byte strings or of
    40-character hex strings."""
    if isinstance(sigs, np.ndarray):
        a = np.ascontiguousarray(sigs, dtype=U8)
    else:
        sigs = [bytes.fromhex(s) if isinstance(s, str) else bytes(s) for s in sigs]
        if any(len(s) != SIG_BYTES for s in sigs):
            raise ValueError("an identity is 20 bytes")
        a = np.frombuffer(b"".join(sigs), dtype=U8).copy()
    return a.reshape(-1, SIG_BYTES)


def prog_hashes(progs=None, hex=False, ctx=None, csr=None):
    """hash.Hash of every program: an (n, 20) uint8 array, or with hex the list of hash.String's."""
    b, off = texts_csr(progs, csr)
    n = off.size - 1
    out = np.empty((n, 2 * SIG_BYTES if hex else SIG_BYTES), U8)
    ptr = _p8(out) if n else None
    call("sg_prog_hashes", _ctx(ctx).h, _bytes_ptr(b), _p64(off), n, None if hex else ptr, ptr if hex else None)
    if hex:
        return [row.tobytes().decode("ascii") for row in out]
    return out


def Hash(*pieces, ctx=None):
    """hash.Hash(pieces...) (pkg/hash/hash.go): SHA-1 of the concatenation, 20 bytes."""
    return prog_hashes([b"".join(bytes(p) for p in pieces)], ctx=ctx)[0].tobytes()


def String(*pieces, ctx=None):
    """hash.String(pieces...): the identity in lower-case hex."""
    return prog_hashes([b"".join(bytes(p) for p in pieces)], hex=True, ctx=ctx)[0]


class SigSet:
    """sg_sigset: map[hash.Sig]bool on the device, insertion-ordered."""

    def __init__(self, capacity_hint=0, ctx=None):
        self.ctx = _ctx(ctx)
        h = c_void_p()
        call("sg_sigset_create", self.ctx.h, int(capacity_hint), byref(h))
        self.h = h

    def close(self):
        if self.h:
            lib.sg_sigset_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def clear(self):
        call("sg_sigset_clear", self.h)

    def count(self):
        n = c_uint64()
        call("sg_sigset_count", self.h, byref(n))
        return n.value

    __len__ = count

    def export(self):
        """The identities in insertion order, (count, 20) uint8."""
        n = self.count()
        out = np.empty((n, SIG_BYTES), U8)
        got = c_size_t()
        call("sg_sigset_export", self.h, _p8(out) if n else None, n, byref(got))
        assert got.value == n
        return out

    def contains(self, sigs):
        a = _sigs(sigs)
        out = np.zeros(a.shape[0], U8)
        if a.shape[0]:
            call("sg_sigset_contains", self.h, _p8(a), a.shape[0], _p8(out))
        return out.astype(bool)

    def add_new(self, sigs):
        """addInput's test over a batch: the mask of identities that were new, first occurrences only."""
        a = _sigs(sigs)
        out = np.zeros(a.shape[0], U8)
        if a.shape[0]:
            call("sg_sigset_add_new", self.h, _p8(a), a.shape[0], _p8(out))
        return out.astype(bool)

    def remove(self, sigs):
        """mgr.Corpus.Delete over a batch (syz-hub/state/state.go:181-183): the mask of identities that were in
        the set, first occurrences only; the rest of the set keeps its order."""
        a = _sigs(sigs)
        out = np.zeros(a.shape[0], U8)
        if a.shape[0]:
            call("sg_sigset_remove", self.h, _p8(a), a.shape[0], _p8(out))
        return out.astype(bool)

    def add_progs(self, progs=None, csr=None, sigs=False):
        """Hashes the programs and adds them: the mask of new ones, and with sigs also the (n, 20) identities."""
        b, off = texts_csr(progs, csr)
        n = off.size - 1
        out = np.zeros(n, U8)
        s = np.empty((n, SIG_BYTES), U8) if sigs else None
        call("sg_sigset_add_progs", self.h, _bytes_ptr(b), _p64(off), n, _p8(s) if sigs and n else None,
             _p8(out) if n else None)
        return (out.astype(bool), s) if sigs else out.astype(bool)


def HubSync(sigset, progs=None, csr=None, sigs=False):
    """hubSync's diff (syz-manager/manager.go:1053-1069): (add_indices, del_hex_strings), mirroring a.Add (as
    indices into progs) and a.Del; the set becomes the corpus' identities.  With sigs, the (n, 20) identities
    of the programs as a third value."""
    b, off = texts_csr(progs, csr)
    n = off.size - 1
    cap = sigset.count()
    add = np.zeros(n, U8)
    dels = np.empty((cap, SIG_BYTES), U8)
    s = np.empty((n, SIG_BYTES), U8) if sigs else None
    nd = c_size_t()
    call("sg_hub_sync", sigset.h, _bytes_ptr(b), _p64(off), n, _p8(s) if sigs and n else None, _p8(add) if n else None,
         _p8(dels) if cap else None, cap, byref(nd))
    out = (np.flatnonzero(add), [row.tobytes().hex() for row in dels[: nd.value]])
    return out + (s,) if sigs else out


def VerifyKeys(progs, keys, ctx=None):
    """loadDB's check (syz-hub/state/state.go:91-101): the mask of records whose key is not hash.String of
    their program."""
    keys = list(keys)
    h = prog_hashes(progs, hex=True, ctx=ctx)
    if len(h) != len(keys):
        raise ValueError("one key per program")
    return np.array([k != g for k, g in zip(keys, h)], dtype=bool)
