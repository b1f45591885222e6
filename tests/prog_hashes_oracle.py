"""The test oracle of the program identities.  Hashes: hashlib.sha1 of the standard library (FIPS 180-4, as
Go's crypto/sha1).  Sets: the cited Go lines restated over a Python dict, which keeps insertion order --
the order the product pins (the reference's own is Go map iteration, which is random)."""
import hashlib

import numpy as np

# FIPS 180-4 / RFC 3174 vectors: message -> hex digest
VECTORS = (
    (b"", "da39a3ee5e6b4b0d3255bfef95601890afd80709"),
    (b"abc", "a9993e364706816aba3e25717850c26c9cd0d89d"),
    (b"abcdbcdecdefdefgefghfghighijhijkijkljklmklmnlmnomnopnopq", "84983e441c3bd26ebaae4aa1f95129e5e54670f1"),
    (b"a" * 1000000, "34aa973cd4c4daa4f61eeb2bdbad27316534016f"),
)


def Hash(*pieces):
    """pkg/hash Hash: sha1 over the pieces in turn."""
    h = hashlib.sha1()
    for p in pieces:
        h.update(bytes(p))
    return h.digest()


def String(*pieces):
    return Hash(*pieces).hex()


def hashes(progs):
    """(n, 20) uint8."""
    out = np.zeros((len(progs), 20), np.uint8)
    for k, p in enumerate(progs):
        out[k] = np.frombuffer(Hash(p), np.uint8)
    return out


class OSigSet:
    """map[hash.Sig]bool."""

    def __init__(self):
        self.m = {}

    def add_new(self, sigs):
        """syz-fuzzer/fuzzer.go:480-484 per identity of the batch, in order."""
        new = np.zeros(len(sigs), bool)
        for k, s in enumerate(sigs):
            s = bytes(s)
            if s not in self.m:
                self.m[s] = True
                new[k] = True
        return new

    def contains(self, sigs):
        return np.array([bytes(s) in self.m for s in sigs], dtype=bool)

    def count(self):
        return len(self.m)

    def export(self):
        return np.frombuffer(b"".join(self.m), np.uint8).reshape(-1, 20)

    def clear(self):
        self.m = {}


def hub_sync(hub, progs):
    """syz-manager/manager.go:1053-1069 for a corpus in a fixed order: (add indices, del hex strings); hub
    (an OSigSet) becomes the corpus' identities in first-occurrence order."""
    corpus = {}
    add = []
    for k, p in enumerate(progs):          # :1053-1061
        h = Hash(p)
        if h in corpus:
            continue
        corpus[h] = True
        if h not in hub.m:
            add.append(k)
    dels = [h.hex() for h in hub.m if h not in corpus]  # :1063-1069
    hub.m = corpus
    return np.array(add, dtype=np.int64), dels
