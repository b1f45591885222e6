"""Cases of tests/test_prog_hashes.py: program texts at the padding, wave and path edges of the SHA-1
kernels, identities crafted for the set's probe paths, and corpus sequences for hubSync's diff.  What each
case relies on is asserted on the case itself by the CPU tests."""
import numpy as np

SHA1_LONG = 65536   # SG_SHA1_LONG
PAD_LENGTHS = tuple(range(0, 131))  # 55/56, 63/64/65, 119/120, 127/128 among them
WAVE_SIZES = (1, 63, 64, 65, 4097)


def text(n, seed):
    return np.random.default_rng(seed).integers(0, 256, size=n, dtype=np.uint8).tobytes()


def padding_batch():
    """Every length of PAD_LENGTHS at every start misalignment 0..3: (progs, [(index, misalignment, length)]).
    A filler program in front of each one moves its first byte to the misalignment wanted."""
    progs, marks, pos = [], [], 0
    for a in range(4):
        for n in PAD_LENGTHS:
            fill = (a - pos) % 4 or 4
            progs.append(text(fill, 1000 + len(progs)))
            pos += fill
            marks.append((len(progs), a, n))
            progs.append(text(n, 2000 + len(progs)))
            pos += n
    return progs, marks


def mixed(nprogs, seed):
    """Lengths 0..300, with runs of empty programs."""
    rng = np.random.default_rng(seed)
    lens = rng.integers(0, 301, size=nprogs)
    for start in rng.integers(0, max(nprogs, 1), size=max(nprogs // 50, 1)):
        lens[start:start + 5] = 0
    return [text(int(n), seed * 100003 + k) for k, n in enumerate(lens)]


def long_batch():
    """The threshold's three lengths, and one long program among 200 short ones: (progs, long programs)."""
    progs = [text(SHA1_LONG - 1, 1), text(SHA1_LONG, 2), text(SHA1_LONG + 1, 3)]
    progs += mixed(100, 4) + [text(SHA1_LONG + 77, 5)] + mixed(100, 6)
    return progs, sum(len(p) > SHA1_LONG for p in progs)


# ---- identities ---------------------------------------------------------------
def home_slot(sig, nslots):
    """The set's documented slot function: the first four bytes, little-endian, masked to the table."""
    return int.from_bytes(bytes(sig[:4]), "little") & (nslots - 1)


def random_sigs(n, seed):
    return np.random.default_rng(seed).integers(0, 256, size=(n, 20), dtype=np.uint8)


def shared_prefix(nshared, n, seed):
    """n distinct identities equal in their first nshared bytes."""
    s = random_sigs(n, seed)
    s[:, :nshared] = s[0, :nshared]
    s[:, 19] = np.arange(n, dtype=np.uint8)  # distinct in the last byte at least (n <= 256)
    return s


def one_home(n, seed):
    """n distinct identities with one home slot in any table of up to 2^16 slots, and different first words."""
    s = random_sigs(n, seed)
    s[:, 0:2] = (0x5A, 0xC3)
    s[:, 2] = np.arange(n) & 255
    s[:, 3] = np.arange(n) >> 8
    return s


ZERO_SIG = np.zeros(20, np.uint8)
FF_SIG = np.full(20, 0xFF, np.uint8)


# ---- corpora ------------------------------------------------------------------
POOL = [text(10 + (k * 37) % 190, 7000 + k) for k in range(400)]


def hub_steps_fixed():
    """An empty set filled, the same corpus again, a step that removes some programs, adds some and repeats
    one inside the corpus, then an empty corpus."""
    first = POOL[:60]
    third = POOL[10:50] + POOL[100:120] + [POOL[12]] + POOL[120:125]
    return [first, list(first), third, []]


def hub_steps_random(nsteps=20, seed=99):
    rng = np.random.default_rng(seed)
    steps = []
    for k in range(nsteps):
        if k == 7:
            steps.append([])
            continue
        pick = rng.choice(len(POOL), size=int(rng.integers(1, 250)), replace=True)  # (repeats inside a corpus)
        steps.append([POOL[i] for i in pick])
    return steps
