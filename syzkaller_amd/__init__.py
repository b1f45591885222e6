"""syzkaller_amd -- MI355X-native coverage-signal triage engine for syzkaller.

The product is libsyzsig.so (HIP kernels for gfx950 behind the C-ABI in
include/syzsig.h).  `syzkaller_amd.cover` mirrors the reference pkg/cover API
and the fuzzer/manager signal loops on top of it; `syzkaller_amd.shard` runs
one batch's triage hash-sharded by signal across GPUs (RCCL all-to-all),
`syzkaller_amd.dist` holds the Poll OR-exchange between independent fuzzers,
`syzkaller_amd.hints` the comparison hints (executor comparisons to CompMaps,
shrinkExpand over batches of argument values), and `syzkaller_amd.prio` the
call priorities (corpus call ids to CalculatePriorities and the ChoiceTable),
and `syzkaller_amd.corpus` the corpus' identities (pkg/hash, the identity sets
and hubSync's Add / Del), and `syzkaller_amd.hub` the hub's corpus (prog.CallSet,
the name dictionary, addInputs, pendingInputs and purgeCorpus), and
`syzkaller_amd.db` the corpus database (raw DEFLATE of every value both ways,
db.Open and loadDB from the file's bytes, Save, Delete, Flush and compact), and
`syzkaller_amd.report` pkg/report over batches of console logs (ContainsCrash,
Parse and ExtractConsoleOutput; imported by name, its functions carry the
reference's names).
"""
from ._lib import LIB_PATH, SyzSigError, lib  # noqa: F401  (fails loudly if the library is missing)

_PRIO = ("PrioTable", "CalculatePriorities", "BuildChoiceTable", "ChoiceTable")
_CORPUS = ("Hash", "String", "prog_hashes", "SigSet", "HubSync", "VerifyKeys")
_HUB = ("NameTable", "call_sets", "CallSet", "HubCorpus", "HubState")
_DB = ("inflate_batch", "db_scan", "DB", "LoadDB", "deflate_batch", "deflate_host", "deflate_bound", "db_serialize")

__all__ = ["LIB_PATH", "SyzSigError", "lib", *_PRIO, *_CORPUS, *_HUB, *_DB]


def __getattr__(name):  # syzkaller_amd.prio's, .corpus', .hub's and .db's names, bound on first use (the modules need numpy)
    if name in _PRIO:
        from . import prio

        return getattr(prio, name)
    if name in _CORPUS:
        from . import corpus

        return getattr(corpus, name)
    if name in _HUB:
        from . import hub

        return getattr(hub, name)
    if name in _DB:
        from . import db

        return getattr(db, name)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
