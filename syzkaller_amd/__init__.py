"""syzkaller_amd -- MI355X-native coverage-signal triage engine for syzkaller.

The product is libsyzsig.so (HIP kernels for gfx950 behind the C-ABI in
include/syzsig.h).  `syzkaller_amd.cover` mirrors the reference pkg/cover API
and the fuzzer/manager signal loops on top of it; `syzkaller_amd.shard` runs
one batch's triage hash-sharded by signal across GPUs (RCCL all-to-all),
`syzkaller_amd.dist` holds the Poll OR-exchange between independent fuzzers,
`syzkaller_amd.hints` the comparison hints (executor comparisons to CompMaps,
shrinkExpand over batches of argument values), and `syzkaller_amd.prio` the
call priorities (corpus call ids to CalculatePriorities and the ChoiceTable).
"""
from ._lib import LIB_PATH, SyzSigError, lib  # noqa: F401  (fails loudly if the library is missing)

__all__ = ["LIB_PATH", "SyzSigError", "lib", "PrioTable", "CalculatePriorities", "BuildChoiceTable", "ChoiceTable"]

_PRIO = ("PrioTable", "CalculatePriorities", "BuildChoiceTable", "ChoiceTable")


def __getattr__(name):  # syzkaller_amd.prio's names, bound on first use (the module needs numpy)
    if name in _PRIO:
        from . import prio

        return getattr(prio, name)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
