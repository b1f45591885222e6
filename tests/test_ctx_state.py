"""What a context holds: the option table (syzkaller_amd/csrc/sg_opts.h) row by row, every counter name with its
value on a fresh context, and the lifecycle of contexts and sets.  The GPU tests only create contexts and sets
and make option and counter calls."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from tests.conftest import ROOT

# name, default, lo, hi: sg_ctx_set_option's range-checked keys, in SgOpt's order
OPTIONS = [
    ("bucket_blocks", 0, 0, 1 << 20),
    ("prefix_pairs", 0, 0, 1),
    ("fold_map", -1, -1, 1),
    ("minimize_filter", 1, 0, 1),
    ("minimize_filter_ranks", 0, 0, 1 << 20),
    ("report_direct", 0, 0, 1),
    ("rpc_encode_elems", -1, -1, 1),
    ("rpc_decode_blocks", -1, -1, 1),
    ("host_slice", 0, 0, 1 << 40),
    ("host_copy_threads", 0, 0, 64),
    ("m0_filter", -1, -1, 1),
    ("m0_filter_halves", -1, -1, 2),
    ("exec_comps_path", -1, -1, 0),
    ("flag_skip", -1, -1, 1),
    ("flag_skip_split", 3, 1, 8),
    ("exec_cover_path", -1, -1, 0),
]
SEED_ENV = ("SG_BUCKET_BLOCKS", "SG_FLAG_SKIP", "SG_PREFIX_PAIRS", "SG_DEBUG_PART")


def _define(name):
    head = open(os.path.join(ROOT, "include", "syzsig.h")).read()
    return int(re.search(r"^#define %s (\d+)$" % name, head, flags=re.M).group(1))


# Every name sg_ctx_counter accepts, with its value on a fresh context (None: checked apart).  The last-call and
# cumulative counters are 0; a context without a first-owner table reports its key space as the floor.
COUNTERS = {
    "owner_resets": 0, "owner_floor": (1 << 32) - 1, "owner_key_space": (1 << 32) - 1, "max_launch_records": 1 << 24,
    "host_copy_bytes": 0, "host_copy_ns": 0, "host_wait_ns": 0, "host_copy_threads": 0,
    "m0_filter_used": 0, "m0_filter_fallback": 0, "m0_filter_survivors": 0,
    "m0_filter_queued_milli": (1 << 64) - 1, "m0_filter_halves_log": 0,
    "flag_skip_used": 0, "flag_skip_full_blocks": 0, "flag_skip_all_flagged": 0,
    "hints_candidates": 0, "exec_comps_general": 0, "exec_cover_general": 0,
    "merge_pairs_generic": 0, "merge_pairs_diff_small": 0, "merge_pairs_gap": 0, "merge_pairs_tile": 0,
    "canon_wave_lists": 0, "canon_block_lists": 0, "canon_big_segments": 0, "canon_merge_passes": 0,
    "owned_big_records": 0,
    "triage_runs_wide": 0, "triage_runs_copied": 0, "triage_runs_sorted": 0, "triage_runs_ranked": 0,
    "triage_runs_foreach": 0,
    "prio_bad_ids": 0, "sha1_long_progs": 0, "inflate_long_streams": 0,
    "sha1_long_len": _define("SG_SHA1_LONG"), "inflate_long_len": _define("SG_INFLATE_LONG"),
    "deflate_long_streams": 0, "deflate_long_len": _define("SG_DEFLATE_LONG"),
    "deflate_stored_streams": 0, "deflate_fixed_streams": 0, "deflate_dynamic_streams": 0,  # (the last call's: none)
    "prio_band_cells": 40960, "prio_short_len": 64, "triage_runs_sort_cap": 8192, "tinput_chunk": 8192,
    "exec_comps_fast_cap": _define("SG_EXEC_COMPS_FAST_CAP"), "exec_cover_fast_cap": _define("SG_EXEC_COVER_FAST_CAP"),
    "cover_pages_tile": 4096,  # kPagesTile
    "cpu_quota_milli": None,
    "workspace_bytes": 0,  # (nothing is reserved before the first call that needs the workspace)
}


def test_option_table_cpp(tmp_path):
    """sg_opts.h builds without HIP, and its rows are the table above: 16 rows, their order, names, defaults and
    bounds."""
    exe = str(tmp_path / "opts_test")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "syzkaller_amd", "csrc"),
                    "-o", exe, os.path.join(ROOT, "tests", "cpp", "opts_test.cc")], check=True)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60, check=True).stdout
    assert len(OPTIONS) == 16
    assert out.splitlines() == ["%d %s %d %d %d" % ((i,) + row) for i, row in enumerate(OPTIONS)]


def test_counter_table_is_complete():
    """COUNTERS holds every row of kCounters (sg_ctx.hip), and nothing else."""
    src = open(os.path.join(ROOT, "syzkaller_amd", "csrc", "sg_ctx.hip")).read()
    table = src[src.index("const Counter kCounters[] = {"):]
    table = table[: table.index("\n};")]
    rows = re.findall(r'^\s*\{"([a-z0-9_]+)",', table, flags=re.M)
    assert len(rows) == len(set(rows)) == 52
    assert set(rows) == set(COUNTERS)


@pytest.fixture
def fresh_ctx(ctx, monkeypatch):
    """A context of this test's own, created without the seeding variables.  (ctx, the session's context, comes
    first so that the library and its HIP runtime are loaded before anything else of the test touches HIP.)"""
    from syzkaller_amd.cover import Context

    for name in SEED_ENV:
        monkeypatch.delenv(name, raising=False)
    c = Context(0)
    yield c
    c.close()


@pytest.mark.gpu
def test_options_defaults_and_bounds(fresh_ctx):
    from syzkaller_amd._lib import SG_EINVAL, SyzSigError

    c = fresh_ctx

    def rejected(key, value):
        with pytest.raises(SyzSigError) as e:
            c.set_option(key, value)
        return e.value.rc == SG_EINVAL

    for name, default, lo, hi in OPTIONS:
        assert c.get_option(name) == default, name
        for ok in (lo, hi):
            c.set_option(name, ok)
            assert c.get_option(name) == ok, (name, ok)
        for bad in (lo - 1, hi + 1):
            assert rejected(name, bad), (name, bad)
            assert c.get_option(name) == hi, (name, bad)
    assert c.get_option("max_launch_records") == 1 << 24
    assert c.get_option("owner_key_space") == (1 << 32) - 1
    assert c.get_option("debug_part") == 0
    for bad in (("no_such_option", 1), ("max_launch_records", (1 << 24) + 1), ("max_launch_records", -2),
                ("m0_filter", 2), ("m0_filter", -2), ("prefix_pairs", -1), ("host_copy_threads", 65)):
        assert rejected(*bad), bad
    with pytest.raises(SyzSigError) as e:
        c.get_option("no_such_option")
    assert e.value.rc == SG_EINVAL


@pytest.mark.gpu
def test_counters_on_a_fresh_context(fresh_ctx):
    from syzkaller_amd._lib import SG_EINVAL, SyzSigError

    c = fresh_ctx
    assert len(COUNTERS) == 52
    for name, want in COUNTERS.items():
        got = c.counter(name)
        if want is not None:
            assert got == want, (name, got)
    assert c.counter("cpu_quota_milli") >= 1000
    for bad in ("no_such", "triage_runs_", "triage_runs_bogus"):
        with pytest.raises(SyzSigError) as e:
            c.counter(bad)
        assert e.value.rc == SG_EINVAL, bad


@pytest.mark.gpu
def test_context_and_set_lifecycle(ctx):
    """Eight contexts in turn, each with a set of its own and a wrapper over a second set that outlives it: the
    wrapper does not free the words it was given, and nothing a context or a set owns stays behind (device free
    memory after the last destroy within one bitmap, 512 MiB, of what it was after the first: a cap that catches
    a leaked bitmap, not a measurement)."""
    import torch

    from syzkaller_amd._lib import call, lib
    from syzkaller_amd.cover import Context, SignalAdd, SignalSet, _p32

    vals = np.arange(1000, dtype=np.uint32) * np.uint32(4099) + np.uint32(3)  # 1,000 distinct values over many words
    free_first = None
    for _ in range(8):
        c = Context(0)
        s = SignalSet(c)
        SignalAdd(s, vals)
        assert len(s) == 1000
        s.close()
        under = SignalSet(c)
        w = ctypes.c_void_p()
        call("sg_set_wrap_dev", c.h, ctypes.c_void_p(under.device_words()), ctypes.byref(w))
        call("sg_set_add", w, _p32(vals), 10)
        lib.sg_set_destroy(w)
        assert len(under) == 10  # (the wrapper's words were the set's, and still are)
        under.close()
        c.close()
        if free_first is None:
            free_first = torch.cuda.mem_get_info(0)[0]
    assert free_first - torch.cuda.mem_get_info(0)[0] < 512 << 20
