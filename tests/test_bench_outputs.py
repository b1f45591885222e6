"""bench.py's plain run and --dump-outputs on a small C2 configuration: the
result line's fields, only the headline measured without --full, and the last
timed step's outputs written as .npy files that repeat from run to run."""
import json
import os
import sys

import numpy as np
import pytest
import torch  # noqa: F401  (before any test loads a HIP runtime: one runtime per process, torch's)

from tests.conftest import ROOT

SMALL = ["--gpus", "1", "--steps", "3", "--warmup", "1", "--programs", "300", "--calls", "5", "--pcs", "96",
         "--m0", "20000"]
FULL_ONLY = ["roofline", "cpu_baseline", "accounting", "ordered_outputs", "steady_state", "from_traces", "host_api",
             "pipelined"]


def _run(monkeypatch, capsys, extra):
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    import bench

    monkeypatch.delenv("WORLD_SIZE", raising=False)
    monkeypatch.setattr(sys, "argv", ["bench.py"] + SMALL + extra)
    bench.main()
    lines = [l for l in capsys.readouterr().out.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    return json.loads(lines[0])


@pytest.mark.gpu
def test_plain_run_dumps_repeatable_outputs(monkeypatch, capsys, tmp_path):
    a, b = str(tmp_path / "a"), str(tmp_path / "b")
    d = _run(monkeypatch, capsys, ["--dump-outputs", a])
    assert d["steps"] == 3 and d["warmup"] == 1 and d["n_gpus"] == 1
    assert d["unit"] == "PCs/s" and d["higher_is_better"] is True and d["dtype"] == "u32"
    assert d["ms_per_step"] > 0
    # value = signal entries of the timed steps / their wall time
    assert d["value"] == pytest.approx(d["config"]["signal_per_step_per_gpu"] / (d["ms_per_step"] / 1e3), rel=1e-9)
    assert d["kernels"]["p1_hist"]["launches"] >= 3  # the timed steps' own kernel table
    for k in FULL_ONLY:
        assert d[k] is None, k
    _run(monkeypatch, capsys, ["--dump-outputs", b])
    names = sorted(os.listdir(a))
    assert names == ["counts.npy", "maxsignal_words.npy", "newsignal_words.npy", "rec_new.npy", "word_index.npy"]
    assert sum(os.path.getsize(os.path.join(a, n)) for n in names) <= 64 << 20
    out = {n: np.load(os.path.join(a, n)) for n in names}
    for n in names:
        assert out[n].dtype in (np.float32, np.float64), n
        assert np.array_equal(out[n], np.load(os.path.join(b, n))), n
    flags = out["rec_new.npy"]
    assert flags.shape == (300 * 5,) and set(np.unique(flags)) <= {0.0, 1.0}
    n_max, n_new, n_flagged = out["counts.npy"]
    assert n_flagged == flags.sum() and n_flagged > 0
    # the last step's maxSignal = the starting one plus what the step added;
    # newSignal holds at least that (it collects every step's new signal)
    assert n_max > d["config"]["maxsignal_start"] and n_new >= n_max - d["config"]["maxsignal_start"]
    mw = out["maxsignal_words.npy"].astype(np.uint32)
    nw = out["newsignal_words.npy"].astype(np.uint32)
    assert mw.shape == nw.shape == out["word_index.npy"].shape
    assert mw.any() and nw.any()


@pytest.mark.gpu
def test_full_run_measures_the_other_legs(monkeypatch, capsys):
    d = _run(monkeypatch, capsys, ["--full", "--cpu-budget", "0.2", "--npop", "64"])
    assert d["steps"] == 3 and d["ms_per_step"] > 0
    for k in ("roofline", "cpu_baseline", "accounting", "ordered_outputs", "steady_state", "from_traces", "host_api"):
        assert d[k] is not None, k
    assert d["accounting"]["paths_agree"] and d["cpu_baseline"]["prefix_parity_vs_gpu"]
    assert d["host_api"]["flags_equal_device_path"]


@pytest.mark.gpu
def test_more_steps_than_resident_batches(monkeypatch, capsys, tmp_path):
    """Past MAX_BATCHES / MAX_STATES the timed steps reuse the batches in turn
    and run as several timed regions: every step is still timed and counted,
    and a step on a reused batch gives what its first use gave."""
    import bench

    one = _run(monkeypatch, capsys, ["--dump-outputs", str(tmp_path / "one")])  # 3 steps, batches 1..3
    monkeypatch.setattr(bench, "MAX_BATCHES", 4)
    monkeypatch.setattr(bench, "MAX_STATES", 2)
    d = _run(monkeypatch, capsys, ["--steps", "7", "--dump-outputs", str(tmp_path / "many")])  # the last step: batch 3 again
    assert d["steps"] == 7 and d["ms_per_step"] > 0
    assert d["kernels"]["p1_hist"]["launches"] >= 7 and one["kernels"]["p1_hist"]["launches"] >= 3
    for n in ("rec_new.npy", "maxsignal_words.npy"):
        assert np.array_equal(np.load(tmp_path / "one" / n), np.load(tmp_path / "many" / n)), n
    assert np.load(tmp_path / "one" / "counts.npy")[0] == np.load(tmp_path / "many" / "counts.npy")[0]
