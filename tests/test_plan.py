"""The buffer planner and the offsets check (syzkaller_amd/csrc/sg_plan.h) on the
CPU: tests/cpp/plan_test.cc, a stand-alone program built with the host compiler."""
import os
import subprocess

from tests.conftest import ROOT


def test_plan_cpp(tmp_path):
    exe = str(tmp_path / "plan_test")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "syzkaller_amd", "csrc"),
                    "-o", exe, os.path.join(ROOT, "tests", "cpp", "plan_test.cc")], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "PASS" in r.stdout
