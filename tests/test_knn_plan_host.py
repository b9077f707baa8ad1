"""The host-side plan of the fused kNN (rp-tree_amd/csrc/knn_plan.h: kernel family, ranking tier, kept
entries, LDS bytes, shadows to build, what a forest learns from a batch) against a table of inputs.
The table is a stand-alone C++ program (tests/knn_plan_check.cpp) built with the address and
undefined-behaviour sanitizers and run as a child process: no GPU, nothing loaded into Python."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
def test_knn_plan_table(tmp_path):
    exe = str(tmp_path / "knn_plan_check")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-I", os.path.join(ROOT, "rp-tree_amd", "csrc"),
                           os.path.join(ROOT, "tests", "knn_plan_check.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "all rows hold" in r.stdout
