"""Where the staged host buffers of a call go in their one device allocation
(raymarching_amd/csrc/rm_stage_plan.h, the arithmetic under rm_stage.h) on the
CPU: tests/host/stage_plan_test.cpp, a stand-alone program built with the host
compiler under the address and undefined-behaviour sanitizers (linked into the
program; nothing is loaded into Python).  No GPU."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCES = [os.path.join(ROOT, "tests", "host", "stage_plan_test.cpp")]
FLAGS = ["-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]


def _compiler():
    if shutil.which("g++"):  # (gcc's sanitizer runtimes are shared by default: link them in, as clang does)
        return ["g++", "-static-libasan", "-static-libubsan"]
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    return [hipcc, "-x", "c++"] if os.path.exists(hipcc) else None


def test_stage_plan_under_sanitizers(tmp_path):
    cxx = _compiler()
    if cxx is None:
        pytest.skip("no host C++ compiler (g++ or hipcc)")
    exe = tmp_path / "stage_plan_test"
    build = subprocess.run(cxx + FLAGS + SOURCES + ["-o", str(exe)], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-4000:]
    run = subprocess.run([str(exe)], cwd=tmp_path, capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, (run.stdout + run.stderr)[-4000:]
    assert "all checks passed" in run.stdout
