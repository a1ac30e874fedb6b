"""Scene T's far-sky shortcut on the CPU (raymarching_amd/csrc/rm_far_sky.h,
DESIGN.md 2.22): the stand-alone program tests/host/far_sky_test.cpp, built with
the host compiler under the address and undefined-behaviour sanitizers (nothing
of it is loaded into Python), as tests/test_aa_host.py builds its program.  It
includes the predicate's header, restates cast_ray_T's loop over the Menger
distance and the reflection march's first step, and checks on 1.2 million seeded
random rays and the directed cases that every accepted ray's march returns
exactly ZFAR within N0 steps and its reflection factor is exactly 1.  No GPU."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCE = os.path.join(ROOT, "tests", "host", "far_sky_test.cpp")
# -O1 under the sanitizers; no contraction: the restated roundings are the source's own
FLAGS = ["-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]


def _compiler():
    if shutil.which("g++"):  # (gcc's sanitizer runtimes are shared by default: link them in, as clang does)
        return ["g++", "-static-libasan", "-static-libubsan"]
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    return [hipcc, "-x", "c++"] if os.path.exists(hipcc) else None


def test_far_sky_predicate_under_sanitizers(tmp_path):
    cxx = _compiler()
    if cxx is None:
        pytest.skip("no host C++ compiler (g++ or hipcc)")
    exe = tmp_path / "far_sky_test"
    build = subprocess.run(cxx + FLAGS + [SOURCE, "-o", str(exe)], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-4000:]
    run = subprocess.run([str(exe)], cwd=tmp_path, capture_output=True, text=True, timeout=600)
    print(run.stdout)
    assert run.returncode == 0, (run.stdout + run.stderr)[-4000:]
    assert "all checks passed" in run.stdout
