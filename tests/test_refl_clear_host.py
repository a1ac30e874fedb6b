"""Scene T's reflection certificate on the CPU (raymarching_amd/csrc/rm_refl_clear.h,
DESIGN.md 2.25): the stand-alone program tests/host/refl_clear_test.cpp, built
with the host compiler under the address and undefined-behaviour sanitizers
(nothing of it is loaded into Python), as tests/test_shadow_clear_host.py builds
its program.  It includes the predicate's header, restates cast_ray_T with the
reference stop over the Menger distance (exact and fast form) and
getColorReflect's factor, and checks on a million seeded random rays and the
directed cases that every accepted ray meets nothing, stands at a depth >= 3
after kSteps steps and gives the bits of 1.0f under caps of kSteps, kSteps + 1,
128, 256 and 512 -- and that under kSteps - 1 some accepted ray does not.  Built
with the ratio lowered to 0.02, where the bound lies below the hit threshold,
the same program must fail.  No GPU."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCE = os.path.join(ROOT, "tests", "host", "refl_clear_test.cpp")
# -O1 under the sanitizers; no contraction: the restated roundings are the source's own
FLAGS = ["-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]


def _compiler():
    if shutil.which("g++"):  # (gcc's sanitizer runtimes are shared by default: link them in, as clang does)
        return ["g++", "-static-libasan", "-static-libubsan"]
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    return [hipcc, "-x", "c++"] if os.path.exists(hipcc) else None


def _build_and_run(tmp_path, name, extra=()):
    cxx = _compiler()
    if cxx is None:
        pytest.skip("no host C++ compiler (g++ or hipcc)")
    exe = tmp_path / name
    build = subprocess.run(cxx + FLAGS + list(extra) + [SOURCE, "-o", str(exe)], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-4000:]
    run = subprocess.run([str(exe)], cwd=tmp_path, capture_output=True, text=True, timeout=900)
    print(run.stdout)
    return run


def test_refl_clear_predicate_under_sanitizers(tmp_path):
    run = _build_and_run(tmp_path, "refl_clear_test")
    assert run.returncode == 0, (run.stdout + run.stderr)[-4000:]
    assert "all checks passed" in run.stdout
    # the committed ratio and step count are the ones the header's proof is written for
    assert "kRatio 0.200, kSteps 28" in run.stdout
    assert "short of depth 3 after 27 steps" in run.stdout


def test_a_ratio_below_the_hit_threshold_fails(tmp_path):
    """kRatio = 0.02: the bound kRatio ZNEAR = 0.0004 lies below cast_ray_T's hit threshold of 0.001, and rays
    are accepted whose first step is a hit (claim (a))."""
    run = _build_and_run(tmp_path, "refl_clear_test_k002", ["-DRM_REFL_CLEAR_RATIO=0.02f"])
    print(run.stderr[-400:])
    assert run.returncode == 1 and "FAILED check_ray" in run.stderr, (run.stdout + run.stderr)[-4000:]
    assert "all checks passed" not in run.stdout


def test_restated_shares_are_what_the_poses_intend():
    """tests/refl_clear_ref.py POSE_SET on the CPU oracle: the numpy restatement clears most hit lanes, few, lanes
    on both sides of kRatio, or finds no hit lane, as each pose of tests/test_refl_clear_gpu.py intends, at every
    size the GPU tests render."""
    from tests import refl_clear_ref as ref
    for name, (pose, intent) in ref.POSE_SET.items():
        for W, H in ref.SIZES:
            got = ref.cleared_share(pose, W, H, 256)
            print(f"{name} {W}x{H}: hit lanes {got[0]}, cleared share {got[1]:.3f}, slopes within 0.05 below / "
                  f"above kRatio {got[2]} / {got[3]} ({intent})")
            assert ref.share_is_as_intended(intent, *got), (name, W, H, intent, got)
