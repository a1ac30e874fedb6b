"""Scene T's near-sky ladder on the CPU (raymarching_amd/csrc/rm_far_sky.h 3.,
DESIGN.md 2.27): the stand-alone program tests/host/near_sky_test.cpp, built with
the host compiler under the address and undefined-behaviour sanitizers (nothing
of it is loaded into Python), as tests/test_far_sky_host.py builds its program.
It includes the header alone, restates cast_ray_T's loop over the Menger distance
in the exact and the fast form and over its box term alone (the least distance
the proof's premise allows), and checks for every rung, on a million seeded
rays and the directed cases, that every accepted ray's march meets nothing and
returns the bits of ZFAR within the rung's N(m) steps.  Two perturbed builds of
it must fail: m = 0.01 under the N of m = 0.02, and the radius chosen without
regard to the step cap.  The same program's other modes (--ladder, --radius,
--eval) give the header's ladder, rung choice and vote for the numpy restatement
(tests/near_sky_ref.py) to be held to, with zero disagreements.  No GPU."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import near_sky_ref as ref
from tests.test_far_sky_host import _random_rays

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCE = os.path.join(ROOT, "tests", "host", "near_sky_test.cpp")
# -O1 under the sanitizers; no contraction: the restated roundings are the source's own
FLAGS = ["-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]


def _compiler():
    if shutil.which("g++"):  # (gcc's sanitizer runtimes are shared by default: link them in, as clang does)
        return ["g++", "-static-libasan", "-static-libubsan"]
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    return [hipcc, "-x", "c++"] if os.path.exists(hipcc) else None


def _build(tmp_path, name="near_sky_test", defines=()):
    cxx = _compiler()
    if cxx is None:
        pytest.skip("no host C++ compiler (g++ or hipcc)")
    exe = tmp_path / name
    build = subprocess.run(cxx + FLAGS + list(defines) + [SOURCE, "-o", str(exe)], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-4000:]
    return exe


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return _build(tmp_path_factory.mktemp("near_sky"))


def test_near_sky_ladder_under_sanitizers(exe):
    run = subprocess.run([str(exe)], cwd=exe.parent, capture_output=True, text=True, timeout=900)
    print(run.stdout)
    assert run.returncode == 0, (run.stdout + run.stderr)[-4000:]
    assert "all checks passed" in run.stdout
    assert run.stdout.count("proven N(m)") == len(ref.LADDER)


@pytest.mark.parametrize("define,where", [("-DNEAR_SKY_TEST_M=0.01f", "check_prim"), ("-DNEAR_SKY_TEST_NO_CAP", "caps")])
def test_perturbed_builds_fail(tmp_path, define, where):
    """m = 0.01 under the N of m = 0.02: a ray along a face's diagonal 0.011 away takes more than 205 steps over
    the box term (over the sponge's own distance the holes' larger steps would let it pass: 202).  The radius of
    the last rung under every step cap: its rays do not reach ZFAR within 38 steps."""
    bad = _build(tmp_path, "near_sky_perturbed", [define])
    run = subprocess.run([str(bad)], cwd=tmp_path, capture_output=True, text=True, timeout=900)
    print(run.stdout[-2000:], run.stderr[-2000:])
    assert run.returncode == 1 and "all checks passed" not in run.stdout
    assert f"FAILED {where}" in run.stderr, run.stderr[-2000:]


def test_numpy_ladder_and_rung_choice_are_the_headers(exe):
    tmp = exe.parent
    run = subprocess.run([str(exe), "--ladder"], cwd=tmp, capture_output=True, text=True, timeout=60)
    assert run.returncode == 0, run.stderr
    rows = [line.split() for line in run.stdout.strip().splitlines()]
    assert len(rows) == len(ref.LADDER)
    for (m, r, n), row in zip(ref.LADDER, rows):
        assert np.float32(float(row[0])) == m and np.float32(float(row[1])) == r and int(row[2]) == n, (row, m, r, n)
    assert ref.N_OF[2] <= 128 and ref.N_OF[3] <= 208  # C2's cap admits m = 0.05, the far-sky vote's N0 m = 0.02
    caps = np.array([[c, u] for c in list(range(-2, 300)) + [1 << 20, 2 ** 31 - 1] for u in (0, 1)], np.int32)
    (tmp / "caps.bin").write_bytes(caps.tobytes())
    run = subprocess.run([str(exe), "--radius", "caps.bin", "radius.bin"], cwd=tmp, capture_output=True, text=True, timeout=60)
    assert run.returncode == 0, run.stderr
    got = np.frombuffer((tmp / "radius.bin").read_bytes(), np.float32)
    want = np.array([ref.radius(int(c), bool(u)) for c, u in caps], np.float32)
    assert len(got) == len(want) and np.array_equal(got, want)
    assert len(np.unique(want)) == len(ref.LADDER) + 1  # every rung and none
    for c, s, ok in [(1.0, 0.0, True), (0.6, 0.8, True), (0.0, 0.0, False), (1.0, 0.02, False), (np.nan, 0.0, False)]:
        assert ref.unit_rotation(c, s) == ok


def test_numpy_restatement_is_the_headers_vote(exe):
    """tests/near_sky_ref.near_sky_ray against rmfs::near_sky_ray itself, ray by ray, at every rung's radius and
    at radii beside them: tests/test_far_sky_host.py's seeded random rays, the same rays drawn round each rung's
    cube, and the frames' own rays of tests/test_near_sky_gpu.py.  Zero disagreements."""
    tmp = exe.parent
    rng = np.random.RandomState(20261020)
    blocks = []
    radii = [r for _, r, _ in ref.LADDER]
    for i, r in enumerate(radii):
        rays = _random_rays(10000, seed=20261021 + i)
        # the rays that graze kFarSkyR, scaled about the centre to graze this rung's cube
        scale = np.float32(r / ref.fs.K_R)
        rays[::2, :3] *= scale
        rr = np.full(len(rays), r, np.float32)
        rr[::7] = np.nextafter(r, np.float32(2.0))
        rr[3::7] = rng.uniform(1.0, 1.3, size=len(rr[3::7])).astype(np.float32)
        blocks.append(np.concatenate([rays, rr[:, None]], -1))
    for name, (pose, _) in ref.POSE_SET.items():
        o, d = ref.frame_rays(pose, 61, 37)
        for r in radii:
            blocks.append(np.concatenate([o, d, np.full((len(o), 1), r, np.float32)], -1))
    bad_r = _random_rays(64, seed=5)
    blocks.append(np.concatenate([bad_r, np.resize(np.array([np.nan, np.inf, 0.0, -1.0], np.float32), 64)[:, None]], -1))
    rec = np.ascontiguousarray(np.concatenate(blocks), np.float32)
    (tmp / "in.bin").write_bytes(rec.tobytes())
    run = subprocess.run([str(exe), "--eval", "in.bin", "out.bin"], cwd=tmp, capture_output=True, text=True, timeout=600)
    assert run.returncode == 0, (run.stdout + run.stderr)[-4000:]
    got = np.frombuffer((tmp / "out.bin").read_bytes(), np.uint8)
    assert len(got) == len(rec)
    want = ref.near_sky_ray(rec[:, :3], rec[:, 3:6], rec[:, 6])
    bad = np.flatnonzero(got.astype(bool) != want)
    print(f"{len(rec)} rays: {int(want.sum())} pass by the restatement, {int(got.sum())} by the header, "
          f"{len(bad)} disagree; first: {rec[bad[:3]].tolist()}")
    assert 0.1 < want.mean() < 0.9  # (both outcomes, in numbers)
    assert len(bad) == 0
    # any other command line is refused, and touches nothing
    assert subprocess.run([str(exe), "--eval", "in.bin"], cwd=tmp, capture_output=True).returncode == 2
