"""Scene T's far-sky shortcut on the CPU (raymarching_amd/csrc/rm_far_sky.h,
DESIGN.md 2.22): the stand-alone program tests/host/far_sky_test.cpp, built with
the host compiler under the address and undefined-behaviour sanitizers (nothing
of it is loaded into Python), as tests/test_aa_host.py builds its program.  It
includes the predicate's header, restates cast_ray_T's loop over the Menger
distance and the reflection march's first step, and checks on 1.2 million seeded
random rays and the directed cases that every accepted ray's march returns
exactly ZFAR within N0 steps and its reflection factor is exactly 1.  The same
program in its second mode (--eval in.bin out.bin) gives rmfs::far_sky_ray for
rays from a file: the numpy restatement that composes the waves of
tests/test_shade_rays_shortcuts.py (tests/far_sky_ref.py) is held to it with zero
disagreements.  No GPU."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import far_sky_ref, shade_t_rays

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCE = os.path.join(ROOT, "tests", "host", "far_sky_test.cpp")
# -O1 under the sanitizers; no contraction: the restated roundings are the source's own
FLAGS = ["-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]


def _compiler():
    if shutil.which("g++"):  # (gcc's sanitizer runtimes are shared by default: link them in, as clang does)
        return ["g++", "-static-libasan", "-static-libubsan"]
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    return [hipcc, "-x", "c++"] if os.path.exists(hipcc) else None


def _build(tmp_path):
    cxx = _compiler()
    if cxx is None:
        pytest.skip("no host C++ compiler (g++ or hipcc)")
    exe = tmp_path / "far_sky_test"
    build = subprocess.run(cxx + FLAGS + [SOURCE, "-o", str(exe)], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-4000:]
    return exe


def test_far_sky_predicate_under_sanitizers(tmp_path):
    exe = _build(tmp_path)
    run = subprocess.run([str(exe)], cwd=tmp_path, capture_output=True, text=True, timeout=600)
    print(run.stdout)
    assert run.returncode == 0, (run.stdout + run.stderr)[-4000:]
    assert "all checks passed" in run.stdout


def _random_rays(n, seed=20261021):
    """sponge-space rays round the predicate's thresholds: origins from 0.3 to 60 from the centre (a few beyond
    |o|_1 = 1024, a few non-finite), directions of unit length and not, and rays built to graze the tested cube"""
    rng = np.random.RandomState(seed)
    u = rng.normal(size=(n, 3))
    u /= np.linalg.norm(u, axis=-1, keepdims=True)
    o = u * np.exp(rng.uniform(np.log(0.3), np.log(60.0), size=(n, 1)))
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=-1, keepdims=True)
    k = np.arange(n) % 8
    # a quarter through a point within 0.01 of the tested cube's surface, across an edge
    g = float(far_sky_ref.K_R) + rng.uniform(-0.01, 0.01, size=n)
    P = np.stack([g * rng.choice([-1.0, 1.0], size=n), g * rng.choice([-1.0, 1.0], size=n), rng.uniform(-1.3, 1.3, size=n)], -1)
    e = np.stack([np.sign(P[:, 0]) * rng.uniform(0.2, 1.0, size=n), -np.sign(P[:, 1]) * rng.uniform(0.2, 1.0, size=n),
                  rng.uniform(-1.0, 1.0, size=n)], -1)
    e /= np.linalg.norm(e, axis=-1, keepdims=True)
    roll = rng.randint(0, 3, size=n)
    P = np.stack([np.roll(p, r) for p, r in zip(P, roll)])
    e = np.stack([np.roll(p, r) for p, r in zip(e, roll)])
    graze = (k == 1) | (k == 5)
    o[graze], d[graze] = (P - e * rng.uniform(0.5, 8.0, size=(n, 1)))[graze], e[graze]
    # an eighth with the far point near kFarSkyFar: 46 to 54 away, passing beside the sponge
    far = k == 2
    o[far] = (u * rng.uniform(46.0, 54.0, size=(n, 1)))[far]
    t = rng.normal(size=(n, 3))
    t = t / np.linalg.norm(t, axis=-1, keepdims=True) * rng.uniform(2.0, 5.0, size=(n, 1)) - o
    d[far] = (t / np.linalg.norm(t, axis=-1, keepdims=True))[far]
    o, d = o.astype(np.float32), d.astype(np.float32)
    d[k == 3] *= np.float32(1.5)                       # not unit: the predicate itself does not ask for it
    o[k == 4] *= np.float32(40.0)                      # up to 2400 away: some beyond |o|_1 = 1024
    axis = k == 6                                      # axis-parallel directions, zeros of both signs
    d[axis] = np.where(np.abs(d[axis]) == np.abs(d[axis]).max(-1, keepdims=True), np.sign(d[axis]), np.float32(-0.0))
    bad = np.flatnonzero(k == 7)[:300]
    for j, i in enumerate(bad):                        # a NaN or an infinity in one component
        (o if j % 2 else d)[i, j % 3] = (np.nan, np.inf, -np.inf)[j % 3]
    return np.concatenate([o, d], -1).astype(np.float32)


def test_numpy_restatement_is_the_headers_predicate(tmp_path):
    """tests/far_sky_ref.far_sky_ray against rmfs::far_sky_ray itself, ray by ray: every ray of the sets of
    tests/shade_t_rays.py (in sponge space, class G's too) and 100 000 seeded random rays.  Zero disagreements."""
    exe = _build(tmp_path)
    rays = [_random_rays(100000)]
    for time in shade_t_rays.TIMES:
        s = shade_t_rays.ray_set(time)
        o, d = far_sky_ref.to_sponge(s["pos"], shade_t_rays.all_dirs(s), time)
        rays.append(np.concatenate([o, d], -1).astype(np.float32))
    rays = np.ascontiguousarray(np.concatenate(rays), np.float32)
    (tmp_path / "in.bin").write_bytes(rays.tobytes())
    run = subprocess.run([str(exe), "--eval", "in.bin", "out.bin"], cwd=tmp_path, capture_output=True, text=True, timeout=600)
    assert run.returncode == 0, (run.stdout + run.stderr)[-4000:]
    got = np.frombuffer((tmp_path / "out.bin").read_bytes(), np.uint8)
    assert len(got) == len(rays)
    want = far_sky_ref.far_sky_ray(rays[:, :3], rays[:, 3:])
    bad = np.flatnonzero(got.astype(bool) != want)
    print(f"{len(rays)} rays: {int(want.sum())} far-sky by the restatement, {int(got.sum())} by the header, "
          f"{len(bad)} disagree; first: {rays[bad[:3]].tolist()}")
    assert 0.1 < want.mean() < 0.9  # (both outcomes, in numbers)
    assert len(bad) == 0
    # any other command line is refused, and touches nothing
    assert subprocess.run([str(exe), "--eval", "in.bin"], cwd=tmp_path, capture_output=True).returncode == 2
