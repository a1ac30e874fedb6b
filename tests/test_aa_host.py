"""Adaptive supersampling's host-only calls (include/rm.h rm_aa_offsets,
rm_aa_edge_mask) against their restatement (tests/aa_ref.py), and the
stand-alone program tests/host/aa_rule_test.cpp, built with the host compiler
under the address and undefined-behaviour sanitizers and linked with
csrc/rm_aa_rule.cpp only (nothing of it is loaded into Python), as
tests/test_uniform_decl_host.py builds its program.  No GPU."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import oracle
import raymarching_amd as rm
from raymarching_amd import POSES
from tests import aa_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCES = [os.path.join(ROOT, "tests", "host", "aa_rule_test.cpp"),
           os.path.join(ROOT, "raymarching_amd", "csrc", "rm_aa_rule.cpp")]
FLAGS = ["-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]


@pytest.mark.parametrize("K", [2, 4, 8])
def test_offsets_are_the_tables(K):
    got = rm.aa_offsets(K)
    assert got.dtype == np.float32 and got.shape == (K, 2)
    assert np.array_equal(got, aa_ref.offsets(K))
    # exact in f32, and so is o + 0.5: u_seed1 = o + 0.5 renders exactly that sample
    assert np.array_equal(got.astype(np.float64) * 16.0, np.rint(got.astype(np.float64) * 16.0))
    for o, seed in zip(got, aa_ref.seeds(K)):
        assert oracle.seed_jitter(seed) == (float(o[0]), float(o[1]))
        assert 0.0 <= float(seed[0]) < 1.0 and 0.0 <= float(seed[1]) < 1.0


@pytest.mark.parametrize("K", [0, 3, 16])
def test_offsets_refuse_other_counts(K):
    with pytest.raises(rm.RmError) as e:
        rm.aa_offsets(K)
    assert e.value.status == 1  # RM_ERR_INVALID_ARGUMENT


@pytest.mark.parametrize("W,H", [(61, 37), (5, 3), (1, 1), (8, 8), (9, 1)])
@pytest.mark.parametrize("threshold", [0, 1, 37, 255])
@pytest.mark.parametrize("contrast", ["full", "low"])
def test_edge_mask_on_noise(W, H, threshold, contrast):
    rng = np.random.default_rng(1000 * W + H)
    frame = rng.integers(0, 2 ** 32, (H, W), dtype=np.uint32)
    if contrast == "low":  # bytes in 64..105, so that threshold 37 gives both answers
        frame = rng.integers(64, 106, (H, W, 4), dtype=np.uint8).view(np.uint32).reshape(H, W)
    got = rm.aa_edge_mask(frame, threshold)
    want = aa_ref.edge_mask(frame, threshold)
    assert got.dtype == np.uint8 and np.array_equal(got, want)
    if threshold == 0:
        assert got.all()
    if (W, H) == (1, 1) and threshold >= 1:
        assert not got.any()
    if (W, H) == (61, 37) and threshold == 37 and contrast == "low":
        assert 0 < int(got.sum()) < W * H


@pytest.mark.parametrize("scene", ["T", "O"])
def test_edge_mask_on_oracle_frames(scene):
    """The packed oracle frames the GPU tests' sizes and poses give: the rule
    against its restatement, and an edge share that exercises both branches
    (measured on the CPU: T 0.148, O 0.595)."""
    pose = POSES["P2"]
    W, H = 61, 37
    img, _ = oracle.render(scene, W, H, pos=pose["pos"], mouse=pose["mouse"], time=pose["time"], max_steps=128)
    frame = oracle.pack_rgba8(img)
    got = rm.aa_edge_mask(frame, 32)
    assert np.array_equal(got, aa_ref.edge_mask(frame, 32))
    share = float(got.mean())
    print(f"edge share {scene} {W}x{H} P2 threshold 32: {share:.3f}")
    assert 0.03 <= share <= 0.7, share


def test_edge_mask_takes_int32_words_and_refuses_bad_input():
    frame = np.array([[0, 0x00ffffff], [-1, 0]], np.int32)  # RGBA8 words as torch holds them
    assert np.array_equal(rm.aa_edge_mask(frame, 1), aa_ref.edge_mask(frame, 1))
    with pytest.raises(rm.RmError):
        rm.aa_edge_mask(frame, 256)
    with pytest.raises(rm.RmError):
        rm.aa_edge_mask(frame, -1)
    with pytest.raises(ValueError):
        rm.aa_edge_mask(np.zeros((2, 2, 4), np.uint8), 1)


def test_tree_mean_is_the_pairwise_tree():
    """aa_ref.tree_mean sums in the stated order (f32, each step rounded)."""
    f = np.float32
    s = [f(1.0), f(2.0 ** -24), f(2.0 ** -24), f(0.0)]
    # ((1 + 2^-24) + (2^-24 + 0)) * 1/4: the first pair rounds to 1, the second survives
    want = (f(f(s[0] + s[1]) + f(s[2] + s[3])) * f(0.25))
    assert aa_ref.tree_mean(s) == want
    rng = np.random.default_rng(7)
    v = rng.random((8, 5, 3), np.float32)
    t = aa_ref.tree_mean(list(v))
    want8 = (((v[0] + v[1]) + (v[2] + v[3])) + ((v[4] + v[5]) + (v[6] + v[7]))) * f(0.125)
    assert t.dtype == np.float32 and np.array_equal(t, want8)


def _compiler():
    if shutil.which("g++"):  # (gcc's sanitizer runtimes are shared by default: link them in, as clang does)
        return ["g++", "-static-libasan", "-static-libubsan"]
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    return [hipcc, "-x", "c++"] if os.path.exists(hipcc) else None


def test_rule_under_sanitizers(tmp_path):
    cxx = _compiler()
    if cxx is None:
        pytest.skip("no host C++ compiler (g++ or hipcc)")
    exe = tmp_path / "aa_rule_test"
    build = subprocess.run(cxx + FLAGS + SOURCES + ["-o", str(exe)], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-4000:]
    run = subprocess.run([str(exe)], cwd=tmp_path, capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, (run.stdout + run.stderr)[-4000:]
    assert "all checks passed" in run.stdout
