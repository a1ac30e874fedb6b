"""bench.py's plain run and --dump-outputs: a plain run prints the headline
line only (what --full adds is absent), and the frame it dumps is the last
timed frame -- bit for bit the instrumented kernel's frame of the same pose.
dump_outputs itself (whole frame, or the fixed seeded sample of a frame over
DUMP_MAX_BYTES) is host logic and is checked without a GPU."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402

FULL_ONLY = ("kernel_ms", "roofline", "frame_check", "post_pass", "bloom_pass", "pipeline", "pipeline_ms",
             "cpu_baseline")


def test_dump_whole_frame(tmp_path):
    import torch
    g = torch.Generator().manual_seed(1)
    frame = torch.randint(-2**31, 2**31 - 1, (37, 61), dtype=torch.int32, generator=g)
    bench.dump_outputs(str(tmp_path), frame, "rgba8")
    assert sorted(os.listdir(tmp_path)) == ["frame.npy"]
    a = np.load(tmp_path / "frame.npy")
    assert a.dtype == np.float32 and a.shape == (37 * 61, 4)
    assert np.array_equal(a.astype(np.uint8).reshape(-1), frame.numpy().view(np.uint8).reshape(-1))
    f4 = torch.rand((5, 7, 4), generator=g)
    bench.dump_outputs(str(tmp_path / "f4"), f4, "float4")
    assert np.array_equal(np.load(tmp_path / "f4" / "frame.npy"), f4.numpy().reshape(-1, 4))


def test_dump_samples_a_large_frame_the_same_way_every_time(tmp_path, monkeypatch):
    import torch
    monkeypatch.setattr(bench, "DUMP_MAX_BYTES", 16 * 1000)  # room for 1000 pixels
    frame = torch.arange(96 * 64, dtype=torch.int32).reshape(64, 96) * 65537
    bench.dump_outputs(str(tmp_path / "a"), frame, "rgba8")
    bench.dump_outputs(str(tmp_path / "b"), frame, "rgba8")
    a, ia = np.load(tmp_path / "a" / "frame.npy"), np.load(tmp_path / "a" / "frame_pixels.npy")
    assert a.dtype == np.float32 and a.shape == (1000, 4) and ia.dtype == np.float64 and ia.shape == (1000,)
    assert np.array_equal(a, np.load(tmp_path / "b" / "frame.npy"))
    assert np.array_equal(ia, np.load(tmp_path / "b" / "frame_pixels.npy"))
    idx = ia.astype(np.int64)
    assert (np.diff(idx) > 0).all() and idx[0] >= 0 and idx[-1] < 96 * 64  # distinct pixels of the frame, ascending
    assert np.array_equal(a.astype(np.uint8), frame.numpy().view(np.uint8).reshape(-1, 4)[idx])


def test_dump_of_the_flagship_frame_fits_the_budget():
    # C3's 4096 x 4096 frame: values (float32 x 4) and indices (float64) of the sampled pixels
    keep = bench.DUMP_MAX_BYTES // 16
    assert keep < 4096 * 4096 and keep * (16 + 8) <= 64 * 10**6


@pytest.mark.gpu
def test_plain_run_prints_the_headline_only_and_dumps_the_last_frame(torch_cuda, tmp_path):
    torch = torch_cuda
    import raymarching_amd as rm
    cmd = [sys.executable, "bench.py", "--steps", "3", "--warmup", "1", "--spinup", "0", "--size", "512",
           "--dump-outputs", str(tmp_path)]
    out = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, (out.returncode, out.stdout[-2000:], out.stderr[-3000:])
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, out.stdout[-2000:]
    res = json.loads(lines[0])
    assert res["steps"] == 3 and res["full"] is False and not [k for k in FULL_ONLY if k in res], sorted(res)
    assert res["unit"] == "ray-steps/s" and res["higher_is_better"] is True and res["dtype"] == "f32", res
    assert res["ms_per_step"] > 0 and res["value"] == pytest.approx(
        res["config"]["ray_steps_per_frame"] / (res["ms_per_step"] / 1e3), rel=1e-9), res
    a = np.load(tmp_path / "frame.npy")
    assert a.dtype == np.float32 and a.shape == (512 * 512, 4) and not os.path.exists(tmp_path / "frame_pixels.npy")
    # the same frame by the instrumented kernel (every reference ray-step), in this process
    pose = rm.POSES["P0"]
    r = rm.Renderer(0)
    r.load_scene(rm.SCENE_FILES["T"])
    r.set_uniform("u_resolution", 512, 512)
    r.set_pose(pose["pos"], pose["mouse"], pose["time"])
    r.set_params(max_steps=256, shadow_max_steps=0, count_evals=1)
    ref = r.render_rgba8(512, 512)
    torch.cuda.synchronize()
    r.close()
    assert np.array_equal(a.astype(np.uint8), ref.cpu().numpy().view(np.uint8).reshape(-1, 4))
