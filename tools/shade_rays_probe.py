#!/usr/bin/env python3
"""rm_shade_rays timed on the GPU beside the frame kernels: scene T at 256
steps and scene O at 512 steps (pose P0, the poses of C3 and of bench.py
--scene O), size^2 rays, RGBA8 targets, display colour.

Per round, interleaved, each between two HIP events on the context's stream:
  (a) rm_render_rgba8 with schedule = 0 (row-major: the shade call has no
      adaptive order), the baseline;
  (b) rm_shade_rays over the frame's own rays (rm_camera_rays) as a ray image
      (width = size, the frame's vignette): the same rays as (a);
  (c) the same rays as a list (width = 0): 64 x 1 strips instead of 8 x 8 tiles;
  (d) cameras.fisheye_rays(size, size, 110) as a ray image;
  (e) the six faces of a --cube^2 cube map, one call per face, beside
      (f) six rm_render_rgba8 frames of --cube^2.
Two warm-up rounds, then --rounds timed ones; medians, with the min..max
spread.  One JSON line per case, appended to --out.

usage: python tools/shade_rays_probe.py [--size 4096] [--cube 1024] [--rounds 12] [--out profiles/shade_rays.jsonl]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import raymarching_amd as rm  # noqa: E402

CASES = [("T", "template.frag", 256), ("O", "output_shader.frag", 512)]


def stat(values):
    v = np.asarray(values, np.float64)
    return dict(median=round(float(np.median(v)), 4), min=round(float(v.min()), 4), max=round(float(v.max()), 4))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=4096)
    ap.add_argument("--cube", type=int, default=1024)
    ap.add_argument("--rounds", type=int, default=12)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "shade_rays.jsonl"))
    a = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "shade_rays_probe.py measures on the GPU"
    r = rm.Renderer(0)
    pose = rm.POSES["P0"]
    W = H = a.size
    C = a.cube
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    sink = open(a.out, "a")

    def emit(**row):
        line = json.dumps(row)
        print(line, flush=True)
        sink.write(line + "\n")
        sink.flush()

    def between_events(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        return e0, e1

    fisheye = torch.from_numpy(rm.fisheye_rays(W, H, 110.0, pose["mouse"])).cuda().reshape(-1, 3)
    faces = [torch.from_numpy(rm.cubemap_rays(C, f)).cuda().reshape(-1, 3) for f in range(6)]
    origin = np.array(pose["pos"], np.float32)
    for scene, file, steps in CASES:
        r.load_scene(file)
        r.set_pose(pose["pos"], pose["mouse"], pose["time"])
        r.set_params(max_steps=steps, shadow_max_steps=0, count_evals=0, kernel="auto", schedule="rowmajor")
        frame = torch.empty((H, W), dtype=torch.int32, device="cuda")
        out = torch.empty(H * W, dtype=torch.int32, device="cuda")
        small = torch.empty((C, C), dtype=torch.int32, device="cuda")
        _, dirs = r.camera_rays(W, H)
        dirs = dirs.reshape(-1, 3)
        r.render_rgba8(W, H, out=frame)
        r.shade_rays(origin, dirs, width=W, vignette=True, rgba8=True, out=out)
        r.synchronize()
        same = bool((frame.reshape(-1) == out).all().item())

        def cube_shade():
            for f in faces:
                r.shade_rays(origin, f, width=C, rgba8=True, out=out)

        def cube_frames():
            for _ in range(6):
                r.render_rgba8(C, C, out=small)

        runs = {
            "a": lambda: r.render_rgba8(W, H, out=frame),
            "b": lambda: r.shade_rays(origin, dirs, width=W, vignette=True, rgba8=True, out=out),
            "c": lambda: r.shade_rays(origin, dirs, width=0, rgba8=True, out=out),
            "d": lambda: r.shade_rays(origin, fisheye, width=W, vignette=True, rgba8=True, out=out),
            "e": cube_shade,
            "f": cube_frames,
        }
        ms = {k: [] for k in runs}
        for rnd in range(2 + a.rounds):
            pending = [(k, between_events(fn)) for k, fn in runs.items()]
            torch.cuda.synchronize()
            if rnd >= 2:
                for k, (e0, e1) in pending:
                    ms[k].append(e0.elapsed_time(e1))
        med = {k: float(np.median(v)) for k, v in ms.items()}
        common = dict(scene=scene, max_steps=steps, size=a.size, rounds=a.rounds, code=rm.render_code_hash())
        emit(case="a: rm_render_rgba8, schedule 0", ms=stat(ms["a"]), **common)
        emit(case="b: rm_shade_rays, the frame's rays, width = size", ms=stat(ms["b"]),
             ratio_to_a=round(med["b"] / med["a"], 4), equals_frame=same, **common)
        emit(case="c: rm_shade_rays, the frame's rays, width = 0", ms=stat(ms["c"]),
             ratio_to_b=round(med["c"] / med["b"], 4), **common)
        emit(case="d: rm_shade_rays, fisheye 110, width = size", ms=stat(ms["d"]),
             ratio_to_a=round(med["d"] / med["a"], 4), **common)
        emit(case=f"e: rm_shade_rays, six {C}^2 cube-map faces", ms=stat(ms["e"]),
             ratio_to_f=round(med["e"] / med["f"], 4), cube=C, **common)
        emit(case=f"f: six rm_render_rgba8 of {C}^2, schedule 0", ms=stat(ms["f"]), cube=C, **common)
        del frame, out, small, dirs
        torch.cuda.empty_cache()
    r.close()


if __name__ == "__main__":
    main()
