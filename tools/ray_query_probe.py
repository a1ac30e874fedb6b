#!/usr/bin/env python3
"""Ray queries (rm_cast_rays) timed on the GPU: the camera rays of a size^2
frame and an incoherent ray set, for scene T (256 steps) and scene O (512
steps) at P0, with distance-only outputs and with position + normal, in 64-
and 256-thread workgroups (RM_CAST_BLOCK, alternated launch by launch), and
rm_render_rgba8 of the same frame beside scene O's G-buffer.

Each case: warm-up launches for 0.3 s, then --reps (>= 20) timed launches,
every one between two HIP events on the renderer's stream; the median is
reported, with rays/s and ray-steps/s (the steps from rm_stats.evals of one
instrumented call).  One JSON line per case, appended to --out.

usage: python tools/ray_query_probe.py [--size 4096] [--incoherent-log2 24] [--reps 20]
                                       [--out profiles/ray_queries.jsonl]
"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import raymarching_amd as rm  # noqa: E402
from raymarching_amd import _lib  # noqa: E402
from tests.ray_ref import ray_set  # noqa: E402

CASES = [("T", "template.frag", 256), ("O", "output_shader.frag", 512)]


def incoherent_rays(log2n, torch):
    """tests/ray_ref.py's 4096-ray set (seed 5, aimed at the sponge), tiled to 2^log2n rays and shuffled"""
    o, d = ray_set("O")
    g = torch.Generator(device="cpu").manual_seed(5)
    idx = (torch.randperm(1 << log2n, generator=g) % len(d)).cuda()
    return torch.from_numpy(o).cuda()[idx].contiguous(), torch.from_numpy(d).cuda()[idx].contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=4096)
    ap.add_argument("--incoherent-log2", type=int, default=24)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ray_queries.jsonl"))
    a = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "ray_query_probe.py measures on the GPU"
    L = rm.lib()
    r = rm.Renderer(0)
    pose = rm.POSES["P0"]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    sink = open(a.out, "a")

    def emit(**row):
        line = json.dumps(row)
        print(line, flush=True)
        sink.write(line + "\n")
        sink.flush()

    def timed(launch, variants):
        """median ms per variant; the variants alternate launch by launch"""
        t_end = time.time() + 0.3
        while time.time() < t_end:
            for v in variants:
                launch(v)
        torch.cuda.synchronize()
        ev = {v: [] for v in variants}
        for _ in range(max(20, a.reps)):
            for v in variants:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                launch(v)
                e1.record()
                ev[v].append((e0, e1))
        torch.cuda.synchronize()
        return {v: float(np.median([x.elapsed_time(y) for x, y in ev[v]])) for v in variants}

    for scene, file, steps in CASES:
        r.load_scene(file)
        r.set_pose(pose["pos"], pose["mouse"], pose["time"])
        r.set_params(max_steps=steps, shadow_max_steps=0, count_evals=0, kernel="auto")
        origin, dirs = r.camera_rays(a.size, a.size)
        sets = [("camera", origin, dirs.reshape(-1, 3), 1)]
        io, idirs = incoherent_rays(a.incoherent_log2, torch)
        sets.append(("incoherent", io, idirs, 0))
        for set_name, o, d, shared in sets:
            n = d.shape[0]
            t = torch.empty(n, device="cuda")
            status = torch.empty(n, dtype=torch.int32, device="cuda")
            nsteps = torch.empty(n, dtype=torch.int32, device="cuda")
            pos = torch.empty((n, 3), device="cuda")
            nrm = torch.empty((n, 3), device="cuda")
            outputs = {"distance": _lib.RmRayHits(t.data_ptr(), None, None, None, None, None),
                       "position+normal": _lib.RmRayHits(t.data_ptr(), status.data_ptr(), nsteps.data_ptr(),
                                                         pos.data_ptr(), nrm.data_ptr(), None)}
            for out_name, hits in outputs.items():
                def launch(block, stats=None):
                    os.environ["RM_CAST_BLOCK"] = str(block)
                    _lib.check(L.rm_cast_rays(r._ctx, o.data_ptr(), shared, d.data_ptr(), n, 0, ctypes.byref(hits),
                                              stats), r._ctx)
                st = _lib.RmStats()
                launch(64, ctypes.byref(st))
                ms = timed(launch, (64, 256))
                for block in (64, 256):
                    emit(scene=scene, max_steps=steps, rays=set_name, n=n, outputs=out_name, block=block,
                         ms=round(ms[block], 4), rays_per_s=n / (ms[block] * 1e-3), ray_steps=int(st.evals),
                         ray_steps_per_s=int(st.evals) / (ms[block] * 1e-3), reps=max(20, a.reps),
                         code=rm.render_code_hash())
            del t, status, nsteps, pos, nrm
        os.environ.pop("RM_CAST_BLOCK", None)
        # the frame the camera rays belong to, beside its G-buffer
        frame = torch.empty((a.size, a.size), dtype=torch.int32, device="cuda")
        ms = timed(lambda _: r.render_rgba8(a.size, a.size, out=frame), ("render",))
        emit(scene=scene, max_steps=steps, rays="camera", n=a.size * a.size, outputs="rm_render_rgba8", block=64,
             ms=round(ms["render"], 4), reps=max(20, a.reps), code=rm.render_code_hash())
        del frame, origin, dirs, io, idirs, sets
        torch.cuda.empty_cache()
    r.close()


if __name__ == "__main__":
    main()
