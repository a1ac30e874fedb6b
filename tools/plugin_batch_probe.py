#!/usr/bin/env python3
"""View batches of scene plugins (rm_render_batch_ex_rgba8) timed on the GPU,
beside the loop a caller writes without them: scenes/output_shader_knobs.hip
(u_ball and u_spin set per view) and scenes/mandelbulb.hip (no uniforms), 512
steps, RGBA8, views from cameras.turntable with u_time advancing, in DESIGN.md
2.26's shapes: 4096 views of 64^2, 256 of 256^2, eight of 1920x1080, one 4096^2.

Per shape and round, interleaved, each region between two HIP events on the
renderer's stream and ended by a synchronise:
  (a) one rm_render_batch_ex_rgba8 of the n views with their per-view uniforms
      (device target, no stats); also the host time of the call alone, up to its
      return (it packs the uniform blocks, builds and uploads the records);
  (b) n x (u_pos, u_mouse, u_time, the scene's per-view uniforms,
      rm_render_rgba8) on the same stream, no stats, rm_params.schedule = 0,
      through ctypes with the arguments prepared beforehand; its host time too.
(b) runs the plugin's frame kernels, which the batch form does not touch.  Two
warm-up rounds of every shape (the first compiles the batch form), then
--rounds timed ones; medians with the min..max spread.  The single 4096^2 view
also states the n = 1 condition: the batch against rm_render_rgba8 (schedule 0)
of the same plugin in the same run, and whether the gap lies within the two
regions' own min..max spread.  One JSON line per row, appended to --out.

usage: python tools/plugin_batch_probe.py [--rounds 8] [--out profiles/plugin_batch.jsonl]
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

STEPS = 512
SHAPES = [(64, 64, 4096), (256, 256, 256), (1920, 1080, 8), (4096, 4096, 1)]
RADIUS, HEIGHT = 5.0, 4.0  # the turntable's circle


def stat(values):
    v = np.asarray(values, np.float64)
    return dict(median=round(float(np.median(v)), 4), min=round(float(v.min()), 4), max=round(float(v.max()), 4))


def knob_uniforms(n):
    """the ball moves on a small circle and the spin changes, view by view"""
    k = np.arange(n, dtype=np.float32)
    a = k * np.float32(2.0 * np.pi / max(n, 1))
    ball = np.stack([3.0 + 0.5 * np.cos(a), np.full(n, 2.0, np.float32), 3.0 + 0.5 * np.sin(a),
                     np.full(n, 1.0, np.float32)], -1).astype(np.float32)
    spin = (2.0 + k / np.float32(max(n, 1))).astype(np.float32)
    return {"u_ball": ball, "u_spin": spin}


CASES = [("knobs", "output_shader_knobs.hip", knob_uniforms), ("mandelbulb", "mandelbulb.hip", lambda n: {})]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=8)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "plugin_batch.jsonl"))
    a = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "plugin_batch_probe.py measures on the GPU"
    L = rm.lib()
    r = rm.Renderer(0)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    sink = open(a.out, "a")

    def emit(**row):
        line = json.dumps(row)
        print(line, flush=True)
        sink.write(line + "\n")
        sink.flush()

    def region(fn):
        """(GPU ms between the events, host ms of fn alone); ends in a synchronise"""
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        t0 = time.perf_counter()
        fn()
        host = (time.perf_counter() - t0) * 1e3
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1), host

    for scene, file, uniforms_of in CASES:
        r.load_scene(os.path.join(rm.SCENES_DIR, file))
        r.set_params(max_steps=STEPS, shadow_max_steps=0, count_evals=0, kernel="auto", schedule=0)
        t0 = time.perf_counter()
        r.batch_prepare()
        prepare_ms = (time.perf_counter() - t0) * 1e3
        ctx = r._ctx
        for W, H, n in SHAPES:
            views = rm.turntable(n, RADIUS, HEIGHT, target_time=0.0)
            for k, v in enumerate(views):
                v["time"] = 0.125 * k  # an animation: u_time advances with the view
            packed = rm.pack_views(views)
            u = uniforms_of(n)
            entries = [_lib.RmViewUniform(name.encode(), int(v.shape[1]) if v.ndim > 1 else 1, 1,
                                          ctypes.c_void_p(v.ctypes.data)) for name, v in u.items()]
            arr = (_lib.RmViewUniform * max(1, len(entries)))(*entries)
            out = torch.empty((n, H, W), dtype=torch.int32, device="cuda")
            frame = torch.empty((H, W), dtype=torch.int32, device="cuda")
            fp = ctypes.c_void_p(frame.data_ptr())

            def batch():
                st = L.rm_render_batch_ex_rgba8(ctx, W, H, ctypes.c_void_p(packed.ctypes.data), n,
                                                ctypes.cast(arr, ctypes.c_void_p) if entries else None, len(entries),
                                                ctypes.c_void_p(out.data_ptr()), None)
                assert st == 0, L.rm_last_error(ctx)

            args = [((float(v[0]), float(v[1]), float(v[2])), (float(v[3]), float(v[4])), float(v[5]),
                     tuple(float(x) for x in u["u_ball"][k]) if u else None, float(u["u_spin"][k]) if u else None)
                    for k, v in enumerate(packed)]

            def loop():
                for pos, mouse, t, ball, spin in args:
                    L.rm_set_uniform3f(ctx, b"u_pos", *pos)
                    L.rm_set_uniform2f(ctx, b"u_mouse", *mouse)
                    L.rm_set_uniform1f(ctx, b"u_time", t)
                    if ball is not None:
                        L.rm_set_uniform4f(ctx, b"u_ball", *ball)
                        L.rm_set_uniform1f(ctx, b"u_spin", spin)
                    L.rm_render_rgba8(ctx, W, H, fp, None)

            res = {k: [] for k in ("batch", "batch_host", "loop", "loop_host")}
            for rnd in range(2 + a.rounds):
                ms_a, host_a = region(batch)
                ms_b, host_b = region(loop)
                if rnd >= 2:
                    for k, v in zip(res, (ms_a, host_a, ms_b, host_b)):
                        res[k].append(v)
            med = {k: float(np.median(v)) for k, v in res.items()}
            row = dict(case="plugin_batch_vs_loop", scene=scene, max_steps=STEPS, W=W, H=H, n=n, rounds=a.rounds,
                       uniforms_per_view=sorted(u), batch_ms=stat(res["batch"]), batch_host_ms=stat(res["batch_host"]),
                       loop_sched0_ms=stat(res["loop"]), loop_sched0_host_ms=stat(res["loop_host"]),
                       loop_over_batch=round(med["loop"] / med["batch"], 4),
                       batch_views_per_s=round(n / (med["batch"] * 1e-3), 1),
                       loop_views_per_s=round(n / (med["loop"] * 1e-3), 1), prepare_ms=round(prepare_ms, 1))
            if n == 1:  # the n = 1 condition: the same code over the same tiles
                spread = max(max(res["batch"]) - min(res["batch"]), max(res["loop"]) - min(res["loop"]))
                row.update(n1_gap_ms=round(med["batch"] - med["loop"], 4), n1_spread_ms=round(spread, 4),
                           n1_within_spread=bool(med["batch"] - med["loop"] <= spread))
            emit(**row)
            del out, frame
            torch.cuda.empty_cache()
    r.close()


if __name__ == "__main__":
    main()
