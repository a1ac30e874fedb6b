#!/usr/bin/env python3
"""Adaptive supersampling of a view batch (rm_render_batch_aa_rgba8) timed on
the GPU, beside the loop a caller writes without it: scene T at 256 steps and
scene O at 512 steps, K = 4, thresholds 32 and 0 (every pixel), views from
cameras.turntable, at 4096 x 64^2, 256 x 256^2, 8 x 1920x1080 and 1 x 4096^2.

Per case and round, interleaved, each region between two HIP events on the
renderer's stream and ended by a synchronise:
  (a) one rm_render_batch_aa_rgba8 of the n views (device target, no mask, no
      stats), once per counter layout of the detect kernel
      (RM_BATCH_AA_COUNTERS=line|packed, alternated call by call in one process);
  (b) n x (u_pos, u_mouse, u_time, rm_render_aa_rgba8) on the same stream, no
      stats, with rm_params.schedule = 0 and again with schedule = 1 (the
      default; it orders the base frame's tiles, which a batch does not),
      through ctypes with the arguments prepared beforehand.  It runs this
      build's single-frame kernels, which the batch does not touch, so it is
      the behaviour without the batch measured in the same session.
The host time of each call sequence alone is reported too.  Two warm-up rounds,
then --rounds timed ones; medians with the min..max spread.  After the rounds,
one pass of each with rm_aa_stats: the batch's base / detect + plan / refine
launch per layout, and the loop's (schedule 0) sums of the same over its n calls, with the
refined totals of both (they must agree).  One JSON line per case and threshold,
appended to --out.

Every case runs in a child process of its own under a time limit
(--case-timeout seconds); the first child that fails or runs out of time ends
the probe, and nothing more is started on the GPU.

usage: python tools/batch_aa_probe.py [--rounds 7] [--out profiles/batch_aa.jsonl] [--scenes T,O]
"""
import argparse
import ctypes
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import raymarching_amd as rm  # noqa: E402

SCENES = {"T": ("template.frag", 256), "O": ("output_shader.frag", 512)}
SHAPES = [(4096, 64, 64), (256, 256, 256), (8, 1920, 1080), (1, 4096, 4096)]
THRESHOLDS = (32, 0)
LAYOUTS = ("line", "packed")
K = 4
RADIUS, HEIGHT = 5.0, 4.0  # the turntable's circle


def stat(values):
    v = np.asarray(values, np.float64)
    return dict(median=round(float(np.median(v)), 4), min=round(float(v.min()), 4), max=round(float(v.max()), 4))


def run_case(scene, n, W, H, rounds, out):
    import torch
    assert torch.cuda.is_available(), "batch_aa_probe.py measures on the GPU"
    from raymarching_amd import _lib
    L = rm.lib()
    r = rm.Renderer(0)
    file, steps = SCENES[scene]
    r.load_scene(file)
    r.set_params(max_steps=steps, shadow_max_steps=0, count_evals=0, kernel="auto", schedule=0)
    ctx = r._ctx
    packed = rm.pack_views(rm.turntable(n, RADIUS, HEIGHT, target_time=0.0))
    frames = torch.empty((n, H, W), dtype=torch.int32, device="cuda")
    frame = torch.empty((H, W), dtype=torch.int32, device="cuda")
    fp, bp, vp = ctypes.c_void_p(frame.data_ptr()), ctypes.c_void_p(frames.data_ptr()), ctypes.c_void_p(packed.ctypes.data)
    args = [((float(v[0]), float(v[1]), float(v[2])), (float(v[3]), float(v[4])), float(v[5])) for v in packed]

    def batch(params, layout, stats=None):
        os.environ["RM_BATCH_AA_COUNTERS"] = layout
        st = L.rm_render_batch_aa_rgba8(ctx, W, H, vp, n, ctypes.byref(params), bp, None, None, stats)
        assert st == 0, st

    def loop(params, sums=None):
        """sums: a dict of rm_aa_stats' fields to add every call's to (each call then waits for its frame)"""
        one = _lib.RmAaStats()
        for pos, mouse, t in args:
            L.rm_set_uniform3f(ctx, b"u_pos", *pos)
            L.rm_set_uniform2f(ctx, b"u_mouse", *mouse)
            L.rm_set_uniform1f(ctx, b"u_time", t)
            st = L.rm_render_aa_rgba8(ctx, W, H, ctypes.byref(params), fp, None,
                                      ctypes.byref(one) if sums is not None else None)
            assert st == 0, st
            if sums is not None:
                for k in sums:
                    sums[k] += getattr(one, k)

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

    sink = open(out, "a")
    for threshold in THRESHOLDS:
        p = _lib.RmAaParams(K, threshold)
        res = {k: [] for k in ("line", "line_host", "packed", "packed_host", "loop", "loop_host", "loop1", "loop1_host")}
        for rnd in range(2 + rounds):
            a = region(lambda: batch(p, "line"))
            b = region(lambda: batch(p, "packed"))
            c = region(lambda: loop(p))
            r.set_params(schedule=1)
            d = region(lambda: loop(p))
            r.set_params(schedule=0)
            if rnd >= 2:
                for k, v in zip(res, a + b + c + d):
                    res[k].append(v)
        parts = {}
        for layout in LAYOUTS:
            st = _lib.RmAaStats()
            batch(p, layout, ctypes.byref(st))
            parts[layout] = st.as_dict()
        sums = dict(refined=0, base_ms=0.0, detect_ms=0.0, refine_ms=0.0)
        loop(p, sums)
        med = {k: float(np.median(v)) for k, v in res.items()}
        best = min(LAYOUTS, key=lambda lay: med[lay])
        row = dict(case="batch_aa_vs_loop", scene=scene, max_steps=steps, n=n, W=W, H=H, samples=K, threshold=threshold,
                   rounds=rounds, code=rm.render_code_hash(),
                   batch_line_ms=stat(res["line"]), batch_line_host_ms=stat(res["line_host"]),
                   batch_packed_ms=stat(res["packed"]), batch_packed_host_ms=stat(res["packed_host"]),
                   loop_sched0_ms=stat(res["loop"]), loop_sched0_host_ms=stat(res["loop_host"]),
                   loop_sched1_ms=stat(res["loop1"]), loop_sched1_host_ms=stat(res["loop1_host"]),
                   loop0_over_batch_line=round(med["loop"] / med["line"], 4),
                   loop0_over_batch_packed=round(med["loop"] / med["packed"], 4),
                   loop1_over_batch_line=round(med["loop1"] / med["line"], 4), faster_layout=best,
                   batch_line_parts={k: round(v, 4) for k, v in parts["line"].items()},
                   batch_packed_parts={k: round(v, 4) for k, v in parts["packed"].items()},
                   loop_sched0_parts_summed={k: round(v, 4) for k, v in sums.items()},
                   refined_agree=bool(parts["line"]["refined"] == parts["packed"]["refined"] == sums["refined"]),
                   edge_share=round(sums["refined"] / (n * W * H), 5))
        line = json.dumps(row)
        print(line, flush=True)
        sink.write(line + "\n")
        sink.flush()
    os.environ.pop("RM_BATCH_AA_COUNTERS", None)
    r.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "batch_aa.jsonl"))
    ap.add_argument("--scenes", default="T,O")
    ap.add_argument("--case-timeout", type=int, default=420)
    ap.add_argument("--case", default="", help="(a child's own arguments) scene,n,W,H")
    a = ap.parse_args()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    if a.case:
        scene, n, W, H = a.case.split(",")
        run_case(scene, int(n), int(W), int(H), a.rounds, a.out)
        return 0
    for scene in a.scenes.split(","):
        for n, W, H in SHAPES:
            cmd = [sys.executable, os.path.abspath(__file__), "--case", f"{scene},{n},{W},{H}", "--rounds", str(a.rounds),
                   "--out", a.out]
            try:
                rc = subprocess.run(cmd, timeout=a.case_timeout).returncode
            except subprocess.TimeoutExpired:
                rc = 124
            if rc != 0:  # a fault, an abort or a time limit: nothing more is started on the GPU
                print(f"batch_aa_probe: case {scene} {n} x {W}x{H} ended with status {rc}; stopping", flush=True)
                return rc if rc > 0 else 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
