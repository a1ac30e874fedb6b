#!/usr/bin/env python3
"""Adaptive supersampling of scene plugins (rm_render_aa_ex_rgba8; DESIGN.md
2.31) timed on the GPU, beside what a plugin's caller pays today:
scenes/output_shader_knobs.hip and scenes/mandelbulb.hip at 512 steps, pose P0,
size^2 pixels, K samples, at edge thresholds 64, 32, 16 and 0 (every pixel).

tools/aa_probe.py's method.  Per round, interleaved: rm_render_rgba8 alone, K
launches of rm_render_accumulate_rgba8 (the same samples everywhere), and per
threshold one rm_render_aa_ex_rgba8 between two HIP events (total_ms,
asynchronous call) and one with rm_aa_stats (base_ms, detect_ms, refine_ms,
refined).  Two warm-up rounds, then --rounds timed ones; medians, with the
min..max spread.  One JSON line per case, appended to --out; prepare_ms is the
rm_aa_prepare before the scene's first call (the AA form's compile and load).

Each scene is measured by a fresh child process under a time limit of its own;
after a child that fails or runs out of time nothing more is started.

usage: python tools/plugin_aa_probe.py [--size 4096] [--samples 4] [--rounds 12] [--out profiles/plugin_aa.jsonl]
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SCENES = ("output_shader_knobs.hip", "mandelbulb.hip")
STEPS = 512
THRESHOLDS = (64, 32, 16, 0)
CHILD_LIMIT_S = 420


def stat(values):
    v = np.asarray(values, np.float64)
    return dict(median=round(float(np.median(v)), 4), min=round(float(v.min()), 4), max=round(float(v.max()), 4))


def measure(a, scene):
    import torch

    import raymarching_amd as rm
    assert torch.cuda.is_available(), "plugin_aa_probe.py measures on the GPU"
    r = rm.Renderer(0)
    pose = rm.POSES["P0"]
    W = H = a.size
    K = a.samples
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

    seeds = [(float(o[0]) + 0.5, float(o[1]) + 0.5) for o in rm.aa_offsets(K)]
    r.load_scene(os.path.join(rm.SCENES_DIR, scene))
    r.set_pose(pose["pos"], pose["mouse"], pose["time"])
    r.set_params(max_steps=STEPS, shadow_max_steps=0, count_evals=0, kernel="auto")
    t0 = time.perf_counter()
    r.aa_prepare()
    prepare_ms = (time.perf_counter() - t0) * 1e3
    frame = torch.empty((H, W), dtype=torch.int32, device="cuda")
    acc = torch.zeros((H, W), dtype=torch.int32, device="cuda")

    def accumulate_k():
        for k, seed in enumerate(seeds, start=1):
            r.set_uniform("u_seed1", *seed)
            r.set_uniform("u_sample_part", 1.0 / k)
            r.render_accumulate(W, H, acc)
        r.set_uniform("u_seed1", 0.5, 0.5)
        r.set_uniform("u_sample_part", 1.0)

    plain, accum = [], []
    aa = {t: dict(total=[], base=[], detect=[], refine=[], refined=0) for t in THRESHOLDS}
    for rnd in range(2 + a.rounds):
        timed = rnd >= 2
        pending = [("plain", between_events(lambda: r.render_rgba8(W, H, out=frame))),
                   ("accum", between_events(accumulate_k))]
        for t in THRESHOLDS:
            pending.append((t, between_events(lambda: r.render_aa_ex(W, H, samples=K, threshold=t, out=frame))))
            _, st = r.render_aa_ex(W, H, samples=K, threshold=t, out=frame, stats=True)
            if timed:
                c = aa[t]
                c["base"].append(st["base_ms"])
                c["detect"].append(st["detect_ms"])
                c["refine"].append(st["refine_ms"])
                c["refined"] = st["refined"]
        torch.cuda.synchronize()
        if not timed:
            continue
        for key, (e0, e1) in pending:
            ms = e0.elapsed_time(e1)
            (plain if key == "plain" else accum if key == "accum" else aa[key]["total"]).append(ms)
    common = dict(scene=scene, max_steps=STEPS, size=a.size, samples=K, rounds=a.rounds, code=rm.render_code_hash())
    emit(case="rm_render_rgba8", ms=stat(plain), ns_per_pixel=round(float(np.median(plain)) * 1e6 / (W * H), 4),
         prepare_ms=round(prepare_ms, 1), **common)
    emit(case=f"{K} x rm_render_accumulate_rgba8", ms=stat(accum),
         ns_per_sample=round(float(np.median(accum)) * 1e6 / (W * H * K), 4), **common)
    for t, c in aa.items():
        n = c["refined"]
        base, refine = float(np.median(c["base"])), float(np.median(c["refine"]))
        per_sample = refine * 1e6 / (n * K) if n else None
        per_pixel = base * 1e6 / (W * H)
        emit(case="rm_render_aa_ex_rgba8", threshold=t, refined=n, edge_share=round(n / (W * H), 5),
             total_ms=stat(c["total"]), base_ms=stat(c["base"]), detect_ms=stat(c["detect"]),
             refine_ms=stat(c["refine"]),
             refine_ns_per_sample=round(per_sample, 4) if per_sample is not None else None,
             base_ns_per_pixel=round(per_pixel, 4),
             incoherence=round(per_sample / per_pixel, 3) if per_sample is not None else None,
             vs_accumulate=round(float(np.median(c["total"])) / float(np.median(accum)), 4), **common)
    r.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=4096)
    ap.add_argument("--samples", type=int, default=4)
    ap.add_argument("--rounds", type=int, default=12)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "plugin_aa.jsonl"))
    ap.add_argument("--scene", default=None, help="measure this scene in this process (what the parent starts)")
    a = ap.parse_args()
    a.out = os.path.abspath(a.out)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    if a.scene:
        measure(a, a.scene)
        return 0
    for scene in SCENES:  # (the parent never opens the GPU)
        cmd = [sys.executable, os.path.abspath(__file__), "--scene", scene, "--size", str(a.size), "--samples",
               str(a.samples), "--rounds", str(a.rounds), "--out", a.out]
        try:
            rc = subprocess.run(cmd, timeout=CHILD_LIMIT_S).returncode
        except subprocess.TimeoutExpired:
            print(f"{scene}: no result within {CHILD_LIMIT_S} s; stopping", file=sys.stderr)
            return 124
        if rc != 0:
            print(f"{scene}: exit status {rc}; stopping", file=sys.stderr)
            return rc
    return 0


if __name__ == "__main__":
    sys.exit(main())
