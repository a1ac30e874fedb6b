#!/usr/bin/env python3
"""Adaptive supersampling of a scene plugin's view batch
(rm_render_batch_aa_ex_rgba8) timed on the GPU, beside the loop a caller writes
without it: scenes/output_shader_knobs.hip (u_ball and u_spin set per view) and
scenes/mandelbulb.hip (no uniforms), 512 steps, K = 4, thresholds 32 and 0,
views from cameras.turntable with u_time advancing, in DESIGN.md 2.30's shapes:
4096 views of 64^2, 256 of 256^2, eight of 1920x1080, one 4096^2.

Per shape, threshold and round, interleaved, each region between two HIP events
on the renderer's stream and ended by a synchronise:
  (a) one rm_render_batch_aa_ex_rgba8 of the n views with their per-view
      uniforms (device targets, no stats), with the default number of columns
      and with RM_PLUGIN_BATCH_AA_COLUMNS set to the rule's G for c = 1, 2, 4, 8
      (rm_plugin_batch_aa_grid.h, restated in columns() below; `waves` is the
      library's own figure, CUs x hipModuleOccupancyMaxActiveBlocksPerMultiprocessor
      of the kernel at 64 threads, asked here of the dumped code object through
      the HIP runtime, so that the c = 4 row runs the default's grid);
  (b) n x (u_pos, u_mouse, u_time, the scene's per-view uniforms,
      rm_render_aa_ex_rgba8) on the same stream, no stats, rm_params.schedule =
      0, through ctypes with the arguments prepared beforehand.
(b) runs the plugin's frame and AA kernels, which the new form does not touch.
After the timed rounds one call of each kind with stats gives the base / detect
+ plan / refine split and the refined totals, which must agree.  --warmup
rounds of everything first (the first compiles the forms), then --rounds timed
ones; medians with the min..max spread.  The single 4096^2 view also states the
n = 1 condition against rm_render_aa_ex_rgba8 (schedule 0), with the spread
profiles/plugin_aa.jsonl records for that single call as the yardstick.  Each scene runs in
a fresh process (--scene, started by the parent); one JSON line per row,
appended to --out.

usage: python tools/plugin_batch_aa_probe.py [--rounds 6] [--warmup 2] [--out profiles/plugin_batch_aa.jsonl]
"""
import argparse
import ctypes
import json
import os
import re
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import raymarching_amd as rm  # noqa: E402
from raymarching_amd import _lib, batch_aa_ex  # noqa: E402

STEPS, SAMPLES, KSHIFT = 512, 4, 2
THRESHOLDS = (32, 0)
SHAPES = [(64, 64, 4096), (256, 256, 256), (1920, 1080, 8), (4096, 4096, 1)]
RADIUS, HEIGHT = 5.0, 4.0  # the turntable's circle
FACTORS = (1, 2, 4, 8)
COLUMNS = "RM_PLUGIN_BATCH_AA_COLUMNS"


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


CASES = {"knobs": ("output_shader_knobs.hip", knob_uniforms), "mandelbulb": ("mandelbulb.hip", lambda n: {})}


def columns(W, H, n, waves, c):
    """rm_plugin_batch_aa_grid.h's rule"""
    ppw = 64 >> KSHIFT
    return int(min(max(-(-c * waves // n), 1), -(-W * H // ppw)))


def kernel_waves(path, cus):
    """(CUs x the occupancy of rm_plugin_batch_aa_refine at 64 threads, its VGPR count): what
    rm_plugin_host.cpp's batch_aa_ready computes, from the dumped code object of the same text"""
    hip = ctypes.CDLL("libamdhip64.so")
    with tempfile.TemporaryDirectory() as d:
        os.environ["RM_PLUGIN_DUMP"] = d
        ok, log = batch_aa_ex.compile_scene_batch_aa(path)
        del os.environ["RM_PLUGIN_DUMP"]
        assert ok, log
        co = os.path.join(d, "plugin_batch_aa.co")
        txt = subprocess.run(["/opt/rocm/llvm/bin/llvm-readelf", "--notes", co], capture_output=True, text=True,
                             check=True).stdout
        image = open(co, "rb").read()
    mod, fn, per_cu = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_int(0)
    assert hip.hipModuleLoadData(ctypes.byref(mod), image) == 0
    assert hip.hipModuleGetFunction(ctypes.byref(fn), mod, b"rm_plugin_batch_aa_refine") == 0
    assert hip.hipModuleOccupancyMaxActiveBlocksPerMultiprocessor(ctypes.byref(per_cu), fn, 64, ctypes.c_size_t(0)) == 0
    hip.hipModuleUnload(mod)
    return max(1, cus * max(per_cu.value, 1)), int(re.search(r"\.vgpr_count:\s+(\d+)", txt).group(1))


def recorded_spread(file, threshold):
    """max - min of rm_render_aa_ex_rgba8's total at this threshold in profiles/plugin_aa.jsonl (4096^2, K = 4), or None"""
    try:
        for line in open(os.path.join(ROOT, "profiles", "plugin_aa.jsonl")):
            row = json.loads(line)
            if row.get("case") == "rm_render_aa_ex_rgba8" and row.get("scene") == file and row.get("threshold") == threshold:
                return round(row["total_ms"]["max"] - row["total_ms"]["min"], 4)
    except OSError:
        pass
    return None


def run_scene(scene, a):
    import torch
    assert torch.cuda.is_available(), "plugin_batch_aa_probe.py measures on the GPU"
    file, uniforms_of = CASES[scene]
    path = os.path.join(rm.SCENES_DIR, file)
    L = rm.lib()
    sink = open(a.out, "a")

    def emit(**row):
        line = json.dumps(row)
        print(line, flush=True)
        sink.write(line + "\n")
        sink.flush()

    def region(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    torch.zeros(1, device="cuda")  # (the runtime is up before the module is loaded)
    waves, vgprs = kernel_waves(path, torch.cuda.get_device_properties(0).multi_processor_count)
    r = rm.Renderer(0)
    r.load_scene(path)
    r.set_params(max_steps=STEPS, shadow_max_steps=0, count_evals=0, kernel="auto", schedule=0)
    t0 = time.perf_counter()
    batch_aa_ex.batch_aa_prepare(r)
    prepare_ms = (time.perf_counter() - t0) * 1e3
    r.aa_prepare()
    ctx = r._ctx
    os.environ.pop(COLUMNS, None)
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
        args = [((float(v[0]), float(v[1]), float(v[2])), (float(v[3]), float(v[4])), float(v[5]),
                 tuple(float(x) for x in u["u_ball"][k]) if u else None, float(u["u_spin"][k]) if u else None)
                for k, v in enumerate(packed)]
        for threshold in THRESHOLDS:
            p = _lib.RmAaParams(SAMPLES, threshold)

            def batch(stats=None):
                st = L.rm_render_batch_aa_ex_rgba8(ctx, W, H, ctypes.c_void_p(packed.ctypes.data), n,
                                                   ctypes.cast(arr, ctypes.c_void_p) if entries else None,
                                                   len(entries), ctypes.byref(p), ctypes.c_void_p(out.data_ptr()),
                                                   None, None, stats)
                assert st == 0, L.rm_last_error(ctx)

            def loop(total=None):
                s = _lib.RmAaStats()
                for pos, mouse, t, ball, spin in args:
                    st = L.rm_set_uniform3f(ctx, b"u_pos", *pos) | L.rm_set_uniform2f(ctx, b"u_mouse", *mouse) | \
                        L.rm_set_uniform1f(ctx, b"u_time", t)
                    if ball is not None:
                        st |= L.rm_set_uniform4f(ctx, b"u_ball", *ball) | L.rm_set_uniform1f(ctx, b"u_spin", spin)
                    st |= L.rm_render_aa_ex_rgba8(ctx, W, H, ctypes.byref(p), fp, None,
                                                  ctypes.byref(s) if total is not None else None)
                    assert st == 0, L.rm_last_error(ctx)
                    if total is not None:
                        for key in total:
                            total[key] += getattr(s, key)

            def with_columns(g):
                def run():
                    os.environ[COLUMNS] = str(g)
                    batch()
                    del os.environ[COLUMNS]
                return run

            g_of = {c: columns(W, H, n, waves, c) for c in FACTORS}
            kinds = [("batch", batch)] + [(f"c{c}", with_columns(g_of[c])) for c in FACTORS] + [("loop", loop)]
            res = {k: [] for k, _ in kinds}
            for rnd in range(a.warmup + a.rounds):
                for k, fn in kinds:
                    ms = region(fn)
                    if rnd >= a.warmup:
                        res[k].append(ms)
            med = {k: float(np.median(v)) for k, v in res.items()}
            bs = _lib.RmAaStats()
            batch(ctypes.byref(bs))
            lt = dict(refined=0, base_ms=0.0, detect_ms=0.0, refine_ms=0.0)
            loop(lt)
            row = dict(case="plugin_batch_aa_vs_loop", scene=scene, max_steps=STEPS, W=W, H=H, n=n, samples=SAMPLES,
                       threshold=threshold, rounds=a.rounds, warmup=a.warmup, uniforms_per_view=sorted(u),
                       kernel_vgprs=vgprs, waves=waves, batch_ms=stat(res["batch"]),
                       columns={f"c{c}": dict(G=g_of[c], ms=stat(res[f"c{c}"])) for c in FACTORS},
                       loop_sched0_ms=stat(res["loop"]), loop_over_batch=round(med["loop"] / med["batch"], 4),
                       batch_stats=dict(refined=int(bs.refined), base_ms=round(bs.base_ms, 4),
                                        detect_plan_ms=round(bs.detect_ms, 4), refine_ms=round(bs.refine_ms, 4)),
                       loop_stats=dict(refined=int(lt["refined"]), base_ms=round(lt["base_ms"], 4),
                                       detect_ms=round(lt["detect_ms"], 4), refine_ms=round(lt["refine_ms"], 4)),
                       refined_agree=bool(int(bs.refined) == int(lt["refined"])),
                       edge_share=round(int(bs.refined) / float(n * W * H), 5), prepare_ms=round(prepare_ms, 1))
            if n == 1:  # the n = 1 condition: the same samples of the same queue
                own = max(max(res["batch"]) - min(res["batch"]), max(res["loop"]) - min(res["loop"]))
                yard = recorded_spread(file, threshold)
                row.update(n1_gap_ms=round(med["batch"] - med["loop"], 4), n1_own_spread_ms=round(own, 4),
                           n1_recorded_spread_ms=yard,
                           n1_within_recorded_spread=None if yard is None else bool(abs(med["batch"] - med["loop"]) <= yard))
            emit(**row)
        del out, frame
        torch.cuda.empty_cache()
    r.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--scene", choices=sorted(CASES), default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "plugin_batch_aa.jsonl"))
    a = ap.parse_args()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    if a.scene:
        return run_scene(a.scene, a)
    for scene in ("knobs", "mandelbulb"):  # each scene in a fresh process
        subprocess.run([sys.executable, os.path.abspath(__file__), "--scene", scene, "--rounds", str(a.rounds),
                        "--warmup", str(a.warmup), "--out", a.out], check=True)


if __name__ == "__main__":
    main()
