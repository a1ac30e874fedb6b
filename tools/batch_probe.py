#!/usr/bin/env python3
"""View batches (rm_render_batch_rgba8) timed on the GPU, beside the loop a
caller writes without them: scene T at 256 steps and scene O at 512 steps,
RGBA8, views from cameras.turntable, at frame sizes 64^2, 128^2, 256^2, 512^2,
1920x1080 and 4096^2, with n views chosen so that n * W * H is closest to
4096^2 (n = 1 at 4096^2).

Per size and round, interleaved, each region between two HIP events on the
renderer's stream and ended by a synchronise:
  (a) one rm_render_batch_rgba8 of the n views (device target, no stats); also
      the host time of the call alone, up to its return (it builds and uploads
      the per-view records);
  (b) n x (u_pos, u_mouse, u_time, rm_render_rgba8) on the same stream, no
      stats, with rm_params.schedule = 0, and again with schedule = 1.  The loop
      calls the C ABI through ctypes with its arguments prepared beforehand (four
      foreign calls per frame); its host time is reported too, so a reader sees
      where the loop is bound by the host and where by the GPU.
(b) runs this build's frame kernels, which a view batch does not touch
(rm_render_code_hash() names them), so it is the behaviour without batches
measured in the same session.  Two warm-up rounds of every shape, then --rounds
timed ones; medians with the min..max spread.  Then, per size, a sweep over
n = 1, 2, 4, ... with --sweep-rounds rounds for the smallest n at which (a)
beats (b, schedule 0).  At 4096^2 the row also states the n = 1 condition: the
batch must not be slower than rm_render_rgba8 (schedule 0) by more than the
run-to-run spread of the two.  One JSON line per row, appended to --out.

usage: python tools/batch_probe.py [--rounds 12] [--sweep-rounds 5] [--out profiles/batch.jsonl]
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

CASES = [("T", "template.frag", 256), ("O", "output_shader.frag", 512)]
SIZES = [(64, 64), (128, 128), (256, 256), (512, 512), (1920, 1080), (4096, 4096)]
TARGET_PIXELS = 4096 * 4096
RADIUS, HEIGHT = 5.0, 4.0  # the turntable's circle


def stat(values):
    v = np.asarray(values, np.float64)
    return dict(median=round(float(np.median(v)), 4), min=round(float(v.min()), 4), max=round(float(v.max()), 4))


def views_for(W, H):
    return max(1, int(round(TARGET_PIXELS / (W * H))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=12)
    ap.add_argument("--sweep-rounds", type=int, default=5)
    ap.add_argument("--sizes", default="", help="comma-separated subset, e.g. 64x64,4096x4096")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "batch.jsonl"))
    a = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "batch_probe.py measures on the GPU"
    sizes = SIZES
    if a.sizes:
        sizes = [tuple(int(x) for x in s.split("x")) for s in a.sizes.split(",")]
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

    for scene, file, steps in CASES:
        r.load_scene(file)
        r.set_params(max_steps=steps, shadow_max_steps=0, count_evals=0, kernel="auto", schedule=0)
        ctx = r._ctx
        for W, H in sizes:
            n_full = views_for(W, H)
            packed_full = rm.pack_views(rm.turntable(n_full, RADIUS, HEIGHT, target_time=0.0))
            out = torch.empty((n_full, H, W), dtype=torch.int32, device="cuda")
            frame = torch.empty((H, W), dtype=torch.int32, device="cuda")
            fp = ctypes.c_void_p(frame.data_ptr())

            def batch(n):
                L.rm_render_batch_rgba8(ctx, W, H, ctypes.c_void_p(packed_full.ctypes.data), n,
                                        ctypes.c_void_p(out.data_ptr()), None)

            def loop_args(n):
                return [((float(v[0]), float(v[1]), float(v[2])), (float(v[3]), float(v[4])), float(v[5]))
                        for v in packed_full[:n]]

            def loop(args):
                for pos, mouse, t in args:
                    L.rm_set_uniform3f(ctx, b"u_pos", *pos)
                    L.rm_set_uniform2f(ctx, b"u_mouse", *mouse)
                    L.rm_set_uniform1f(ctx, b"u_time", t)
                    L.rm_render_rgba8(ctx, W, H, fp, None)

            def measure(n, rounds, warm):
                args = loop_args(n)
                res = {k: [] for k in ("batch", "batch_host", "loop0", "loop0_host", "loop1", "loop1_host")}
                for rnd in range(warm + rounds):
                    ms_a, host_a = region(lambda: batch(n))
                    r.set_params(schedule=0)
                    ms_b0, host_b0 = region(lambda: loop(args))
                    r.set_params(schedule=1)
                    ms_b1, host_b1 = region(lambda: loop(args))
                    r.set_params(schedule=0)
                    if rnd >= warm:
                        for k, v in zip(res, (ms_a, host_a, ms_b0, host_b0, ms_b1, host_b1)):
                            res[k].append(v)
                return res

            common = dict(scene=scene, max_steps=steps, W=W, H=H, code=rm.render_code_hash())
            m = measure(n_full, a.rounds, 2)
            med = {k: float(np.median(v)) for k, v in m.items()}
            row = dict(case="batch_vs_loop", n=n_full, rounds=a.rounds, batch_ms=stat(m["batch"]),
                       batch_host_ms=stat(m["batch_host"]), loop_sched0_ms=stat(m["loop0"]),
                       loop_sched0_host_ms=stat(m["loop0_host"]), loop_sched1_ms=stat(m["loop1"]),
                       loop_sched1_host_ms=stat(m["loop1_host"]),
                       loop0_over_batch=round(med["loop0"] / med["batch"], 4),
                       loop1_over_batch=round(med["loop1"] / med["batch"], 4),
                       batch_ms_per_view=round(med["batch"] / n_full, 6),
                       batch_views_per_s=round(n_full / (med["batch"] * 1e-3), 1),
                       loop0_views_per_s=round(n_full / (med["loop0"] * 1e-3), 1))
            if n_full == 1:
                # the n = 1 condition: the same code over the same tiles
                spread = max(max(m["batch"]) - min(m["batch"]), max(m["loop0"]) - min(m["loop0"]))
                row.update(n1_gap_ms=round(med["batch"] - med["loop0"], 4), n1_spread_ms=round(spread, 4),
                           n1_within_spread=bool(med["batch"] - med["loop0"] <= spread))
            emit(**row, **common)
            # the smallest n at which the batch beats the loop (schedule 0)
            if n_full > 1:
                sweep, first = [], None
                k = 1
                while k <= n_full:
                    s = measure(k, a.sweep_rounds, 1)
                    b, l0 = float(np.median(s["batch"])), float(np.median(s["loop0"]))
                    sweep.append(dict(n=k, batch_ms=round(b, 4), loop_sched0_ms=round(l0, 4)))
                    if first is None and b < l0:
                        first = k
                    k *= 2
                emit(case="smallest_n", rounds=a.sweep_rounds, smallest_n_batch_wins=first, sweep=sweep, **common)
            del out, frame
            torch.cuda.empty_cache()
    r.close()


if __name__ == "__main__":
    main()
