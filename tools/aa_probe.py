#!/usr/bin/env python3
"""Adaptive supersampling (rm_render_aa_rgba8) timed on the GPU, beside what a
caller pays today: scene T at 256 steps and scene O at 512 steps (pose P0, the
poses of C3 and of bench.py --scene O), size^2 pixels, K samples, at edge
thresholds 16, 32, 64 and 0 (every pixel), in both lane layouts of the refine
kernel (RM_AA_LAYOUT, alternated call by call in one process), and at
thresholds 8, 4, 2 and 1 in the default layout (denser edge sets).

Per round, interleaved: rm_render_rgba8 alone, K launches of
rm_render_accumulate_rgba8 (the same samples everywhere), and per threshold and
layout one rm_render_aa_rgba8 between two HIP events (total_ms, asynchronous
call) and one with rm_aa_stats (base_ms, detect_ms, refine_ms, refined).  Two
warm-up rounds, then --rounds timed ones; medians, with the min..max spread.
One JSON line per case, appended to --out.

usage: python tools/aa_probe.py [--size 4096] [--samples 4] [--rounds 12] [--out profiles/aa.jsonl]
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
THRESHOLDS = (16, 32, 64, 0)
LAYOUTS = ("sample", "pixel")
# lower thresholds, in the default layout only: edge shares between the rows
# above and 1, to place the share at which K accumulate launches become cheaper
SWEEP = (8, 4, 2, 1)


def stat(values):
    v = np.asarray(values, np.float64)
    return dict(median=round(float(np.median(v)), 4), min=round(float(v.min()), 4), max=round(float(v.max()), 4))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=4096)
    ap.add_argument("--samples", type=int, default=4)
    ap.add_argument("--rounds", type=int, default=12)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "aa.jsonl"))
    a = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "aa_probe.py measures on the GPU"
    r = rm.Renderer(0)
    pose = rm.POSES["P0"]
    W = H = a.size
    K = a.samples
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

    seeds = [(float(o[0]) + 0.5, float(o[1]) + 0.5) for o in rm.aa_offsets(K)]
    for scene, file, steps in CASES:
        r.load_scene(file)
        r.set_pose(pose["pos"], pose["mouse"], pose["time"])
        r.set_params(max_steps=steps, shadow_max_steps=0, count_evals=0, kernel="auto")
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
        variants = [(t, lay) for t in THRESHOLDS for lay in LAYOUTS] + [(t, LAYOUTS[0]) for t in SWEEP]
        aa = {v: dict(total=[], base=[], detect=[], refine=[], refined=0) for v in variants}
        for rnd in range(2 + a.rounds):
            timed = rnd >= 2
            pending = [("plain", between_events(lambda: r.render_rgba8(W, H, out=frame))),
                       ("accum", between_events(accumulate_k))]
            for t, lay in variants:
                os.environ["RM_AA_LAYOUT"] = lay
                pending.append(((t, lay), between_events(
                    lambda: r.render_aa(W, H, samples=K, threshold=t, out=frame))))
                _, st = r.render_aa(W, H, samples=K, threshold=t, out=frame, stats=True)
                if timed:
                    c = aa[(t, lay)]
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
        os.environ.pop("RM_AA_LAYOUT", None)
        common = dict(scene=scene, max_steps=steps, size=a.size, samples=K, rounds=a.rounds, code=rm.render_code_hash())
        emit(case="rm_render_rgba8", ms=stat(plain), ns_per_pixel=round(float(np.median(plain)) * 1e6 / (W * H), 4),
             **common)
        emit(case=f"{K} x rm_render_accumulate_rgba8", ms=stat(accum),
             ns_per_sample=round(float(np.median(accum)) * 1e6 / (W * H * K), 4), **common)
        for (t, lay), c in aa.items():
            n = c["refined"]
            base, refine = float(np.median(c["base"])), float(np.median(c["refine"]))
            per_sample = refine * 1e6 / (n * K) if n else None
            per_pixel = base * 1e6 / (W * H)
            emit(case="rm_render_aa_rgba8", threshold=t, layout=lay, refined=n, edge_share=round(n / (W * H), 5),
                 total_ms=stat(c["total"]), base_ms=stat(c["base"]), detect_ms=stat(c["detect"]),
                 refine_ms=stat(c["refine"]),
                 refine_ns_per_sample=round(per_sample, 4) if per_sample is not None else None,
                 base_ns_per_pixel=round(per_pixel, 4),
                 incoherence=round(per_sample / per_pixel, 3) if per_sample is not None else None,
                 vs_accumulate=round(float(np.median(c["total"])) / float(np.median(accum)), 4), **common)
        del frame, acc
        torch.cuda.empty_cache()
    r.close()


if __name__ == "__main__":
    main()
