#!/usr/bin/env python3
"""The batched post chain (rm_post_chain_batch) timed on the GPU, beside the
loop a caller writes without it: frames rendered by render_batch of scene T at
256 steps and scene O at 512 steps (views from cameras.turntable), at
4096 x 64^2, 256 x 256^2, 8 x 1920x1080 and 1 x 4096^2, with the chains
(fxaa, none) and (chromatic, aces).

Per case and round, interleaved, each region between two HIP events on the
renderer's stream and ended by a synchronise:
  (a) one rm_post_chain_batch of the n frames under the default scratch limit;
  (b) where that makes more than one group (4096 x 64^2), the same call with
      the limit raised so that the batch is one group: what the groups cost;
  (c) n x rm_post_chain (or rm_post_chain_ex) over the same device frames on
      the same stream, through ctypes with the arguments prepared beforehand.
      It runs this build's single-frame kernels, which the batch does not
      touch, so it is the behaviour without the batch measured in the same
      session.
The host time of each call sequence alone is reported too, and the plan's
`launches` and `groups` (rm_post_batch_plan).  Two warm-up rounds, then --rounds
timed ones; medians with the min..max spread.  Before the rounds the batch's
`out` is compared with the loop's, byte for byte.  One JSON line per case and
chain, appended to --out.

Every case runs in a child process of its own under a time limit
(--case-timeout seconds); the first child that fails or runs out of time ends
the probe, and nothing more is started on the GPU.

usage: python tools/batch_post_probe.py [--rounds 7] [--out profiles/batch_post.jsonl] [--scenes T,O]
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
CHAINS = (("fxaa", "none"), ("chromatic", "aces"))
RADIUS, HEIGHT = 5.0, 4.0  # the turntable's circle


def stat(values):
    v = np.asarray(values, np.float64)
    return dict(median=round(float(np.median(v)), 4), min=round(float(v.min()), 4), max=round(float(v.max()), 4))


def run_case(scene, n, W, H, rounds, out):
    import torch
    assert torch.cuda.is_available(), "batch_post_probe.py measures on the GPU"
    from raymarching_amd import _lib
    L = rm.lib()
    r = rm.Renderer(0)
    file, steps = SCENES[scene]
    r.load_scene(file)
    r.set_params(max_steps=steps, shadow_max_steps=0, count_evals=0)
    ctx = r._ctx
    frames = r.render_batch(W, H, rm.turntable(n, RADIUS, HEIGHT, target_time=0.0))
    mid, dst = torch.empty_like(frames), torch.empty_like(frames)
    mid1, dst1 = torch.empty_like(frames), torch.empty_like(frames)  # the loop's targets
    px = W * H * 4
    ptr = lambda t, v=0: ctypes.c_void_p(t.data_ptr() + v * px)  # noqa: E731
    per_view = [(ptr(frames, v), ptr(mid1, v), ptr(dst1, v)) for v in range(n)]
    plan = rm.post_batch_plan(W, H, n)
    one_group = plan["shared_bytes"] + n * plan["per_view_bytes"]

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
    for sample, tonemap in CHAINS:
        s, t = _lib.POST_SAMPLES[sample], _lib.TONEMAPS[tonemap]
        plain = (sample, tonemap) == ("fxaa", "none")

        def batch():
            st = L.rm_post_chain_batch(ctx, W, H, n, s, t, ptr(frames), ptr(mid), ptr(dst))
            assert st == 0, st

        def loop():
            for a, b, c in per_view:
                st = L.rm_post_chain(ctx, W, H, a, b, c) if plain else L.rm_post_chain_ex(ctx, W, H, s, t, a, b, c)
                assert st == 0, st

        batch()
        loop()
        torch.cuda.synchronize()
        same = bool(torch.equal(mid, mid1) and torch.equal(dst, dst1))
        names = ["batch", "batch_host", "loop", "loop_host"] + (["batch1", "batch1_host"] if plan["groups"] > 1 else [])
        res = {k: [] for k in names}
        for rnd in range(2 + rounds):
            got = region(batch) + region(loop)
            if plan["groups"] > 1:
                r.set_post_batch_scratch_limit(one_group)
                got += region(batch)
                r.set_post_batch_scratch_limit(0)
            if rnd >= 2:
                for k, v in zip(names, got):
                    res[k].append(v)
        med = {k: float(np.median(v)) for k, v in res.items()}
        row = dict(case="post_chain_batch_vs_loop", scene=scene, max_steps=steps, n=n, W=W, H=H, sample=sample,
                   tonemap=tonemap, rounds=rounds, same_bytes=same, launches=plan["launches"], groups=plan["groups"],
                   group_views=plan["group_views"], scratch_bytes=plan["scratch_bytes"],
                   loop_launches=n * (plan["launches"] - 1) // plan["groups"] if plan["groups"] else 0,
                   batch_ms=stat(res["batch"]), batch_host_ms=stat(res["batch_host"]), loop_ms=stat(res["loop"]),
                   loop_host_ms=stat(res["loop_host"]), loop_over_batch=round(med["loop"] / med["batch"], 4))
        if plan["groups"] > 1:
            row.update(one_group_scratch_bytes=one_group, batch_one_group_ms=stat(res["batch1"]),
                       batch_one_group_host_ms=stat(res["batch1_host"]),
                       groups_over_one_group=round(med["batch"] / med["batch1"], 4))
        line = json.dumps(row)
        print(line, flush=True)
        sink.write(line + "\n")
        sink.flush()
        if not same:
            raise SystemExit("batch_post_probe: the batch's bytes are not the loop's")
    r.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "batch_post.jsonl"))
    ap.add_argument("--scenes", default="T,O")
    ap.add_argument("--case-timeout", type=int, default=240)
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
                print(f"batch_post_probe: case {scene} {n} x {W}x{H} ended with status {rc}; stopping", flush=True)
                return rc if rc > 0 else 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
