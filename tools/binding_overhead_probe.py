"""Host cost per call of the Python binding: the wall clock of N back-to-back
Renderer.render_rgba8(W, H) calls on scene S0 (each allocates its frame), with
one synchronize() at the end.  Prints one JSON line: us_per_call is that wall
clock per call, host_us_per_call the part before the synchronize (the calls
alone: where the GPU is the slower side, only this one shows the binding).

--package-root DIR imports raymarching_amd from DIR instead of this tree (another
commit's Python files; set RM_LIB to the librm.so to load), for an A/B of the
binding alone over one library.
"""
import argparse
import json
import os
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("--package-root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument("--label", default="head")
ap.add_argument("--calls", type=int, default=1000)
ap.add_argument("--size", type=int, nargs=2, default=(40, 24), metavar=("W", "H"))
args = ap.parse_args()
sys.path.insert(0, args.package_root)

import raymarching_amd as rm  # noqa: E402

W, H = args.size
r = rm.Renderer(0)
r.load_scene(rm.SCENE_FILES["S0"])
r.set_pose(rm.S0_POSE["pos"], rm.S0_POSE["mouse"], rm.S0_POSE["time"])
for _ in range(200):  # warm up: the resolution cache, the adaptive order's first launches, torch's allocator
    r.render_rgba8(W, H)
r.synchronize()
t0 = time.perf_counter()
for _ in range(args.calls):
    r.render_rgba8(W, H)
host = time.perf_counter() - t0
r.synchronize()
dt = time.perf_counter() - t0
print(json.dumps({"label": args.label, "package": os.path.dirname(rm.__file__), "calls": args.calls, "W": W, "H": H,
                  "wall_ms": round(dt * 1e3, 3), "us_per_call": round(dt * 1e6 / args.calls, 3),
                  "host_us_per_call": round(host * 1e6 / args.calls, 3)}), flush=True)
r.close()
