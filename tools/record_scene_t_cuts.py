#!/usr/bin/env python3
"""Record the cases of tests/test_scene_t_cuts_gpu.py from the library in the
tree (instrumented kernels, on the GPU) into an .npz: run it on the commit whose
frames a later change must keep (tools/record_scene_t_frames.py does the same
for tests/test_scene_t_trim.py).  usage: record_scene_t_cuts.py OUT.npz"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import raymarching_amd as rm  # noqa: E402
from tests.test_scene_t_cuts_gpu import CASES, render_instrumented  # noqa: E402

r = rm.Renderer(0)
rec = {}
for name in CASES:
    for k, v in render_instrumented(r, name).items():
        rec[f"{name}.{k}"] = v
    print(name, rec[f"{name}.stats"].tolist(), flush=True)
r.close()
np.savez_compressed(sys.argv[1], **rec)
print(sys.argv[1], os.path.getsize(sys.argv[1]), "bytes,", rm.render_code_hash())
