#!/usr/bin/env python3
"""Record the cases of tests/test_near_sky_gpu.py from the library in the tree
(instrumented kernels, on the GPU) into an .npz: run it on the commit whose
frames the near-sky ladder must keep (tools/record_refl_clear.py does the same
for tests/test_refl_clear_gpu.py).  It reads rm_stats' evals, flop and skipped
and the certified and reflection-cleared counts only, so it runs against a
library from before rm_near_sky_steps.
usage: record_near_sky.py OUT.npz"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import raymarching_amd as rm  # noqa: E402
from tests.test_near_sky_gpu import CASES, record  # noqa: E402

r = rm.Renderer(0)
rec = {}
for name in CASES:
    rec.update(record(r, name))
    print(name, rec[f"{name}.stats"].tolist(), flush=True)
r.close()
np.savez_compressed(sys.argv[1], **rec)
print(sys.argv[1], os.path.getsize(sys.argv[1]), "bytes,", rm.render_code_hash())
