"""raymarching_amd/csrc/rm_libm_ref.h: the C library's sinf and powf restated
for the device (scene O's floor material in ray queries, rm_rays.h), built
here for the host and compared with the C library itself."""
import json
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_restatement_returns_the_c_librarys_floats(tmp_path):
    """A million arguments per range (|x| < pi/4 with tiny ones, floorMat's
    range, the large-argument reduction; pow(x, 1.3) on (0, 70]).  The C
    library ships fused and unfused builds of these routines and picks one by
    CPU; they differ from each other on about 1e-7 of arguments, so at most
    1e-5 of a range may differ here."""
    exe = tmp_path / "libm_ref_test"
    subprocess.run(["g++", "-O2", "-std=c++17", "-fno-builtin", os.path.join(ROOT, "tests", "host", "libm_ref_test.cpp"),
                    "-o", str(exe)], check=True)
    out = json.loads(subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout)
    print(out)
    for k in ("sin_small", "sin_mid", "sin_large", "pow"):
        assert out[k] <= 1e-5 * out["n"], out
