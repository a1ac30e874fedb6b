"""Adaptive supersampling of a view batch, the host-only parts (no GPU):
rm_batch_aa_scratch_bytes against the formula include/rm.h documents, every
edge of the size rule of the three calls, the ctypes prototypes, the ABI
version, and the stand-alone program tests/host/batch_aa_plan_test.cpp, built
with the host compiler under the address and undefined-behaviour sanitizers
from csrc/rm_batch_aa_plan.h alone (nothing of it is loaded into Python), as
tests/test_aa_host.py builds its program."""
import ctypes
import os
import re
import shutil
import subprocess

import pytest

import raymarching_amd as rm
from raymarching_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCES = [os.path.join(ROOT, "tests", "host", "batch_aa_plan_test.cpp")]
FLAGS = ["-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
INVALID = 1  # RM_ERR_INVALID_ARGUMENT


def _scratch(W, H, n):
    b = ctypes.c_int64(-1)
    st = rm.lib().rm_batch_aa_scratch_bytes(W, H, n, ctypes.byref(b))
    return st, b.value


def _formula(W, H, n):
    """include/rm.h: 4 * (32 * n + roundup32(n + 2) + n * W * H)"""
    return 4 * (32 * n + (n + 2 + 31) // 32 * 32 + n * W * H)


@pytest.mark.parametrize("W,H,n", [(61, 37, 6), (8, 8, 4096), (64, 64, 4096), (256, 256, 256), (1920, 1080, 8),
                                   (4096, 4096, 1), (1, 1, 1), (5, 3, 30), (5, 3, 31), (8, 8, 65535), (8, 8, 0)])
def test_scratch_bytes_is_the_documented_formula(W, H, n):
    assert _scratch(W, H, n) == (0, _formula(W, H, n))
    assert rm.batch_aa_scratch_bytes(W, H, n) == _formula(W, H, n)


def test_scratch_bytes_by_hand():
    # six views of 61 x 37: six counter lines, one line of plan (8 words used), 6 * 2257 queue words
    assert _scratch(61, 37, 6) == (0, 4 * (192 + 32 + 13542))
    # `bytes` may be NULL
    assert rm.lib().rm_batch_aa_scratch_bytes(61, 37, 6, None) == 0
    assert rm.lib().rm_batch_aa_scratch_bytes(61, 37, 65536, None) == INVALID


def test_size_rule_edges():
    """tests/test_batch_host.py::test_size_rule_edges' cases, and W * H < 2^30"""
    ok = lambda W, H, n: _scratch(W, H, n)[0] == 0  # noqa: E731
    bad = lambda W, H, n: _scratch(W, H, n)[0] == INVALID  # noqa: E731
    # 0 <= n <= 65535
    assert ok(8, 8, 65535) and bad(8, 8, 65536) and bad(8, 8, -1)
    # ceil(H / 8) <= 65535
    H = 65535 * 8
    assert _scratch(1, H, 1) == (0, _formula(1, H, 1))
    assert ok(1, H - 7, 1) and bad(1, H + 1, 1)
    # n * W * H <= 2^31
    assert _scratch(1 << 10, 1 << 10, 1 << 11) == (0, 4 * (32 * 2048 + 2080 + (1 << 31)))  # = 2^31 pixels
    assert bad(1 << 10, 1 << 10, (1 << 11) + 1)
    # W * H < 2^30: a view batch takes one frame of 2^31 pixels, its supersampling does not
    assert rm.lib().rm_batch_bytes(1 << 16, 1 << 15, 1, 1, None, None) == 0
    assert bad(1 << 16, 1 << 15, 1) and bad((1 << 16) + 1, 1 << 15, 1)
    assert bad(0x7FFFFFFF, 65535 * 8, 65535)  # (no overflow in the product)
    assert bad(1 << 15, 1 << 15, 1) and bad(1 << 15, 1 << 15, 0)               # W * H = 2^30
    assert _scratch((1 << 30) - 1, 1, 1) == (0, _formula((1 << 30) - 1, 1, 1))  # W * H = 2^30 - 1
    assert ok(32769, 32767, 1) and ok(32769, 32767, 2)                          # 2^30 - 1 = 32769 * 32767; twice: < 2^31
    assert bad(32769, 32767, 3)
    assert bad(1 << 30, 1, 1)
    # W, H > 0
    for W, H in [(0, 8), (8, 0), (-1, 8), (8, -1)]:
        assert bad(W, H, 1) and bad(W, H, 0), (W, H)


def test_render_calls_refuse_a_null_context():
    """No GPU work: a NULL context is refused before any pointer (junk here) is used."""
    L = rm.lib()
    p = _lib.RmAaParams(4, 32)
    junk = ctypes.c_void_p(16)
    for fn in (L.rm_refine_batch_rgba8, L.rm_render_batch_aa_rgba8):
        assert fn(None, 8, 8, junk, 1, ctypes.byref(p), junk, None, None, None) == INVALID  # a NULL context


def test_prototypes_and_abi():
    L = rm.lib()
    for name in ("rm_batch_aa_scratch_bytes", "rm_refine_batch_rgba8", "rm_render_batch_aa_rgba8"):
        assert name in rm.EXPORTS
        fn = getattr(L, name)
        assert fn.restype is ctypes.c_int and fn.argtypes is not None
    assert len(L.rm_refine_batch_rgba8.argtypes) == 10 and len(L.rm_render_batch_aa_rgba8.argtypes) == 10
    assert len(L.rm_batch_aa_scratch_bytes.argtypes) == 4
    # no existing struct changed: the ABI version is still 3, in the library, the binding and the header
    assert L.rm_abi_version() == 3 == _lib.ABI_VERSION
    header = open(os.path.join(ROOT, "include", "rm.h")).read()
    assert re.search(r"^#define RM_ABI_VERSION 3$", header, re.M)
    for name in ("rm_batch_aa_scratch_bytes", "rm_refine_batch_rgba8", "rm_render_batch_aa_rgba8"):
        assert re.search(rf"^rm_status {name}\(", header, re.M), name
    assert hasattr(rm.Renderer, "render_batch_aa") and hasattr(rm.Renderer, "refine_batch")


def _compiler():
    if shutil.which("g++"):  # (gcc's sanitizer runtimes are shared by default: link them in, as clang does)
        return ["g++", "-static-libasan", "-static-libubsan"]
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    return [hipcc, "-x", "c++"] if os.path.exists(hipcc) else None


def test_plan_under_sanitizers(tmp_path):
    cxx = _compiler()
    if cxx is None:
        pytest.skip("no host C++ compiler (g++ or hipcc)")
    exe = tmp_path / "batch_aa_plan_test"
    build = subprocess.run(cxx + FLAGS + SOURCES + ["-o", str(exe)], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-4000:]
    run = subprocess.run([str(exe)], cwd=tmp_path, capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, (run.stdout + run.stderr)[-4000:]
    assert "all checks passed" in run.stdout
