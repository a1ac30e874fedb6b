"""The batched post passes, the host-only parts (no GPU): rm_post_batch_plan
against the relations include/rm.h documents (under the default limit, a limit
of 1 byte, one view's worth and exactly shared + 3 views), every edge of the
size rule, the ctypes prototypes, the ABI version, and the stand-alone program
tests/host/post_batch_plan_test.cpp, built with the host compiler under the
address and undefined-behaviour sanitizers from csrc/rm_post_batch_plan.h alone
(nothing of it is loaded into Python), as tests/test_batch_aa_host.py builds
its program."""
import ctypes
import math
import os
import re
import subprocess

import numpy as np
import pytest

import raymarching_amd as rm
from raymarching_amd import _lib
from tests.test_batch_aa_host import FLAGS, _compiler

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCES = [os.path.join(ROOT, "tests", "host", "post_batch_plan_test.cpp")]
INVALID = 1  # RM_ERR_INVALID_ARGUMENT
DEFAULT = 512 << 20
SHAPES = [(61, 37, 7), (64, 64, 4096), (256, 256, 256), (1920, 1080, 8), (4096, 4096, 1), (40, 16, 3), (8, 8, 65535)]


def _plan(W, H, n, limit=0):
    p = _lib.RmPostBatchPlan()
    st = rm.lib().rm_post_batch_plan(W, H, n, limit, ctypes.byref(p))
    return st, p.as_dict()


def _bloom_levels(W, H):
    """bloom.frag's level pair in float32, as the library's plan forms it, and the sizes of levels 0..d2"""
    lod = float(np.log2(np.float32(0.05) * np.float32(H), dtype=np.float32))
    q = max(W, H).bit_length() - 1
    d1 = d2 = 0
    if lod > 0:
        d1 = min(int(math.floor(lod)), q)
        d2 = min(d1 + 1, q)
    sizes = [(W, H)]
    for _ in range(d2):
        w, h = sizes[-1]
        sizes.append((max(w >> 1, 1), max(h >> 1, 1)))
    return lod, d1, d2, sizes


def _expected(W, H, n, limit):
    """include/rm.h's formulas"""
    lod, d1, d2, sizes = _bloom_levels(W, H)
    lim = limit or DEFAULT
    if lod <= 0:
        per_view, launches_bloom, once = 0, 1, 0
    else:
        levels = sum(w * h for w, h in sizes[1:])
        runs = lambda pixels, lw: min(pixels, 5 * lw + 1)  # noqa: E731
        pairs = sum(runs(W, sizes[d][0]) * runs(H, sizes[d][1]) for d in (d1, d2))
        per_view = 4 * ((levels + 3) // 4 * 4 + 12 * pairs)
        s0 = max(d2 - 8, 0)
        pyramid = d2 - s0 >= 5 and W % (1 << d2) == 0 and H % (1 << d2) == 0
        launches_bloom, once = (s0 + 1 if pyramid else d2) + 2, 1
    return per_view, launches_bloom, once, lim


@pytest.mark.parametrize("W,H,n", SHAPES)
def test_plan_is_the_documented_formula(W, H, n):
    st, base = _plan(W, H, n)
    assert st == 0
    shared, per_view = base["shared_bytes"], base["per_view_bytes"]
    for limit in (0, 1, shared + per_view, shared + 3 * per_view, 1 << 40):
        st, p = _plan(W, H, n, limit)
        assert st == 0
        want_per_view, launches_bloom, once, lim = _expected(W, H, n, limit)
        assert p["per_view_bytes"] == want_per_view == per_view and p["shared_bytes"] == shared
        assert shared >= per_view and (shared > per_view or per_view == 0)  # the single-frame layout holds a view's part
        g = max(1, min(n, (lim - shared) // per_view)) if per_view else n
        assert p["group_views"] == g
        assert p["groups"] == -(-n // g)
        assert p["scratch_bytes"] == shared + g * per_view
        assert p["launches"] == p["groups"] * (1 + launches_bloom) + once
        assert rm.post_batch_plan(W, H, n, limit) == p
    if per_view:
        assert _plan(W, H, n, 1)[1]["group_views"] == 1 and _plan(W, H, n, 1)[1]["groups"] == n
        assert _plan(W, H, n, shared + per_view)[1]["group_views"] == 1
        assert _plan(W, H, n, shared + 3 * per_view)[1]["group_views"] == min(3, n)
        assert _plan(W, H, n, shared + 3 * per_view - 1)[1]["group_views"] == min(2, n)
        assert _plan(W, H, n, 1 << 40)[1]["groups"] == 1


def test_plan_by_hand():
    # 64 x 64: levels 1 and 2 (1024 + 256 texels), 64 x 64 run pairs of 12 floats on each: ~390 KB a view
    st, p = _plan(64, 64, 4096)
    assert st == 0 and p["per_view_bytes"] == 4 * (1280 + 2 * 12 * 4096) == 398336
    assert p["group_views"] == (DEFAULT - p["shared_bytes"]) // 398336 and p["groups"] == -(-4096 // p["group_views"])
    assert p["launches"] == 5 * p["groups"] + 1  # the launches do not depend on n but through the groups
    assert _plan(64, 64, 8)[1]["launches"] == 6 == _plan(64, 64, 1)[1]["launches"]
    # 4096 x 4096: post.frag, one pyramid launch, polynomials, strips, and the run tables
    assert _plan(4096, 4096, 1)[1]["launches"] == 5
    # 40 x 16: lod <= 0 -- no scratch at all, post.frag and rm_bloom_kernel whatever the limit
    assert _plan(40, 16, 3, 1)[1] == dict(per_view_bytes=0, shared_bytes=0, group_views=3, groups=1, scratch_bytes=0,
                                          launches=2)
    # n = 0: nothing is allocated or launched
    st, p = _plan(64, 64, 0)
    assert st == 0 and p["groups"] == 0 and p["scratch_bytes"] == 0 and p["launches"] == 0
    # `out` may be NULL; a negative limit is refused
    assert rm.lib().rm_post_batch_plan(64, 64, 4, 0, None) == 0
    assert rm.lib().rm_post_batch_plan(64, 64, 4, -1, None) == INVALID
    assert _lib.POST_BATCH_SCRATCH_DEFAULT == DEFAULT


def test_size_rule_edges():
    ok = lambda W, H, n: _plan(W, H, n)[0] == 0  # noqa: E731
    bad = lambda W, H, n: _plan(W, H, n)[0] == INVALID  # noqa: E731
    # 0 <= n <= 65535
    assert ok(8, 8, 65535) and bad(8, 8, 65536) and bad(8, 8, -1) and ok(8, 8, 0)
    # n * W * H <= 2^31
    assert ok(1 << 10, 1 << 10, 1 << 11) and bad(1 << 10, 1 << 10, (1 << 11) + 1)
    # W * H < 2^30
    assert ok((1 << 30) - 1, 1, 1) and ok((1 << 30) - 1, 1, 2) and bad((1 << 30) - 1, 1, 3)
    assert bad(1 << 30, 1, 1) and bad(1 << 15, 1 << 15, 1) and bad(1 << 15, 1 << 15, 0)
    assert ok(32769, 32767, 1) and ok(32769, 32767, 2) and bad(32769, 32767, 3)  # 2^30 - 1 = 32769 * 32767
    assert bad(0x7FFFFFFF, 0x7FFFFFFF, 65535)  # (no overflow in the product)
    # W, H > 0
    for W, H in [(0, 8), (8, 0), (-1, 8), (8, -1)]:
        assert bad(W, H, 1) and bad(W, H, 0), (W, H)
    # the view batch's cap on tile rows does not apply: nothing is rendered
    assert ok(1, 65535 * 8 + 1, 1)


def test_calls_refuse_a_null_context():
    """No GPU work: a NULL context is refused before any pointer (junk here) is used."""
    L = rm.lib()
    junk = ctypes.c_void_p(16)
    assert L.rm_post_frag_batch(None, 8, 8, 1, 0, 0, junk, junk) == INVALID
    assert L.rm_bloom_batch(None, 8, 8, 1, junk, junk) == INVALID
    assert L.rm_post_chain_batch(None, 8, 8, 1, 0, 0, junk, junk, junk) == INVALID
    assert L.rm_set_post_batch_scratch_limit(None, 0) == INVALID


def test_prototypes_and_abi():
    L = rm.lib()
    names = {"rm_post_batch_plan": 5, "rm_set_post_batch_scratch_limit": 2, "rm_post_frag_batch": 8,
             "rm_bloom_batch": 6, "rm_post_chain_batch": 9}
    header = open(os.path.join(ROOT, "include", "rm.h")).read()
    for name, nargs in names.items():
        assert name in rm.EXPORTS
        fn = getattr(L, name)
        assert fn.restype is ctypes.c_int and len(fn.argtypes) == nargs, name
        assert re.search(rf"^rm_status {name}\(", header, re.M), name
    assert ctypes.sizeof(_lib.RmPostBatchPlan) == 40
    # new calls, no struct changed: the ABI version is still 3, in the library, the binding and the header
    assert L.rm_abi_version() == 3 == _lib.ABI_VERSION
    assert re.search(r"^#define RM_ABI_VERSION 3$", header, re.M)
    assert re.search(r"^#define RM_POST_BATCH_SCRATCH_DEFAULT \(\(int64_t\)512 << 20\)", header, re.M)
    for method in ("post_frag_batch", "bloom_batch", "post_chain_batch", "set_post_batch_scratch_limit"):
        assert hasattr(rm.Renderer, method), method


def test_plan_under_sanitizers(tmp_path):
    cxx = _compiler()
    if cxx is None:
        pytest.skip("no host C++ compiler (g++ or hipcc)")
    exe = tmp_path / "post_batch_plan_test"
    build = subprocess.run(cxx + FLAGS + SOURCES + ["-o", str(exe)], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-4000:]
    run = subprocess.run([str(exe)], cwd=tmp_path, capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, (run.stdout + run.stderr)[-4000:]
    assert "all checks passed" in run.stdout
