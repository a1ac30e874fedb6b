"""View batches, the host-only parts (no GPU): rm_batch_bytes and every edge of
the size rule include/rm.h states for rm_render_batch, the layout of rm_view
from the C compiler against the ctypes struct, raymarching_amd.pack_views and
cameras.turntable."""
import ctypes
import math
import os
import subprocess

import numpy as np
import pytest

import raymarching_amd as rm
from raymarching_amd import POSES, _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = 1  # RM_ERR_INVALID_ARGUMENT


def _bytes(W, H, n, rgba8):
    frame, total = ctypes.c_int64(-1), ctypes.c_int64(-1)
    st = rm.lib().rm_batch_bytes(W, H, n, rgba8, ctypes.byref(frame), ctypes.byref(total))
    return st, frame.value, total.value


def test_batch_bytes_counts():
    assert _bytes(61, 37, 3, 1) == (0, 61 * 37 * 4, 3 * 61 * 37 * 4)
    assert _bytes(61, 37, 3, 0) == (0, 61 * 37 * 16, 3 * 61 * 37 * 16)
    assert _bytes(4096, 4096, 1, 1) == (0, 1 << 26, 1 << 26)
    assert _bytes(8, 8, 0, 0) == (0, 8 * 8 * 16, 0)
    # either pointer may be NULL
    total = ctypes.c_int64(-1)
    assert rm.lib().rm_batch_bytes(5, 3, 2, 1, None, ctypes.byref(total)) == 0 and total.value == 120
    assert rm.lib().rm_batch_bytes(5, 3, 2, 1, None, None) == 0


def test_size_rule_edges():
    # 0 <= n <= 65535
    assert _bytes(8, 8, 65535, 1)[0] == 0
    assert _bytes(8, 8, 65536, 1)[0] == INVALID
    assert _bytes(8, 8, -1, 1)[0] == INVALID
    # ceil(H / 8) <= 65535
    H = 65535 * 8
    assert _bytes(1, H, 1, 1) == (0, 4 * H, 4 * H)
    assert _bytes(1, H - 7, 1, 1)[0] == 0       # ceil((H - 7) / 8) = 65535 still
    assert _bytes(1, H + 1, 1, 1)[0] == INVALID  # ceil = 65536
    # n * W * H <= 2^31
    assert _bytes(1 << 10, 1 << 10, 1 << 11, 1) == (0, 1 << 22, 1 << 33)  # = 2^31 pixels
    assert _bytes(1 << 10, 1 << 10, 1 << 11, 0) == (0, 1 << 24, 1 << 35)
    assert _bytes(1 << 10, 1 << 10, (1 << 11) + 1, 1)[0] == INVALID       # 2^31 + W * H
    assert _bytes(1 << 16, 1 << 15, 1, 1)[0] == 0                         # one frame of 2^31
    assert _bytes((1 << 16) + 1, 1 << 15, 1, 1)[0] == INVALID
    assert _bytes(0x7FFFFFFF, 65535 * 8, 65535, 1)[0] == INVALID          # (no overflow in the product)
    # W, H > 0
    for W, H in [(0, 8), (8, 0), (-1, 8), (8, -1)]:
        assert _bytes(W, H, 1, 1)[0] == INVALID, (W, H)
        assert _bytes(W, H, 0, 1)[0] == INVALID, (W, H)


def test_rm_view_layout_matches_binding(tmp_path):
    """The C compiler's rm_view is the ctypes struct (sizeof and every offsetof),
    and a row of pack_views' array."""
    V = _lib.RmView
    src = tmp_path / "layout.c"
    src.write_text('#include "rm.h"\n#include <stddef.h>\n'
                   f'_Static_assert(sizeof(rm_view) == {ctypes.sizeof(V)}, "rm_view");\n' +
                   "".join(f'_Static_assert(offsetof(rm_view, {name}) == {getattr(V, name).offset}, "{name}");\n'
                           for name, _ in V._fields_))
    subprocess.run(["gcc", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)], check=True)
    assert [f[0] for f in V._fields_] == ["pos", "mouse", "time", "offset"]
    assert (V.pos.offset, V.mouse.offset, V.time.offset, V.offset.offset) == (0, 12, 20, 24)
    assert ctypes.sizeof(V) == 32 == rm.pack_views([POSES["P0"]]).strides[0]


def test_pack_views_forms():
    p1, p2 = POSES["P1"], POSES["P2"]
    a = rm.pack_views([p1, dict(p2, offset=(0.25, -0.5))])
    assert a.dtype == np.float32 and a.shape == (2, 8) and a.flags["C_CONTIGUOUS"]
    want = np.array([p1["pos"] + p1["mouse"] + (p1["time"], 0.0, 0.0),
                     p2["pos"] + p2["mouse"] + (p2["time"], 0.25, -0.5)], np.float32)
    assert np.array_equal(a, want)
    # POSES entries as they are; offsets default to 0
    b = rm.pack_views(list(POSES.values()))
    assert b.shape == (len(POSES), 8) and not b[:, 6:].any()
    assert np.array_equal(b[0], np.array([2, 3, 3, 0, 0, 0, 0, 0], np.float32))
    # (n, 6) and (n, 8) arrays, any float dtype; tuples of dicts; empty
    assert np.array_equal(rm.pack_views(want[:, :6].astype(np.float64))[:, :6], want[:, :6])
    assert not rm.pack_views(want[:, :6])[:, 6:].any()
    assert np.array_equal(rm.pack_views(want), want)
    assert np.array_equal(rm.pack_views((p1,)), want[:1])
    assert rm.pack_views([]).shape == (0, 8)
    assert rm.pack_views(np.zeros((0, 6), np.float32)).shape == (0, 8)
    # the result is the caller's own copy
    c = rm.pack_views(want)
    c[0, 0] = 99.0
    assert want[0, 0] != 99.0


def test_pack_views_takes_tensors():
    import torch
    t = torch.tensor([[2.0, 3.0, 3.0, 0.0, 0.0, 0.0], [1.0, 2.0, 3.0, 0.1, 0.2, 7.0]])
    a = rm.pack_views(t)
    assert a.shape == (2, 8) and np.array_equal(a[:, :6], t.numpy()) and not a[:, 6:].any()


@pytest.mark.parametrize("bad", [
    np.zeros((2, 7), np.float32), np.zeros((6,), np.float32), np.zeros((2, 3, 8), np.float32),
    [dict(pos=(0, 0, 0), mouse=(0, 0))], [dict(pos=(0, 0), mouse=(0, 0), time=0.0)],
    [dict(pos=(0, 0, 0), mouse=(0, 0), time=0.0, offset=(0.0,))], [dict(pos=(0, 0, 0), mouse=(0, 0), time=0.0, fov=1)],
    [(0, 0, 0, 0, 0, 0)],
])
def test_pack_views_refuses_wrong_shapes(bad):
    with pytest.raises(ValueError):
        rm.pack_views(bad)


def test_pack_views_refuses_bad_offsets():
    base = dict(POSES["P0"])
    assert rm.pack_views([dict(base, offset=(-0.5, 0.49999997))]).shape == (1, 8)  # both ends of [-0.5, 0.5)
    for off in [(0.5, 0.0), (0.0, 0.5), (-0.50000006, 0.0), (float("nan"), 0.0), (0.0, float("inf"))]:
        with pytest.raises(ValueError):
            rm.pack_views([dict(base, offset=off)])
    row = np.array([[2, 3, 3, 0, 0, 0, 0.5, 0]], np.float32)
    with pytest.raises(ValueError):
        rm.pack_views(row)
    with pytest.raises(ValueError):
        rm.pack_views([dict(base, time=float("nan"))])


def test_turntable():
    n, radius, height = 12, 4.0, 6.0
    views = rm.turntable(n, radius, height)
    assert len(views) == n and all(set(v) == {"pos", "mouse", "time"} for v in views)
    a = rm.pack_views(views)
    # on the circle, at the height, around the sponge's axis x = z = 0
    assert np.allclose(np.hypot(a[:, 0], a[:, 2]), radius, rtol=0, atol=1e-6)
    assert np.array_equal(a[:, 1], np.full(n, height, np.float32))
    assert not a[:, 5].any() and not a[:, 6:].any()
    # view 0 by hand: phi = 0, so the camera stands at (0, 6, 4) on the +Z side.  The centre (0, 3, 0) is then at
    # (0, -3, -4) from it, L = 5: forward = (cos my sin mx, -sin my, -cos my cos mx) = (0, -3/5, -4/5) needs
    # mx = 0 (yaw) and sin my = 3/5, cos my = 4/5, my = atan2(3, 4) = 0.6435011 (pitch, looking down)
    assert views[0]["pos"] == (0.0, 6.0, 4.0)
    assert views[0]["mouse"][0] == 0.0 and math.copysign(1.0, views[0]["mouse"][0]) == 1.0
    assert views[0]["mouse"][1] == float(np.float32(0.6435011087932844))
    # view 3 of 12 by hand: phi = 90 degrees, the camera at (4, 6, 0) looks down -X: yaw -pi/2
    assert np.allclose(views[3]["pos"], (4.0, 6.0, 0.0), atol=1e-6)
    assert views[3]["mouse"][0] == float(np.float32(-math.pi / 2))
    # every view looks at the centre: camera_ray's rotations of (0, 0, -1), in double
    for v in views:
        mx, my = v["mouse"]
        fwd = np.array([math.cos(my) * math.sin(mx), -math.sin(my), -math.cos(my) * math.cos(mx)])
        to_centre = np.array([0.0, 3.0, 0.0]) - np.array(v["pos"])
        assert np.allclose(fwd, to_centre / np.linalg.norm(to_centre), atol=1e-6)
        assert -math.pi < mx <= float(np.float32(math.pi))  # (-pi, pi], the bound rounded to f32 as the yaw is
    assert views[6]["mouse"][0] == float(np.float32(math.pi))  # phi = 180 degrees: +pi, not -pi
    # the time of every view; the level camera; no views
    assert all(v["time"] == 12.5 for v in rm.turntable(3, 2.0, 3.0, target_time=12.5))
    assert all(v["mouse"][1] == 0.0 for v in rm.turntable(3, 2.0, 3.0))
    assert rm.turntable(0, 1.0, 1.0) == []
    with pytest.raises(ValueError):
        rm.turntable(3, 0.0, 1.0)
