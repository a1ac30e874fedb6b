"""Scene T's soft-shadow certificate (raymarching_amd/csrc/rm_shadow_clear.h,
DESIGN.md 2.24) restated in numpy on the pixel-centre rays of a frame, for
tests/test_shadow_clear_gpu.py: which pixels hit the sponge, which of those are
lit (phong's dot(L, N) >= 0) and which lit ones pass the predicate, so that a
pose can be chosen, and asserted, to clear no lane, some lanes or most lanes.

The march and the normal are the CPU oracle's (oracle.scene_dist,
oracle.normal), in float32; the kernels' hardware reciprocals and fused
operations are not restated, so a lane within a few ulps of a threshold may be
decided differently: the poses are chosen with the shares far from where that
matters, and the tests compare shares and signs, never single lanes.  CPU only.
"""
import math

import numpy as np

import oracle
from raymarching_amd.poses import POSES

F32 = np.float32
ZNEAR, ZFAR = F32(0.02), F32(50.0)
K_RATIO = F32(0.35)          # rmsc::kRatio
MINT = F32(0.01)             # render_T_from's mint
LIGHT = np.array([20.0, 50.0, 0.0], F32)

# The poses of tests/test_shadow_clear_gpu.py and what each intends for the share of lit lanes the certificate
# clears ("most": above 0.5, "some": strictly between 0 and 1, "none": 0 with lit lanes in the frame).  The
# light stands at (20, 50, 0): seen from the sponge its direction is (0.37, 0.92, 0), so at u_time 0 the lit
# side face x = +1 leaves at a slope of 0.37 and the top face at 0.92; the sponge turns by 2 u_time degrees.
POSE_SET = {
    # the headline pose: the lit side face fills the sponge's region, whole waves clear
    "P0": (POSES["P0"], "most"),
    # from above, looking down: the top face, lit at a slope of 0.9
    "above": (dict(pos=(0.5, 7.0, 2.0), mouse=(0.0, 1.0), time=0.0), "most"),
    # the side face turned by 12 degrees: its lanes' slopes straddle kRatio
    "side_above": (dict(pos=(2.0, 2.6, 3.0), mouse=(0.0, 0.0), time=6.0), "some"),
    # turned by 20 degrees: every lane's slope is below kRatio (and the top edge is out of sight)
    "side_below": (dict(pos=(2.0, 2.6, 3.0), mouse=(0.0, 0.0), time=10.0), "none"),
    # turned by 40 degrees: a second face is lit, at slopes of 0.23-0.25, where a march does lower the shadow
    # factor: no lane may clear (a ratio of 0.2 instead of kRatio would clear these lanes and change their pixels)
    "side_low": (dict(pos=(2.0, 2.4, 3.0), mouse=(0.0, 0.0), time=20.0), "none"),
    # from the unlit side, through the holes: only inner walls are lit, and their rays start inside the cube
    "inner": (dict(pos=(-2.5, 3.4, 0.2), mouse=(math.pi / 2, 0.1), time=0.0), "none"),
}
SIZES = [(64, 64), (96, 54), (61, 37)]  # 61x37: ragged tiles, partly filled waves


def share_is_as_intended(intent, lit, share):
    if intent == "most":
        return lit > 0 and share > 0.5
    if intent == "some":
        return lit > 0 and 0.0 < share < 1.0
    return lit > 0 and share == 0.0


def camera_dirs(W, H, mouse):
    """main()'s ray directions at the pixel centres (output_shader.frag:388-405) -> [H * W, 3] float32"""
    tcx = (np.arange(W, dtype=F32) + F32(0.5)) / F32(W)
    tcy = (np.arange(H, dtype=F32) + F32(0.5)) / F32(H)
    ux = ((tcx - F32(0.5)) * F32(W) / F32(H)).astype(F32)
    uy = (tcy - F32(0.5)).astype(F32)
    v = np.stack([np.broadcast_to(ux[None, :], (H, W)), np.broadcast_to(-uy[:, None], (H, W)),
                  np.full((H, W), F32(-1.0))], -1).reshape(-1, 3).astype(F32)
    v = (v / np.sqrt((v * v).sum(-1, dtype=F32))[:, None]).astype(F32)
    c1, s1 = F32(np.cos(-mouse[1])), F32(np.sin(-mouse[1]))
    c2, s2 = F32(np.cos(mouse[0])), F32(np.sin(mouse[0]))
    y1 = v[:, 1] * c1 - v[:, 2] * s1
    z1 = v[:, 1] * s1 + v[:, 2] * c1
    x2 = v[:, 0] * c2 - z1 * s2
    z2 = v[:, 0] * s2 + z1 * c2
    return np.stack([x2, y1, z2], -1).astype(F32)


def primary_hits(pose, W, H, max_steps):
    """castRay (common.frag:931-954) over scene T's distance -> (points [n, 3], hit [n] bool)"""
    rd = camera_dirs(W, H, pose["mouse"])
    ro = np.asarray(pose["pos"], F32)
    n = len(rd)
    depth = np.full(n, ZNEAR, F32)
    hit = np.zeros(n, bool)
    live = np.arange(n)
    for _ in range(int(max_steps)):
        if not len(live):
            break
        p = (ro + rd[live] * depth[live, None]).astype(F32)
        d = oracle.scene_dist("T", p, time=pose["time"])
        h = d < F32(0.001)
        hit[live[h]] = True
        nd = (depth[live] + d).astype(F32)
        depth[live[~h]] = nd[~h]
        live = live[~h & (nd < ZFAR)]
    return (ro + rd * depth[:, None]).astype(F32), hit


def sponge_rotation(time):
    """transformR(.., vec3(180, 2 u_time, 0)): (ry_c, ry_s, rx_c, rx_s), frame_const's angles"""
    ay = -F32(time) * F32(2.0) * F32(0.017453292519943295)
    ax = F32(-180.0) * F32(0.017453292519943295)
    return F32(np.cos(ay)), F32(np.sin(ay)), F32(np.cos(ax)), F32(np.sin(ax))


def sponge_rot(R, v):
    """sponge_rot<false> (rm_device.h), rows of v"""
    yc, ys, xc, xs = R
    x1 = v[:, 0] * yc + v[:, 2] * ys
    z1 = v[:, 2] * yc - v[:, 0] * ys
    y2 = v[:, 1] * xc - z1 * xs
    z2 = z1 * xc + v[:, 1] * xs
    return np.stack([x1, y2, z2], -1).astype(F32)


def shadow_clear(o, d, mint=MINT, ratio=K_RATIO):
    """rmsc::shadow_clear on rows of sponge-space origins o and directions d -> [n] bool"""
    o, d = np.asarray(o, F32), np.asarray(d, F32)
    with np.errstate(invalid="ignore"):
        ok = (np.abs(o).sum(-1, dtype=F32) <= F32(1024.0)) & (np.abs(d) <= F32(1.0 + 2.0 ** -10)).all(-1)
        ok &= bool(F32(0.01) <= mint <= F32(1.0))
        u = np.where(o < 0, -d, d).astype(F32)
        b0 = (np.abs(o) - F32(1.0)).astype(F32)
        axis = (u >= ratio) & ((b0 + u * mint).astype(F32) >= F32(ratio * mint))
    return ok & axis.any(-1)


def frame_masks(pose, W, H, max_steps):
    """-> dict of [H * W] bool masks: hit, lit (hit and phong's dot(L, N) >= 0), clear (lit and certified)"""
    p, hit = primary_hits(pose, W, H, max_steps)
    lit = np.zeros(len(p), bool)
    clear = np.zeros(len(p), bool)
    if hit.any():
        ph = p[hit]
        n = oracle.normal("T", ph, time=pose["time"])
        L = (LIGHT - ph).astype(F32)
        L = (L / np.sqrt((L * L).sum(-1, dtype=F32))[:, None]).astype(F32)
        l = ~((L * n).sum(-1, dtype=F32) < 0)
        R = sponge_rotation(pose["time"])
        o = sponge_rot(R, (ph - np.array([0.0, 3.0, 0.0], F32)).astype(F32))
        c = l & shadow_clear(o, sponge_rot(R, L))
        lit[hit], clear[hit] = l, c
    return dict(hit=hit, lit=lit, clear=clear)


def cleared_share(pose, W, H, max_steps):
    """-> (lit lanes, cleared lanes / lit lanes) of the frame"""
    m = frame_masks(pose, W, H, max_steps)
    nl = int(m["lit"].sum())
    return nl, (float(m["clear"].sum()) / nl if nl else 0.0)
