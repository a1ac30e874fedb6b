"""Scene T's reflection certificate (raymarching_amd/csrc/rm_refl_clear.h,
DESIGN.md 2.25) restated in numpy on the pixel-centre rays of a frame, for
tests/test_refl_clear_gpu.py: which pixels hit the sponge and which of those
pass the predicate on their reflection ray, so that a pose can be chosen, and
asserted, to clear most lanes, few lanes, lanes on both sides of kRatio, or to
have no hit lane at all.

The camera rays, the primary march and the sponge's rotation are those of
tests/shadow_clear_ref.py (imported); the normal is the CPU oracle's.  All in
float32; the kernels' hardware reciprocals and fused operations are not
restated, so a lane within a few ulps of a threshold may be decided
differently: the poses are chosen with the shares far from where that matters,
and the tests compare shares and signs, never single lanes.  CPU only.
"""

import numpy as np

import oracle
from raymarching_amd.poses import POSES
from tests.shadow_clear_ref import camera_dirs, primary_hits, sponge_rot, sponge_rotation  # noqa: F401

F32 = np.float32
ZNEAR = F32(0.02)
K_RATIO = F32(0.2)           # rmrc::kRatio
K_STEPS = 28                 # rmrc::kSteps: ceil(log(150) / log(1 + kRatio))
MAX_DIR = F32(1.0 + 2.0 ** -10)
MIN_LEN2 = F32(1.0 - 2.0 ** -10)

# The poses of tests/test_refl_clear_gpu.py and what each intends for the share of hit lanes the certificate
# clears: "most" (above 0.5), "few" (below 0.1, with hit lanes in the frame), "straddle" (strictly between 0 and
# 1, with hit lanes whose best slope lies within 0.05 of kRatio on either side), "nohit" (no lane hits).
POSE_SET = {
    # the headline pose: the faces z = +1 head-on and x = +1 at slopes of 0.2-0.4; inner walls do not clear
    "P0": (POSES["P0"], "most"),
    # from above, looking down on the top face
    "above": (dict(pos=(0.5, 7.0, 2.0), mouse=(0.0, 1.0), time=0.0), "most"),
    # the camera in the sponge's central void: only inner walls, whose reflection rays start inside the cube
    # (walls at a hole's mouth do clear: the share is small, not 0)
    "void": (dict(pos=(0.0, 3.0, 0.0), mouse=(0.0, 0.0), time=0.0), "few"),
    # looking along the face x = +1 from 0.3 in front of its plane: the reflected slope is 0.3 / the distance
    # along the face, 0.3 at its near edge and 0.1 at its far edge, so its lanes lie on both sides of kRatio
    # (from 0.2 in front of the plane no lane of the face would reach kRatio)
    "grazing": (dict(pos=(1.3, 3.0, 2.0), mouse=(-0.3, 0.0), time=0.0), "straddle"),
    # the sponge turned by 40 degrees
    "turned": (dict(POSES["P0"], time=20.0), "most"),
    # no hit at all
    "P7": (POSES["P7"], "nohit"),
    # 0.1 in front of a solid patch of the face z = +1, head-on: every lane hits within 12 steps and reflects
    # straight back, so every lane clears, under any step cap >= 12 (test_count_is_the_steps_below_depth_3)
    "wall": (dict(pos=(0.43, 3.56, 1.1), mouse=(0.0, 0.0), time=0.0), "most"),
}
SIZES = [(64, 64), (96, 54), (61, 37)]  # 61x37: ragged tiles, partly filled waves


def refl_clear(o, d, ratio=K_RATIO):
    """rmrc::refl_clear on rows of sponge-space origins o and directions d -> ([n] bool, [n] best slope):
    the second is max_i u_i over the axes whose second condition holds (-inf if none), what kRatio is held against"""
    o, d = np.asarray(o, F32), np.asarray(d, F32)
    ratio = F32(ratio)
    with np.errstate(invalid="ignore", over="ignore"):
        len2 = (d[:, 2] * d[:, 2] + (d[:, 1] * d[:, 1] + d[:, 0] * d[:, 0])).astype(F32)
        ok = (np.abs(o).sum(-1, dtype=F32) <= F32(1024.0)) & (np.abs(d) <= MAX_DIR).all(-1) & (len2 >= MIN_LEN2)
        u = np.where(o < 0, -d, d).astype(F32)
        b0 = (np.abs(o) - F32(1.0)).astype(F32)
        second = (b0 + u * ZNEAR).astype(F32) >= F32(ratio * ZNEAR)
        axis = (u >= ratio) & second
        # (the slope the ratio is compared with: on the axes that are outside the face at ZNEAR at all)
        outside = (b0 + u * ZNEAR).astype(F32) >= F32(0.0)
        best = np.where(outside, u, -np.inf).max(-1)
    return ok & axis.any(-1), best


def frame_masks(pose, W, H, max_steps, ratio=K_RATIO):
    """-> dict: hit [H * W] bool, clear [H * W] bool (hit and certified), slope [H * W] (best outward slope of
    the hit lanes' reflection rays, nan elsewhere)"""
    p, hit = primary_hits(pose, W, H, max_steps)
    clear = np.zeros(len(p), bool)
    slope = np.full(len(p), np.nan)
    if hit.any():
        ph = p[hit]
        rd = camera_dirs(W, H, pose["mouse"])[hit]
        n = oracle.normal("T", ph, time=pose["time"]).astype(F32)
        dn = (rd * n).sum(-1, dtype=F32)
        rdir = (rd - F32(2.0) * dn[:, None] * n).astype(F32)  # reflect(rd, n)
        ror = (ph + rdir * F32(0.01)).astype(F32)
        R = sponge_rotation(pose["time"])
        o = sponge_rot(R, (ror - np.array([0.0, 3.0, 0.0], F32)).astype(F32))
        c, best = refl_clear(o, sponge_rot(R, rdir), ratio)
        clear[hit], slope[hit] = c, best
    return dict(hit=hit, clear=clear, slope=slope)


def cleared_steps(pose, W, H, max_steps):
    """-> (cleared lanes, the steps of their reflection marches that begin at a depth < 3): what
    rm_reflection_cleared_steps counts outside far-sky waves.  castRay in world space over the oracle's distance:
    a lane's count may differ from the kernels' sponge-space march by a step where a depth lands within
    roundings of 3, so the tests allow one step per cleared lane."""
    m = frame_masks(pose, W, H, max_steps)
    sel = m["clear"]
    if not sel.any():
        return 0, 0
    p, _ = primary_hits(pose, W, H, max_steps)
    ph = p[sel]
    rd = camera_dirs(W, H, pose["mouse"])[sel]
    n = oracle.normal("T", ph, time=pose["time"]).astype(F32)
    rdir = (rd - F32(2.0) * (rd * n).sum(-1, dtype=F32)[:, None] * n).astype(F32)
    ror = (ph + rdir * F32(0.01)).astype(F32)
    depth = np.full(len(ph), ZNEAR, F32)
    live = np.arange(len(ph))
    steps = 0
    for _ in range(int(max_steps)):
        if not len(live):
            break
        steps += int((depth[live] < F32(3.0)).sum())
        d = oracle.scene_dist("T", (ror[live] + rdir[live] * depth[live, None]).astype(F32), time=pose["time"])
        h = d < F32(0.001)
        nd = (depth[live] + d).astype(F32)
        depth[live[~h]] = nd[~h]
        live = live[~h & (nd < F32(50.0))]
    return int(sel.sum()), steps


def cleared_share(pose, W, H, max_steps):
    """-> (hit lanes, cleared lanes / hit lanes, hit lanes with slope in [kRatio - 0.05, kRatio),
    hit lanes with slope in [kRatio, kRatio + 0.05]) of the frame"""
    m = frame_masks(pose, W, H, max_steps)
    nh = int(m["hit"].sum())
    s = m["slope"][m["hit"]]
    k = float(K_RATIO)
    below = int(((s >= k - 0.05) & (s < k)).sum())
    above = int(((s >= k) & (s <= k + 0.05)).sum())
    return nh, (float(m["clear"].sum()) / nh if nh else 0.0), below, above


def share_is_as_intended(intent, hit, share, below, above):
    if intent == "most":
        return hit > 0 and share > 0.5
    if intent == "few":
        return hit > 0 and share < 0.1
    if intent == "straddle":
        return hit > 0 and 0.0 < share < 1.0 and below > 0 and above > 0
    return hit == 0 and share == 0.0
