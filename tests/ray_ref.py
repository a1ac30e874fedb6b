"""Reference for the ray queries (rm_cast_rays, rm_camera_rays): castRayD /
castRayDI (common.frag:879-925) as a numpy march over a distance callable,
every operation rounded to float32 and none fused, as the GLSL restatement
(oracle/rm_oracle.c) evaluates them:

    p = ro + (rd * depth);  hit iff d < 0.001f * depth;  else depth = depth + d;
    miss iff depth >= ZFAR

tests/test_rays.py pins it against oracle.render_diag's primary hit depths
(bit for bit) and compares the kernels with it.
"""
import numpy as np

F32 = np.float32
ZNEAR, ZFAR = F32(0.02), F32(50.0)
MISS, HIT, EXHAUSTED = 0, 1, 2  # include/rm.h RM_RAY_*


def march(dist, origins, directions, max_steps, inside=False):
    """dist: points [m, 3] f32 -> distances [m] f32.  origins [n, 3] or [3],
    directions [n, 3].  Returns dict(t, status, steps, last, position): t is
    castRayD's dist, last the last point evaluated (the origin without steps),
    position = ro + rd * t where t > 0, else 0."""
    rd = np.ascontiguousarray(directions, F32).reshape(-1, 3)
    n = len(rd)
    ro = np.ascontiguousarray(np.broadcast_to(np.asarray(origins, F32), (n, 3)))
    depth = np.full(n, ZNEAR, F32)
    t = np.zeros(n, F32)
    status = np.full(n, EXHAUSTED, np.int32)
    steps = np.zeros(n, np.int32)
    last = ro.copy()
    live = np.arange(n)
    with np.errstate(all="ignore"):
        for _ in range(int(max_steps)):
            if not len(live):
                break
            dp = depth[live]
            p = (ro[live] + (rd[live] * dp[:, None]).astype(F32)).astype(F32)
            res = np.asarray(dist(p), F32)
            d = -res if inside else res
            last[live] = p
            steps[live] += 1
            t[live] = res
            hit = d < (F32(0.001) * dp).astype(F32)
            nd = (dp + d).astype(F32)
            miss = ~hit & (nd >= ZFAR)
            t[live[hit]] = dp[hit]
            status[live[hit]] = HIT
            t[live[miss]] = F32(-1.0)
            status[live[miss]] = MISS
            go = ~hit & ~miss
            depth[live[go]] = nd[go]
            live = live[go]
        shade = t > 0
        pos = np.zeros((n, 3), F32)
        pos[shade] = (ro[shade] + (rd[shade] * t[shade, None]).astype(F32)).astype(F32)
    return dict(t=t, status=status, steps=steps, last=last, position=pos)


def ray_set(scene, seed=5, n=4096):
    """The test rays: origins uniform in [-6, 0.05, -6]..[6, 6, 6]; the first
    half of the directions aimed at c + U(-1.5, 1.5)^3 (c: the sphere of S0,
    the sponge of T/O/OG), the second half isotropic; normalised in double,
    then rounded to float32."""
    rng = np.random.default_rng(seed)
    o = rng.uniform([-6.0, 0.05, -6.0], [6.0, 6.0, 6.0], (n, 3))
    c = np.array([0.0, 1.0, -3.0] if scene == "S0" else [0.0, 3.0, 0.0])
    h = n // 2
    aimed = c + rng.uniform(-1.5, 1.5, (h, 3)) - o[:h]
    d = np.concatenate([aimed, rng.normal(size=(n - h, 3))])
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return o.astype(F32), d.astype(F32)


def inside_ray_set(seed=5, n=1024):
    """Rays that start inside scene OG's glass sphere ((3, 2, 3), r = 1):
    origins (3, 2, 3) + N(0, 0.3^2), isotropic directions."""
    rng = np.random.default_rng(seed)
    o = np.array([3.0, 2.0, 3.0]) + rng.normal(scale=0.3, size=(n, 3))
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return o.astype(F32), d.astype(F32)


def camera_dirs_unrotated(W, H, res=None):
    """main()'s ray directions with u_mouse = (0, 0) (output_shader.frag:
    388-405), float32, no fused operations: normalize(uv.x, -uv.y, -1) as
    v * (1 / length(v)) at the pixel centres -> [H, W, 3]."""
    rx, ry = (F32(W), F32(H)) if res is None else (F32(res[0]), F32(res[1]))
    tcx = (np.arange(W, dtype=F32) + F32(0.5)) / F32(W)
    tcy = (np.arange(H, dtype=F32) + F32(0.5)) / F32(H)
    ux = ((tcx - F32(0.5)) * rx / ry).astype(F32)
    uy = ((tcy - F32(0.5)) * ry / ry).astype(F32)
    vx = np.broadcast_to(ux[None, :], (H, W))
    vy = np.broadcast_to(-uy[:, None], (H, W))
    vz = np.full((H, W), F32(-1.0))
    l2 = ((vx * vx + vy * vy).astype(F32) + vz * vz).astype(F32)
    inv = (F32(1.0) / np.sqrt(l2).astype(F32)).astype(F32)
    x, y, z = vx * inv, vy * inv, vz * inv
    # rd.yz *= rot(-0); rd.xz *= rot(0) with cos = 1, sin = 0 (row vector x mat2(c, -s, s, c)): the values
    # stay, but a -0 component (the centre row of an odd H) becomes +0, as in the GLSL
    c, s = F32(1.0), F32(0.0)
    y1 = y * c + z * -s
    z1 = y * s + z * c
    x2 = x * c + z1 * -s
    z2 = x * s + z1 * c
    return np.stack([x2, y1, z2], -1).astype(F32)
