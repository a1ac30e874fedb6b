"""Ray images for Renderer.shade_rays (rm_shade_rays): cameras other than the
pass's pinhole, built on the host in numpy.  No GPU, no librm.

Every function returns unit directions, float32 [H, W, 3], row 0 first, one
ray through each pixel centre; shade them with width=W (and vignette=True for
the frame's vignette).  The camera looks down -Z with +Y up, as main()'s does
before the mouse rotations.
"""
from __future__ import annotations

import numpy as np

F32 = np.float32


def _rot_rows(a, b, angle):
    """(a, b) *= rot(angle), GLSL's row vector times mat2(c, -s, s, c)
    (common.frag:1088-1092), in f32."""
    c, s = np.cos(angle, dtype=F32), np.sin(angle, dtype=F32)
    return a * c + b * -s, a * s + b * c


def _uv(W, H):
    """main()'s uv at the pixel centres of a W x H frame with u_resolution =
    (W, H) (output_shader.frag:390), f32: ([H, W], [H, W])"""
    tcx = (np.arange(W, dtype=F32) + F32(0.5)) / F32(W)
    tcy = (np.arange(H, dtype=F32) + F32(0.5)) / F32(H)
    ux = (tcx - F32(0.5)) * F32(W) / F32(H)
    uy = (tcy - F32(0.5)) * F32(H) / F32(H)
    return np.broadcast_to(ux[None, :], (H, W)), np.broadcast_to(uy[:, None], (H, W))


def fisheye_rays(W: int, H: int, fov_deg: float = 110.0, mouse=(0.0, 0.0)) -> np.ndarray:
    """The fisheye camera main() carries commented out
    (output_shader.frag:396-400): (0, 0, -1) turned by -uv.y and uv.x times
    radians(fov) / 2, then by the two mouse rotations (:403-404), operation
    for operation in f32."""
    ux, uy = _uv(W, H)
    coeff = F32(fov_deg) * F32(0.017453292519943295) * F32(0.5)
    x = np.zeros((H, W), F32)
    y = np.zeros((H, W), F32)
    z = np.full((H, W), -1.0, F32)
    y, z = _rot_rows(y, z, -uy * coeff)
    x, z = _rot_rows(x, z, ux * coeff)
    y, z = _rot_rows(y, z, F32(-mouse[1]))
    x, z = _rot_rows(x, z, F32(mouse[0]))
    return np.ascontiguousarray(np.stack([x, y, z], axis=-1), F32)


# OpenGL's cube-map faces (the major axis, and the axes s and t run along):
# direction = major + s * sc + t * tc with s, t in (-1, 1), t growing with the row
CUBE_FACES = ("+X", "-X", "+Y", "-Y", "+Z", "-Z")
_CUBE_AXES = {
    "+X": ((1, 0, 0), (0, 0, -1), (0, -1, 0)),
    "-X": ((-1, 0, 0), (0, 0, 1), (0, -1, 0)),
    "+Y": ((0, 1, 0), (1, 0, 0), (0, 0, 1)),
    "-Y": ((0, -1, 0), (1, 0, 0), (0, 0, -1)),
    "+Z": ((0, 0, 1), (1, 0, 0), (0, -1, 0)),
    "-Z": ((0, 0, -1), (-1, 0, 0), (0, -1, 0)),
}


def cube_face_axes(face):
    """(major, s, t) axes of a face, float64 [3] each"""
    if isinstance(face, int):
        face = CUBE_FACES[face]
    return tuple(np.array(a, np.float64) for a in _CUBE_AXES[face])


def cubemap_rays(size: int, face) -> np.ndarray:
    """One face (a name of CUBE_FACES or its index) of a cube map in the
    OpenGL convention: 90 degrees, size x size pixel centres."""
    major, sc, tc = cube_face_axes(face)
    c = (np.arange(size, dtype=np.float64) + 0.5) * (2.0 / size) - 1.0
    d = major[None, None, :] + c[None, :, None] * sc[None, None, :] + c[:, None, None] * tc[None, None, :]
    d /= np.linalg.norm(d, axis=-1, keepdims=True)
    return np.ascontiguousarray(d, F32)


SPONGE_CENTRE = (0.0, 3.0, 0.0)  # the sponge of scenes T and O (transformR's translation, common.frag:434-441)


def turntable(n: int, radius: float, height: float, target_time=None) -> list:
    """n views for Renderer.render_batch on a circle of `radius` at y =
    `height` around the sponge at (0, 3, 0), each looking at its centre: a list
    of dicts in POSES' form (pos, mouse, time), values rounded to float32.
    target_time: the u_time of every view (the sponge's own rotation is
    2 * u_time degrees); None: 0.

    View k stands at the angle phi = 2 pi k / n: pos = (radius sin phi, height,
    radius cos phi), so view 0 is on the +Z side looking down -Z, as main()'s
    camera does before the mouse rotations.  camera_ray turns the forward ray
    (0, 0, -1) by rd.yz *= rot(-u_mouse.y), then rd.xz *= rot(u_mouse.x), with
    rot(a) = mat2(cos a, -sin a, sin a, cos a) applied to a row vector
    (output_shader.frag:403-404), which gives
        forward = (cos my sin mx, -sin my, -cos my cos mx).
    The direction to the centre is (-radius sin phi, 3 - height, -radius cos phi)
    / L with L = sqrt(radius^2 + (3 - height)^2); equating the two,
        yaw   u_mouse.x = -phi  (wrapped into (-pi, pi]),
        pitch u_mouse.y = atan2(height - 3, radius)  (positive: looking down).
    """
    if n < 0 or not radius > 0.0:
        raise ValueError("turntable: n >= 0 and radius > 0")
    pitch = float(F32(np.arctan2(float(height) - SPONGE_CENTRE[1], float(radius))))
    t = float(F32(0.0 if target_time is None else target_time))
    views = []
    for k in range(int(n)):
        phi = 2.0 * np.pi * k / n
        yaw = (-phi if phi < np.pi else 2.0 * np.pi - phi) + 0.0  # (+ 0.0: view 0's yaw is 0, not -0)
        pos = (float(F32(radius * np.sin(phi))), float(F32(height)), float(F32(radius * np.cos(phi))))
        views.append(dict(pos=pos, mouse=(float(F32(yaw)), pitch), time=t))
    return views


def equirect_rays(W: int, H: int) -> np.ndarray:
    """An equirectangular panorama: longitude -pi..pi along a row (the centre
    column looks down -Z, +X to its right), latitude +pi/2 (up, +Y) at the top
    to -pi/2 at the bottom."""
    lon = ((np.arange(W, dtype=np.float64) + 0.5) / W) * (2.0 * np.pi) - np.pi
    lat = np.pi / 2.0 - ((np.arange(H, dtype=np.float64) + 0.5) / H) * np.pi
    cl = np.cos(lat)[:, None]
    d = np.stack([cl * np.sin(lon)[None, :], np.broadcast_to(np.sin(lat)[:, None], (H, W)), -cl * np.cos(lon)[None, :]],
                 axis=-1)
    d /= np.linalg.norm(d, axis=-1, keepdims=True)
    return np.ascontiguousarray(d, F32)
