"""float32 numpy restatement of the generalised post.frag pass (rm_post_frag,
DESIGN.md 2.18): the statement of post.frag's main() with a choice of sample
(fxaa / texel / chromaticAberration) and of tonemap operator, operation for
operation in float32 (no contraction, correctly rounded division, mix(x, y, a)
= x + (y - x) a, clamp = min(max()), dot left to right).

Two sampler rules turn a texture coordinate into a texel index:
  "float"    the product's: clamp(floor(u * W)) in float32;
  "fixed16"  SwiftShader's: (floor(u * 65536) * W) >> 16, clamped.
They differ only where u * W lands on a texel boundary.

The FXAA branch does not restate FXAA: it takes oracle.fxaa's float frame.
"""
import numpy as np

POST_SAMPLES = {"fxaa": 0, "texel": 1, "chromatic": 2}
TONEMAPS = {"none": 0, "aces": 1, "reinhard": 2, "jodie": 3, "uncharted2": 4}

f32 = np.float32


def _tex_index(u, n, sampler):
    """Texel index of coordinate u (float32 array) on an axis of n texels."""
    if sampler == "float":
        i = np.floor(u * f32(n)).astype(np.int64)
    elif sampler == "fixed16":
        i = (np.floor(u * f32(65536.0)).astype(np.int64) * n) >> 16
    else:
        raise ValueError(sampler)
    return np.clip(i, 0, n - 1)


def _fetch(img, u, v, sampler):
    H, W = img.shape
    return img[_tex_index(v, H, sampler), _tex_index(u, W, sampler)]


def _chan(t, k):
    return ((t >> np.uint32(8 * k)) & np.uint32(255)).astype(f32) * f32(1.0 / 255.0)


def _clamp01(c):
    return np.minimum(np.maximum(c, f32(0.0)), f32(1.0))


def chromatic_factors():
    """The 8 x 3 channel factors: rf *= 0.9972, gf *= 0.998, bf /= 0.9988 in float32."""
    rf = gf = bf = f32(1.0)
    out = []
    for _ in range(8):
        out.append((rf, gf, bf))
        rf = f32(rf * f32(0.9972))
        gf = f32(gf * f32(0.998))
        bf = f32(bf / f32(0.9988))
    return out


def chromatic(img, U, V, sampler, taps=None):
    """post.frag:113-131 at coordinates (U, V): [H, W, 3] float32."""
    ux = f32(1.0) - f32(2.0) * U
    uy = f32(1.0) - f32(2.0) * V
    c = [np.zeros(U.shape, f32) for _ in range(3)]
    f = f32(1.0 / 8.0)
    for fac in chromatic_factors():
        for k in range(3):
            u = f32(0.5) - f32(0.5) * (ux * fac[k])
            v = f32(0.5) - f32(0.5) * (uy * fac[k])
            if taps is not None:
                taps.append((u, v))
            c[k] = c[k] + f * _chan(_fetch(img, u, v, sampler), k)
        c = [_clamp01(x) for x in c]
    return np.stack(c, -1)


def _aces(x):
    a, b, c, d, e = f32(2.51), f32(0.03), f32(2.43), f32(0.59), f32(0.14)
    return (x * (a * x + b)) / (x * (c * x + d) + e)


def _reinhard(c):
    return c / (c + f32(1.0))


def _jodie(c):
    lum = (c[..., 0] * f32(0.2126) + c[..., 1] * f32(0.7152)) + c[..., 2] * f32(0.0722)
    tc = c / (c + f32(1.0))
    x = c / (lum[..., None] + f32(1.0))
    return x + (tc - x) * tc


def _u2_partial(x):
    A, B, C, D, E, F = f32(0.15), f32(0.50), f32(0.10), f32(0.20), f32(0.02), f32(0.30)
    CB, DE, DF, EF = f32(C * B), f32(D * E), f32(D * F), f32(E / F)
    return ((x * (A * x + CB) + DE) / (x * (A * x + B) + DF)) - EF


def _uncharted2(v):
    white_scale = f32(f32(1.0) / _u2_partial(f32(11.2)))
    return _u2_partial(v * f32(2.0)) * white_scale


_TONEMAP_FN = {"none": lambda c: c, "aces": _aces, "reinhard": _reinhard, "jodie": _jodie,
               "uncharted2": _uncharted2}


def tonemap(rgb, name):
    return np.asarray(_TONEMAP_FN[name](np.asarray(rgb, f32)), f32)


def store(rgba):
    """gl_FragColor -> RGBA8 word: rint(clamp(c, 0, 1) * 255) per channel."""
    q = np.rint(_clamp01(np.asarray(rgba, f32)) * f32(255.0)).astype(np.uint32)
    return q[..., 0] | (q[..., 1] << 8) | (q[..., 2] << 16) | (q[..., 3] << 24)


def post_frag(img_u32, sample="fxaa", tonemap_name="none", sampler="float", fxaa_float=None, return_taps=False):
    """The pass over an [H, W] RGBA8 frame -> [H, W] RGBA8 (flipped vertically,
    as post.frag:140).  sample "fxaa" needs fxaa_float = oracle.fxaa(img)[1].
    return_taps: also the list of (u, v) float32 coordinate arrays of every
    texture() call of the pixel (the centre sample first)."""
    img = np.ascontiguousarray(img_u32, np.uint32)
    H, W = img.shape
    with np.errstate(all="ignore"):
        tx = (np.arange(W, dtype=f32) + f32(0.5)) / f32(W)
        ty = (np.arange(H, dtype=f32) + f32(0.5)) / f32(H)
        U = np.broadcast_to(tx[None, :], (H, W))
        V = np.broadcast_to((f32(1.0) - ty)[:, None], (H, W))
        taps = [(U, V)]
        if sample == "fxaa":
            if fxaa_float is None:
                raise ValueError("sample='fxaa' takes oracle.fxaa's float frame")
            color = np.asarray(fxaa_float, f32)
        else:
            centre = _fetch(img, U, V, sampler)
            alpha = _chan(centre, 3)
            if sample == "texel":
                rgb = np.stack([_chan(centre, k) for k in range(3)], -1)
            elif sample == "chromatic":
                rgb = chromatic(img, U, V, sampler, taps)
            else:
                raise ValueError(sample)
            color = np.concatenate([rgb, alpha[..., None]], -1)
        out = store(np.concatenate([tonemap(color[..., :3], tonemap_name), color[..., 3:]], -1))
    return (out, taps) if return_taps else out


COMBOS = [(s, t) for s in POST_SAMPLES for t in TONEMAPS]
