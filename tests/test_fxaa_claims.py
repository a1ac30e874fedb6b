"""The claims rm_fxaa.hip's LDS kernel rests on, checked on the CPU against the
oracle and its numpy restatement (tests/fxaa_ref.py), at the shapes the GPU
tests run (tests/test_fxaa_shapes_gpu.py) up to about 3.2 M pixels:

1. the five +-1 / centre taps address integer texels x + s, H - 1 - y + s
   (test_integer_taps, test_fixed_taps_of_the_frames);
2. every span tap addresses a texel within 4 of the pixel's on both axes, and
   noise reaches 4 (test_span_taps_within_halo);
3. a pixel whose span is at most 0.5 texel outputs its flipped centre texel
   (test_short_span_outputs_centre_texel), on frames that have such pixels
   (sparks) and frames that have almost none (noise).

The restatement is licensed by test_restatement_equals_oracle.
"""
import functools

import numpy as np
import pytest

import fxaa_ref as fr
import oracle

M = fr.M
SHAPES = [s for s in fr.SMALL + fr.RAGGED + fr.LIMIT + fr.FALLBACK if s[0] * s[1] <= 3_200_000]
CASES = [(w, h, c) for w, h in SHAPES for c in fr.CONTENTS]
case = pytest.mark.parametrize("W,H,content", CASES, ids=[f"{w}x{h}-{c}" for w, h, c in CASES])


@functools.lru_cache(maxsize=None)
def facts(W, H, content):
    """What the tests below assert on, from one oracle frame and one
    restatement of the case (a few numbers; the frames are not kept)."""
    img = fr.CONTENTS[content](W, H)
    want = oracle.fxaa(img)[0]
    r = fr.fxaa(img)
    x = np.arange(W, dtype=np.int64)[None, :]
    ty = (H - 1 - np.arange(H, dtype=np.int64))[:, None]  # the pixel's texel row
    short = fr.short_mask(r)
    first = np.argwhere(r.out != want)
    return dict(
        differing=int((r.out != want).sum()), first=tuple(first[0][::-1]) if len(first) else None,
        fixed_wrong=sum(int((tx != x + sx).sum()) + int((tyk != ty + sy).sum())
                        for (tx, tyk), (sx, sy) in zip(r.fixed_taps, fr.FIXED)),
        reach_x=max(int(np.abs(tx - x).max()) for tx, _ in r.span_taps),
        reach_y=max(int(np.abs(tyk - ty).max()) for _, tyk in r.span_taps),
        short_share=float(short.mean()),
        short_not_centre=int((want[short] != img[::-1][short]).sum()),
        changed_share=float((want != img[::-1]).mean()))


@case
def test_restatement_equals_oracle(W, H, content):
    f = facts(W, H, content)
    assert f["differing"] == 0, f"{f['differing']} pixels differ, the first at (x, y) = {f['first']}"


SIDES = [1, 2, 3, 5, 61, 1000, 4096, 65537, 999983, M - 1, M]


@pytest.mark.parametrize("n", SIDES)
def test_integer_taps(n):
    """floor((fx + s / W) W) = x + s and floor((1 - (y + .5) / H + s / H) H) =
    H - 1 - y + s for s = -1, 0, 1, at every pixel of the axis: no exception."""
    c = np.arange(n, dtype=np.int64)
    steps = np.array([-1, 0, 1])[:, None]
    assert np.array_equal(fr.fixed_tap_coords(n, False), c[None, :] + steps)
    assert np.array_equal(fr.fixed_tap_coords(n, True), (n - 1 - c)[None, :] + steps)


@case
def test_fixed_taps_of_the_frames(W, H, content):
    """The same identity through the restatement's own five taps (it also
    holds one past FXL_MAX_DIM = 2^20, where the kernel no longer relies on it)."""
    assert facts(W, H, content)["fixed_wrong"] == 0


@case
def test_span_taps_within_halo(W, H, content):
    f = facts(W, H, content)
    assert f["reach_x"] <= 4 and f["reach_y"] <= 4, f
    if content == "noise" and W >= 63 and H >= 31:
        # the input reaches the halo's edge: a halo of 3 would not hold it
        assert f["reach_x"] == 4 and f["reach_y"] == 4, f


@case
def test_short_span_outputs_centre_texel(W, H, content):
    """The proof of the LDS kernel's short-span shortcut: at every pixel with
    max(|dxs|, |dys|) <= 0.5 the oracle's word is the flipped centre texel."""
    f = facts(W, H, content)
    assert f["short_not_centre"] == 0, f
    # neither vacuous (sparks is mostly short) nor all there is (noise is not)
    if content == "sparks":
        assert f["short_share"] >= 0.9, f
    elif W * H >= 64:
        assert f["short_share"] <= 0.1, f
