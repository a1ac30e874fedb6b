"""Targets that show a pixel no launch wrote.

A test that compares `R.render(W, H)` with a reference in a loop gives every
launch after the first a target the caching allocator has just taken back from
the previous iteration: the block still holds the identical frame, and a tile
the dispatch order never reached compares equal.  `target` returns a tensor
filled with a word no render kernel can write, to pass as `out=`;
`assert_frame` compares the launch's words with the reference's and says how
much of the target still holds that word."""
import numpy as np

# RGBA8: every rendered word has alpha 0xFF (pack_rgba8(..., 1.0f) and
# pack_rgb8_opaque), so the word 0 is never written.
RGBA8_WORD = 0x00000000
# float32: a NaN with a payload no arithmetic produces, in all four channels.
FLOAT_WORD = 0x7FC0DEAD


def target(torch, shape, dtype):
    """A device tensor of `shape` and `dtype` (torch.int32: RGBA8 words, or
    torch.float32) filled with the sentinel word of that type."""
    if dtype == torch.int32:
        return torch.full(tuple(shape), RGBA8_WORD, dtype=torch.int32, device="cuda")
    assert dtype == torch.float32, dtype
    return torch.full(tuple(shape), FLOAT_WORD, dtype=torch.int32, device="cuda").view(torch.float32)


def words(t):
    """A torch tensor or numpy array of 32-bit elements as uint32 words (numpy)."""
    a = t.detach().cpu().numpy() if hasattr(t, "detach") else np.asarray(t)
    assert a.dtype.itemsize == 4, a.dtype
    return np.ascontiguousarray(a).view(np.uint32)


def assert_frame(out, ref, what=""):
    """`out`, a frame rendered into a `target`, equals `ref` (a tensor or an
    array of the same shape) word for word.  On a mismatch: how many words
    differ, how many still hold the sentinel, and the 8x8 tile coordinates of
    the first few such pixels."""
    o, r = words(out), words(ref)
    assert o.shape == r.shape, (what, o.shape, r.shape)
    if np.array_equal(o, r):
        return
    is_float = (out.dtype.is_floating_point if hasattr(out, "is_floating_point") else out.dtype.kind == "f")
    s = FLOAT_WORD if is_float else RGBA8_WORD
    px = (o == s) if o.ndim == 2 else (o == s).all(axis=-1)  # (a float4 pixel: all four channels)
    diff = (o != r) if o.ndim == 2 else (o != r).any(axis=-1)
    ys, xs = np.nonzero(px)
    tiles = sorted({(int(x) // 8, int(y) // 8) for x, y in zip(xs[:4096], ys[:4096])}, key=lambda t: (t[1], t[0]))
    dy, dx = np.nonzero(diff)
    raise AssertionError(
        f"{what}: {int(diff.sum())} of {diff.size} pixels differ from the reference (the first at x {int(dx[0])}, "
        f"y {int(dy[0])}); {int(px.sum())} pixels still hold the sentinel word {s:#010x}: no launch wrote them"
        + (f", first in the 8x8 tiles (x, y) {tiles[:8]}" if tiles else ""))
