"""Both FXAA kernels of rm_fxaa.hip against the oracle, bit for bit, at the
sizes and on the content their shortcuts are argued for:

* frames smaller than the LDS kernel's halo, ragged tiles, sides at the LDS
  kernel's limit of 2^20, and one past it, where rm_fxaa_kernel takes over;
* `noise` (almost every pixel long-span: the span taps and the halo) and
  `sparks` (workgroups that mix wholly short 8 x 8 blocks, which take the
  short-span shortcut, with blocks that do not), tests/fxaa_ref.py;
* FXAA under every tonemap operator, and the (fxaa, none) forms of
  rm_post_frag and rm_post_chain against rm_fxaa;
* the 2^30-texel guards of rm_fxaa and rm_post_chain.

The claims themselves are checked on the CPU in tests/test_fxaa_claims.py.
"""
import ctypes
import functools

import numpy as np
import pytest

import fxaa_ref as fr
import oracle
import post_frag_ref

M = fr.M
TONEMAPS = ("aces", "reinhard", "jodie", "uncharted2")


def cases(shapes):
    c = [(w, h, k) for w, h in shapes for k in fr.CONTENTS]
    return pytest.mark.parametrize("W,H,content", c, ids=[f"{w}x{h}-{k}" for w, h, k in c])


def _reference(W, H, content):
    img = fr.CONTENTS[content](W, H)
    out, outf = oracle.fxaa(img)
    for a in (img, out, outf):
        a.setflags(write=False)
    return img, out, outf


_small_reference = functools.lru_cache(maxsize=None)(_reference)


def reference(W, H, content):
    """(frame, oracle's RGBA8 frame, oracle's float frame) of a case; the small
    ones are computed once and shared, read-only."""
    return (_small_reference if W * H <= 1 << 16 else _reference)(W, H, content)


@pytest.fixture(scope="module")
def renderer(torch_cuda):
    import raymarching_amd as rm
    r = rm.Renderer(0)
    yield r
    r.close()


def to_dev(torch, img):
    return torch.from_numpy(np.array(img, np.uint32).view(np.int32)).cuda()  # (a copy: the references are read-only)


def to_host(t):
    return t.cpu().numpy().view(np.uint32)


def assert_same(got, want, what):
    if not np.array_equal(got, want):
        bad = np.argwhere(got != want)
        y, x = bad[0]
        raise AssertionError(f"{what}: {len(bad)} of {want.size} pixels differ, the first at (x, y) = ({x}, {y}): "
                             f"{got[y, x]:#010x}, expected {want[y, x]:#010x}")


def assert_content_bites(W, H, content, img, want):
    """A pass means something only if the frame exercises what it is for."""
    if content == "noise":
        if W >= 3 and H >= 3:  # (a frame one pixel wide comes back unchanged)
            changed = float((want != img[::-1]).mean())
            print(f"noise {W}x{H}: {changed:.3f} of the output words differ from the flipped input")
            assert changed >= 0.5, changed
        return
    # sparks: workgroups mix wholly short 8 x 8 blocks with blocks that have long pixels
    thin = max(W, H) >= M - 1
    if not (thin or (W >= 63 and H >= 31)):
        return
    cols = (0, 4096) if (W, H) == (M + 1, 18) else None  # (19 M pixels: the statistic of its first 4096 columns)
    share = fr.short_block_share(fr.short_mask(fr.fxaa(img, x_range=cols)))
    print(f"sparks {W}x{H}: {share:.3f} of the 8x8 blocks are wholly short")
    assert 0.2 <= share <= (0.95 if thin else 0.9), share


def check_fxaa(renderer, torch, W, H, content):
    img, want, _ = reference(W, H, content)
    assert_content_bites(W, H, content, img, want)
    got = to_host(renderer.fxaa(to_dev(torch, img)))
    assert_same(got, want, f"rm_fxaa {W}x{H} {content}")


@pytest.mark.gpu
@cases(fr.SMALL + fr.RAGGED + fr.LIMIT)
def test_lds_kernel_bit_exact(W, H, content, renderer, torch_cuda):
    assert W <= 2**20 and H <= 2**20  # FXL_MAX_DIM: rm_fxaa_lds_kernel
    check_fxaa(renderer, torch_cuda, W, H, content)


@pytest.mark.gpu
@cases(fr.FALLBACK)
def test_fallback_kernel_bit_exact(W, H, content, renderer, torch_cuda):
    # a side above FXL_MAX_DIM (rm_fxaa.hip) is what sends a frame to rm_fxaa_kernel: if that
    # constant moves, fail here instead of testing the LDS kernel twice
    assert W > 2**20 or H > 2**20
    check_fxaa(renderer, torch_cuda, W, H, content)


@pytest.mark.gpu
@cases([(7, 5), (130, 70), (M, 3), (M + 1, 2)])
def test_fxaa_tonemap_bit_exact(W, H, content, renderer, torch_cuda):
    """FXAA under each tonemap operator: the LDS kernel's and (at 2^20 + 1) the
    fallback kernel's four instantiations besides rm_fxaa's own."""
    if (W, H) == (M + 1, 2):
        assert W > 2**20 or H > 2**20  # FXL_MAX_DIM: rm_fxaa_kernel
    img, _, wantf = reference(W, H, content)
    dev = to_dev(torch_cuda, img)
    for t in TONEMAPS:
        want = post_frag_ref.post_frag(img, "fxaa", t, fxaa_float=wantf)
        got = to_host(renderer.post_frag(dev, "fxaa", t))
        assert_same(got, want, f"rm_post_frag fxaa/{t} {W}x{H} {content}")


@pytest.mark.gpu
@cases([(130, 70), (M + 1, 2)])
def test_post_frag_none_and_chain_equal_fxaa(W, H, content, renderer, torch_cuda):
    if (W, H) == (M + 1, 2):
        assert W > 2**20 or H > 2**20  # FXL_MAX_DIM: rm_fxaa_kernel
    img, want, _ = reference(W, H, content)
    dev = to_dev(torch_cuda, img)
    got = to_host(renderer.fxaa(dev))
    assert_same(got, want, f"rm_fxaa {W}x{H} {content}")
    assert_same(to_host(renderer.post_frag(dev, "fxaa", "none")), got, f"rm_post_frag fxaa/none {W}x{H} {content}")
    assert_same(to_host(renderer.post_chain(dev)[0]), got, f"rm_post_chain's FXAA frame {W}x{H} {content}")


@pytest.mark.gpu
def test_texel_count_guards(renderer, torch_cuda):
    """rm_fxaa and rm_post_chain reject frames of 2^30 texels or more (the
    kernels' 32-bit byte offsets) before anything is launched."""
    from raymarching_amd import _lib
    torch = torch_cuda
    L = _lib.lib()
    a, b, c = (torch.zeros((4, 8), dtype=torch.int32, device="cuda") for _ in range(3))
    pa, pb, pc = (ctypes.c_void_p(t.data_ptr()) for t in (a, b, c))
    ctx = renderer._ctx
    bad = _lib.STATUS_CODES["RM_ERR_INVALID_ARGUMENT"]
    assert L.rm_fxaa(ctx, 1 << 15, 1 << 15, pa, pb) == bad
    assert "rm_fxaa" in L.rm_last_error(ctx).decode()
    assert L.rm_post_chain(ctx, 1 << 15, 1 << 15, pa, pb, pc) == bad
    assert "rm_post_chain" in L.rm_last_error(ctx).decode()
    # the same buffers at their own size pass
    assert L.rm_fxaa(ctx, 8, 4, pa, pb) == 0
    assert L.rm_post_chain(ctx, 8, 4, pa, pb, pc) == 0
    torch.cuda.synchronize()
