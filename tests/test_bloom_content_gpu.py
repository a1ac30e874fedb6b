"""rm_bloom against oracle.bloom, bit for bit, on content that bloom's mip
levels keep (bloom_content.py), at the smallest sizes that reach each path of
launch_bloom: the four pyramid kernels, the pyramid started at level s0 = 1
and 2 behind rm_mip_down_kernel, the per-level resample with odd level sizes
and chunked scans, strip and batch tails, 0 < lod <= 1.26 and lod <= 0.
test_bloom_content.py (CPU) holds oracle.bloom to the float64 definition on
the same content, and checks what is claimed of these sizes: the pyramid plan,
fr, and both sides of the base texel's fast path.

All kinds of content of a size run in one test, to keep the launches of a
size together (one run-table build).
"""
import numpy as np
import pytest

import bloom_content as bc
import oracle
import raymarching_amd as rm


def ids(sizes):
    return [f"{w}x{h}" for w, h in sizes]


@pytest.fixture(scope="module")
def R(torch_cuda):
    r = rm.Renderer(0)
    yield r
    r.close()


def to_dev(img):
    import torch
    return torch.from_numpy(img.view(np.int32)).cuda()


def to_host(t):
    return t.cpu().numpy().view(np.uint32)


def hip_bloom(R, img):
    import torch
    out = R.bloom(to_dev(img))
    torch.cuda.synchronize()
    return to_host(out)


@pytest.mark.gpu
@pytest.mark.parametrize("W,H", bc.GPU_SIZES, ids=ids(bc.GPU_SIZES))
def test_hip_bloom_bit_exact_on_content(R, W, H):
    """Every kind of content; at the pyramid sizes also `block2` with one
    2^d2-texel block changed: the HIP output must change in the same pixels as
    the restatement's, some of them outside the block -- a pyramid workgroup
    that wrote its tile elsewhere would move the change."""
    rng = np.random.default_rng(W * 7919 + H)
    for kind, gen in bc.KINDS.items():
        img = gen(W, H, rng)
        got, ref = hip_bloom(R, img), oracle.bloom(img)[0]
        assert np.array_equal(got, ref), (kind, float(np.mean(got != ref)))
        if kind == "block2" and (W, H) in bc.PYRAMID + bc.FR0:
            img2, (y0, y1, x0, x1) = bc.one_block_changed(img, rng)
            got2, ref2 = hip_bloom(R, img2), oracle.bloom(img2)[0]
            moved = ref2 != ref
            assert np.array_equal(got2 != got, moved), "the change of one block lands elsewhere"
            inside = moved[H - y1:H - y0, x0:x1].copy()  # (bloom.frag:36 flips v: the block's rows from the bottom)
            moved[H - y1:H - y0, x0:x1] = False
            assert inside.mean() > 0.5 and moved.any()  # (beyond the block: through the levels alone)


@pytest.mark.gpu
@pytest.mark.parametrize("W,H", [(1100, 640), (128, 896)], ids=ids([(1100, 640), (128, 896)]))
def test_hip_bloom_cached_run_tables_on_content(R, W, H):
    """test_hip_bloom_cached_run_tables' sequence on `block` content -- same
    size, same size, smaller size, same size again, other stream -- with a
    bloom of the transposed size H x W between the two same-size calls: the
    tables of one size must not serve the other."""
    import torch
    rng = np.random.default_rng(W + 7 * H)
    imgs = [bc.block(W, H, rng) for _ in range(2)]
    small = bc.block(W // 2, H // 2, rng)
    turned = bc.block(H, W, rng)

    def same(img):
        return np.array_equal(hip_bloom(R, img), oracle.bloom(img)[0])

    for n, img in enumerate((imgs[0], turned, imgs[1], small, imgs[1])):
        assert same(img), n
    s = torch.cuda.Stream()
    try:
        with torch.cuda.stream(s):
            R.set_stream(s)
            got = hip_bloom(R, imgs[0])  # rebuilt (stream)
    finally:
        R.set_stream(torch.cuda.current_stream())
    assert np.array_equal(got, oracle.bloom(imgs[0])[0])
    assert same(imgs[1])


@pytest.mark.gpu
@pytest.mark.parametrize("W,H", [(128, 896), (1100, 640)], ids=ids([(128, 896), (1100, 640)]))
def test_post_chain_blooms_its_own_mid(R, W, H):
    """rm_post_chain and rm_post_chain_ex (texel, none) on `dark` and `checker`
    frames: `out` is oracle.bloom of the chain's own `mid`, byte for byte."""
    rng = np.random.default_rng(W * 31 + H)
    for kind in ("dark", "checker"):
        dev = to_dev(bc.KINDS[kind](W, H, rng))
        for choice in ({}, dict(sample="texel", tonemap="none")):
            mid, out = R.post_chain(dev, **choice)
            ref = oracle.bloom(to_host(mid))[0]
            got = to_host(out)
            assert np.array_equal(got, ref), (kind, choice, float(np.mean(got != ref)))
