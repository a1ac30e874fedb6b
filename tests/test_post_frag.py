"""The generalised post.frag pass (rm_post_frag): post.frag's
main() with its sample (fxaa / texel / chromaticAberration) and tonemap
operator chosen.

CPU: the float32 restatement (tests/post_frag_ref.py) against SwiftShader
renders of the reference's post.frag (tests/golden/POSTFRAG_*.npz, written by
tests/golden/make_post_goldens.py), under SwiftShader's sampler rule
("fixed16") and against the product's ("float").  GPU: the HIP pass against
the restatement, bit for bit.

With RM_PARITY_LOG set the CPU tests append their exact / within-1-LSB figures
to that file, one JSON line per comparison.
"""
import functools
import glob
import json
import os
import re

import numpy as np
import pytest

import oracle
import post_frag_ref as ref

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
FXAA_INPUTS = ("FXAA_T_64_P0", "FXAA_O_96x54_P2", "FXAA_synthetic_61x37")
NOISE_INPUTS = ("noise_96x64", "noise_61x37")
INPUTS = FXAA_INPUTS + NOISE_INPUTS
SAMPLES = tuple(ref.POST_SAMPLES)
TONEMAPS = tuple(ref.TONEMAPS)
GATHER = [(s, t) for s in ("texel", "chromatic") for t in TONEMAPS]  # the 10 combinations without FXAA


def combos_of(name):
    return ref.COMBOS if name in FXAA_INPUTS else GATHER


def bytes_of(u32):
    return np.ascontiguousarray(u32, np.uint32).view(np.uint8).reshape(u32.shape + (4,)).astype(np.int64)


def lsb_stats(a, b):
    d = np.abs(bytes_of(a) - bytes_of(b)).max(-1)
    return float(np.mean(d == 0)), float(np.mean(d <= 1)), int(d.max())


def log(**kw):
    print(json.dumps(kw))
    if os.environ.get("RM_PARITY_LOG"):
        with open(os.environ["RM_PARITY_LOG"], "a") as fh:
            fh.write(json.dumps(dict(test="post_frag", **kw)) + "\n")


@functools.lru_cache(maxsize=None)
def fixture(name):
    z = np.load(os.path.join(HERE, "golden", f"POSTFRAG_{name}.npz"), allow_pickle=False)
    return {k: z[k] for k in z.files}


@functools.lru_cache(maxsize=None)
def fxaa_float(name):
    return oracle.fxaa(fixture(name)["input"])[1]


@functools.lru_cache(maxsize=None)
def restated(name, sample, tonemap, sampler):
    """The restatement's frame of a fixture input (computed once, shared, read-only)."""
    out = ref.post_frag(fixture(name)["input"], sample, tonemap, sampler,
                        fxaa_float=fxaa_float(name) if sample == "fxaa" else None)
    out.setflags(write=False)
    return out


# ---------------------------------------------------------------- CPU tests


def test_fixtures_present():
    paths = sorted(glob.glob(os.path.join(HERE, "golden", "POSTFRAG_*.npz")))
    assert sorted(os.path.basename(p)[9:-4] for p in paths) == sorted(INPUTS)
    for name in INPUTS:
        z = fixture(name)
        assert sorted(z) == sorted(["input", "meta"] + [f"{s}_{t}" for s, t in combos_of(name)]), name
        H, W = z["input"].shape
        assert (f"{W}x{H}" in name) or (W == H and f"_{W}_" in name)
        for s, t in combos_of(name):
            assert z[f"{s}_{t}"].shape == (H, W) and z[f"{s}_{t}"].dtype == np.uint32
    # full 32-bit noise: alpha is random too
    assert len(np.unique(fixture("noise_96x64")["input"] >> 24)) > 200


@pytest.mark.parametrize("name", INPUTS)
def test_fixed16_restatement_matches_reference_glsl(name):
    """Under SwiftShader's sampler rule the restatement is SwiftShader's frame:
    every pixel within 1 LSB, >= 0.85 exact (FXAA's policy; the differences are
    the float -> unorm8 store's rounding)."""
    for s, t in GATHER:
        exact, within1, mx = lsb_stats(restated(name, s, t, "fixed16"), fixture(name)[f"{s}_{t}"])
        log(check="fixed16_vs_swiftshader", input=name, sample=s, tonemap=t, exact=exact, within1=within1, max=mx)
        assert mx <= 1 and exact >= 0.85, (name, s, t, exact, within1, mx)


@functools.lru_cache(maxsize=None)
def taps_of(name, sample):
    return ref.post_frag(fixture(name)["input"], sample, "none", "float", return_taps=True)[1]


def near_texel_boundary(name, sample, y, x):
    """Whether a tap of pixel (y, x) has u W or v H within 1e-3 of an integer."""
    H, W = fixture(name)["input"].shape
    for u, v in taps_of(name, sample):
        for c, n in ((u[y, x], W), (v[y, x], H)):
            p = float(c) * n
            if abs(p - round(p)) <= 1e-3:
                return True
    return False


@pytest.mark.parametrize("name", INPUTS)
def test_float_rule_against_fixed16(name):
    """The product's sampler rule gives the fixed16 frame except where a tap
    lands on a texel boundary."""
    img = fixture(name)["input"]
    cap = {"FXAA_synthetic_61x37": 1, "noise_61x37": int(0.02 * img.size)}.get(name, 0)
    for s, t in GATHER:
        diff = restated(name, s, t, "float") != restated(name, s, t, "fixed16")
        n = int(diff.sum())
        log(check="float_vs_fixed16", input=name, sample=s, tonemap=t, differing=n, pixels=int(img.size))
        assert n <= cap, (name, s, t, n, cap)
        for y, x in zip(*np.nonzero(diff)):
            assert near_texel_boundary(name, s, y, x), (name, s, t, y, x)


@pytest.mark.parametrize("name", FXAA_INPUTS)
def test_fxaa_tonemap_matches_reference_glsl(name):
    """oracle.fxaa's float frame, tonemapped and stored, against SwiftShader
    (tests/test_fxaa.py's thresholds)."""
    for t in TONEMAPS:
        exact, within1, mx = lsb_stats(restated(name, "fxaa", t, "float"), fixture(name)[f"fxaa_{t}"])
        log(check="fxaa_tonemap_vs_swiftshader", input=name, tonemap=t, exact=exact, within1=within1, max=mx)
        assert within1 >= 0.999 and exact >= 0.85, (name, t, exact, within1, mx)


@pytest.mark.parametrize("name", INPUTS)
def test_restatement_identities(name):
    img = fixture(name)["input"]
    assert np.array_equal(restated(name, "texel", "none", "float"), img[::-1])
    if name in FXAA_INPUTS:
        assert np.array_equal(restated(name, "fxaa", "none", "float"), oracle.fxaa(img)[0])
    for s, t in combos_of(name):
        for sampler in ("float", "fixed16"):
            assert np.array_equal(restated(name, s, t, sampler) >> 24, img[::-1] >> 24), (s, t, sampler)


def test_python_tables_match_header():
    import raymarching_amd as rm
    txt = open(os.path.join(ROOT, "include", "rm.h")).read()

    def enum(prefix):
        return {m.group(1).lower(): int(m.group(2)) for m in re.finditer(prefix + r"(\w+) = (\d+)", txt)}
    assert rm.POST_SAMPLES == enum("RM_POST_SAMPLE_") == ref.POST_SAMPLES
    header = enum("RM_TONEMAP_")
    header["jodie"] = header.pop("reinhard_jodie")
    assert rm.TONEMAPS == header == ref.TONEMAPS


# ---------------------------------------------------------------- GPU tests


@pytest.fixture(scope="module")
def renderer(torch_cuda):
    import raymarching_amd as rm
    r = rm.Renderer(0)
    yield r
    r.close()


def to_dev(torch, img):
    return torch.from_numpy(np.ascontiguousarray(img).view(np.int32)).cuda()


def to_host(t):
    return t.cpu().numpy().view(np.uint32)


@pytest.mark.gpu
@pytest.mark.parametrize("name", INPUTS)
def test_hip_bit_exact_on_fixture_inputs(name, renderer, torch_cuda):
    """All 15 combinations: the HIP pass equals the float-rule restatement."""
    img = fixture(name)["input"]
    dev = to_dev(torch_cuda, img)
    for s, t in ref.COMBOS:
        want = restated(name, s, t, "float")
        got = to_host(renderer.post_frag(dev, s, t))
        assert np.array_equal(got, want), (name, s, t, int((got != want).sum()))


# partial tiles and clamp on all four edges; more than one tile per axis; a
# displacement far beyond a tile, per axis
SHAPES = [(1, 1), (257, 3), (8, 200), (130, 70), (4096, 64), (64, 4096)]


@pytest.mark.gpu
@pytest.mark.parametrize("W,H", SHAPES, ids=[f"{w}x{h}" for w, h in SHAPES])
def test_hip_bit_exact_on_noise(W, H, renderer, torch_cuda):
    img = np.random.default_rng(W * 65536 + H).integers(0, 2**32, (H, W), dtype=np.uint64).astype(np.uint32)
    dev = to_dev(torch_cuda, img)
    for s, t in GATHER:
        want = ref.post_frag(img, s, t)
        got = to_host(renderer.post_frag(dev, s, t))
        assert np.array_equal(got, want), (W, H, s, t, int((got != want).sum()))


@pytest.mark.gpu
def test_hip_bit_exact_on_rendered_frame(renderer, torch_cuda):
    """One scene-T P0 frame at 1024x576, 128 steps."""
    import raymarching_amd as rm
    r = renderer
    r.load_scene("template.frag")
    p = rm.POSES["P0"]
    r.set_pose(p["pos"], p["mouse"], p["time"])
    r.set_params(max_steps=128)
    f8 = r.render_rgba8(1024, 576)
    img = to_host(f8)
    assert np.array_equal(to_host(r.post_frag(f8, "chromatic", "aces")), ref.post_frag(img, "chromatic", "aces"))
    want = ref.post_frag(img, "fxaa", "reinhard", fxaa_float=oracle.fxaa(img)[1])
    assert np.array_equal(to_host(r.post_frag(f8, "fxaa", "reinhard")), want)


@pytest.mark.gpu
@pytest.mark.parametrize("W,H", [(96, 54), (1024, 576)])
def test_hip_chaining(W, H, renderer, torch_cuda):
    torch = torch_cuda
    r = renderer
    rng = np.random.default_rng(5)
    yy, xx = np.mgrid[0:H, 0:W]
    # edges (FXAA has work) over noise
    img = (rng.integers(0, 2**32, (H, W), dtype=np.uint64).astype(np.uint32) & np.uint32(0x3f3f3f3f)) | \
        np.where((xx // 9 + yy // 7) % 2, np.uint32(0xffc08040), np.uint32(0xff000000))
    dev = to_dev(torch, img)
    assert torch.equal(r.post_frag(dev), r.fxaa(dev))
    assert torch.equal(r.post_frag(dev, "fxaa", "none"), r.fxaa(dev))
    mid, out = r.post_chain(dev, sample="chromatic", tonemap="aces")
    mid2 = r.post_frag(dev, "chromatic", "aces")
    assert torch.equal(mid, mid2) and torch.equal(out, r.bloom(mid2))
    mid0, out0 = r.post_chain(dev)
    mid1, out1 = r.post_chain(dev, sample="fxaa", tonemap="none")
    assert torch.equal(mid0, mid1) and torch.equal(out0, out1)
    # (fxaa, none) through rm_post_chain_ex itself
    import ctypes
    from raymarching_amd import _lib
    mid3, out3 = torch.empty_like(dev), torch.empty_like(dev)
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    _lib.check(_lib.lib().rm_post_chain_ex(r._ctx, W, H, 0, 0, ptr(dev), ptr(mid3), ptr(out3)), r._ctx)
    assert torch.equal(mid0, mid3) and torch.equal(out0, out3)


@pytest.mark.gpu
def test_hip_errors(renderer, torch_cuda):
    import ctypes
    from raymarching_amd import _lib
    torch = torch_cuda
    L = _lib.lib()
    a = torch.zeros((4, 8), dtype=torch.int32, device="cuda")
    b = torch.zeros_like(a)
    pa, pb = ctypes.c_void_p(a.data_ptr()), ctypes.c_void_p(b.data_ptr())
    ctx = renderer._ctx
    bad = _lib.STATUS_CODES["RM_ERR_INVALID_ARGUMENT"]
    cases = {"in == out": (8, 4, 0, 0, pa, pa), "null in": (8, 4, 0, 0, None, pb), "null out": (8, 4, 0, 0, pa, None),
             "sample": (8, 4, 3, 0, pa, pb), "negative sample": (8, 4, -1, 0, pa, pb), "tonemap": (8, 4, 0, 5, pa, pb),
             "2^30 texels": (1 << 15, 1 << 15, 2, 1, pa, pb)}
    for what, args in cases.items():
        assert L.rm_post_frag(ctx, *args) == bad, what
        assert "rm_post_frag" in L.rm_last_error(ctx).decode(), what
    assert L.rm_post_frag(ctx, 8, 4, 2, 4, pa, pb) == 0
    with pytest.raises(ValueError):
        renderer.post_frag(a, sample="bilinear")
