"""The post passes over a batch of frames on the GPU (include/rm.h
rm_post_frag_batch, rm_bloom_batch, rm_post_chain_batch): every
view against this build's own single-frame call on the same frame -- every byte,
no tolerance; the single calls are tied to the oracle by tests/test_post_frag.py,
tests/test_bloom_content_gpu.py and tests/test_gpu_parity.py.  Every (sample,
tonemap) and bloom on each path of the mip chain with strongly differing
neighbouring views, rendered batches, groups under a scratch limit, more views
than a byte counts, n = 1 and 0, the life of bloom's scratch across single calls,
sizes and streams, the argument checks and the headless app."""
import ctypes
import json
import os
import subprocess

import numpy as np
import pytest

import oracle
import raymarching_amd as rm
from raymarching_amd import POSES, _lib
from tests import bloom_content as bc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = 1
STEPS = 128
SENTINEL = 0x5A5A5A5A  # (alpha 0x5A: bloom writes alpha 255, and no test frame below carries this word)
SAMPLES, TONEMAPS = tuple(_lib.POST_SAMPLES), tuple(_lib.TONEMAPS)
# neighbouring views differ strongly: structured content next to flat 0 and flat 255
KINDS = ("block", "flat255", "dark", "flat0", "checker", "border", "impulse")


@pytest.fixture(scope="module")
def R(torch_cuda):
    r = rm.Renderer(0)
    yield r
    r.close()


def _dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int32)).cuda()


def _frames(W, H, n, seed):
    """n frames of W x H, view v of kind KINDS[(seed + v) % 7], as [n, H, W] uint32; no word is SENTINEL"""
    rng = np.random.default_rng(1000 + seed)
    f = np.stack([bc.KINDS[KINDS[(seed + v) % len(KINDS)]](W, H, rng) for v in range(n)])
    f[f == SENTINEL] ^= 1
    return f


def _target(torch, n, H, W):
    """a target one frame longer than the batch, filled with the sentinel"""
    return torch.full((n + 1, H, W), SENTINEL, dtype=torch.int32, device="cuda")


def _intact(t, n):
    """views 0..n-1 written (no sentinel word left: the alpha differs), the frame after them untouched"""
    return bool((t[n] == SENTINEL).all())


# ------------------------------------------------- 1. every view is the single call

SHAPES = [(61, 37, 4), (64, 64, 4), (40, 16, 3), (200, 150, 3), bc.PYRAMID[0] + (3,), bc.PYRAMID[1] + (3,),
          bc.PYRAMID[2] + (3,), bc.PYRAMID[3] + (3,), bc.PYRAMID[4] + (2,)]


def test_shapes_take_the_paths_they_are_here_for():
    """(CPU) the plan's launches tell the path: d1 = 0, resampled levels, lod <= 0, pyramid <0>..<3>, s0 = 1"""
    assert bc.PYRAMID[:5] == [(64, 448), (128, 896), (256, 1792), (256, 3584), (512, 7168)]
    launches = {s: rm.post_batch_plan(*s)["launches"] for s in SHAPES}
    assert launches[(61, 37, 4)] == 1 + 1 + 2 + 1 and oracle.bloom_levels(61, 37)[1:] == (0, 1)
    assert launches[(64, 64, 4)] == 1 + 2 + 2 + 1 and oracle.bloom_levels(64, 64)[1:] == (1, 2)
    assert launches[(40, 16, 3)] == 2 and oracle.bloom_levels(40, 16)[0] <= 0
    assert launches[(200, 150, 3)] == 1 + 3 + 2 + 1  # (200 x 150 -> 100 x 75 -> 50 x 37 -> 25 x 18: odd sizes)
    for W, H, n in SHAPES[4:8]:  # one pyramid launch: d2 = 5..8 levels below the frame
        assert launches[(W, H, n)] == 1 + 1 + 2 + 1 and oracle.bloom_levels(W, H)[2] == 5 + SHAPES.index((W, H, n)) - 4
    assert launches[(512, 7168, 2)] == 1 + 2 + 2 + 1 and oracle.bloom_levels(512, 7168)[2] == 9  # s0 = 1: one level, then the pyramid


@pytest.mark.parametrize("W,H,n", SHAPES, ids=[f"{w}x{h}x{n}" for w, h, n in SHAPES])
def test_every_view_is_the_single_call(R, torch_cuda, W, H, n):
    torch = torch_cuda
    frames = _dev(torch, _frames(W, H, n, SHAPES.index((W, H, n))))
    assert not torch.equal(frames[0], frames[1])
    out = _target(torch, n, H, W)
    R.bloom_batch(frames, out=out)
    for v in range(n):
        assert torch.equal(out[v], R.bloom(frames[v])), ("bloom", v)
    assert _intact(out, n)
    for sample in SAMPLES:
        for tonemap in TONEMAPS:
            out = _target(torch, n, H, W)
            R.post_frag_batch(frames, sample, tonemap, out=out)
            for v in range(n):
                assert torch.equal(out[v], R.post_frag(frames[v], sample, tonemap)), (sample, tonemap, v)
            assert _intact(out, n)
    # (FXAA, NONE) is rm_fxaa; and the views are not each other's (a batch that wrote view 0 everywhere fails above)
    out = R.post_frag_batch(frames)
    assert all(torch.equal(out[v], R.fxaa(frames[v])) for v in range(n))
    # the chain: mid and out are the two batch calls' and post_chain's
    mid, out = _target(torch, n, H, W), _target(torch, n, H, W)
    R.post_chain_batch(frames, mid, out, "chromatic", "aces")
    for v in range(n):
        m1, o1 = R.post_chain(frames[v], sample="chromatic", tonemap="aces")
        assert torch.equal(mid[v], m1) and torch.equal(out[v], o1), v
    assert _intact(mid, n) and _intact(out, n)


def test_a_view_does_not_read_its_neighbours(R, torch_cuda):
    """Changing views 0 and 2 changes no byte of view 1 (flat 0 between two bright views: a tap, a halo texel or
    a table entry read across the border would lift it), on the resample and the pyramid path."""
    torch = torch_cuda
    for W, H in [(61, 37), (64, 448)]:
        rng = np.random.default_rng(5)
        quiet = bc.flat0(W, H, rng)
        a = np.stack([bc.flat255(W, H, rng), quiet, bc.block(W, H, rng)])
        b = np.stack([bc.block2(W, H, rng), quiet, bc.flat255(W, H, rng)])
        (ma, oa), (mb, ob) = R.post_chain_batch(_dev(torch, a)), R.post_chain_batch(_dev(torch, b))
        assert torch.equal(ma[1], mb[1]) and torch.equal(oa[1], ob[1])
        assert bool(((oa[1] & 0xFFFFFF) == 0).all())  # black stays black: nothing bloomed in from the neighbours


# ------------------------------------------------- 2. rendered batches

@pytest.mark.parametrize("scene", ["T", "O"])
@pytest.mark.parametrize("W,H", [(61, 37), (64, 64)])
def test_chain_on_rendered_batches(R, torch_cuda, scene, W, H):
    torch = torch_cuda
    R.load_scene(rm.SCENE_FILES[scene])
    R.set_params(max_steps=STEPS, shadow_max_steps=0, count_evals=0)
    views = [POSES[k] for k in ("P0", "P1", "P2", "P7")]
    frames = R.render_batch(W, H, views)
    mid, out = R.post_chain_batch(frames)
    for v in range(4):
        m1, o1 = R.post_chain(frames[v])
        assert torch.equal(mid[v], m1) and torch.equal(out[v], o1), v
    if (scene, W, H) == ("T", 61, 37):  # ... and the oracle's, on one shape
        for v in range(4):
            f = frames[v].cpu().numpy().view(np.uint32)
            want_mid = oracle.fxaa(f)[0]
            assert np.array_equal(mid[v].cpu().numpy().view(np.uint32), want_mid), v
            assert np.array_equal(out[v].cpu().numpy().view(np.uint32), oracle.bloom(want_mid)[0]), v


# ------------------------------------------------- 3. groups

def test_groups_give_the_same_bytes(R, torch_cuda):
    torch = torch_cuda
    W, H, n = 61, 37, 7
    frames = _dev(torch, _frames(W, H, n, 3))
    plan = rm.post_batch_plan(W, H, n)
    assert plan["groups"] == 1 and plan["per_view_bytes"] > 0
    want_mid, want_out = R.post_chain_batch(frames)
    for v in range(n):
        m1, o1 = R.post_chain(frames[v])
        assert torch.equal(want_mid[v], m1) and torch.equal(want_out[v], o1), v
    three = plan["shared_bytes"] + 3 * plan["per_view_bytes"]
    try:
        for limit, groups in [(three, 3), (plan["per_view_bytes"] - 1, 7), (1, 7)]:
            p = rm.post_batch_plan(W, H, n, limit)
            assert p["groups"] == groups and p["group_views"] == -(-n // groups)
            R.set_post_batch_scratch_limit(limit)
            mid, out = _target(torch, n, H, W), _target(torch, n, H, W)
            R.post_chain_batch(frames, mid, out)
            assert torch.equal(mid[:n], want_mid) and torch.equal(out[:n], want_out), limit
            assert _intact(mid, n) and _intact(out, n)
            assert torch.equal(R.bloom_batch(want_mid), want_out), limit
    finally:
        R.set_post_batch_scratch_limit(0)
    assert torch.equal(R.post_chain_batch(frames)[1], want_out)


# ------------------------------------------------- 4. many views, one view, none

@pytest.mark.parametrize("W,H", [(8, 8), (33, 20)])
def test_more_views_than_a_byte_counts(R, torch_cuda, W, H):
    torch = torch_cuda
    n = 300
    rng = np.random.default_rng(8)
    frames = _dev(torch, np.stack([bc.noise(W, H, rng) for _ in range(n)]))
    mid, out = _target(torch, n, H, W), _target(torch, n, H, W)
    R.post_chain_batch(frames, mid, out)
    for v in (0, 255, 256, n - 1):
        m1, o1 = R.post_chain(frames[v])
        assert torch.equal(mid[v], m1) and torch.equal(out[v], o1), v
    assert _intact(mid, n) and _intact(out, n)


def test_one_view_and_none(R, torch_cuda):
    torch = torch_cuda
    W, H = 64, 64
    frames = _dev(torch, _frames(W, H, 1, 0))
    mid, out = _target(torch, 1, H, W), _target(torch, 1, H, W)
    R.post_chain_batch(frames, mid, out)
    m1, o1 = R.post_chain(frames[0])
    assert torch.equal(mid[0], m1) and torch.equal(out[0], o1) and _intact(mid, 1) and _intact(out, 1)
    # n = 0: RM_OK, nothing written (and the buffers may be NULL)
    L = rm.lib()
    mid, out = _target(torch, 0, H, W), _target(torch, 0, H, W)
    p = [ctypes.c_void_p(t.data_ptr()) for t in (frames, mid, out)]
    assert L.rm_post_chain_batch(R._ctx, W, H, 0, 0, 0, *p) == 0
    assert L.rm_post_frag_batch(R._ctx, W, H, 0, 0, 0, p[0], p[1]) == 0
    assert L.rm_bloom_batch(R._ctx, W, H, 0, p[0], p[2]) == 0
    assert L.rm_post_chain_batch(R._ctx, W, H, 0, 0, 0, None, None, None) == 0
    torch.cuda.synchronize()
    assert _intact(mid, 0) and _intact(out, 0)


# ------------------------------------------------- 5. the life of bloom's scratch

def test_scratch_across_single_calls_and_sizes(R, torch_cuda):
    """A batch, a single bloom of its size, a batch of another size, a single bloom of the first size: the run
    tables are shared with rm_bloom, kept where the size and stream stay, rebuilt where they change."""
    torch = torch_cuda
    a = _dev(torch, _frames(64, 64, 4, 1))
    b = _dev(torch, _frames(61, 37, 3, 2))
    r2 = rm.Renderer(0)  # a context that has never bloomed gives the reference bytes
    try:
        want_a = [r2.bloom(a[v]) for v in range(4)]
        want_b = [r2.bloom(b[v]) for v in range(3)]
    finally:
        torch.cuda.synchronize()
        r2.close()
    out_a = R.bloom_batch(a)
    single_1 = R.bloom(a[2])
    out_b = R.bloom_batch(b)
    single_2 = R.bloom(a[3])
    out_a2 = R.bloom_batch(a)
    single_3 = R.bloom(b[1])
    assert all(torch.equal(out_a[v], want_a[v]) and torch.equal(out_a2[v], want_a[v]) for v in range(4))
    assert all(torch.equal(out_b[v], want_b[v]) for v in range(3))
    assert torch.equal(single_1, want_a[2]) and torch.equal(single_2, want_a[3]) and torch.equal(single_3, want_b[1])


def test_two_batches_in_flight_and_stream_changes(R, torch_cuda):
    torch = torch_cuda
    a = _dev(torch, _frames(64, 64, 4, 4))
    b = _dev(torch, _frames(64, 64, 4, 5))
    want = {}
    for name, f in (("a", a), ("b", b)):
        pairs = [R.post_chain(f[v]) for v in range(4)]
        want[name] = (torch.stack([p[0] for p in pairs]), torch.stack([p[1] for p in pairs]))
    torch.cuda.synchronize()
    # two batches in flight on one stream: the second reuses the scratch behind the first
    ra, rb = R.post_chain_batch(a), R.post_chain_batch(b)
    assert torch.equal(ra[0], want["a"][0]) and torch.equal(ra[1], want["a"][1])
    assert torch.equal(rb[0], want["b"][0]) and torch.equal(rb[1], want["b"][1])
    for kept in (False, True):  # (kept: PyTorch's pool streams are never destroyed)
        s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
        r = rm.Renderer(0)
        torch.cuda.synchronize()
        try:
            r.set_stream(s1, kept=kept)
            with torch.cuda.stream(s1):
                ra = r.post_chain_batch(a)
            r.set_stream(s2, kept=kept)
            with torch.cuda.stream(s2):
                rb = r.post_chain_batch(b)
                single = r.bloom(want["a"][0][1])
            r.set_stream(None)
            rc = r.post_chain_batch(a)  # back on the default stream
            torch.cuda.synchronize()
        finally:
            r.close()
        assert torch.equal(ra[1], want["a"][1]) and torch.equal(rb[1], want["b"][1]), kept
        assert torch.equal(rb[0], want["b"][0]) and torch.equal(single, want["a"][1][1]), kept
        assert torch.equal(rc[1], want["a"][1]), kept


# ------------------------------------------------- 6. arguments

def test_arguments(R, torch_cuda):
    torch = torch_cuda
    L = rm.lib()
    W, H, n = 8, 8, 2
    buf = torch.full((8, H, W), SENTINEL, dtype=torch.int32, device="cuda")  # in: views 0-1, mid: 3-4, out: 6-7
    before = buf.clone()
    px = W * H * 4
    base = buf.data_ptr()
    i, m, o = base, base + 3 * px, base + 6 * px
    vp = lambda a: ctypes.c_void_p(a) if a else None  # noqa: E731

    def chain(W=W, H=H, n=n, s=0, t=0, i=i, m=m, o=o):
        return L.rm_post_chain_batch(R._ctx, W, H, n, s, t, vp(i), vp(m), vp(o))

    def frag(W=W, H=H, n=n, s=0, t=0, i=i, o=o):
        return L.rm_post_frag_batch(R._ctx, W, H, n, s, t, vp(i), vp(o))

    def bloom(W=W, H=H, n=n, i=i, o=o):
        return L.rm_bloom_batch(R._ctx, W, H, n, vp(i), vp(o))

    # overlapping ranges: mid inside in, out == in + W * H, and equal buffers
    assert chain(m=i + px) == INVALID and chain(o=i + px) == INVALID and chain(o=m + px) == INVALID
    assert chain(m=i) == INVALID and frag(o=i + px) == INVALID and bloom(o=i + px) == INVALID and bloom(o=i) == INVALID
    assert "overlap" in L.rm_last_error(R._ctx).decode()
    # NULL pointers
    assert chain(i=0) == INVALID and chain(m=0) == INVALID and chain(o=0) == INVALID
    assert frag(i=0) == INVALID and frag(o=0) == INVALID and bloom(i=0) == INVALID and bloom(o=0) == INVALID
    # enum values out of range
    for s, t in [(-1, 0), (3, 0), (0, -1), (0, 5)]:
        assert chain(s=s, t=t) == INVALID and frag(s=s, t=t) == INVALID, (s, t)
    # the size rule, before any pointer is used (junk pointers here)
    junk = 16
    for Wb, Hb, nb in [(0, 8, 2), (8, 0, 2), (-1, 8, 2), (8, 8, -1), (8, 8, 65536), (1 << 10, 1 << 10, (1 << 11) + 1),
                       (1 << 15, 1 << 15, 1), (1 << 30, 1, 0)]:
        assert chain(W=Wb, H=Hb, n=nb, i=junk, m=junk + 4, o=junk + 8) == INVALID, (Wb, Hb, nb)
        assert frag(W=Wb, H=Hb, n=nb, i=junk, o=junk + 4) == INVALID and bloom(W=Wb, H=Hb, n=nb, i=junk, o=junk + 4) == INVALID
    # host pointers
    host = np.zeros((n, H, W), np.uint32)
    assert chain(i=host.ctypes.data) == INVALID and bloom(o=host.ctypes.data) == INVALID
    assert L.rm_set_post_batch_scratch_limit(R._ctx, -1) == INVALID
    torch.cuda.synchronize()
    assert torch.equal(buf, before)
    # ... and the same buffers are accepted
    assert chain() == 0 and frag() == 0 and bloom() == 0
    torch.cuda.synchronize()
    assert torch.equal(buf[2], before[2]) and torch.equal(buf[5], before[5]) and not torch.equal(buf[6:], before[6:])


# ------------------------------------------------- 7. the headless app

def _ppm_rgb(path, W, H):
    data = path.read_bytes()
    return np.frombuffer(data[data.index(b"255\n") + 4:], np.uint8).reshape(H, W, 3)


@pytest.mark.parametrize("aa", [False, True], ids=["plain", "aa"])
def test_headless_app_writes_the_post_frames(R, torch_cuda, tmp_path, aa):
    """apps/raymarch_headless --views F --post [--aa 4:32] (rm::PostShader::drawChainBatch): three PPMs that equal
    a per-view post_chain of the batch's frames, and "post": true in the JSON line."""
    W, H = 48, 32
    exe = os.path.join(ROOT, "apps", "raymarch_headless")
    views = [POSES["P0"], POSES["P1"], POSES["P2"]]
    lines = ["# px py pz mx my t"]
    for row in rm.pack_views(views):
        lines.append(" ".join(repr(float(x)) for x in row[:6]))  # (repr of a float32's double: reads back exactly)
    (tmp_path / "views.txt").write_text("\n".join(lines) + "\n")
    cmd = [exe, "--scene", "template.frag", "--w", str(W), "--h", str(H), "--steps", str(STEPS), "--views",
           str(tmp_path / "views.txt"), "--post", "--post-sample", "chromatic", "--tonemap", "reinhard", "--ppm",
           str(tmp_path / "v")] + (["--aa", "4:32"] if aa else [])
    run = subprocess.run(cmd, capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stderr
    info = json.loads(run.stdout.strip().splitlines()[-1])
    assert info["views"] == 3 and info["post"] is True and (info["aa"] == 4 if aa else "aa" not in info)
    R.load_scene(rm.SCENE_FILES["T"])
    R.set_params(max_steps=STEPS, shadow_max_steps=0, count_evals=0)
    R.set_uniform("u_seed1", 0.5, 0.5)
    R.set_uniform("u_sample_part", 1.0)
    frames = R.render_batch_aa(W, H, views, samples=4, threshold=32) if aa else R.render_batch(W, H, views)
    for k in range(3):
        want = R.post_chain(frames[k], sample="chromatic", tonemap="reinhard")[1].cpu().numpy().view(np.uint32)
        rgb = np.stack([(want >> s) & 255 for s in (0, 8, 16)], -1).astype(np.uint8)
        assert np.array_equal(_ppm_rgb(tmp_path / f"v.{k:04d}.ppm", W, H), rgb), k
        raw = frames[k].cpu().numpy().view(np.uint32)
        assert not np.array_equal(rgb, np.stack([(raw >> s) & 255 for s in (0, 8, 16)], -1).astype(np.uint8))
