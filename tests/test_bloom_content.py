"""Bloom on content its mip levels keep (CPU; the GPU half is
test_bloom_content_gpu.py, which holds rm_bloom to oracle.bloom on the same
images).

Uniform noise is flat at the levels bloom.frag reads, so on noise a wrong tap
cell or a late run boundary changes a few per cent of the channels by one LSB
and the 0.3 threshold never fires.  Here the restatement (oracle.bloom: run
tables, one polynomial per run pair) is held to the float64 per-tap definition
(bloom_ref.per_tap_bloom) on the block-aligned images of bloom_content.py, at
sizes where an axis exceeds 1024 pixels (the HIP scan's chunk > 1, ragged last
chunk), and one-line mutants of the definition must break the same rule on at
least one kind of content at every size.  The rest are conditions on the test
inputs themselves: that each kind of content does what it is there for, that
the run tables fit what bloom_plan allocates, and that the GPU sizes reach both
sides of the base texel's exact-zero fast path.
"""
import functools

import numpy as np
import pytest

import bloom_content as bc
import bloom_ref as br
import oracle
from bloom_content import FR0, GPU_SIZES, LOD_BELOW_1, LOW_FR, MAGNIFY, PYRAMID, RESAMPLE, TAILS

# restatement against definition: an axis above 1024 (chunk 2 and 3, ragged
# last chunk), lod barely above an integer, 0 < lod < 1 (d1 = the frame itself;
# 2049 x 48 has lod 1.26: d1 = 1), one exact-halving pyramid size
CPU_SIZES = [(1025, 333), (333, 1025), (2100, 1300), (70, 30), (2049, 48), (2049, 30), (128, 896)]

def ids(sizes):
    return [f"{w}x{h}" for w, h in sizes]


def seed(W, H):
    return W * 7919 + H


@functools.lru_cache(maxsize=2)
def images(W, H):
    """{kind: (image, oracle.bloom's output, its levels)} with "noise" added, and the subset (rows, cols)."""
    rng = np.random.default_rng(seed(W, H))
    out = {}
    for kind, gen in list(bc.KINDS.items()) + [("noise", bc.noise)]:
        img = gen(W, H, rng)
        out[kind] = (img,) + oracle.bloom(img)
    return out, br.subset(W, H, rng)


def compare(got, ref, rows, cols):
    """(largest difference, identical fraction) of the RGB bytes on rows x cols."""
    d = np.abs(br.channels(got[np.ix_(rows, cols)])[..., :3] - ref)
    return int(d.max()), float(np.mean(d == 0))


def within_rule(dmax, same):
    """The project's rule for the restated order (test_bloom.py): at most 1 LSB, >= 99.5 % identical."""
    return dmax <= 1 and same >= 0.995


def test_matrix_form_is_the_gather_form():
    """per_tap_bloom sums a tap row as one matrix product; tap by tap with gathers it is the same sum."""
    W, H = 96, 54
    img = bc.block(W, H, np.random.default_rng(1))
    _, levels = oracle.bloom(img)
    lod, d1, d2 = oracle.bloom_levels(W, H)
    fr = lod - np.floor(lod)
    lv = [br.channels(img)[..., :3] / 255.0] + [br.channels(m)[..., :3] / 255.0 for m in levels]
    u, v = (np.arange(W) + 0.5) / W, 1.0 - (np.arange(H) + 0.5) / H
    acc = 0.0
    for L, wgt in ((lv[d1], 1 - fr), (lv[d2], fr)):
        for j in range(-2, 3):
            for i in range(-2, 3):
                acc = acc + wgt * br.GAUSS[abs(i), abs(j)] * br.bilinear(L, u + i * (H / W) * 0.05, v + j * 0.05)
    assert np.abs(acc - br.blurred(img, levels)).max() < 1e-14
    rows, cols = np.array([0, 7, 53]), np.array([3, 95])
    assert np.array_equal(br.per_tap_bloom(img, levels, rows, cols), br.per_tap_bloom(img, levels)[np.ix_(rows, cols)])


@pytest.mark.parametrize("W,H", CPU_SIZES, ids=ids(CPU_SIZES))
def test_restatement_equals_definition(W, H):
    """oracle.bloom against the float64 per-tap definition over the oracle's
    own levels, on every kind of content: at most 1 LSB apart and identical on
    >= 99.5 % of the channels (above 0.5 M pixels on the rows and columns where
    a run starts, their predecessors, the edges and 300 random others).

    Measured minima of the identical fraction over these sizes (CPU, this
    commit; never more than 1 LSB apart): block 0.99993 (2049 x 30), block2
    0.99986 (2049 x 48), dark 0.99984, border 0.99968 and impulse 0.99984 (all
    70 x 30: 1 or 2 of 6300 channels), checker 0.99993 (128 x 896), flat0 and
    flat255 1.0."""
    data, (rows, cols) = images(W, H)
    ops = br.tap_operators(W, H, rows, cols)
    for kind in bc.KINDS:
        img, out, levels = data[kind]
        dmax, same = compare(out, br.per_tap_bloom(img, levels, rows, cols, ops=ops), rows, cols)
        print(f"{W}x{H} {kind}: max {dmax} LSB, identical {same:.5f} of {len(rows)}x{len(cols)} pixels")
        assert within_rule(dmax, same), (kind, dmax, same)
        assert np.all(out >> 24 == 255)


@pytest.mark.parametrize("mutant", list(br.MUTANTS))
@pytest.mark.parametrize("W,H", CPU_SIZES, ids=ids(CPU_SIZES))
def test_mutant_is_caught(W, H, mutant):
    """Each one-line error of the definition breaks the rule above against
    oracle.bloom on at least one kind of content at every size (on at most 400
    of the subset's rows and columns).  The printed line and the assertion
    message carry what it does on noise of the same size: where d1 >= 4 the
    errors confined to one tap or to level d2 move a few per cent of the noise
    channels, or fewer, by one LSB (tap_x at 128 x 896: 0.14 %, within the
    rule), and a third to a half of the block channels by several."""
    data, (rows, cols) = images(W, H)
    rng = np.random.default_rng(seed(W, H) + 1)
    rows, cols = (np.sort(rng.choice(a, 400, replace=False)) if len(a) > 400 else a for a in (rows, cols))
    ops = br.tap_operators(W, H, rows, cols, mutant)
    img, out, levels = data["noise"]
    nmax, nsame = compare(out, br.per_tap_bloom(img, levels, rows, cols, mutant, ops), rows, cols)
    seen = [f"noise: {1 - nsame:.4f} of the channels moved, by at most {nmax} LSB"
            f" ({'caught' if not within_rule(nmax, nsame) else 'not caught'})"]
    caught = []
    for kind in bc.KINDS:
        img, out, levels = data[kind]
        dmax, same = compare(out, br.per_tap_bloom(img, levels, rows, cols, mutant, ops), rows, cols)
        seen.append(f"{kind}: {1 - same:.4f}, {dmax} LSB")
        if not within_rule(dmax, same):
            caught.append(kind)
    print(f"{W}x{H} {mutant} ({br.MUTANTS[mutant]}): " + "; ".join(seen))
    assert caught, f"{mutant} survives every kind of content at {W}x{H}: " + "; ".join(seen)


# ------------------------------------------------ the content does what it claims


@pytest.mark.parametrize("W,H", CPU_SIZES + PYRAMID[:4], ids=ids(CPU_SIZES + PYRAMID[:4]))
def test_dark_straddles_the_threshold(W, H):
    rng = np.random.default_rng(seed(W, H))
    img = bc.dark(W, H, rng)
    rows, cols = br.subset(W, H, rng)
    bl = br.blurred(img, oracle.bloom(img)[1], rows, cols)
    below = float(np.mean(bl < 0.3))
    assert 0.2 <= below <= 0.8, below


@pytest.mark.parametrize("kind", ["block", "block2"])
@pytest.mark.parametrize("W,H", CPU_SIZES + PYRAMID[:4], ids=ids(CPU_SIZES + PYRAMID[:4]))
def test_block_content_saturates_in_part(W, H, kind):
    img = bc.KINDS[kind](W, H, np.random.default_rng(seed(W, H)))
    rgb = br.channels(oracle.bloom(img)[0])[..., :3]
    sat = float(np.mean(rgb == 255))
    assert 0.1 <= sat <= 0.9, sat


@pytest.mark.parametrize("W,H", PYRAMID, ids=ids(PYRAMID))
def test_checker_rounds_exact_ties(W, H):
    """Where every level is an exact halving a texel is the mean of four,
    rounded half to even: a tie when their sum = 2 (mod 4).  The checker has
    ties at level 1 (the dark cells: half of the texels) and at level d2 (every
    texel); the levels between average equal texels."""
    img = bc.checker(W, H, np.random.default_rng(seed(W, H)))
    _, d1, d2 = oracle.bloom_levels(W, H)
    levels = [img] + oracle.bloom(img)[1]
    for k, share in ((1, 0.4), (d2, 1.0)):
        c = br.channels(levels[k - 1])[..., :3]
        s = c[0::2, 0::2] + c[0::2, 1::2] + c[1::2, 0::2] + c[1::2, 1::2]
        assert np.mean(s % 4 == 2) >= share, (k, float(np.mean(s % 4 == 2)))
        assert np.array_equal(br.channels(levels[k])[..., :3], np.rint(s / 4.0).astype(np.int64))  # half to even
    assert set(np.unique(br.channels(levels[d1])[..., :3])) == {0, 255}  # full contrast at d1


def test_fr_of_the_gpu_sizes():
    """Level d2 carries weight at every GPU size with lod > 0 (fr within 0.25
    .. 0.75), except the sizes kept because they have fr = 0 exactly and the
    two resample sizes with lod just above an integer."""
    for W, H in GPU_SIZES:
        lod, d1, d2 = oracle.bloom_levels(W, H)
        fr = lod - np.floor(lod)
        if (W, H) in MAGNIFY:
            assert lod <= 0
        elif (W, H) in FR0:
            assert fr == 0 and lod > 0
        elif (W, H) in LOW_FR:
            assert 0 < fr < 0.1
        else:
            assert 0.25 <= fr <= 0.75, (W, H, fr)
    for W, H in LOD_BELOW_1[:1] + LOD_BELOW_1[2:]:
        assert 0 < oracle.bloom_levels(W, H)[0] < 1
    for H in (h for _, h in TAILS):
        assert H % 16 in (1, 5, 15)


def test_pyramid_plan_of_the_gpu_sizes():
    """launch_bloom's choice, restated: the pyramid when W and H are multiples
    of 2^d2 and d2 >= 5, started at level s0 = max(d2 - 8, 0) with
    2^(d2 - s0 - 5)-texel blocks per lane."""
    def plan(W, H):
        lod, d1, d2 = oracle.bloom_levels(W, H)
        s0 = max(d2 - 8, 0)
        if not (lod > 0 and d2 - s0 >= 5 and W % (1 << d2) == 0 and H % (1 << d2) == 0):
            return None
        return s0, d2 - s0 - 5
    assert [plan(W, H) for W, H in PYRAMID] == [(0, 0), (0, 1), (0, 2), (0, 3), (1, 3), (2, 3)]
    assert [plan(W, H) for W, H in FR0] == [(0, 1), (0, 3)]
    assert all(plan(W, H) is None for W, H in RESAMPLE + TAILS + LOD_BELOW_1 + MAGNIFY)


# ------------------------------------------------ run tables


def sweep_sizes():
    rng = np.random.default_rng(2)
    small = [(int(w), int(h)) for w, h in zip(rng.integers(1, 128, 2500), rng.integers(21, 128, 2500))]  # lod > 0: H > 20
    grid = [(w, h) for w in range(21, 128, 9) for h in range(21, 128, 7)]
    strided = [(w, h) for w in range(128, 8193, 733) for h in range(128, 8193, 877)]
    thin = [(1, 256), (256, 1), (8, 2048), (2048, 8), (32, 8192), (8192, 32), (21, 5376), (5376, 21)]
    return small + grid + strided + thin + GPU_SIZES + CPU_SIZES


def test_run_tables_fit_and_keys_are_monotone():
    """Along each of the four axes the cell tuples are monotone cell by cell
    (so neighbours with equal keys -- the sum of the five cells -- have equal
    tuples, which is what the scan compares), and there are at most
    min(n, 5 lw + 1) distinct ones, the room bloom_plan gives a run table."""
    sizes = [s for s in sweep_sizes() if oracle.bloom_levels(*s)[0] > 0]
    assert len(sizes) > 2000
    for W, H in sizes:
        for A in br.axes(W, H):
            cells = A["cells"]
            step = np.diff(cells, axis=0) * (-1 if A["is_y"] else 1)
            assert step.min(initial=0) >= 0, (W, H, A["is_y"], A["lw"])
            key = (cells + 1).sum(1) * (-1 if A["is_y"] else 1)
            assert np.all(np.diff(key) >= 0)
            nruns = len(br.run_starts(cells))
            assert nruns == 1 + np.count_nonzero(np.diff(key)), (W, H)  # equal keys <=> equal tuples
            assert nruns <= min(A["N"], 5 * A["lw"] + 1), (W, H, A["is_y"], nruns, A["lw"])
            assert cells.min() >= -1 and cells.max() <= A["lw"] - 1


# ------------------------------------------------ the base texel's fast path


def test_gpu_sizes_reach_both_sides_of_the_base_fast_path():
    """rm_bloom_min_kernel reads the pixel's own texel without filtering when
    the base weights of a whole wave (64 columns) and 4-row batch are exactly 0
    in float32.  The GPU sizes have waves and batches of both kinds: all of
    W = 256 and 512, and 63 columns of W = 1100 with a non-zero weight."""
    def waves(W):
        f = br.base_weights(W, 0)
        return [bool(np.all(f[k:k + 64] == 0)) for k in range(0, W, 64)]

    def batches(H):
        f = br.base_weights(H, 1)
        return [bool(np.all(f[yb:min(yb + 4, y0 + 16, H)] == 0)) for y0 in range(0, H, 16)
                for yb in range(y0, min(y0 + 16, H), 4)]

    for W, H in [(256, 1792), (512, 7168)]:  # every wave exact; batches of both kinds
        assert all(waves(W)) and any(batches(H)) and not all(batches(H))
    assert int(np.count_nonzero(br.base_weights(1100, 0))) == 63
    assert int(np.count_nonzero(br.base_weights(1100, 1))) == 452
    for H in (449, 453, 463):  # W = 1100: waves of both kinds against batches of both kinds
        assert any(waves(1100)) and not all(waves(1100)) and any(batches(H)) and not all(batches(H))
