"""The context's scratch buffers across streams, where the existing stream tests
leave a path open: a scratch that has to GROW on a second stream while its use
on the first is still queued (rm_ctx_streams.cpp scratch_acquire: the wait for
the event recorded when the context left the first stream, then the free and
the larger allocation).  One case per scratch -- the supersampling queue, the
view-batch records, the batch supersampling scratch and bloom's buffer -- each
on a fresh renderer, whose scratch starts empty, at the smallest sizes that
still make it grow.  Every result must equal what the helpers of the respective
test files give for the same inputs on a quiet default stream (another
renderer's: computing them must not size the scratch under test)."""
import numpy as np
import pytest

import raymarching_amd as rm
import test_aa_gpu as aa_t
import test_batch_aa_gpu as baa_t
import test_batch_gpu as batch_t
import test_post_batch_gpu as post_t
from raymarching_amd import POSES

pytestmark = pytest.mark.gpu

SMALL, LARGE = (24, 16), (61, 37)
NAMES = ("P0", "P1", "P2", "P7")


@pytest.fixture(scope="module")
def R(torch_cuda):
    """the quiet renderer: the references, on the default stream"""
    r = rm.Renderer(0)
    yield r
    r.close()


@pytest.fixture
def fresh(torch_cuda):
    """the renderer under test: no scratch yet"""
    r = rm.Renderer(0)
    yield r
    r.set_stream(None)
    r.close()


def test_supersampling_queue_grows_on_a_second_stream(R, fresh, torch_cuda):
    torch = torch_cuda
    K, pose = 4, POSES["P2"]
    want = {}
    for W, H in (SMALL, LARGE):
        aa_t._setup(R, "T", pose, 128)
        want[(W, H)] = aa_t._supersampled(torch, R, "T", W, H, "P2", pose, 128, K)
    aa_t._setup(fresh, "T", pose, 128)
    torch.cuda.synchronize()
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    fresh.set_stream(s1)
    first = fresh.render_aa(*SMALL, samples=K, threshold=0)
    fresh.set_stream(s2)
    grown = fresh.render_aa(*LARGE, samples=K, threshold=0)  # (the queue of 24 x 16 words does not hold 61 x 37)
    fresh.set_stream(s1)
    again = fresh.render_aa(*SMALL, samples=K, threshold=0)
    torch.cuda.synchronize()
    assert np.array_equal(aa_t._words(first), want[SMALL])
    assert np.array_equal(aa_t._words(grown), want[LARGE])
    assert np.array_equal(aa_t._words(again), want[SMALL])


def test_batch_records_grow_on_a_second_stream(R, fresh, torch_cuda):
    torch = torch_cuda
    W, H = LARGE
    views = [POSES[k] for k in NAMES]
    batch_t._setup(R, "T")
    want = batch_t._singles(R, W, H, views)
    batch_t._setup(fresh, "T")
    torch.cuda.synchronize()
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    fresh.set_stream(s1)
    first = fresh.render_batch(W, H, views[:1])
    fresh.set_stream(s2)
    grown = fresh.render_batch(W, H, views)  # (one record's buffer does not hold four)
    fresh.set_stream(s1)
    again = fresh.render_batch(W, H, views[3:])
    torch.cuda.synchronize()
    assert batch_t._same(batch_t._np(first), want[:1])
    assert batch_t._same(batch_t._np(grown), want)
    assert batch_t._same(batch_t._np(again), want[3:])


def test_batch_supersampling_scratch_grows_on_a_second_stream(R, fresh, torch_cuda):
    torch = torch_cuda
    K, threshold = 4, 32
    views = [POSES[k] for k in NAMES[:3]]
    baa_t._setup(R, "T")
    want1 = baa_t._loop(R, ("T", NAMES[:1]), *SMALL, views[:1], K, threshold)
    want3 = baa_t._loop(R, ("T", NAMES[:3]), *LARGE, views, K, threshold)
    assert rm.batch_aa_scratch_bytes(*LARGE, 3) > rm.batch_aa_scratch_bytes(*SMALL, 1)
    baa_t._setup(fresh, "T")
    torch.cuda.synchronize()
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    fresh.set_stream(s1)
    first = fresh.render_batch_aa(*SMALL, views[:1], samples=K, threshold=threshold, mask=True, refined=True)
    fresh.set_stream(s2)
    grown = fresh.render_batch_aa(*LARGE, views, samples=K, threshold=threshold, mask=True, refined=True)
    torch.cuda.synchronize()
    for (out, mask, refined), (frames, masks, counts) in ((first, want1), (grown, want3)):
        assert baa_t._same(baa_t._np(out), frames) and baa_t._same(mask.cpu().numpy(), masks)
        assert np.array_equal(baa_t._np(refined).astype(np.int64), counts)


@pytest.mark.parametrize("kept", [False, True], ids=["left", "kept"])
def test_bloom_scratch_grows_on_a_second_stream(R, fresh, torch_cuda, kept):
    torch = torch_cuda
    W, H, n = 64, 64, 4
    frames = post_t._dev(torch, post_t._frames(W, H, n, 11))
    want_bloom = R.bloom(frames[0])
    want = [R.post_chain(frames[v]) for v in range(n)]  # (mid, out) per frame
    plan = rm.post_batch_plan(W, H, n)
    assert plan["groups"] == 1 and plan["scratch_bytes"] > plan["shared_bytes"] > 0  # the batch asks for more
    torch.cuda.synchronize()
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    fresh.set_stream(s1, kept=kept)
    first = fresh.bloom(frames[0])
    fresh.set_stream(s2, kept=kept)
    mid, out = fresh.post_chain_batch(frames)
    fresh.set_stream(s1, kept=kept)
    again = fresh.bloom(frames[0])
    # ... and in two groups, which share the views' part of the buffer one after the other
    two = plan["shared_bytes"] + 2 * plan["per_view_bytes"]
    assert rm.post_batch_plan(W, H, n, two)["groups"] == 2
    fresh.set_post_batch_scratch_limit(two)
    fresh.set_stream(s2, kept=kept)
    mid2, out2 = fresh.post_chain_batch(frames)
    torch.cuda.synchronize()
    assert torch.equal(first, want_bloom) and torch.equal(again, want_bloom)
    for v in range(n):
        assert torch.equal(mid[v], want[v][0]) and torch.equal(out[v], want[v][1]), v
        assert torch.equal(mid2[v], want[v][0]) and torch.equal(out2[v], want[v][1]), ("two groups", v)
