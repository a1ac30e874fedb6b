"""Adaptive supersampling of a view batch of any scene, a scene plugin included,
with the scene's own uniforms set per view (include/rm.h
rm_render_batch_aa_ex_rgba8, rm_refine_batch_ex_rgba8, rm_batch_aa_prepare,
rm_compile_scene_batch_aa).

These are functions of a module of their own, taking the Renderer first, and not
methods of Renderer: the public surface of api.py is pinned by a committed
listing (tests/api_surface.json), and folding them into Renderer waits for a
change that regenerates that listing on purpose.

    from raymarching_amd import batch_aa_ex
    frames = batch_aa_ex.render_batch_aa_ex(r, 256, 256, views, {"u_ball": balls}, samples=4)
"""
from __future__ import annotations

from ._lib import check, lib
from .api import _compile, pack_views


def _call(renderer, entry, what, W, H, v, uniforms, samples, threshold, frames8, mask, refined, stats):
    """Renderer._batch_aa around the _ex entry point: the uniform list goes between the views and the params"""
    arr, n_entries, _keep = renderer._view_uniforms(what, uniforms, len(v))

    def fn(ctx, w, h, views, n, params, frames, m, r, s):
        return entry(ctx, w, h, views, n, arr, n_entries, params, frames, m, r, s)

    return renderer._batch_aa(fn, W, H, v, samples, threshold, frames8, mask, refined, stats)


def render_batch_aa_ex(renderer, W: int, H: int, views, uniforms=None, samples=4, threshold=32, out=None,
                       mask=False, refined=False, stats=False):
    """Renderer.render_batch_aa for any scene, a scene plugin included, with the
    scene's own uniforms set per view.  View v's frame, mask and count are byte
    for byte what set_pose + set_uniform of view v's values + render_aa_ex
    gives with the same samples and threshold; an unlisted uniform has the
    renderer's current value, and the renderer's own pose and uniform values
    are neither read nor changed.  uniforms: the dict render_batch_ex takes.
    views, out, mask, refined, stats and the results: as render_batch_aa's.  A
    plugin's batch and batch-refine kernels are compiled on the first call
    after load_scene (batch_aa_prepare compiles them ahead).  For a built-in
    scene: render_batch_aa, and a non-empty `uniforms` raises."""
    v = pack_views(views)
    return _call(renderer, lib().rm_render_batch_aa_ex_rgba8, "render_batch_aa_ex", W, H, v, uniforms, samples,
                 threshold, renderer._out(out, (len(v), H, W)), mask, refined, stats)


def refine_batch_ex(renderer, frames8, views, uniforms=None, samples=4, threshold=32, mask=False, refined=False,
                    stats=False):
    """rm_refine_batch_ex_rgba8: the supersampling step of render_batch_aa_ex on
    any [n, H, W] RGBA8 frames of the views (normally render_batch_ex's), in
    place; returns as render_batch_aa_ex does."""
    n, H, W = frames8.shape
    v = pack_views(views)
    if n != len(v):
        raise ValueError(f"refine_batch_ex: {n} frames for {len(v)} views")
    return _call(renderer, lib().rm_refine_batch_ex_rgba8, "refine_batch_ex", W, H, v, uniforms, samples, threshold,
                 frames8, mask, refined, stats)


def batch_aa_prepare(renderer) -> None:
    """rm_batch_aa_prepare: compile and load the loaded plugin's batch and
    batch-refine kernels now, not inside the first render_batch_aa_ex (nothing
    to do for a built-in scene or once they are loaded)."""
    check(lib().rm_batch_aa_prepare(renderer._ctx), renderer._ctx)


def compile_scene_batch_aa(file_name: str):
    """rm_compile_scene_batch_aa: compile_scene for the batch-refine form of a
    plugin's code object (no GPU needed) -> (ok, log)."""
    return _compile(lib().rm_compile_scene_batch_aa, file_name)
