"""Host-side mirror of the reference's shader-pass surface, over librm.so.

The reference drives its ray-march pass through SFML (main.cpp:52-54,187-207):

    sf::Shader shader;
    ShaderLoader::loadFromFile("output_shader.frag", sf::Shader::Fragment, shader);
    shader.setUniform("u_resolution", sf::Vector2f(wf, hf));
    ...
    shader.setUniform("u_pos", pos); shader.setUniform("u_mouse", ...);
    shader.setUniform("u_time", t);
    outputTexture.draw(firstTextureSpriteFlipped, &shader);

The same names, argument meaning and error behaviour exist here:
``ShaderLoader.loadFromFile(file, Shader.Fragment, shader) -> bool`` (prints
and returns False on failure, source/shader_loader.cpp:26-30),
``Shader.setUniform(name, value)`` and ``RenderTexture.draw(shader)``, whose
target is a W x H x 4 float32 tensor resident in HBM.  ``Renderer`` is the
lower-level handle (one librm context) used by bench.py and the tests.
"""
from __future__ import annotations

import ctypes
import math
import sys

from . import _lib
from ._lib import RmParams, RmStats, check, lib


def _torch():
    import torch  # noqa: PLC0415  (torch provides device memory and streams only)
    return torch


class Renderer:
    """One librm context on one HIP device."""

    def __init__(self, device: int = 0):
        L = lib()
        self._ctx = ctypes.c_void_p()
        st = L.rm_create(ctypes.byref(self._ctx), int(device))
        if st != 0:
            raise _lib.RmError(st, f"rm_create(device={device}) failed")
        self.device = int(device)
        self._uniform_types = {}  # of the loaded scene's own uniforms: name -> "float" | "int" | "bool"

    def close(self):
        if self._ctx:
            lib().rm_destroy(self._ctx)
            self._ctx = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:  # interpreter shutdown
            pass

    # --- state ---------------------------------------------------------
    def load_scene(self, name: str) -> None:
        check(lib().rm_load_scene(self._ctx, name.encode()), self._ctx)
        self._uniform_types = {u.name.decode(): _lib.UNIFORM_TYPES[u.type] for u in self._uniform_infos()}

    def set_uniform(self, name: str, *v) -> None:
        """rm_set_uniform{1,2,3,4}f; a uniform the loaded scene declares as
        int or bool goes through rm_set_uniform1i."""
        L = lib()
        n = name.encode()
        if len(v) == 1 and self._uniform_types.get(name) in ("int", "bool"):
            st = L.rm_set_uniform1i(self._ctx, n, int(v[0]))
        elif len(v) == 1:
            st = L.rm_set_uniform1f(self._ctx, n, float(v[0]))
        elif len(v) == 2:
            st = L.rm_set_uniform2f(self._ctx, n, float(v[0]), float(v[1]))
        elif len(v) == 3:
            st = L.rm_set_uniform3f(self._ctx, n, float(v[0]), float(v[1]), float(v[2]))
        elif len(v) == 4:
            st = L.rm_set_uniform4f(self._ctx, n, float(v[0]), float(v[1]), float(v[2]), float(v[3]))
        else:
            raise ValueError("uniforms have 1..4 components")
        check(st, self._ctx)

    def set_uniform_array(self, name: str, array) -> None:
        """rm_set_uniformfv: elements [0, len(array)) of an array uniform from a
        [count] (float elements) or [count, components] array."""
        import numpy as np
        a = np.ascontiguousarray(array, np.float32)
        if a.ndim == 1:
            a = a.reshape(-1, 1)
        if a.ndim != 2 or a.shape[0] < 1 or not 1 <= a.shape[1] <= 4:
            raise ValueError("set_uniform_array: a [count] or [count, 1..4] array of floats")
        check(lib().rm_set_uniformfv(self._ctx, name.encode(), int(a.shape[1]), ctypes.c_void_p(a.ctypes.data),
                                     int(a.shape[0])), self._ctx)

    def _uniform_infos(self):
        n = ctypes.c_int()
        check(lib().rm_uniform_count(self._ctx, ctypes.byref(n)), self._ctx)
        infos = []
        for i in range(n.value):
            u = _lib.RmUniformInfo()
            check(lib().rm_uniform_info_at(self._ctx, i, ctypes.byref(u)), self._ctx)
            infos.append(u)
        return infos

    def uniforms(self) -> dict:
        """The uniforms the loaded scene declares, in declaration order:
        {name: dict(type, components, count, value)} with type "float", "int"
        or "bool", count 0 for a non-array, and value a float / int / bool, a
        tuple of floats (vec2..vec4), or a [count, components] float32 array
        ([count] for an array of floats)."""
        import numpy as np
        out = {}
        for u in self._uniform_infos():
            name, ty = u.name.decode(), _lib.UNIFORM_TYPES[u.type]
            if ty == "float":
                v = np.zeros(u.components * max(1, u.count), np.float32)
                check(lib().rm_get_uniformfv(self._ctx, u.name, ctypes.c_void_p(v.ctypes.data), len(v), None),
                      self._ctx)
                if u.count:
                    value = v.reshape(u.count, u.components) if u.components > 1 else v
                else:
                    value = float(v[0]) if u.components == 1 else tuple(float(x) for x in v)
            else:
                i = ctypes.c_int32()
                check(lib().rm_get_uniform1i(self._ctx, u.name, ctypes.byref(i)), self._ctx)
                value = bool(i.value) if ty == "bool" else int(i.value)
            out[name] = dict(type=ty, components=int(u.components), count=int(u.count), value=value)
        return out

    def set_pose(self, pos, mouse, time) -> None:
        self.set_uniform("u_pos", *pos)
        self.set_uniform("u_mouse", *mouse)
        self.set_uniform("u_time", time)

    def set_params(self, max_steps=None, shadow_max_steps=None, count_evals=None, kernel=None,
                   schedule=None) -> None:
        p = self.params()
        if schedule is not None:
            p.schedule = _lib.named(schedule, _lib.SCHEDULES, "schedule")
        if max_steps is not None:
            p.max_steps = int(max_steps)
        if shadow_max_steps is not None:
            p.shadow_max_steps = int(shadow_max_steps)
        if count_evals is not None:
            p.count_evals = int(bool(count_evals))
        if kernel is not None:
            p.kernel = _lib.named(kernel, _lib.KERNELS, "kernel")
        check(lib().rm_set_params(self._ctx, ctypes.byref(p)), self._ctx)

    def params(self) -> RmParams:
        p = RmParams()
        check(lib().rm_get_params(self._ctx, ctypes.byref(p)), self._ctx)
        return p

    def set_stream(self, stream, kept: bool = False) -> None:
        """stream: a torch.cuda.Stream, a raw hipStream_t int, or None.  kept:
        the stream outlives this renderer (rm_set_stream_kept; PyTorch's pool
        streams are never destroyed), so leaving it records no marker."""
        raw = getattr(stream, "cuda_stream", stream)
        fn = lib().rm_set_stream_kept if kept else lib().rm_set_stream
        check(fn(self._ctx, ctypes.c_void_p(raw or 0)), self._ctx)

    def tile_grid(self, W: int, rows: int) -> tuple:
        """(tiles_x, tiles_y) of a render launch over W x rows pixels."""
        tx, ty = ctypes.c_int(), ctypes.c_int()
        p = self.params()
        check(lib().rm_tile_grid(ctypes.byref(p), int(W), int(rows), ctypes.byref(tx), ctypes.byref(ty)))
        return tx.value, ty.value

    def set_tile_order(self, order=None) -> None:
        """rm_set_tile_order: workgroup i renders tile order[i] (None clears)."""
        import numpy as np
        if order is None:
            check(lib().rm_set_tile_order(self._ctx, None, 0), self._ctx)
            return
        o = np.ascontiguousarray(order, np.uint32)
        check(lib().rm_set_tile_order(self._ctx, ctypes.c_void_p(o.ctypes.data), len(o)), self._ctx)

    def synchronize(self) -> None:
        check(lib().rm_synchronize(self._ctx), self._ctx)

    def resolution_cache(self) -> tuple:
        """rm_resolution_cache_info: (entries, capacity) of the context's
        per-resolution cache of scenes S0/T's camera reciprocals."""
        n, cap = ctypes.c_int(), ctypes.c_int()
        check(lib().rm_resolution_cache_info(self._ctx, ctypes.byref(n), ctypes.byref(cap)), self._ctx)
        return n.value, cap.value

    # --- passes ----------------------------------------------------------
    @staticmethod
    def _ptr(t):
        if t is None:
            return None
        return ctypes.c_void_p(t.data_ptr()) if hasattr(t, "data_ptr") else ctypes.c_void_p(t.ctypes.data)

    def _steps(self, fn) -> int:
        n = ctypes.c_uint64(0)
        check(fn(self._ctx, ctypes.byref(n)), self._ctx)
        return int(n.value)

    def certified_steps(self) -> int:
        """rm_certified_steps: of the last counted render's evals, the soft-shadow
        ray-steps scene T's certificate proves away; 0 elsewhere."""
        return self._steps(lib().rm_certified_steps)

    def reflection_cleared_steps(self) -> int:
        """rm_reflection_cleared_steps: of the last counted render's evals, the reflection-march
        ray-steps scene T's reflection certificate proves away; 0 elsewhere."""
        return self._steps(lib().rm_reflection_cleared_steps)

    def near_sky_steps(self) -> int:
        """rm_near_sky_steps: of the last counted render's evals, the primary- and reflection-march ray-steps of
        scene T's waves that the near-sky ladder lets skip both marches; 0 elsewhere."""
        return self._steps(lib().rm_near_sky_steps)

    def _stats(self, s) -> dict:
        """rm_stats as a dict, with `certified` (rm_certified_steps of the same call), `reflection_cleared`
        (rm_reflection_cleared_steps) and `near_sky` (rm_near_sky_steps): every stats dict
        made from an rm_stats carries the key (render_aa's is an rm_aa_stats: other members, no ray-step counts)"""
        return dict(s.as_dict(), certified=self.certified_steps(), reflection_cleared=self.reflection_cleared_steps(),
                    near_sky=self.near_sky_steps())

    def _out(self, out, shape, dtype="int32", like=None):
        """The caller's buffer after _check_out for `shape` 32-bit elements, or,
        for None, a new tensor of that shape and dtype (a torch dtype or its
        name; int32: RGBA8 words) on this renderer's device -- where `like`
        lives, if given."""
        if out is not None:
            _check_out(out, math.prod(shape))
            return out
        torch = _torch()
        return torch.empty(shape, dtype=getattr(torch, dtype) if isinstance(dtype, str) else dtype,
                           device=f"cuda:{self.device}" if like is None else like.device)

    def _like(self, src, *targets):
        """src, an RGBA8 frame or batch of frames, checked; every target
        checked, or allocated like src where it is None -> the targets."""
        _check_out(src, src.numel())
        return [self._out(t, src.shape, src.dtype, like=src) for t in targets]

    def _call(self, fn, out, stats, *args, handle=None):
        """fn(ctx (or handle), *args, an rm_stats or NULL), checked -> out, or
        (out, the stats dict) with stats=True."""
        if not stats:
            check(fn(handle or self._ctx, *args, None), self._ctx)
            return out
        s = RmStats()
        check(fn(handle or self._ctx, *args, ctypes.byref(s)), self._ctx)
        return out, self._stats(s)

    def _render(self, entry, rgba8, dims, out, stats, *args):
        """One render entry point in its float form or, with rgba8, its RGBA8
        form (entry + "_rgba8"), into `dims` pixels: entry(ctx, *args, out, stats)."""
        if rgba8:
            out, fn = self._out(out, dims), getattr(lib(), entry + "_rgba8")
        else:
            out, fn = self._out(out, dims + (4,), "float32"), getattr(lib(), entry)
        return self._call(fn, out, stats, *args, self._ptr(out))

    def render(self, W: int, H: int, out=None, stats: bool = False):
        """Full frame into `out` (device tensor [H,W,4] f32; allocated if None)."""
        return self._render("rm_render", False, (H, W), out, stats, int(W), int(H))

    def render_accumulate(self, W: int, H: int, accum, stats: bool = False):
        """Progressive accumulation (rm_render_accumulate[_rgba8]): `accum` holds
        the previous frame (u_sample) and receives mix(u_sample, colour,
        u_sample_part), the colour rendered with the sub-pixel offset
        fract(u_seed1) - 0.5.  float32 [H, W, 4] or RGBA8 int32 [H, W] words."""
        torch = _torch()
        rgba8 = accum.dtype == torch.int32
        if not rgba8 and accum.dtype != torch.float32:
            raise ValueError("render_accumulate: accum must be float32 [H, W, 4] or int32 RGBA8 words [H, W]")
        return self._render("rm_render_accumulate", rgba8, (H, W), accum, stats, int(W), int(H))

    def render_step_map(self, W: int, H: int, out=None, evals_map=None):
        """Full frame plus the per-pixel sceneSDF call counts: (float32 [H, W, 4],
        int32 [H, W], stats), device tensors (allocated if None)."""
        out = self._out(out, (H, W, 4), "float32")
        evals_map = self._out(evals_map, (H, W))
        s = RmStats()
        check(lib().rm_render_step_map(self._ctx, int(W), int(H), self._ptr(out), self._ptr(evals_map),
                                       ctypes.byref(s)), self._ctx)
        return out, evals_map, self._stats(s)

    def render_band(self, W: int, H: int, band: int, nshards: int, shard: int, out=None, stats: bool = False):
        """Rows y with (y // band) % nshards == shard, packed in increasing y."""
        return self._render("rm_render_band", False, (shard_rows(H, band, nshards, shard), W), out, stats,
                            int(W), int(H), int(band), int(nshards), int(shard))

    def render_rows(self, W, H, band, nshards, shard, row_begin, row_count, out, stats=False):
        """Packed rows [row_begin, row_begin + row_count) of a shard into `out`
        (float32 [rows, W, 4], or int32 [rows, W] RGBA8 words: the kernel packs)."""
        return self._render("rm_render_rows", out.dtype != _torch().float32, (row_count, W), out, stats, int(W), int(H),
                            int(band), int(nshards), int(shard), int(row_begin), int(row_count))

    def render_cycle_rows(self, W, H, cycle, offset, run, row_begin, row_count, out, stats=False):
        """Packed rows [row_begin, row_begin + row_count) of the cyclic part
        (y mod cycle) - offset in [0, run), as render_rows (float32 or RGBA8 out)."""
        return self._render("rm_render_cycle_rows", out.dtype != _torch().float32, (row_count, W), out, stats, int(W),
                            int(H), int(cycle), int(offset), int(run), int(row_begin), int(row_count))

    def deinterleave_cycle_rgb8(self, W, H, cycle, offsets, runs, part_bytes, gathered, out=None):
        """The RGBA8 frame (alpha 255) from cyclic parts' packed RGB8 rows:
        part i (offsets[i], runs[i], tiling [0, cycle) in order) starts at byte
        part_bytes[i] of the contiguous uint8 `gathered`."""
        torch = _torch()
        n = len(offsets)
        if len(runs) != n or len(part_bytes) != n:
            raise ValueError("deinterleave_cycle_rgb8: offsets, runs and part_bytes differ in length")
        if gathered.dtype != torch.uint8 or not gathered.is_contiguous():
            raise ValueError("deinterleave_cycle_rgb8: gathered must be a contiguous uint8 tensor")
        for o, r, b in zip(offsets, runs, part_bytes):
            if b + cycle_rows(H, cycle, o, r) * 3 * W > gathered.numel():
                raise ValueError("deinterleave_cycle_rgb8: a part's rows run past the end of gathered")
        out = self._out(out, (H, W), like=gathered)
        check(lib().rm_deinterleave_cycle_rgb8(self._ctx, int(W), int(H), int(cycle), n,
                                               (ctypes.c_int * n)(*offsets), (ctypes.c_int * n)(*runs),
                                               (ctypes.c_int64 * n)(*part_bytes), self._ptr(gathered),
                                               self._ptr(out)), self._ctx)
        return out

    def render_cycle_rows_wire(self, W, H, cycle, offset, run, row_begin, row_count, msg, workspace, size_out=None,
                               stats=False):
        """render_cycle_rows's RGBA8 rows as the compressed wire's message,
        encoded by the render kernel's epilogue (rm_render_cycle_rows_wire):
        `msg` uint8 of wire_capacity(W, row_count) bytes, `workspace` of
        wire_workspace_bytes(W, row_count), `size_out` an optional int64
        device tensor [1] for the message size (asynchronously)."""
        _check_wire("render_cycle_rows_wire", W, row_count, msg, workspace, size_out)
        return self._call(lib().rm_render_cycle_rows_wire, msg, stats, int(W), int(H), int(cycle), int(offset), int(run),
                          int(row_begin), int(row_count), self._ptr(msg), self._ptr(workspace), self._ptr(size_out))

    def wire_encode(self, rows, msg, workspace, size_out=None):
        """Compressed wire of packed RGBA8 rows (int32 [n, W]) into the uint8
        `msg` (>= wire_capacity bytes), with a uint8 `workspace` of
        wire_workspace_bytes; size_out: optional int64 device tensor [1] that
        receives the message size (asynchronously)."""
        torch = _torch()
        n, W = (int(rows.shape[0]), int(rows.shape[1])) if rows.dim() == 2 else (0, 0)
        if rows.dtype != torch.int32 or not rows.is_contiguous() or rows.dim() != 2:
            raise ValueError("wire_encode: rows must be contiguous int32 [n, W] RGBA8 words")
        _check_wire("wire_encode", W, n, msg, workspace, size_out)
        check(lib().rm_wire_encode(self._ctx, W, n, self._ptr(rows), self._ptr(msg), self._ptr(workspace),
                                   self._ptr(size_out)), self._ctx)
        return msg

    def wire_decode(self, W, H, cycle, offset, run, nrows, msg, frame):
        """A wire message of `nrows` rows of the cyclic part into the int32
        [H, W] RGBA8 frame (alpha 255)."""
        _check_out(frame, H * W)
        check(lib().rm_wire_decode(self._ctx, int(W), int(H), int(cycle), int(offset), int(run), int(nrows),
                                   self._ptr(msg), self._ptr(frame)), self._ctx)
        return frame

    def wire_decode_parts(self, W, H, cycle, offsets, runs, nrows, msgs, frame):
        """rm_wire_decode_parts: several parts' messages (uint8 device tensors)
        into the int32 [H, W] frame in one launch."""
        _check_out(frame, H * W)
        n = len(msgs)
        check(lib().rm_wire_decode_parts(self._ctx, int(W), int(H), int(cycle), n, (ctypes.c_int * n)(*offsets),
                                         (ctypes.c_int * n)(*runs), (ctypes.c_int * n)(*nrows),
                                         (ctypes.c_void_p * n)(*[m.data_ptr() for m in msgs]), self._ptr(frame)),
              self._ctx)
        return frame

    def scatter_part_rgba8(self, W, H, cycle, offset, run, nrows, rows, frame):
        """A part's packed RGBA8 rows (int32 [nrows, W]) into their frame rows."""
        _check_out(frame, H * W)
        _check_out(rows, nrows * W)
        check(lib().rm_scatter_part_rgba8(self._ctx, int(W), int(H), int(cycle), int(offset), int(run), int(nrows),
                                          self._ptr(rows), self._ptr(frame)), self._ctx)
        return frame

    def render_band_rgba8(self, W, H, band, nshards, shard, out=None, stats=False):
        """render_band into RGBA8 words ([rows, W] int32)."""
        return self._render("rm_render_band", True, (shard_rows(H, band, nshards, shard), W), out, stats,
                            int(W), int(H), int(band), int(nshards), int(shard))

    def deinterleave(self, W, H, band, nshards, rows_per_shard, gathered, out=None):
        """gathered: [nshards, rows_per_shard, W, 4] f32, [nshards, rows_per_shard, W] RGBA8 words, or
        [nshards, rows_per_shard, 3 * W] uint8 (the RGB8 wire; the frame is RGBA8 words, alpha 255)."""
        torch = _torch()
        wire = gathered.dtype == torch.uint8
        rgba8 = gathered.dtype != torch.float32  # RGBA8 words travel as int32
        out = self._out(out, (H, W) if rgba8 else (H, W, 4), "int32" if wire else gathered.dtype, like=gathered)
        if wire:
            if gathered.numel() < nshards * rows_per_shard * W * 3 or not gathered.is_contiguous():
                raise ValueError("deinterleave: RGB8 wire must be contiguous with 3*W bytes per row")
            fn = lib().rm_deinterleave_rgb8
        else:
            _check_out(gathered, nshards * rows_per_shard * W * (1 if rgba8 else 4))
            fn = lib().rm_deinterleave_rgba8 if rgba8 else lib().rm_deinterleave
        check(fn(self._ctx, W, H, band, nshards, rows_per_shard, self._ptr(gathered), self._ptr(out)), self._ctx)
        return out

    def pack_rgb8(self, frame8, out=None):
        """RGBA8 words -> the 3 B/px RGB8 wire (alpha dropped; the pass writes alpha 1)."""
        torch = _torch()
        _check_out(frame8, frame8.numel())
        npx = frame8.numel()
        if out is None:
            out = torch.empty(tuple(frame8.shape[:-1]) + (3 * frame8.shape[-1],), dtype=torch.uint8,
                              device=frame8.device)
        if out.numel() < 3 * npx or out.dtype != torch.uint8 or not out.is_contiguous() or not frame8.is_contiguous():
            raise ValueError("pack_rgb8: out must be a contiguous uint8 tensor with 3 bytes per pixel")
        check(lib().rm_pack_rgb8(self._ctx, npx, self._ptr(frame8), self._ptr(out)), self._ctx)
        return out

    def pack_rgba8(self, frame, out=None):
        torch = _torch()
        if frame.dtype != torch.float32 or not frame.is_contiguous() or frame.numel() % 4:
            raise ValueError("pack_rgba8: frame must be a contiguous float32 tensor of RGBA pixels")
        npx = frame.numel() // 4
        if out is None:
            out = torch.empty(frame.shape[:-1], dtype=torch.int32, device=frame.device)
        if out.numel() < npx or out.element_size() != 4 or not out.is_contiguous():
            raise ValueError("pack_rgba8: out must be a contiguous 32-bit tensor with one element per pixel")
        check(lib().rm_pack_rgba8(self._ctx, npx, self._ptr(frame), self._ptr(out)), self._ctx)
        return out

    def fxaa(self, frame8, out=None):
        """post.frag's FXAA over an [H, W] RGBA8 (int32 words) device frame."""
        H, W = frame8.shape
        (out,) = self._like(frame8, out)
        check(lib().rm_fxaa(self._ctx, W, H, self._ptr(frame8), self._ptr(out)), self._ctx)
        return out

    def bloom(self, frame8, out=None):
        """bloom.frag (with its mip chain) over an [H, W] RGBA8 (int32 words) device frame."""
        H, W = frame8.shape
        (out,) = self._like(frame8, out)
        check(lib().rm_bloom(self._ctx, W, H, self._ptr(frame8), self._ptr(out)), self._ctx)
        return out

    @staticmethod
    def _post_choice(sample, tonemap):
        """(sample, tonemap) names or rm.h values -> values; an int passes
        through for the library to judge."""
        return (int(_lib.named(sample, _lib.POST_SAMPLES, "sample")),
                int(_lib.named(tonemap, _lib.TONEMAPS, "tonemap")))

    def post_frag(self, frame8, sample="fxaa", tonemap="none", out=None):
        """post.frag's main() over an [H, W] RGBA8 (int32 words) device frame
        with its sample ("fxaa", "texel", "chromatic": POST_SAMPLES) and tonemap
        operator (TONEMAPS) chosen (rm_post_frag); the defaults are fxaa()."""
        s, t = self._post_choice(sample, tonemap)
        H, W = frame8.shape
        (out,) = self._like(frame8, out)
        check(lib().rm_post_frag(self._ctx, W, H, s, t, self._ptr(frame8), self._ptr(out)), self._ctx)
        return out

    def post_chain(self, frame8, mid=None, out=None, sample="fxaa", tonemap="none"):
        """main.cpp:209-214's post passes of a frame: FXAA of frame8 into mid,
        then bloom of mid into out (rm_post_chain); returns (mid, out).  With a
        sample or tonemap other than the defaults the first pass is post_frag's
        (rm_post_chain_ex)."""
        H, W = frame8.shape
        mid, out = self._like(frame8, mid, out)
        if (sample, tonemap) == ("fxaa", "none"):
            check(lib().rm_post_chain(self._ctx, W, H, self._ptr(frame8), self._ptr(mid), self._ptr(out)), self._ctx)
        else:
            s, t = self._post_choice(sample, tonemap)
            check(lib().rm_post_chain_ex(self._ctx, W, H, s, t, self._ptr(frame8), self._ptr(mid), self._ptr(out)),
                  self._ctx)
        return mid, out

    # --- the post passes over a batch of frames (rm_post_chain_batch) ---
    def post_frag_batch(self, frames8, sample="fxaa", tonemap="none", out=None):
        """post_frag of every frame of an [n, H, W] RGBA8 (int32 words) device
        batch in one launch (rm_post_frag_batch): out[v] is byte for byte
        post_frag(frames8[v]) with the same sample and tonemap."""
        s, t = self._post_choice(sample, tonemap)
        n, H, W = frames8.shape
        (out,) = self._like(frames8, out)
        check(lib().rm_post_frag_batch(self._ctx, W, H, n, s, t, self._ptr(frames8), self._ptr(out)), self._ctx)
        return out

    def bloom_batch(self, frames8, out=None):
        """bloom of every frame of an [n, H, W] RGBA8 device batch
        (rm_bloom_batch): out[v] is byte for byte bloom(frames8[v]).  The
        launches do not grow with n, but for the groups the scratch limit
        makes (post_batch_plan, set_post_batch_scratch_limit)."""
        n, H, W = frames8.shape
        (out,) = self._like(frames8, out)
        check(lib().rm_bloom_batch(self._ctx, W, H, n, self._ptr(frames8), self._ptr(out)), self._ctx)
        return out

    def post_chain_batch(self, frames8, mid=None, out=None, sample="fxaa", tonemap="none"):
        """post_chain of every frame of an [n, H, W] RGBA8 device batch, such
        as render_batch's or render_batch_aa's (rm_post_chain_batch): returns
        (mid, out), whose view v is byte for byte post_chain(frames8[v]) with
        the same sample and tonemap.  frames8, mid and out must not overlap."""
        s, t = self._post_choice(sample, tonemap)
        n, H, W = frames8.shape
        mid, out = self._like(frames8, mid, out)
        check(lib().rm_post_chain_batch(self._ctx, W, H, n, s, t, self._ptr(frames8), self._ptr(mid),
                                        self._ptr(out)), self._ctx)
        return mid, out

    def set_post_batch_scratch_limit(self, nbytes: int) -> None:
        """The most bloom scratch a batched bloom of this renderer asks for
        (rm_set_post_batch_scratch_limit); 0 restores the default,
        POST_BATCH_SCRATCH_DEFAULT (512 MiB).  A batch whose views need more
        runs in groups (post_batch_plan)."""
        check(lib().rm_set_post_batch_scratch_limit(self._ctx, int(nbytes)), self._ctx)

    SCENE_FORMS = _lib.SCENE_FORMS  # rm.h rm_form

    def scene_eval(self, points, material: bool = False, form: str = "exact", aux: bool = False):
        """sceneSDF(p) of the loaded scene at points [n, 3] (host, numpy):
        dist [n], and with material=True also the [n, 16] Material floats.
        form: "exact" (rm_scene_eval), "probe" or "probe_nb1"
        (rm_scene_eval_form: the probe form of the distance; with one fold exit
        test).  aux=True appends the [n] floats of rm_scene_eval_form's aux
        (the compiled-in scene O's probe-form slack, 0 for other scenes).
        Returns dist, or the tuple (dist[, material][, aux])."""
        import numpy as np
        if form not in self.SCENE_FORMS:
            raise ValueError(f"form must be one of {sorted(self.SCENE_FORMS)}, not {form!r}")
        pts = np.ascontiguousarray(points, np.float32).reshape(-1, 3)
        n = len(pts)
        dist = np.zeros(n, np.float32)
        mat = np.zeros((n, 16), np.float32) if material else None
        ax = np.zeros(n, np.float32) if aux else None
        if form == "exact" and not aux:
            check(lib().rm_scene_eval(self._ctx, self._ptr(pts), n, self._ptr(dist),
                                      self._ptr(mat)), self._ctx)
        else:
            check(lib().rm_scene_eval_form(self._ctx, self._ptr(pts), n, self.SCENE_FORMS[form], self._ptr(dist),
                                           self._ptr(mat), self._ptr(ax)),
                  self._ctx)
        out = (dist,) + ((mat,) if material else ()) + ((ax,) if aux else ())
        return out if len(out) > 1 else dist

    def cast_rays(self, origins, directions, inside: bool = False, normal: bool = True, material: bool = False,
                  stats: bool = False) -> dict:
        """rm_cast_rays: castRayD (castRayDI with inside=True) of the loaded
        scene along rays directions [n, 3] (used as given, not normalised) from
        origins [n, 3], or [3] for one origin shared by all rays.  numpy
        arrays: staged, numpy results.  torch tensors on this renderer's
        device: the results are device tensors and the call is asynchronous on
        the renderer's stream (unless stats=True).  Returns dict(t [n] f32,
        status [n] i32 (RM_RAY_*), steps [n] i32, position [n, 3][, normal
        [n, 3]][, material [n, 16]][, stats])."""
        import numpy as np
        o, d, n, shared, on_device = _ray_inputs("cast_rays", origins, directions, shared_on_host=False)
        if on_device:
            torch = _torch()

            def empty(shape, dtype=torch.float32):
                return torch.empty(shape, dtype=dtype, device=d.device)
            i32 = torch.int32
        else:
            def empty(shape, dtype=np.float32):
                return np.empty(shape, dtype)
            i32 = np.int32
        out = dict(t=empty(n), status=empty(n, i32), steps=empty(n, i32), position=empty((n, 3)))
        if normal:
            out["normal"] = empty((n, 3))
        if material:
            out["material"] = empty((n, 16))
        hits = _lib.RmRayHits(*(self._ptr(out[k]) if k in out and n else None
                                for k in ("t", "status", "steps", "position", "normal", "material")))
        res = self._call(lib().rm_cast_rays, out, stats, self._ptr(o), int(shared), self._ptr(d), n,
                         int(bool(inside)), ctypes.byref(hits))
        if stats:
            out["stats"] = res[1]
        return out

    def camera_rays(self, W: int, H: int):
        """rm_camera_rays: (origin [3], directions [H, W, 3]) on the device, the
        rays main() builds for the W x H frame; cast_rays(origin, directions.
        reshape(-1, 3)) gives the frame's depth / normal / material buffers."""
        torch = _torch()
        dev = f"cuda:{self.device}"
        origin = torch.empty(3, dtype=torch.float32, device=dev)
        directions = torch.empty((H, W, 3), dtype=torch.float32, device=dev)
        check(lib().rm_camera_rays(self._ctx, int(W), int(H), self._ptr(origin), self._ptr(directions)), self._ctx)
        return origin, directions

    def shade_rays(self, origins, directions, width: int = 0, output: str = "display", vignette: bool = False,
                   rgba8: bool = False, out=None, stats: bool = False, normalize: bool = False):
        """rm_shade_rays: the pass's colour (render(ro, rd): light, AO, soft
        shadow, SSS, reflection, refraction, fog) along rays directions [..., 3]
        (unit vectors; normalize=True normalises them in f32 first) from
        origins [n, 3], or [3] for one origin shared by all rays (the launch's
        u_pos).  width > 0: the rays are a width x (n / width) image, shaded in
        8x8 tiles; 0: a list.  output "linear" (render()'s colour) or "display"
        (tonemap -> contrast, times the ray image's vignette with
        vignette=True, as a frame's pixels).  Returns [n, 4] f32 (alpha 1), or
        [n] RGBA8 words with rgba8=True; a ray that is not a finite unit ray
        gives zeros (alpha 0).  numpy arrays: staged, a numpy result.  torch
        tensors on this renderer's device: a device tensor, asynchronous on the
        renderer's stream (unless stats=True).  camera_rays' rays with
        width=W, vignette=True give render(W, H) / render_rgba8(W, H) bit for
        bit.  -> colours[, stats]."""
        import numpy as np
        if output not in _lib.SHADE_OUTPUTS:
            raise ValueError(f"shade_rays: output {output!r}; expected one of {sorted(_lib.SHADE_OUTPUTS)}")
        # the shared origin is read on the host (cast_rays reads it where the directions live)
        o, d, n, shared, on_device = _ray_inputs("shade_rays", origins, directions, shared_on_host=True,
                                                 normalize=normalize)
        if out is None and not on_device:
            out = np.empty((n,) if rgba8 else (n, 4), np.uint32 if rgba8 else np.float32)
        out = self._out(out, (n,), like=d) if rgba8 else self._out(out, (n, 4), "float32", like=d)
        p = _lib.RmShadeParams(int(width), _lib.SHADE_OUTPUTS[output], int(bool(vignette)))
        return self._call(lib().rm_shade_rays, out, stats, self._ptr(o), int(shared), self._ptr(d), n, ctypes.byref(p),
                          None if rgba8 else self._ptr(out), self._ptr(out) if rgba8 else None)

    def render_rgba8(self, W, H, out=None, stats=False):
        return self._render("rm_render", True, (H, W), out, stats, W, H)

    # --- view batches (rm_render_batch, rm_render_batch_rgba8) -------------
    def render_batch(self, W: int, H: int, views, out=None, rgba8: bool = True, stats: bool = False):
        """n views of the loaded scene from one launch (rm_render_batch[_rgba8];
        DESIGN.md 2.26).  views: anything pack_views takes -- a sequence of
        dicts in POSES' form (pos, mouse, time) with an optional `offset`
        (sub-pixel, each component in [-0.5, 0.5)), or an (n, 6) / (n, 8)
        float32 array or tensor of rows px py pz mx my t [ox oy].  A CUDA
        tensor of views is copied to the host first, which synchronises.
        Returns [n, H, W] int32 RGBA8 words (rgba8=True) or [n, H, W, 4]
        float32, view v's frame byte for byte what set_pose + render_rgba8 /
        render gives; `out`: a device tensor of that many elements (allocated
        if None; asynchronous on the renderer's stream unless stats=True) or a
        numpy array (staged).  u_resolution, max_steps and shadow_max_steps
        are the renderer's; its own pose is neither read nor changed.  The
        timed kernels in row-major one-wave tiles, always: kernel, schedule,
        count_evals and set_tile_order do not apply.  Built-in scenes only."""
        v = pack_views(views)
        return self._render("rm_render_batch", rgba8, (len(v), H, W), out, stats, int(W), int(H), self._ptr(v), len(v))

    def render_batch_ex(self, W: int, H: int, views, uniforms=None, out=None, rgba8: bool = True,
                        stats: bool = False):
        """render_batch for any scene, a scene plugin included, with the scene's
        own uniforms set per view (rm_render_batch_ex[_rgba8]).
        uniforms: a dict from the name of a uniform the loaded scene declares to
        an array of shape [n] (a float, an int or a bool per view),
        [n, components] (a vecN per view; for an array of floats, its leading
        elements) or [n, count, components] (the leading `count` elements of an
        array uniform).  An int or bool uniform, by its declared type, takes
        integers (non-zero: true), every other floats.  View v's frame is byte
        for byte what set_pose + set_uniform of view v's values + render_rgba8 /
        render gives; an unlisted uniform has the renderer's current value.  The
        renderer's own pose and uniform values are neither read nor changed.
        A plugin's batch kernel is compiled on the first call after load_scene
        (batch_prepare compiles it ahead).  For a built-in scene: render_batch,
        and a non-empty `uniforms` raises.  views, out, rgba8, stats: as
        render_batch."""
        v = pack_views(views)
        n = len(v)
        arr, n_entries, _keep = self._view_uniforms("render_batch_ex", uniforms, n)
        return self._render("rm_render_batch_ex", rgba8, (n, H, W), out, stats, int(W), int(H), self._ptr(v), n, arr,
                            n_entries)

    def _view_uniforms(self, what, uniforms, n):
        """The rm_view_uniform list of a `uniforms` dict (render_batch_ex's) for n
        views -> (pointer to the list or None, entries, what must stay alive
        until the call returns: the list and the arrays it points into)."""
        import numpy as np
        infos = {u.name.decode(): u for u in self._uniform_infos()}
        entries, keep = [], []
        for name, values in (uniforms or {}).items():
            info = infos.get(name)
            ints = info is not None and _lib.UNIFORM_TYPES[info.type] in ("int", "bool")
            a = np.ascontiguousarray(values.cpu().numpy() if hasattr(values, "cpu") else values,
                                     np.int32 if ints else np.float32)
            if a.ndim == 1:
                a = a.reshape(-1, 1, 1)
            elif a.ndim == 2 and info is not None and info.count and info.components == 1:
                a = a.reshape(a.shape[0], a.shape[1], 1)
            elif a.ndim == 2:
                a = a.reshape(a.shape[0], 1, a.shape[1])
            if a.ndim != 3 or a.shape[0] != n:
                raise ValueError(f"{what}: uniform {name!r} needs [n], [n, components] or "
                                 f"[n, count, components] values for n = {n} views")
            keep.append((name.encode(), a))
            entries.append(_lib.RmViewUniform(keep[-1][0], int(a.shape[2]), int(a.shape[1]),
                                              ctypes.c_void_p(a.ctypes.data)))
        arr = (_lib.RmViewUniform * max(1, len(entries)))(*entries)
        return (ctypes.cast(arr, ctypes.c_void_p) if entries else None), len(entries), (arr, keep)

    def batch_prepare(self) -> None:
        """rm_batch_prepare: compile and load the loaded plugin's batch kernel
        now, not inside the first render_batch_ex (nothing to do for a built-in
        scene or once it is loaded)."""
        check(lib().rm_batch_prepare(self._ctx), self._ctx)

    # --- adaptive supersampling (rm_render_aa_rgba8, rm_refine_rgba8) -----
    def _aa(self, fn, W, H, samples, threshold, frame8, mask, stats):
        """frame8: [H, W] RGBA8 words, a device tensor or a numpy array (staged);
        the mask lives where the frame does.  -> frame8[, mask][, stats]."""
        import numpy as np
        on_device = hasattr(frame8, "data_ptr")
        _check_out(frame8, H * W)
        m = None
        if mask:
            m = (_torch().empty((H, W), dtype=_torch().uint8, device=frame8.device) if on_device
                 else np.empty((H, W), np.uint8))
        p = _lib.RmAaParams(int(samples), int(threshold))
        s = _lib.RmAaStats()
        check(fn(self._ctx, int(W), int(H), ctypes.byref(p), self._ptr(frame8), self._ptr(m),
                 ctypes.byref(s) if stats else None), self._ctx)
        res = (frame8,) + ((m,) if mask else ()) + ((s.as_dict(),) if stats else ())
        return res if len(res) > 1 else frame8

    def render_aa(self, W, H, samples=4, threshold=32, out=None, mask=False, stats=False):
        """One antialiased RGBA8 frame (rm_render_aa_rgba8): render_rgba8's frame
        with its edge pixels -- a colour channel's spread over the 3x3
        neighbourhood >= threshold, 0..255 -- replaced by the mean of `samples`
        (2, 4 or 8) sub-pixel samples, byte for byte what blending
        render_accumulate's jittered frames gives there.  The default
        threshold 32 is a convenience, not a tuned value; 0 supersamples every
        pixel.  out: [H, W] int32 device tensor (allocated if None) or a numpy
        array.  Returns out, then with mask=True the uint8 [H, W] mask of the
        refined pixels, then with stats=True dict(refined, base_ms, detect_ms,
        refine_ms) (which waits for the frame).  Built-in scenes only."""
        return self._aa(lib().rm_render_aa_rgba8, W, H, samples, threshold, self._out(out, (H, W)), mask, stats)

    def refine(self, frame8, samples=4, threshold=32, mask=False, stats=False):
        """rm_refine_rgba8: the supersampling step of render_aa on any [H, W]
        RGBA8 frame of the current uniforms (normally render_rgba8's), in
        place; returns as render_aa does."""
        H, W = frame8.shape
        return self._aa(lib().rm_refine_rgba8, W, H, samples, threshold, frame8, mask, stats)

    def render_aa_ex(self, W, H, samples=4, threshold=32, out=None, mask=False, stats=False):
        """render_aa for any scene, a scene plugin included
        (rm_render_aa_ex_rgba8).  For a plugin a refined pixel
        is byte for byte the pack of the tree mean of render_accumulate's
        `samples` jittered float frames of the plugin, under the renderer's
        current uniforms, the scene's own included.  A plugin's refine kernel
        is compiled on the first call after load_scene (aa_prepare compiles it
        ahead).  For a built-in scene: render_aa.  Arguments and results as
        render_aa's."""
        return self._aa(lib().rm_render_aa_ex_rgba8, W, H, samples, threshold, self._out(out, (H, W)), mask, stats)

    def refine_ex(self, frame8, samples=4, threshold=32, mask=False, stats=False):
        """rm_refine_ex_rgba8: refine for any scene, a scene plugin included;
        the supersampling step of render_aa_ex on an [H, W] RGBA8 frame, in
        place."""
        H, W = frame8.shape
        return self._aa(lib().rm_refine_ex_rgba8, W, H, samples, threshold, frame8, mask, stats)

    def aa_prepare(self) -> None:
        """rm_aa_prepare: compile and load the loaded plugin's refine kernel
        now, not inside the first render_aa_ex / refine_ex (nothing to do for a
        built-in scene or once it is loaded)."""
        check(lib().rm_aa_prepare(self._ctx), self._ctx)

    # --- adaptive supersampling of a view batch (rm_render_batch_aa_rgba8, rm_refine_batch_rgba8) ---
    def _batch_aa(self, fn, W, H, v, samples, threshold, frames8, mask, refined, stats):
        """v: the packed views.  frames8: [n, H, W] RGBA8 words, a device tensor
        or a numpy array (staged); the mask and the per-view counts live where
        the frames do.  -> frames8[, mask][, refined][, stats]."""
        import numpy as np
        n = len(v)
        on_device = hasattr(frames8, "data_ptr")
        _check_out(frames8, n * H * W)
        m = r = None
        if mask:
            m = (_torch().empty((n, H, W), dtype=_torch().uint8, device=frames8.device) if on_device
                 else np.empty((n, H, W), np.uint8))
        if refined:
            r = (_torch().empty((n,), dtype=_torch().int32, device=frames8.device) if on_device
                 else np.empty((n,), np.uint32))
        p = _lib.RmAaParams(int(samples), int(threshold))
        s = _lib.RmAaStats()
        check(fn(self._ctx, int(W), int(H), ctypes.c_void_p(v.ctypes.data), n, ctypes.byref(p), self._ptr(frames8),
                 self._ptr(m), self._ptr(r),
                 ctypes.byref(s) if stats else None), self._ctx)
        res = (frames8,) + ((m,) if mask else ()) + ((r,) if refined else ()) + ((s.as_dict(),) if stats else ())
        return res if len(res) > 1 else frames8

    def render_batch_aa(self, W: int, H: int, views, samples=4, threshold=32, out=None, mask=False, refined=False,
                        stats=False):
        """n antialiased RGBA8 views from one call (rm_render_batch_aa_rgba8;
        DESIGN.md 2.28): render_batch's frames with every view's edge pixels
        supersampled, view v's frame byte for byte what set_pose + render_aa
        gives with the same samples and threshold.  views: as render_batch
        takes them, every offset (0, 0).  out: [n, H, W] int32 device tensor
        (allocated if None; asynchronous on the renderer's stream unless
        stats=True) or a numpy array (staged).  Returns out, then with
        mask=True the uint8 [n, H, W] mask of the refined pixels, then with
        refined=True the [n] per-view counts of refined pixels (int32 on the
        device, uint32 in numpy), then with stats=True dict(refined, base_ms,
        detect_ms, refine_ms) -- refined summed over the views, detect_ms with
        the plan step (which waits for the frames).  Built-in scenes only."""
        v = pack_views(views)
        return self._batch_aa(lib().rm_render_batch_aa_rgba8, W, H, v, samples, threshold,
                              self._out(out, (len(v), H, W)), mask, refined, stats)

    def refine_batch(self, frames8, views, samples=4, threshold=32, mask=False, refined=False, stats=False):
        """rm_refine_batch_rgba8: the supersampling step of render_batch_aa on
        any [n, H, W] RGBA8 frames of the views (normally render_batch's), in
        place; returns as render_batch_aa does."""
        n, H, W = frames8.shape
        v = pack_views(views)
        if n != len(v):
            raise ValueError(f"refine_batch: {n} frames for {len(v)} views")
        return self._batch_aa(lib().rm_refine_batch_rgba8, W, H, v, samples, threshold, frames8, mask, refined, stats)


def batch_aa_scratch_bytes(W: int, H: int, n: int) -> int:
    """rm_batch_aa_scratch_bytes: the bytes of the renderer's scratch buffer
    (counters, plan, queue) for render_batch_aa of n views of W x H; RmError
    where the size rule refuses them.  No GPU."""
    b = ctypes.c_int64(0)
    check(lib().rm_batch_aa_scratch_bytes(int(W), int(H), int(n), ctypes.byref(b)))
    return int(b.value)


def post_batch_plan(W: int, H: int, n: int, limit: int = 0) -> dict:
    """rm_post_batch_plan: how post_chain_batch of n frames of W x H uses the
    renderer's bloom scratch under a limit of `limit` bytes (0: the default) --
    dict(per_view_bytes, shared_bytes, group_views, groups, scratch_bytes,
    launches); RmError where the size rule refuses them.  No GPU."""
    p = _lib.RmPostBatchPlan()
    check(lib().rm_post_batch_plan(int(W), int(H), int(n), int(limit), ctypes.byref(p)))
    return p.as_dict()


def pack_views(views):
    """The views of Renderer.render_batch as the contiguous float32 [n, 8]
    array rm_render_batch reads (rm.h rm_view: px py pz mx my t ox oy).  No
    GPU, no librm.  views: a sequence of dicts in POSES' form -- pos (3),
    mouse (2), time, and optionally offset (2; default (0, 0), the pixel
    centres) -- or an (n, 6) array or tensor (offsets 0) or an (n, 8) one.  A
    CUDA tensor is copied to the host (which synchronises).  An empty sequence
    gives [0, 8].  ValueError: another shape, a value that is not finite, or an
    offset component outside [-0.5, 0.5)."""
    import numpy as np
    if hasattr(views, "detach"):  # a torch tensor
        views = views.detach().cpu().numpy()
    if isinstance(views, np.ndarray):
        a = np.asarray(views, np.float32)
        if a.ndim != 2 or a.shape[1] not in (6, 8):
            raise ValueError(f"pack_views: an (n, 6) or (n, 8) array, not {tuple(a.shape)}")
    else:
        rows = []
        for i, v in enumerate(views):
            if not hasattr(v, "keys"):
                raise ValueError(f"pack_views: view {i} is not a dict (pos, mouse, time[, offset])")
            extra = set(v.keys()) - {"pos", "mouse", "time", "offset"}
            if extra or not {"pos", "mouse", "time"} <= set(v.keys()):
                raise ValueError(f"pack_views: view {i} needs pos, mouse, time and optionally offset")
            pos, mouse, off = tuple(v["pos"]), tuple(v["mouse"]), tuple(v.get("offset", (0.0, 0.0)))
            if (len(pos), len(mouse), len(off)) != (3, 2, 2):
                raise ValueError(f"pack_views: view {i}: pos has 3 components, mouse and offset 2")
            rows.append(pos + mouse + (float(v["time"]),) + off)
        a = np.asarray(rows, np.float32).reshape(len(rows), 8)
    out = np.zeros((a.shape[0], 8), np.float32)
    out[:, :a.shape[1]] = a
    if not np.isfinite(out).all():
        raise ValueError("pack_views: a value is not finite")
    if ((out[:, 6:] < np.float32(-0.5)) | (out[:, 6:] >= np.float32(0.5))).any():
        raise ValueError("pack_views: an offset component is outside [-0.5, 0.5)")
    return out


def aa_offsets(samples: int):
    """rm_aa_offsets: the [samples, 2] float32 sub-pixel offsets (x, y), in
    pixels from the pixel centre, of render_aa's samples (samples = 2, 4, 8)."""
    import numpy as np
    xy = np.zeros((max(int(samples), 0), 2), np.float32)
    buf = xy if xy.size else np.zeros((1, 2), np.float32)
    check(lib().rm_aa_offsets(int(samples), ctypes.c_void_p(buf.ctypes.data)))
    return xy


def aa_edge_mask(frame, threshold: int):
    """rm_aa_edge_mask: render_aa's edge rule on a host [H, W] RGBA8 frame
    (numpy, 32-bit words) -> uint8 [H, W], 1 = edge pixel.  No GPU."""
    import numpy as np
    f = np.ascontiguousarray(frame)
    if f.ndim != 2 or f.itemsize != 4:
        raise ValueError("aa_edge_mask: an [H, W] array of RGBA8 words")
    H, W = f.shape
    mask = np.empty((H, W), np.uint8)
    check(lib().rm_aa_edge_mask(int(W), int(H), int(threshold), ctypes.c_void_p(f.ctypes.data),
                                ctypes.c_void_p(mask.ctypes.data)))
    return mask


def sharded_layout(W: int, H: int, band: int, nranks: int, rank: int) -> dict:
    """rm_sharded_layout: the row/byte layout of rm_render_sharded (no GPU)."""
    L = _lib.RmShardLayout()
    check(lib().rm_sharded_layout(int(W), int(H), int(band), int(nranks), int(rank), ctypes.byref(L)))
    return L.as_dict()


def comm_get_id() -> bytes:
    """rm_comm_get_id (ncclGetUniqueId): rank 0 makes it, every rank passes it to Comm."""
    cid = _lib.RmCommId()
    check(lib().rm_comm_get_id(ctypes.byref(cid)))
    return ctypes.string_at(ctypes.addressof(cid), 128)


class Comm:
    """A librm RCCL communicator bound to a Renderer (rm_comm_*): row-sharded
    RGBA8 frames, rank r rendering the rows (y // band) % nranks == r and
    rank 0 receiving the frame (rm_render_sharded)."""

    def __init__(self, renderer: Renderer, nranks: int = 1, rank: int = 0, comm_id: bytes | None = None,
                 _handle=None):
        self.r, self.nranks, self.rank = renderer, int(nranks), int(rank)
        if _handle is not None:
            self._h = _handle
            return
        cid = _lib.RmCommId()
        if comm_id is None and self.nranks == 1:
            comm_id = comm_get_id()  # a one-rank communicator needs no exchange of the id
        if comm_id is not None:
            ctypes.memmove(ctypes.addressof(cid), comm_id, 128)
        self._h = ctypes.c_void_p()
        check(lib().rm_comm_init_rank(ctypes.byref(self._h), renderer._ctx, self.nranks, ctypes.byref(cid),
                                      self.rank), renderer._ctx)

    @staticmethod
    def init_all(renderers) -> list:
        """One process driving len(renderers) GPUs (rm_comm_init_all)."""
        n = len(renderers)
        hs = (ctypes.c_void_p * n)()
        ctxs = (ctypes.c_void_p * n)(*[r._ctx.value for r in renderers])
        check(lib().rm_comm_init_all(hs, ctxs, n), renderers[0]._ctx)
        return [Comm(r, n, i, _handle=ctypes.c_void_p(hs[i])) for i, r in enumerate(renderers)]

    def render(self, W: int, H: int, band: int = 16, frame=None, stats: bool = False, runs=None):
        """One sharded frame (collective over the ranks).  Rank 0 gets the
        [H, W] RGBA8 (int32 words) frame, the others None.  runs: weighted
        parts (rm_render_sharded_runs, one run per rank) instead of bands."""
        if self.rank == 0 or frame is not None:
            frame = self.r._out(frame, (H, W))
        if runs is not None:
            if len(runs) != self.nranks:
                raise ValueError(f"runs needs {self.nranks} entries")
            fn, part = lib().rm_render_sharded_runs, (ctypes.c_int * len(runs))(*runs)
        else:
            fn, part = lib().rm_render_sharded, int(band)
        return self.r._call(fn, frame, stats, int(W), int(H), part, self.r._ptr(frame), handle=self._h)

    @staticmethod
    def render_all(comms, W: int, H: int, band: int = 16, frame=None, stats: bool = False, runs=None):
        """rm_render_sharded_all (or, with runs, rm_render_sharded_runs_all)
        over the communicators of init_all."""
        n = len(comms)
        frame = comms[0].r._out(frame, (H, W))
        hs = (ctypes.c_void_p * n)(*[c._h.value for c in comms])
        st = (RmStats * n)()
        if runs is not None:
            if len(runs) != n:
                raise ValueError(f"runs needs {n} entries")
            check(lib().rm_render_sharded_runs_all(hs, n, int(W), int(H), (ctypes.c_int * n)(*runs),
                                                   comms[0].r._ptr(frame), st if stats else None), comms[0].r._ctx)
        else:
            check(lib().rm_render_sharded_all(hs, n, int(W), int(H), int(band), comms[0].r._ptr(frame),
                                              st if stats else None), comms[0].r._ctx)
        return (frame, [c.r._stats(x) for c, x in zip(comms, st)]) if stats else frame

    @property
    def uses_rccl(self) -> bool:
        n, r, u = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
        check(lib().rm_comm_info(self._h, ctypes.byref(n), ctypes.byref(r), ctypes.byref(u)))
        return bool(u.value)

    def close(self):
        if self._h:
            lib().rm_comm_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:  # interpreter shutdown
            pass


def _compile(fn, file_name):
    buf = ctypes.create_string_buffer(1 << 16)
    st = fn(file_name.encode(), ctypes.cast(buf, ctypes.c_void_p), len(buf))
    log = buf.value.decode(errors="replace")
    if st == _lib.STATUS_CODES["RM_ERR_FILE"]:
        raise _lib.RmError(st, log)
    return st == 0, log


def compile_scene(file_name: str):
    """rm_compile_scene: compile a scene plugin with hiprtc, no GPU needed.
    Returns (ok, log); a missing file or #include raises RmError."""
    return _compile(lib().rm_compile_scene, file_name)


def compile_scene_batch(file_name: str):
    """rm_compile_scene_batch: compile_scene for the batch form of a plugin's
    code object (Renderer.render_batch_ex's kernel).  (False, log) for a scene
    that defines RM_PLUGIN_EVAL_ONLY."""
    return _compile(lib().rm_compile_scene_batch, file_name)


def compile_scene_aa(file_name: str):
    """rm_compile_scene_aa: compile_scene for the AA form of a plugin's code
    object (Renderer.render_aa_ex's refine kernel).  (False, log) for a scene
    that defines RM_PLUGIN_EVAL_ONLY."""
    return _compile(lib().rm_compile_scene_aa, file_name)


def _check_out(t, n):
    """A buffer the C ABI reads or writes as 32-bit words: a contiguous torch
    tensor or numpy array of 4-byte elements with at least `n` of them."""
    if hasattr(t, "is_contiguous"):
        ok, have, es = t.is_contiguous(), t.numel(), t.element_size()
    else:
        ok, have, es = bool(t.flags["C_CONTIGUOUS"]), t.size, t.itemsize
    if not ok or have < n or es != 4:
        raise ValueError(f"buffer must be contiguous 32-bit with >= {n} elements")


def _check_wire(what, W, nrows, msg, workspace, size_out):
    """The buffers of a wire message of nrows rows of W pixels."""
    torch = _torch()
    if msg.dtype != torch.uint8 or msg.numel() < wire_capacity(W, nrows) or not msg.is_contiguous():
        raise ValueError(f"{what}: msg must be a contiguous uint8 tensor of wire_capacity bytes")
    if workspace.numel() * workspace.element_size() < wire_workspace_bytes(W, nrows):
        raise ValueError(f"{what}: workspace too small")
    if size_out is not None and (size_out.dtype != torch.int64 or size_out.numel() < 1):
        raise ValueError(f"{what}: size_out must be an int64 tensor")


def _ray_inputs(what, origins, directions, shared_on_host, normalize=False):
    """The rays of cast_rays / shade_rays -> (origins, directions, n, shared,
    on_device): float32, directions contiguous [n, 3] (normalised in f32 with
    normalize), origins [3] (shared by all rays) or [n, 3].  numpy arrays, or,
    where directions is a CUDA tensor, torch tensors on its device -- but for a
    shared origin with shared_on_host, which then stays on the host."""
    import numpy as np
    on_device = hasattr(directions, "data_ptr") and directions.is_cuda
    if on_device:
        torch = _torch()
        d = directions.to(torch.float32).reshape(-1, 3)
        if normalize:
            d = d / torch.linalg.vector_norm(d, dim=1, keepdim=True)
        d = d.contiguous()
        o = torch.as_tensor(origins, dtype=torch.float32)
        o = (o.cpu() if o.ndim == 1 and shared_on_host else o.to(d.device)).contiguous()
    else:
        d = np.ascontiguousarray(np.asarray(directions), np.float32).reshape(-1, 3)
        if normalize:
            d = d / np.sqrt((d * d).sum(1, dtype=np.float32, keepdims=True), dtype=np.float32)
        if hasattr(origins, "data_ptr"):
            origins = origins.cpu().numpy()
        o = np.ascontiguousarray(np.asarray(origins), np.float32)
    n, shared = len(d), o.ndim == 1
    if tuple(o.shape) != ((3,) if shared else (n, 3)):
        raise ValueError(f"{what}: origins {tuple(o.shape)} for {n} directions; expected [3] or [{n}, 3]")
    return o, d, n, shared, on_device


def render_code_hash() -> str:
    """The render kernels' code objects by content (rm_render_code_hash): the
    build a PMC counter set was taken with (bench.py)."""
    return lib().rm_render_code_hash().decode()


def wire_capacity(W: int, nrows: int) -> int:
    """Largest wire message of nrows rows of W pixels (rm_wire_capacity)."""
    v = int(lib().rm_wire_capacity(int(W), int(nrows)))
    if v < 0:
        raise ValueError("wire_capacity: bad size")
    return v


def wire_workspace_bytes(W: int, nrows: int) -> int:
    v = int(lib().rm_wire_workspace_bytes(int(W), int(nrows)))
    if v < 0:
        raise ValueError("wire_workspace_bytes: bad size")
    return v


def cycle_rows(H: int, cycle: int, offset: int, run: int) -> int:
    """Frame rows y < H with (y mod cycle) - offset in [0, run) (rm_cycle_rows)."""
    n = ctypes.c_int()
    check(lib().rm_cycle_rows(int(H), int(cycle), int(offset), int(run), ctypes.byref(n)))
    return n.value


def shard_rows(H: int, band: int, nshards: int, shard: int) -> int:
    n = ctypes.c_int()
    check(lib().rm_shard_rows(int(H), int(band), int(nshards), int(shard), ctypes.byref(n)))
    return n.value


# ------------------------------------------------ the reference's surface


class Shader(Renderer):
    """sf::Shader as main.cpp uses it: a loaded scene plus its uniforms."""

    Fragment = "Fragment"

    def __init__(self, device: int = 0):
        super().__init__(device)
        self.loaded = False

    def setUniform(self, name: str, value) -> None:  # noqa: N802 (SFML name)
        vals = tuple(value) if isinstance(value, (tuple, list)) else (value,)
        self.set_uniform(name, *vals)


class ShaderLoader:
    """source/shader_loader.h:8-15."""

    @staticmethod
    def loadFromFile(file_name: str, type_, out_shader: Shader) -> bool:  # noqa: N802
        if type_ != Shader.Fragment:
            print(f"ShaderLoader: only fragment passes exist here (got {type_})", file=sys.stderr)
            return False
        try:
            out_shader.load_scene(file_name)
        except _lib.RmError as e:
            print(str(e), file=sys.stderr)
            return False
        out_shader.loaded = True
        return True


class RenderTexture:
    """sf::RenderTexture stand-in: a W x H float4 target resident in HBM."""

    def __init__(self):
        self.texture = None

    def create(self, W: int, H: int, device: int = 0) -> bool:
        torch = _torch()
        self.W, self.H = int(W), int(H)
        self.texture = torch.zeros((H, W, 4), dtype=torch.float32, device=f"cuda:{device}")
        return True

    def draw(self, shader: Shader, stats: bool = False):
        """Run `shader`'s pass over the whole target (main.cpp:199,205)."""
        r = shader.render(self.W, self.H, out=self.texture, stats=stats)
        return r[1] if stats else None

    def getTexture(self):  # noqa: N802
        return self.texture
