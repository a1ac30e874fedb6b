"""ctypes binding of librm.so (include/rm.h).

The product path has no CPU fallback: if librm.so is missing or fails to
load, every entry point raises.
"""
from __future__ import annotations

import ctypes
import os

HERE = os.path.dirname(os.path.abspath(__file__))
# RM_LIB may point at an alternative in-tree build (experiments); default librm.so
LIB_PATH = os.environ.get("RM_LIB") or os.path.join(HERE, "librm.so")

RM_OK = 0
STATUS = {0: "RM_OK", 1: "RM_ERR_INVALID_ARGUMENT", 2: "RM_ERR_FILE", 3: "RM_ERR_SCENE",
          4: "RM_ERR_NO_SCENE", 5: "RM_ERR_DEVICE", 6: "RM_ERR_OUT_OF_MEMORY"}
STATUS_CODES = {v: k for k, v in STATUS.items()}

# every symbol include/rm.h declares
EXPORTS = ("rm_create", "rm_destroy", "rm_load_scene", "rm_set_uniform1f", "rm_set_uniform2f",
           "rm_set_uniform3f", "rm_set_params", "rm_get_params", "rm_set_stream", "rm_set_stream_kept",
           "rm_synchronize",
           "rm_render", "rm_render_band", "rm_render_rows", "rm_shard_rows", "rm_deinterleave", "rm_deinterleave_rgba8",
           "rm_pack_rgba8", "rm_pack_rgb8", "rm_deinterleave_rgb8",
           "rm_render_rgba8", "rm_render_accumulate", "rm_render_accumulate_rgba8", "rm_render_band_rgba8", "rm_render_rows_rgba8", "rm_fxaa", "rm_bloom", "rm_post_chain", "rm_post_frag", "rm_post_chain_ex",
           "rm_render_code_hash", "rm_render_cycle_rows_wire", "rm_last_error", "rm_status_string",
           "rm_compile_scene", "rm_scene_eval", "rm_render_step_map", "rm_sharded_layout", "rm_comm_get_id",
           "rm_comm_init_rank", "rm_comm_init_all", "rm_comm_destroy", "rm_render_sharded", "rm_render_sharded_all",
           "rm_set_tile_order", "rm_tile_grid", "rm_comm_info", "rm_abi_version", "rm_cycle_rows",
           "rm_render_cycle_rows", "rm_render_cycle_rows_rgba8", "rm_deinterleave_cycle_rgb8",
           "rm_render_sharded_runs", "rm_render_sharded_runs_all", "rm_wire_capacity", "rm_wire_workspace_bytes",
           "rm_wire_encode", "rm_wire_decode", "rm_scatter_part_rgba8", "rm_wire_decode_parts",
           "rm_set_uniform4f", "rm_set_uniform1i", "rm_set_uniformfv", "rm_uniform_count", "rm_uniform_info_at",
           "rm_get_uniformfv", "rm_get_uniform1i", "rm_cast_rays", "rm_camera_rays",
           "rm_aa_offsets", "rm_aa_edge_mask", "rm_refine_rgba8", "rm_render_aa_rgba8", "rm_shade_rays", "rm_scene_eval_form",
           "rm_resolution_cache_info", "rm_certified_steps", "rm_reflection_cleared_steps",
           "rm_near_sky_steps",
           "rm_batch_bytes", "rm_render_batch", "rm_render_batch_rgba8",
           "rm_batch_aa_scratch_bytes", "rm_refine_batch_rgba8", "rm_render_batch_aa_rgba8",
           "rm_post_batch_plan", "rm_set_post_batch_scratch_limit", "rm_post_frag_batch", "rm_bloom_batch",
           "rm_post_chain_batch",
           "rm_render_batch_ex", "rm_render_batch_ex_rgba8", "rm_batch_prepare", "rm_compile_scene_batch",
           "rm_refine_ex_rgba8", "rm_render_aa_ex_rgba8", "rm_aa_prepare", "rm_compile_scene_aa")

# include/rm.h RM_ABI_VERSION: the struct layouts below
ABI_VERSION = 3
DISPATCH = {0: "row-major", 1: "explicit", 2: "adaptive"}
# include/rm.h rm_post_sample, rm_tonemap (rm_post_frag, rm_post_chain_ex)
POST_SAMPLES = {"fxaa": 0, "texel": 1, "chromatic": 2}
TONEMAPS = {"none": 0, "aces": 1, "reinhard": 2, "jodie": 3, "uncharted2": 4}


class RmParams(ctypes.Structure):
    _fields_ = [("max_steps", ctypes.c_int32), ("shadow_max_steps", ctypes.c_int32),
                ("count_evals", ctypes.c_int32), ("kernel", ctypes.c_int32), ("schedule", ctypes.c_int32)]


class RmStats(ctypes.Structure):
    _fields_ = [("evals", ctypes.c_uint64), ("pixels", ctypes.c_uint64), ("kernel_ms", ctypes.c_float),
                ("scene", ctypes.c_int32), ("flop", ctypes.c_uint64), ("skipped", ctypes.c_uint64),
                ("dispatch", ctypes.c_int32), ("lat_tiles", ctypes.c_int32), ("gather_ms", ctypes.c_float),
                ("deinterleave_ms", ctypes.c_float)]

    def as_dict(self):
        return dict(evals=int(self.evals), pixels=int(self.pixels), kernel_ms=float(self.kernel_ms),
                    scene=int(self.scene), flop=int(self.flop), skipped=int(self.skipped),
                    dispatch=DISPATCH.get(int(self.dispatch), int(self.dispatch)), lat_tiles=int(self.lat_tiles),
                    gather_ms=float(self.gather_ms), deinterleave_ms=float(self.deinterleave_ms))


class RmShardLayout(ctypes.Structure):
    _fields_ = [("rows_mine", ctypes.c_int32), ("rows_per_shard", ctypes.c_int32), ("wire_bytes", ctypes.c_int64),
                ("gathered_bytes", ctypes.c_int64)]


class RmUniformInfo(ctypes.Structure):
    _fields_ = [("name", ctypes.c_char * 64), ("type", ctypes.c_int32), ("components", ctypes.c_int32),
                ("count", ctypes.c_int32)]


UNIFORM_TYPES = {0: "float", 1: "int", 2: "bool"}  # include/rm.h rm_uniform_type


class RmRayHits(ctypes.Structure):
    """include/rm.h rm_ray_hits: the outputs of rm_cast_rays (NULL: not written; t is required)."""
    _fields_ = [("t", ctypes.c_void_p), ("status", ctypes.c_void_p), ("steps", ctypes.c_void_p),
                ("position", ctypes.c_void_p), ("normal", ctypes.c_void_p), ("material", ctypes.c_void_p)]


class RmAaParams(ctypes.Structure):
    """include/rm.h rm_aa_params."""
    _fields_ = [("samples", ctypes.c_int32), ("threshold", ctypes.c_int32)]


class RmAaStats(ctypes.Structure):
    """include/rm.h rm_aa_stats."""
    _fields_ = [("refined", ctypes.c_int64), ("base_ms", ctypes.c_float), ("detect_ms", ctypes.c_float),
                ("refine_ms", ctypes.c_float)]

    def as_dict(self):
        return dict(refined=int(self.refined), base_ms=float(self.base_ms), detect_ms=float(self.detect_ms),
                    refine_ms=float(self.refine_ms))


class RmView(ctypes.Structure):
    """include/rm.h rm_view: one view of a batch (rm_render_batch*)."""
    _fields_ = [("pos", ctypes.c_float * 3), ("mouse", ctypes.c_float * 2), ("time", ctypes.c_float),
                ("offset", ctypes.c_float * 2)]


class RmViewUniform(ctypes.Structure):
    """include/rm.h rm_view_uniform: one uniform of the loaded scene, set per view (rm_render_batch_ex*)."""
    _fields_ = [("name", ctypes.c_char_p), ("components", ctypes.c_int32), ("count", ctypes.c_int32),
                ("values", ctypes.c_void_p)]


class RmPostBatchPlan(ctypes.Structure):
    """include/rm.h struct rm_post_batch_plan."""
    _fields_ = [("per_view_bytes", ctypes.c_int64), ("shared_bytes", ctypes.c_int64),
                ("group_views", ctypes.c_int32), ("groups", ctypes.c_int32), ("scratch_bytes", ctypes.c_int64),
                ("launches", ctypes.c_int32), ("reserved", ctypes.c_int32)]

    def as_dict(self):
        return dict(per_view_bytes=int(self.per_view_bytes), shared_bytes=int(self.shared_bytes),
                    group_views=int(self.group_views), groups=int(self.groups),
                    scratch_bytes=int(self.scratch_bytes), launches=int(self.launches))


POST_BATCH_SCRATCH_DEFAULT = 512 << 20  # include/rm.h RM_POST_BATCH_SCRATCH_DEFAULT

RAY_STATUS = {0: "miss", 1: "hit", 2: "exhausted"}  # include/rm.h RM_RAY_*


class RmShadeParams(ctypes.Structure):
    """include/rm.h rm_shade_params."""
    _fields_ = [("width", ctypes.c_int32), ("output", ctypes.c_int32), ("vignette", ctypes.c_int32)]


RM_SHADE_LINEAR, RM_SHADE_DISPLAY = 0, 1  # include/rm.h
SHADE_OUTPUTS = {"linear": RM_SHADE_LINEAR, "display": RM_SHADE_DISPLAY}


class RmCommId(ctypes.Structure):
    _fields_ = [("internal", ctypes.c_char * 128)]


class RmError(RuntimeError):
    def __init__(self, status, msg):
        super().__init__(f"{STATUS.get(status, status)}: {msg}")
        self.status = status


_LIB = None


def lib() -> ctypes.CDLL:
    """Load librm.so (raises if it is missing: no fallback path exists)."""
    global _LIB
    if _LIB is not None:
        return _LIB
    if not os.path.exists(LIB_PATH):
        raise ImportError(f"{LIB_PATH} not built; run `make -C raymarching_amd` (or __graft_entry__.build())")
    # torch ships its own libamdhip64.so.7: load it first so that librm.so binds
    # to the same HIP runtime (one runtime per process; tensors and streams
    # are then shared).  A process without torch uses /opt/rocm's runtime.
    try:
        import torch  # noqa: F401,PLC0415
    except ImportError:
        pass
    L = ctypes.CDLL(LIB_PATH)
    vp, c = ctypes.c_void_p, ctypes
    cp = c.c_char_p
    sig = {
        "rm_create": ([c.POINTER(vp), c.c_int], c.c_int),
        "rm_destroy": ([vp], c.c_int),
        "rm_load_scene": ([vp, cp], c.c_int),
        "rm_set_uniform1f": ([vp, cp, c.c_float], c.c_int),
        "rm_set_uniform2f": ([vp, cp, c.c_float, c.c_float], c.c_int),
        "rm_set_uniform3f": ([vp, cp, c.c_float, c.c_float, c.c_float], c.c_int),
        "rm_set_uniform4f": ([vp, cp, c.c_float, c.c_float, c.c_float, c.c_float], c.c_int),
        "rm_set_uniform1i": ([vp, cp, c.c_int32], c.c_int),
        "rm_set_uniformfv": ([vp, cp, c.c_int, vp, c.c_int], c.c_int),
        "rm_uniform_count": ([vp, c.POINTER(c.c_int)], c.c_int),
        "rm_uniform_info_at": ([vp, c.c_int, c.POINTER(RmUniformInfo)], c.c_int),
        "rm_get_uniformfv": ([vp, cp, vp, c.c_int, c.POINTER(c.c_int)], c.c_int),
        "rm_get_uniform1i": ([vp, cp, c.POINTER(c.c_int32)], c.c_int),
        "rm_set_params": ([vp, c.POINTER(RmParams)], c.c_int),
        "rm_get_params": ([vp, c.POINTER(RmParams)], c.c_int),
        "rm_set_stream": ([vp, vp], c.c_int),
        "rm_set_stream_kept": ([vp, vp], c.c_int),
        "rm_synchronize": ([vp], c.c_int),
        "rm_render": ([vp, c.c_int, c.c_int, vp, c.POINTER(RmStats)], c.c_int),
        "rm_render_step_map": ([vp, c.c_int, c.c_int, vp, vp, c.POINTER(RmStats)], c.c_int),
        "rm_render_band": ([vp, c.c_int, c.c_int, c.c_int, c.c_int, c.c_int, vp, c.POINTER(RmStats)], c.c_int),
        "rm_render_rows": ([vp, c.c_int, c.c_int, c.c_int, c.c_int, c.c_int, c.c_int, c.c_int, vp,
                            c.POINTER(RmStats)], c.c_int),
        "rm_shard_rows": ([c.c_int, c.c_int, c.c_int, c.c_int, c.POINTER(c.c_int)], c.c_int),
        "rm_deinterleave": ([vp, c.c_int, c.c_int, c.c_int, c.c_int, c.c_int, vp, vp], c.c_int),
        "rm_deinterleave_rgba8": ([vp, c.c_int, c.c_int, c.c_int, c.c_int, c.c_int, vp, vp], c.c_int),
        "rm_pack_rgba8": ([vp, c.c_int64, vp, vp], c.c_int),
        "rm_pack_rgb8": ([vp, c.c_int64, vp, vp], c.c_int),
        "rm_deinterleave_rgb8": ([vp, c.c_int, c.c_int, c.c_int, c.c_int, c.c_int, vp, vp], c.c_int),
        "rm_render_rgba8": ([vp, c.c_int, c.c_int, vp, c.POINTER(RmStats)], c.c_int),
        "rm_render_accumulate": ([vp, c.c_int, c.c_int, vp, c.POINTER(RmStats)], c.c_int),
        "rm_render_accumulate_rgba8": ([vp, c.c_int, c.c_int, vp, c.POINTER(RmStats)], c.c_int),
        "rm_render_band_rgba8": ([vp, c.c_int, c.c_int, c.c_int, c.c_int, c.c_int, vp, c.POINTER(RmStats)],
                                 c.c_int),
        "rm_render_rows_rgba8": ([vp, c.c_int, c.c_int, c.c_int, c.c_int, c.c_int, c.c_int, c.c_int, vp,
                                  c.POINTER(RmStats)], c.c_int),
        "rm_fxaa": ([vp, c.c_int, c.c_int, vp, vp], c.c_int),
        "rm_bloom": ([vp, c.c_int, c.c_int, vp, vp], c.c_int),
        "rm_post_chain": ([vp, c.c_int, c.c_int, vp, vp, vp], c.c_int),
        "rm_post_frag": ([vp, c.c_int, c.c_int, c.c_int, c.c_int, vp, vp], c.c_int),
        "rm_post_chain_ex": ([vp, c.c_int, c.c_int, c.c_int, c.c_int, vp, vp, vp], c.c_int),
        "rm_render_code_hash": ([], cp),
        "rm_render_cycle_rows_wire": ([vp, c.c_int, c.c_int, c.c_int, c.c_int, c.c_int, c.c_int, c.c_int, vp, vp, vp,
                                       c.POINTER(RmStats)], c.c_int),
        "rm_compile_scene": ([cp, vp, c.c_size_t], c.c_int),
        "rm_compile_scene_batch": ([cp, vp, c.c_size_t], c.c_int),
        "rm_compile_scene_aa": ([cp, vp, c.c_size_t], c.c_int),
        "rm_scene_eval": ([vp, vp, c.c_int64, vp, vp], c.c_int),
        "rm_scene_eval_form": ([vp, vp, c.c_int64, c.c_int, vp, vp, vp], c.c_int),
        "rm_cast_rays": ([vp, vp, c.c_int, vp, c.c_int64, c.c_int, c.POINTER(RmRayHits), c.POINTER(RmStats)], c.c_int),
        "rm_camera_rays": ([vp, c.c_int, c.c_int, vp, vp], c.c_int),
        "rm_aa_offsets": ([c.c_int, vp], c.c_int),
        "rm_aa_edge_mask": ([c.c_int, c.c_int, c.c_int, vp, vp], c.c_int),
        "rm_refine_rgba8": ([vp, c.c_int, c.c_int, c.POINTER(RmAaParams), vp, vp, c.POINTER(RmAaStats)], c.c_int),
        "rm_render_aa_rgba8": ([vp, c.c_int, c.c_int, c.POINTER(RmAaParams), vp, vp, c.POINTER(RmAaStats)], c.c_int),
        "rm_refine_ex_rgba8": ([vp, c.c_int, c.c_int, c.POINTER(RmAaParams), vp, vp, c.POINTER(RmAaStats)], c.c_int),
        "rm_render_aa_ex_rgba8": ([vp, c.c_int, c.c_int, c.POINTER(RmAaParams), vp, vp, c.POINTER(RmAaStats)], c.c_int),
        "rm_aa_prepare": ([vp], c.c_int),
        "rm_batch_bytes": ([c.c_int, c.c_int, c.c_int, c.c_int, c.POINTER(c.c_int64), c.POINTER(c.c_int64)], c.c_int),
        "rm_render_batch": ([vp, c.c_int, c.c_int, vp, c.c_int, vp, c.POINTER(RmStats)], c.c_int),
        "rm_render_batch_rgba8": ([vp, c.c_int, c.c_int, vp, c.c_int, vp, c.POINTER(RmStats)], c.c_int),
        "rm_render_batch_ex": ([vp, c.c_int, c.c_int, vp, c.c_int, vp, c.c_int, vp, c.POINTER(RmStats)], c.c_int),
        "rm_render_batch_ex_rgba8": ([vp, c.c_int, c.c_int, vp, c.c_int, vp, c.c_int, vp, c.POINTER(RmStats)], c.c_int),
        "rm_batch_prepare": ([vp], c.c_int),
        "rm_batch_aa_scratch_bytes": ([c.c_int, c.c_int, c.c_int, c.POINTER(c.c_int64)], c.c_int),
        "rm_refine_batch_rgba8": ([vp, c.c_int, c.c_int, vp, c.c_int, c.POINTER(RmAaParams), vp, vp, vp,
                                   c.POINTER(RmAaStats)], c.c_int),
        "rm_render_batch_aa_rgba8": ([vp, c.c_int, c.c_int, vp, c.c_int, c.POINTER(RmAaParams), vp, vp, vp,
                                      c.POINTER(RmAaStats)], c.c_int),
        "rm_post_batch_plan": ([c.c_int, c.c_int, c.c_int, c.c_int64, c.POINTER(RmPostBatchPlan)], c.c_int),
        "rm_set_post_batch_scratch_limit": ([vp, c.c_int64], c.c_int),
        "rm_post_frag_batch": ([vp, c.c_int, c.c_int, c.c_int, c.c_int, c.c_int, vp, vp], c.c_int),
        "rm_bloom_batch": ([vp, c.c_int, c.c_int, c.c_int, vp, vp], c.c_int),
        "rm_post_chain_batch": ([vp, c.c_int, c.c_int, c.c_int, c.c_int, c.c_int, vp, vp, vp], c.c_int),
        "rm_shade_rays": ([vp, vp, c.c_int, vp, c.c_int64, c.POINTER(RmShadeParams), vp, vp, c.POINTER(RmStats)],
                          c.c_int),
        "rm_sharded_layout": ([c.c_int, c.c_int, c.c_int, c.c_int, c.c_int, c.POINTER(RmShardLayout)], c.c_int),
        "rm_comm_get_id": ([c.POINTER(RmCommId)], c.c_int),
        "rm_comm_init_rank": ([c.POINTER(vp), vp, c.c_int, c.POINTER(RmCommId), c.c_int], c.c_int),
        "rm_comm_init_all": ([c.POINTER(vp), c.POINTER(vp), c.c_int], c.c_int),
        "rm_comm_destroy": ([vp], c.c_int),
        "rm_comm_info": ([vp, c.POINTER(c.c_int), c.POINTER(c.c_int), c.POINTER(c.c_int)], c.c_int),
        "rm_render_sharded": ([vp, c.c_int, c.c_int, c.c_int, vp, c.POINTER(RmStats)], c.c_int),
        "rm_render_sharded_all": ([c.POINTER(vp), c.c_int, c.c_int, c.c_int, c.c_int, vp, c.POINTER(RmStats)],
                                  c.c_int),
        "rm_set_tile_order": ([vp, vp, c.c_int64], c.c_int),
        "rm_tile_grid": ([c.POINTER(RmParams), c.c_int, c.c_int, c.POINTER(c.c_int), c.POINTER(c.c_int)], c.c_int),
        "rm_abi_version": ([], c.c_int),
        "rm_resolution_cache_info": ([vp, c.POINTER(c.c_int), c.POINTER(c.c_int)], c.c_int),
        "rm_certified_steps": ([vp, c.POINTER(c.c_uint64)], c.c_int),
        "rm_reflection_cleared_steps": ([vp, c.POINTER(c.c_uint64)], c.c_int),
        "rm_near_sky_steps": ([vp, c.POINTER(c.c_uint64)], c.c_int),
        "rm_cycle_rows": ([c.c_int, c.c_int, c.c_int, c.c_int, c.POINTER(c.c_int)], c.c_int),
        "rm_render_cycle_rows": ([vp, c.c_int, c.c_int, c.c_int, c.c_int, c.c_int, c.c_int, c.c_int, vp,
                                  c.POINTER(RmStats)], c.c_int),
        "rm_render_cycle_rows_rgba8": ([vp, c.c_int, c.c_int, c.c_int, c.c_int, c.c_int, c.c_int, c.c_int, vp,
                                        c.POINTER(RmStats)], c.c_int),
        "rm_deinterleave_cycle_rgb8": ([vp, c.c_int, c.c_int, c.c_int, c.c_int, vp, vp, vp, vp, vp], c.c_int),
        "rm_wire_capacity": ([c.c_int, c.c_int], c.c_int64),
        "rm_wire_workspace_bytes": ([c.c_int, c.c_int], c.c_int64),
        "rm_wire_encode": ([vp, c.c_int, c.c_int, vp, vp, vp, vp], c.c_int),
        "rm_wire_decode": ([vp, c.c_int, c.c_int, c.c_int, c.c_int, c.c_int, c.c_int, vp, vp], c.c_int),
        "rm_scatter_part_rgba8": ([vp, c.c_int, c.c_int, c.c_int, c.c_int, c.c_int, c.c_int, vp, vp], c.c_int),
        "rm_wire_decode_parts": ([vp, c.c_int, c.c_int, c.c_int, c.c_int, vp, vp, vp, vp, vp], c.c_int),
        "rm_render_sharded_runs": ([vp, c.c_int, c.c_int, vp, vp, c.POINTER(RmStats)], c.c_int),
        "rm_render_sharded_runs_all": ([c.POINTER(vp), c.c_int, c.c_int, c.c_int, vp, vp, c.POINTER(RmStats)],
                                       c.c_int),
        "rm_last_error": ([vp], cp),
        "rm_status_string": ([c.c_int], cp),
    }
    for name, (args, res) in sig.items():
        fn = getattr(L, name)
        fn.argtypes = args
        fn.restype = res
    v = L.rm_abi_version()
    if v != ABI_VERSION:  # a stale build: its structs differ from the ones bound here
        raise ImportError(f"{LIB_PATH} has ABI version {v}, this binding expects {ABI_VERSION}; rebuild it")
    _LIB = L
    return L


def check(status: int, ctx=None) -> None:
    if status != RM_OK:
        msg = lib().rm_last_error(ctx).decode() if ctx else ""
        raise RmError(status, msg)
