"""ctypes binding of librm.so (include/rm.h).

The product path has no CPU fallback: if librm.so is missing or fails to
load, every entry point raises.

Everything here that mirrors the header is checked against it by
tests/test_capi.py: SIGNATURES (every prototype), STRUCTS (every struct the
binding passes) and the name-to-value tables of the header's enums.
"""
from __future__ import annotations

import ctypes
import os

HERE = os.path.dirname(os.path.abspath(__file__))
# RM_LIB may point at an alternative in-tree build (experiments); default librm.so
LIB_PATH = os.environ.get("RM_LIB") or os.path.join(HERE, "librm.so")

# include/rm.h RM_ABI_VERSION: the struct layouts below
ABI_VERSION = 3

# --- enums: each table names the header constants it mirrors -----------------
RM_OK = 0
# rm_status RM_OK, RM_ERR_*: value -> the constant's name (rm_status_string's)
STATUS = {0: "RM_OK", 1: "RM_ERR_INVALID_ARGUMENT", 2: "RM_ERR_FILE", 3: "RM_ERR_SCENE",
          4: "RM_ERR_NO_SCENE", 5: "RM_ERR_DEVICE", 6: "RM_ERR_OUT_OF_MEMORY"}
STATUS_CODES = {v: k for k, v in STATUS.items()}
DISPATCH = {0: "row-major", 1: "explicit", 2: "adaptive"}  # RM_DISPATCH_* (rm_stats.dispatch)
# rm_post_sample RM_POST_SAMPLE_*, rm_tonemap RM_TONEMAP_* (rm_post_frag, rm_post_chain_ex)
POST_SAMPLES = {"fxaa": 0, "texel": 1, "chromatic": 2}
TONEMAPS = {"none": 0, "aces": 1, "reinhard": 2, "jodie": 3, "uncharted2": 4}
UNIFORM_TYPES = {0: "float", 1: "int", 2: "bool"}  # rm_uniform_type RM_UNIFORM_*
RAY_STATUS = {0: "miss", 1: "hit", 2: "exhausted"}  # RM_RAY_*
RM_SHADE_LINEAR, RM_SHADE_DISPLAY = 0, 1  # RM_SHADE_*
SHADE_OUTPUTS = {"linear": RM_SHADE_LINEAR, "display": RM_SHADE_DISPLAY}
SCENE_FORMS = {"exact": 0, "probe": 1, "probe_nb1": 2}  # rm_form RM_FORM_*
# rm_params.kernel and rm_params.schedule have no constants: the numbers of the members' comments
KERNELS = {"auto": 0, "tile16": 1, "tile8": 2, "tile16x4": 3, "persist": 4}
SCHEDULES = {"rowmajor": 0, "adaptive": 1}
POST_BATCH_SCRATCH_DEFAULT = 512 << 20  # RM_POST_BATCH_SCRATCH_DEFAULT


def named(value, table, what):
    """A name of a name-to-value table -> its value (ValueError lists the
    names); anything but a str passes through as it is, for the library (or
    ctypes) to judge."""
    if isinstance(value, str):
        if value not in table:
            raise ValueError(f"{what} must be one of {sorted(table)}, not {value!r}")
        return table[value]
    return value


# --- structs -----------------------------------------------------------------
class _Struct(ctypes.Structure):
    _hidden = ()  # members as_dict leaves out

    def as_dict(self) -> dict:
        return {f[0]: getattr(self, f[0]) for f in self._fields_ if f[0] not in self._hidden}


class RmParams(_Struct):
    _fields_ = [("max_steps", ctypes.c_int32), ("shadow_max_steps", ctypes.c_int32),
                ("count_evals", ctypes.c_int32), ("kernel", ctypes.c_int32), ("schedule", ctypes.c_int32)]


class RmStats(_Struct):
    _fields_ = [("evals", ctypes.c_uint64), ("pixels", ctypes.c_uint64), ("kernel_ms", ctypes.c_float),
                ("scene", ctypes.c_int32), ("flop", ctypes.c_uint64), ("skipped", ctypes.c_uint64),
                ("dispatch", ctypes.c_int32), ("lat_tiles", ctypes.c_int32), ("gather_ms", ctypes.c_float),
                ("deinterleave_ms", ctypes.c_float)]

    def as_dict(self) -> dict:
        d = super().as_dict()
        d["dispatch"] = DISPATCH.get(d["dispatch"], d["dispatch"])
        return d


class RmShardLayout(_Struct):
    _fields_ = [("rows_mine", ctypes.c_int32), ("rows_per_shard", ctypes.c_int32), ("wire_bytes", ctypes.c_int64),
                ("gathered_bytes", ctypes.c_int64)]


class RmUniformInfo(_Struct):
    _fields_ = [("name", ctypes.c_char * 64), ("type", ctypes.c_int32), ("components", ctypes.c_int32),
                ("count", ctypes.c_int32)]


class RmRayHits(_Struct):
    """include/rm.h rm_ray_hits: the outputs of rm_cast_rays (NULL: not written; t is required)."""
    _fields_ = [("t", ctypes.c_void_p), ("status", ctypes.c_void_p), ("steps", ctypes.c_void_p),
                ("position", ctypes.c_void_p), ("normal", ctypes.c_void_p), ("material", ctypes.c_void_p)]


class RmAaParams(_Struct):
    """include/rm.h rm_aa_params."""
    _fields_ = [("samples", ctypes.c_int32), ("threshold", ctypes.c_int32)]


class RmAaStats(_Struct):
    """include/rm.h rm_aa_stats."""
    _fields_ = [("refined", ctypes.c_int64), ("base_ms", ctypes.c_float), ("detect_ms", ctypes.c_float),
                ("refine_ms", ctypes.c_float)]


class RmView(_Struct):
    """include/rm.h rm_view: one view of a batch (rm_render_batch*)."""
    _fields_ = [("pos", ctypes.c_float * 3), ("mouse", ctypes.c_float * 2), ("time", ctypes.c_float),
                ("offset", ctypes.c_float * 2)]


class RmViewUniform(_Struct):
    """include/rm.h rm_view_uniform: one uniform of the loaded scene, set per view (rm_render_batch_ex*)."""
    _fields_ = [("name", ctypes.c_char_p), ("components", ctypes.c_int32), ("count", ctypes.c_int32),
                ("values", ctypes.c_void_p)]


class RmPostBatchPlan(_Struct):
    """include/rm.h struct rm_post_batch_plan."""
    _fields_ = [("per_view_bytes", ctypes.c_int64), ("shared_bytes", ctypes.c_int64),
                ("group_views", ctypes.c_int32), ("groups", ctypes.c_int32), ("scratch_bytes", ctypes.c_int64),
                ("launches", ctypes.c_int32), ("reserved", ctypes.c_int32)]
    _hidden = ("reserved",)


class RmShadeParams(_Struct):
    """include/rm.h rm_shade_params."""
    _fields_ = [("width", ctypes.c_int32), ("output", ctypes.c_int32), ("vignette", ctypes.c_int32)]


class RmCommId(_Struct):
    _fields_ = [("internal", ctypes.c_char * 128)]


# every struct the binding passes, by its C type in include/rm.h
STRUCTS = {"rm_params": RmParams, "rm_stats": RmStats, "rm_shard_layout": RmShardLayout,
           "rm_uniform_info": RmUniformInfo, "rm_ray_hits": RmRayHits, "rm_aa_params": RmAaParams,
           "rm_aa_stats": RmAaStats, "rm_view": RmView, "rm_view_uniform": RmViewUniform,
           "struct rm_post_batch_plan": RmPostBatchPlan, "rm_shade_params": RmShadeParams, "rm_comm_id": RmCommId}


class RmError(RuntimeError):
    def __init__(self, status, msg):
        super().__init__(f"{STATUS.get(status, status)}: {msg}")
        self.status = status


# --- prototypes: every symbol include/rm.h declares -> (argtypes, restype) -----
vp, c = ctypes.c_void_p, ctypes
cp = c.c_char_p
SIGNATURES = {
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
    "rm_refine_batch_ex_rgba8": ([vp, c.c_int, c.c_int, vp, c.c_int, vp, c.c_int, c.POINTER(RmAaParams), vp, vp, vp,
                                  c.POINTER(RmAaStats)], c.c_int),
    "rm_render_batch_aa_ex_rgba8": ([vp, c.c_int, c.c_int, vp, c.c_int, vp, c.c_int, c.POINTER(RmAaParams), vp, vp, vp,
                                     c.POINTER(RmAaStats)], c.c_int),
    "rm_batch_aa_prepare": ([vp], c.c_int),
    "rm_compile_scene_batch_aa": ([cp, vp, c.c_size_t], c.c_int),
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


del vp, c, cp
EXPORTS = tuple(SIGNATURES)

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
    for name, (args, res) in SIGNATURES.items():
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
