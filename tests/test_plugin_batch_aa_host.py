"""Adaptive supersampling of a scene plugin's view batch, the parts that need no
GPU (include/rm.h rm_render_batch_aa_ex_rgba8, rm_compile_scene_batch_aa;
DESIGN.md 2.32): the batch-AA form of every scene under raymarching_amd/scenes/
compiles (hiprtc cross-compiles for gfx950), an RM_PLUGIN_EVAL_ONLY scene has
none, its translation unit is the frame form's behind one #define, its code
object holds the one refine kernel without scratch, the ctypes prototypes match
the header, and the stand-alone program tests/host/plugin_batch_aa_grid_test.cpp
(the rule for the refine's grid), built with the host compiler under the address
and undefined-behaviour sanitizers from csrc/rm_plugin_batch_aa_grid.h alone."""
import ctypes
import glob
import os
import re
import shutil
import subprocess

import pytest

import raymarching_amd as rm
from raymarching_amd import _lib, batch_aa_ex

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCENES = sorted(glob.glob(os.path.join(rm.SCENES_DIR, "*.hip")))
OK, INVALID, FILE, SCENE = 0, 1, 2, 3
EVAL_ONLY = ("#define RM_PLUGIN_EVAL_ONLY 1\nSdResult sceneSDF(vec3 p)\n{\n    return SdResult(sphere(vec4(0.0, 3.0, "
             "0.0, 1.0), p), Material(vec3(0.5), vec3(0.0), 1.0, 0.0, 0.0, vec3(0.0), 1.0, vec3(0.0)));\n}\n")
SOURCES = [os.path.join(ROOT, "tests", "host", "plugin_batch_aa_grid_test.cpp")]
FLAGS = ["-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]


def _compile(path):
    buf = ctypes.create_string_buffer(1 << 16)
    st = rm.lib().rm_compile_scene_batch_aa(str(path).encode(), ctypes.cast(buf, ctypes.c_void_p), len(buf))
    return st, buf.value.decode(errors="replace")


def test_there_are_scenes():
    assert len(SCENES) >= 5


@pytest.mark.parametrize("scene", SCENES, ids=[os.path.basename(s) for s in SCENES])
def test_batch_aa_form_of_every_scene_compiles(scene):
    st, log = _compile(scene)
    assert st == OK, log
    assert batch_aa_ex.compile_scene_batch_aa(scene)[0] is True


def test_compile_scene_batch_aa_contract(tmp_path):
    # an eval-only scene compiles as a frame-form plugin and has no batch-AA form; the log names file and line
    p = tmp_path / "ball.hip"
    p.write_text(EVAL_ONLY)
    assert rm.compile_scene(str(p))[0] is True
    st, log = _compile(p)
    assert st == SCENE and "RM_PLUGIN_EVAL_ONLY" in log and "it has no batch-AA form" in log
    assert re.search(r"rm_plugin_kernels\.h:\d+:", log), log
    assert batch_aa_ex.compile_scene_batch_aa(str(p))[0] is False
    # a missing file
    st, log = _compile(tmp_path / "missing.hip")
    assert st == FILE and "missing.hip" in log
    with pytest.raises(rm.RmError):
        batch_aa_ex.compile_scene_batch_aa(str(tmp_path / "missing.hip"))
    # a syntax error: the diagnostics name the scene's file and the line, as rm_compile_scene's do
    bad = tmp_path / "broken.hip"
    bad.write_text("// a comment line\nSdResult sceneSDF(vec3 p) { return nope; }\n")
    st, log = _compile(bad)
    assert st == SCENE and "nope" in log
    assert re.search(r"broken\.hip:2:", log), log
    # a NULL file name; a NULL log is allowed
    assert rm.lib().rm_compile_scene_batch_aa(None, None, 0) == INVALID
    assert rm.lib().rm_compile_scene_batch_aa(SCENES[0].encode(), None, 0) == OK


REF = "/root/reference"  # build container only, as tests/test_plugin_batch_host.py's test of the same contract


@pytest.mark.skipif(not os.path.isdir(REF), reason="reference tree absent (GPU box)")
def test_built_in_scene_files_need_no_batch_aa_compile(tmp_path, monkeypatch):
    """rm_compile_scene's contract for the reference's own scene files: RM_OK with the compiled-in log"""
    for name in ("output_shader.frag", "common.frag", "template.frag"):
        shutil.copy(os.path.join(REF, name), tmp_path / name)
    monkeypatch.chdir(tmp_path)
    assert _compile("template.frag") == (OK, "compiled-in scene T")
    assert _compile("output_shader.frag") == (OK, "compiled-in scene O")
    assert batch_aa_ex.compile_scene_batch_aa("template.frag") == (True, "compiled-in scene T")


def _kernels(code_object):
    """{kernel name: {key: int}} from the AMDGPU metadata note of a code object (names, not instructions)"""
    tool = shutil.which("llvm-readelf") or "/opt/rocm/llvm/bin/llvm-readelf"
    txt = subprocess.run([tool, "--notes", str(code_object)], capture_output=True, text=True, check=True).stdout
    out = {}
    for block in re.split(r"\n  - \.agpr_count", txt)[1:]:
        name = re.search(r"\.name:\s+(\S+)", block).group(1)
        out[name] = {k: int(v) for k, v in re.findall(r"\.(\w+):\s+(\d+)\n", block)}
    return out


@pytest.mark.parametrize("scene", ["output_shader.hip", "output_shader_knobs.hip", "metaballs.hip"])
def test_batch_aa_form_is_the_frame_form_behind_one_define_and_has_one_kernel(scene, tmp_path, monkeypatch):
    monkeypatch.setenv("RM_PLUGIN_DUMP", str(tmp_path))
    path = os.path.join(rm.SCENES_DIR, scene)
    assert rm.compile_scene(path)[0] and rm.compile_scene_aa(path)[0] and batch_aa_ex.compile_scene_batch_aa(path)[0]
    # the two translation units differ in the one #define at the head
    tu_f, tu_b = (tmp_path / "plugin_tu.hip").read_text(), (tmp_path / "plugin_batch_aa_tu.hip").read_text()
    assert tu_b == "#define RM_PLUGIN_BATCH_AA 1\n" + tu_f
    # the new form holds its one kernel; the frame and AA forms keep theirs and do not have it
    frame, aa = _kernels(tmp_path / "plugin.co"), _kernels(tmp_path / "plugin_aa.co")
    baa = _kernels(tmp_path / "plugin_batch_aa.co")
    assert list(baa) == ["rm_plugin_batch_aa_refine"]
    assert list(aa) == ["rm_plugin_aa_refine"]
    assert {"rm_plugin_render", "rm_plugin_render_count", "rm_plugin_shade", "rm_plugin_eval", "rm_plugin_cast"} <= \
        set(frame)
    assert "rm_plugin_batch_aa_refine" not in frame
    a, b = aa["rm_plugin_aa_refine"], baa["rm_plugin_batch_aa_refine"]
    print(f"{scene}: AA scratch {a['private_segment_fixed_size']} VGPRs {a['vgpr_count']} SGPRs {a['sgpr_count']} "
          f"spills {a['vgpr_spill_count']}/{a['sgpr_spill_count']}; batch-AA scratch {b['private_segment_fixed_size']} "
          f"VGPRs {b['vgpr_count']} SGPRs {b['sgpr_count']} spills {b['vgpr_spill_count']}/{b['sgpr_spill_count']}")
    assert b["max_flat_workgroup_size"] == 64
    # no scratch, and no more VGPR spills than the single frame's refine of the same scene
    assert b["private_segment_fixed_size"] == 0
    assert b["vgpr_spill_count"] <= a["vgpr_spill_count"]
    # records, kshift, counters, cstride, queue, frames (8 + 4 (+4) + 8 + 4 (+4) + 8 + 8 = 48 bytes), then the hidden
    # arguments: no FrameConst (584 bytes) and no uniform block by value, whatever the scene declares
    assert 48 <= b["kernarg_segment_size"] < 584 <= a["kernarg_segment_size"]


def test_prototypes_and_header():
    L = rm.lib()
    names = ("rm_refine_batch_ex_rgba8", "rm_render_batch_aa_ex_rgba8", "rm_batch_aa_prepare",
             "rm_compile_scene_batch_aa")
    header = open(os.path.join(ROOT, "include", "rm.h")).read()
    for name in names:
        assert name in rm.EXPORTS
        fn = getattr(L, name)
        assert fn.restype is ctypes.c_int and fn.argtypes is not None
        assert re.search(rf"^rm_status {name}\(", header, re.M), name
    # the built-in calls' arguments with the list and its length after n
    for ex, plain in ((L.rm_refine_batch_ex_rgba8, L.rm_refine_batch_rgba8),
                      (L.rm_render_batch_aa_ex_rgba8, L.rm_render_batch_aa_rgba8)):
        a = list(plain.argtypes)
        assert list(ex.argtypes) == a[:5] + [ctypes.c_void_p, ctypes.c_int] + a[5:]
    assert len(L.rm_batch_aa_prepare.argtypes) == 1 and len(L.rm_compile_scene_batch_aa.argtypes) == 3
    # no existing struct changed
    assert L.rm_abi_version() == 3 == _lib.ABI_VERSION
    for name in ("render_batch_aa_ex", "refine_batch_ex", "batch_aa_prepare", "compile_scene_batch_aa"):
        assert callable(getattr(batch_aa_ex, name))
    assert rm.batch_aa_ex is batch_aa_ex
    # a NULL context is refused before any pointer (junk here) is used
    junk = ctypes.c_void_p(16)
    p = _lib.RmAaParams(4, 32)
    for fn in (L.rm_refine_batch_ex_rgba8, L.rm_render_batch_aa_ex_rgba8):
        assert fn(None, 8, 8, junk, 2, junk, 1, ctypes.byref(p), junk, None, None, None) == INVALID
    assert L.rm_batch_aa_prepare(None) == INVALID
    # the documented order of the checks is in the header
    doc = header[header.index("rm_refine_batch_ex_rgba8 and rm_render_batch_aa_ex_rgba8 take any scene"):]
    order = ["the size rule", "NULL params", "samples not 2, 4 or 8", "offset is not exactly (0, 0)", "n_uniforms < 0",
             "no scene", "RM_PLUGIN_EVAL_ONLY (RM_ERR_SCENE)", "a built-in scene with n_uniforms > 0", "per entry",
             "n = 0", "mixed host and device", "fails to compile"]
    at = [doc.index(k) for k in order]
    assert at == sorted(at)


def _compiler():
    if shutil.which("g++"):  # (gcc's sanitizer runtimes are shared by default: link them in, as clang does)
        return ["g++", "-static-libasan", "-static-libubsan"]
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    return [hipcc, "-x", "c++"] if os.path.exists(hipcc) else None


def test_grid_rule_under_sanitizers(tmp_path):
    cxx = _compiler()
    if cxx is None:
        pytest.skip("no host C++ compiler (g++ or hipcc)")
    exe = tmp_path / "plugin_batch_aa_grid_test"
    build = subprocess.run(cxx + FLAGS + SOURCES + ["-o", str(exe)], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-4000:]
    run = subprocess.run([str(exe)], cwd=tmp_path, capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, (run.stdout + run.stderr)[-4000:]
    assert "all checks passed" in run.stdout
