"""Adaptive supersampling of scene plugins, the parts that need no GPU
(include/rm.h rm_refine_ex_rgba8, rm_compile_scene_aa): the AA
form of every scene under raymarching_amd/scenes/ compiles (hiprtc
cross-compiles for gfx950), an RM_PLUGIN_EVAL_ONLY scene has none, its
translation unit is the frame form's behind one #define, its code object holds
the refine kernel alone, and the ctypes prototypes match the header."""
import ctypes
import glob
import os
import re
import shutil
import subprocess

import pytest

import raymarching_amd as rm
from raymarching_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCENES = sorted(glob.glob(os.path.join(rm.SCENES_DIR, "*.hip")))
OK, INVALID, FILE, SCENE = 0, 1, 2, 3
EVAL_ONLY = ("#define RM_PLUGIN_EVAL_ONLY 1\nSdResult sceneSDF(vec3 p)\n{\n    return SdResult(sphere(vec4(0.0, 3.0, "
             "0.0, 1.0), p), Material(vec3(0.5), vec3(0.0), 1.0, 0.0, 0.0, vec3(0.0), 1.0, vec3(0.0)));\n}\n")


def _compile_aa(path):
    buf = ctypes.create_string_buffer(1 << 16)
    st = rm.lib().rm_compile_scene_aa(str(path).encode(), ctypes.cast(buf, ctypes.c_void_p), len(buf))
    return st, buf.value.decode(errors="replace")


def test_there_are_scenes():
    assert len(SCENES) >= 5


@pytest.mark.parametrize("scene", SCENES, ids=[os.path.basename(s) for s in SCENES])
def test_aa_form_of_every_scene_compiles(scene):
    st, log = _compile_aa(scene)
    assert st == OK, log
    assert rm.compile_scene_aa(scene)[0] is True


def test_compile_scene_aa_contract(tmp_path):
    # an eval-only scene compiles as a frame-form plugin and has no AA form; the log names file and line
    p = tmp_path / "ball.hip"
    p.write_text(EVAL_ONLY)
    assert rm.compile_scene(str(p))[0] is True
    st, log = _compile_aa(p)
    assert st == SCENE and "RM_PLUGIN_EVAL_ONLY" in log and "it has no AA form" in log
    assert re.search(r"rm_plugin_kernels\.h:\d+:", log), log
    assert rm.compile_scene_aa(str(p))[0] is False
    # a missing file
    st, log = _compile_aa(tmp_path / "missing.hip")
    assert st == FILE and "missing.hip" in log
    with pytest.raises(rm.RmError):
        rm.compile_scene_aa(str(tmp_path / "missing.hip"))
    # a syntax error: the diagnostics name the scene's file and the line, as rm_compile_scene's do
    bad = tmp_path / "broken.hip"
    bad.write_text("// a comment line\nSdResult sceneSDF(vec3 p) { return nope; }\n")
    st, log = _compile_aa(bad)
    assert st == SCENE and "nope" in log
    assert re.search(r"broken\.hip:2:", log), log
    # a NULL file name; a NULL log is allowed
    assert rm.lib().rm_compile_scene_aa(None, None, 0) == INVALID
    assert rm.lib().rm_compile_scene_aa(SCENES[0].encode(), None, 0) == OK


REF = "/root/reference"  # build container only, as tests/test_plugin_batch_host.py's test of the same contract


@pytest.mark.skipif(not os.path.isdir(REF), reason="reference tree absent (GPU box)")
def test_built_in_scene_files_need_no_aa_compile(tmp_path, monkeypatch):
    """rm_compile_scene's contract for the reference's own scene files: RM_OK with the compiled-in log"""
    for name in ("output_shader.frag", "common.frag", "template.frag"):
        shutil.copy(os.path.join(REF, name), tmp_path / name)
    monkeypatch.chdir(tmp_path)
    assert _compile_aa("template.frag") == (OK, "compiled-in scene T")
    assert _compile_aa("output_shader.frag") == (OK, "compiled-in scene O")
    assert rm.compile_scene_aa("template.frag") == (True, "compiled-in scene T")


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
def test_aa_form_is_the_frame_form_behind_one_define_and_has_one_kernel(scene, tmp_path, monkeypatch):
    monkeypatch.setenv("RM_PLUGIN_DUMP", str(tmp_path))
    path = os.path.join(rm.SCENES_DIR, scene)
    assert rm.compile_scene(path)[0] and rm.compile_scene_aa(path)[0]
    # the two translation units differ in the one #define at the head
    tu_f, tu_a = (tmp_path / "plugin_tu.hip").read_text(), (tmp_path / "plugin_aa_tu.hip").read_text()
    assert tu_a == "#define RM_PLUGIN_AA 1\n" + tu_f
    # the AA form holds its one kernel, the frame form keeps all of its own and has no refine
    frame, aa = _kernels(tmp_path / "plugin.co"), _kernels(tmp_path / "plugin_aa.co")
    assert list(aa) == ["rm_plugin_aa_refine"]
    assert {"rm_plugin_render", "rm_plugin_render_count", "rm_plugin_shade", "rm_plugin_eval", "rm_plugin_cast"} <= \
        set(frame)
    assert "rm_plugin_aa_refine" not in frame
    f, a = frame["rm_plugin_render"], aa["rm_plugin_aa_refine"]
    print(f"{scene}: frame scratch {f['private_segment_fixed_size']} VGPRs {f['vgpr_count']} SGPRs {f['sgpr_count']}; "
          f"AA scratch {a['private_segment_fixed_size']} VGPRs {a['vgpr_count']} SGPRs {a['sgpr_count']}")
    assert a["max_flat_workgroup_size"] == 64
    # F, the uniform block (output_shader_knobs.hip alone declares uniforms), kshift and three pointers: the
    # frame kernel's head, so that the scene's functions read both at the frame kernel's offsets
    head = f["kernarg_segment_size"] - (8 + 4 + 4 + 8)  # (rm_plugin_render: out, rgba8, padding, evals)
    assert a["kernarg_segment_size"] == head + 4 + 4 + 3 * 8


def test_prototypes_and_header():
    L = rm.lib()
    names = ("rm_refine_ex_rgba8", "rm_render_aa_ex_rgba8", "rm_aa_prepare", "rm_compile_scene_aa")
    header = open(os.path.join(ROOT, "include", "rm.h")).read()
    for name in names:
        assert name in rm.EXPORTS
        fn = getattr(L, name)
        assert fn.restype is ctypes.c_int and fn.argtypes is not None
        assert re.search(rf"^rm_status {name}\(", header, re.M), name
    assert L.rm_refine_ex_rgba8.argtypes == L.rm_refine_rgba8.argtypes
    assert L.rm_render_aa_ex_rgba8.argtypes == L.rm_render_aa_rgba8.argtypes
    assert len(L.rm_aa_prepare.argtypes) == 1 and len(L.rm_compile_scene_aa.argtypes) == 3
    # no existing struct changed
    assert L.rm_abi_version() == 3 == _lib.ABI_VERSION
    for name in ("render_aa_ex", "refine_ex", "aa_prepare"):
        assert hasattr(rm.Renderer, name)
    assert callable(rm.compile_scene_aa)
    # a NULL context is refused before any pointer (junk here) is used
    junk = ctypes.c_void_p(16)
    p = _lib.RmAaParams(4, 32)
    for fn in (L.rm_refine_ex_rgba8, L.rm_render_aa_ex_rgba8):
        assert fn(None, 8, 8, ctypes.byref(p), junk, None, None) == INVALID
    assert L.rm_aa_prepare(None) == INVALID
