"""View batches of scene plugins, the parts that need no GPU (include/rm.h
rm_render_batch_ex, rm_compile_scene_batch): the batch form of
every scene under raymarching_amd/scenes/ compiles (hiprtc cross-compiles for
gfx950), an RM_PLUGIN_EVAL_ONLY scene has none, the batch kernel's scratch is
no larger than the frame kernel's by the code objects' metadata, the ctypes
prototypes and the header, and the stand-alone program
tests/host/plugin_batch_pack_test.cpp, built with the host compiler under the
address and undefined-behaviour sanitizers from csrc/rm_plugin_batch_pack.h and
rm_uniform_decl.cpp alone (nothing of it is loaded into Python), as
tests/test_uniform_decl_host.py builds its program."""
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
SOURCES = [os.path.join(ROOT, "tests", "host", "plugin_batch_pack_test.cpp"),
           os.path.join(ROOT, "raymarching_amd", "csrc", "rm_uniform_decl.cpp")]
FLAGS = ["-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
SCENES = sorted(glob.glob(os.path.join(rm.SCENES_DIR, "*.hip")))
OK, INVALID, FILE, SCENE = 0, 1, 2, 3
EVAL_ONLY = ("#define RM_PLUGIN_EVAL_ONLY 1\nSdResult sceneSDF(vec3 p)\n{\n    return SdResult(sphere(vec4(0.0, 3.0, "
             "0.0, 1.0), p), Material(vec3(0.5), vec3(0.0), 1.0, 0.0, 0.0, vec3(0.0), 1.0, vec3(0.0)));\n}\n")


def _compile_batch(path):
    buf = ctypes.create_string_buffer(1 << 16)
    st = rm.lib().rm_compile_scene_batch(str(path).encode(), ctypes.cast(buf, ctypes.c_void_p), len(buf))
    return st, buf.value.decode(errors="replace")


def test_there_are_scenes():
    assert len(SCENES) >= 5


@pytest.mark.parametrize("scene", SCENES, ids=[os.path.basename(s) for s in SCENES])
def test_batch_form_of_every_scene_compiles(scene):
    st, log = _compile_batch(scene)
    assert st == OK, log
    assert rm.compile_scene_batch(scene)[0] is True


def test_compile_scene_batch_contract(tmp_path):
    # an eval-only scene compiles as a frame-form plugin and has no batch form
    p = tmp_path / "ball.hip"
    p.write_text(EVAL_ONLY)
    assert rm.compile_scene(str(p))[0] is True
    st, log = _compile_batch(p)
    assert st == SCENE and "RM_PLUGIN_EVAL_ONLY" in log
    assert rm.compile_scene_batch(str(p))[0] is False
    # a missing file
    st, log = _compile_batch(tmp_path / "missing.hip")
    assert st == FILE and "missing.hip" in log
    with pytest.raises(rm.RmError):
        rm.compile_scene_batch(str(tmp_path / "missing.hip"))
    # a scene that does not compile: the diagnostics, as rm_compile_scene gives them
    bad = tmp_path / "broken.hip"
    bad.write_text("SdResult sceneSDF(vec3 p) { return nope; }\n")
    st, log = _compile_batch(bad)
    assert st == SCENE and "nope" in log
    # a NULL file name; a NULL log is allowed
    assert rm.lib().rm_compile_scene_batch(None, None, 0) == INVALID
    assert rm.lib().rm_compile_scene_batch(SCENES[0].encode(), None, 0) == OK


REF = "/root/reference"  # build container only, as tests/test_plugins.py's reload tests


@pytest.mark.skipif(not os.path.isdir(REF), reason="reference tree absent (GPU box)")
def test_built_in_scene_files_need_no_batch_compile(tmp_path, monkeypatch):
    """rm_compile_scene's contract for the reference's own scene files: RM_OK with the compiled-in log"""
    for name in ("output_shader.frag", "common.frag", "template.frag"):
        shutil.copy(os.path.join(REF, name), tmp_path / name)
    monkeypatch.chdir(tmp_path)
    assert _compile_batch("template.frag") == (OK, "compiled-in scene T")
    assert _compile_batch("output_shader.frag") == (OK, "compiled-in scene O")
    assert rm.compile_scene_batch("template.frag") == (True, "compiled-in scene T")


def _kernels(code_object):
    """{kernel name: {key: int}} from the AMDGPU metadata note of a code object"""
    tool = shutil.which("llvm-readelf") or "/opt/rocm/llvm/bin/llvm-readelf"
    txt = subprocess.run([tool, "--notes", str(code_object)], capture_output=True, text=True, check=True).stdout
    out = {}
    for block in re.split(r"\n  - \.agpr_count", txt)[1:]:
        name = re.search(r"\.name:\s+(\S+)", block).group(1)
        out[name] = {k: int(v) for k, v in re.findall(r"\.(\w+):\s+(\d+)\n", block)}
    return out


@pytest.mark.parametrize("scene", ["output_shader.hip", "output_shader_knobs.hip", "metaballs.hip"])
def test_batch_kernel_has_no_more_scratch_than_the_frame_kernel(scene, tmp_path, monkeypatch):
    """The failure csrc/rm_batch.h documents is a view's whole record copied per
    lane (608 bytes of scratch): the batch kernel must read its record in
    place.  The private-segment sizes come from the code objects' metadata."""
    monkeypatch.setenv("RM_PLUGIN_DUMP", str(tmp_path))
    path = os.path.join(rm.SCENES_DIR, scene)
    assert rm.compile_scene(path)[0] and rm.compile_scene_batch(path)[0]
    frame, batch = _kernels(tmp_path / "plugin.co"), _kernels(tmp_path / "plugin_batch.co")
    # the batch form holds its one kernel, the frame form keeps all of its own
    assert list(batch) == ["rm_plugin_render_batch"]
    assert {"rm_plugin_render", "rm_plugin_render_count", "rm_plugin_shade", "rm_plugin_eval", "rm_plugin_cast"} <= \
        set(frame)
    f, b = frame["rm_plugin_render"], batch["rm_plugin_render_batch"]
    print(f"{scene}: frame scratch {f['private_segment_fixed_size']} VGPRs {f['vgpr_count']} SGPRs {f['sgpr_count']}; "
          f"batch scratch {b['private_segment_fixed_size']} VGPRs {b['vgpr_count']} SGPRs {b['sgpr_count']}")
    assert b["private_segment_fixed_size"] <= f["private_segment_fixed_size"]
    assert b["vgpr_spill_count"] <= f["vgpr_spill_count"]
    # the kernel takes the records' pointer, the target and the format: 20 bytes, no record by value
    assert b["kernarg_segment_size"] == 20 and b["max_flat_workgroup_size"] == 64
    # the two translation units differ in the one #define at the head
    tu_f, tu_b = (tmp_path / "plugin_tu.hip").read_text(), (tmp_path / "plugin_batch_tu.hip").read_text()
    assert tu_b == "#define RM_PLUGIN_BATCH 1\n" + tu_f


def test_prototypes_and_header():
    L = rm.lib()
    names = ("rm_render_batch_ex", "rm_render_batch_ex_rgba8", "rm_batch_prepare", "rm_compile_scene_batch")
    header = open(os.path.join(ROOT, "include", "rm.h")).read()
    for name in names:
        assert name in rm.EXPORTS
        fn = getattr(L, name)
        assert fn.restype is ctypes.c_int and fn.argtypes is not None
        assert re.search(rf"^rm_status {name}\(", header, re.M), name
    assert len(L.rm_render_batch_ex.argtypes) == 9 and len(L.rm_render_batch_ex_rgba8.argtypes) == 9
    assert len(L.rm_batch_prepare.argtypes) == 1 and len(L.rm_compile_scene_batch.argtypes) == 3
    assert "typedef struct rm_view_uniform" in header
    # the struct the binding passes: a pointer, two int32, a pointer
    assert ctypes.sizeof(_lib.RmViewUniform) == 24 and _lib.RmViewUniform.values.offset == 16
    # no existing struct changed
    assert L.rm_abi_version() == 3 == _lib.ABI_VERSION
    for name in ("render_batch_ex", "batch_prepare"):
        assert hasattr(rm.Renderer, name)
    # a NULL context is refused before any pointer (junk here) is used
    junk = ctypes.c_void_p(16)
    for fn in (L.rm_render_batch_ex, L.rm_render_batch_ex_rgba8):
        assert fn(None, 8, 8, junk, 1, junk, 1, junk, None) == INVALID
    assert L.rm_batch_prepare(None) == INVALID


def _compiler():
    if shutil.which("g++"):  # (gcc's sanitizer runtimes are shared by default: link them in, as clang does)
        return ["g++", "-static-libasan", "-static-libubsan"]
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    return [hipcc, "-x", "c++"] if os.path.exists(hipcc) else None


def test_packing_under_sanitizers(tmp_path):
    cxx = _compiler()
    if cxx is None:
        pytest.skip("no host C++ compiler (g++ or hipcc)")
    exe = tmp_path / "plugin_batch_pack_test"
    build = subprocess.run(cxx + FLAGS + SOURCES + ["-o", str(exe)], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-4000:]
    run = subprocess.run([str(exe)], cwd=tmp_path, capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, (run.stdout + run.stderr)[-4000:]
    assert "all checks passed" in run.stdout
