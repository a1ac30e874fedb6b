"""`uniform` declarations in a scene plugin's source (include/rm.h,
rm_load_scene; csrc/rm_uniform_decl.cpp): what compiles, what is refused and
with which line, and what is not a declaration at all.  hiprtc needs no GPU;
the GPU side is tests/test_uniforms_gpu.py."""
import os
import re

import pytest

import raymarching_amd as rm

MAT = "Material(vec3(0.5), vec3(0.0), 1.0, 0.0, 0.0, vec3(0.0), 1.0, vec3(0.0))"
SCENE = "SdResult sceneSDF(vec3 p)\n{\n    return SdResult(length(p) - 1.0, " + MAT + ");\n}\n"

ALL_TYPES = (
    "uniform float u_f = 0.75;\n"
    "uniform vec2 u_v2 = vec2(0.5, -1.5);\n"
    "uniform vec3 u_v3 = vec3(0.25);\n"
    "uniform vec4 u_v4 = vec4(1.0, 2.0, 3.0, 0.5);\n"
    "uniform int u_i = 3;\n"
    "uniform bool u_b = true;\n"
    "uniform float u_fs[4];\n"
    "uniform vec2 u_v2s[2];\n"
    "uniform vec3 u_v3s[3];\n"
    "uniform vec4 u_v4s[5];\n"
    "SdResult sceneSDF(vec3 p)\n{\n"
    "    float d = length(p - u_v3) - u_f + u_v2.x * u_v2.y + u_fs[1];\n"
    "    for (int i = 0; i < u_i; i++)\n"
    "        d = min(d, length(p - u_v4s[i].xyz) - u_v4s[i].w + u_v2s[i & 1].y + u_v3s[i].z);\n"
    "    if (u_b) d = max(d, -sphere(u_v4, p));\n"
    "    return SdResult(d, " + MAT + ");\n}\n")


def _compile(tmp_path, text, name="scene.hip"):
    p = tmp_path / name
    p.write_text(text)
    return rm.compile_scene(str(p))


@pytest.mark.parametrize("name", ["output_shader_knobs.hip", "metaballs.hip"])
def test_example_scene_with_uniforms_compiles(name):
    ok, log = rm.compile_scene(os.path.join(rm.SCENES_DIR, name))
    assert ok, log


def test_every_uniform_type_compiles(tmp_path):
    ok, log = _compile(tmp_path, ALL_TYPES)
    assert ok, log


REFUSED = {
    "expression_initialiser": ("uniform float u_k = 1.0 + 2.0;\n", 2),
    "call_initialiser": ("uniform float u_k = radians(90.0);\n", 2),
    "several_names": ("uniform float u_a, u_b;\n", 2),
    "sampler2D": ("uniform sampler2D u_tex;\n", 2),
    "int_array": ("uniform int u_n[4];\n", 2),
    "bool_array": ("uniform bool u_n[4];\n", 2),
    "array_of_none": ("uniform float u_a[0];\n", 2),
    "array_of_65": ("uniform float u_a[65];\n", 2),
    "array_initialiser": ("uniform float u_a[2] = 1.0;\n", 2),
    "wrong_literal_count": ("uniform vec3 u_a = vec3(1.0, 2.0);\n", 2),
    "65_slots": ("uniform vec4 u_a[64];\nuniform float u_one_more;\n", 3),
    "65_slots_one_by_one": ("".join(f"uniform float u_{i};\n" for i in range(65)), 66),
    "declared_twice": ("uniform float u_a;\nuniform vec2 u_a;\n", 3),
    "long_name": ("uniform float " + "n" * 64 + ";\n", 2),
    "no_semicolon": ("uniform float u_a\n", 2),
}


@pytest.mark.parametrize("case", sorted(REFUSED))
def test_declaration_outside_the_dialect_is_refused_with_its_line(tmp_path, case):
    decl, line = REFUSED[case]
    ok, log = _compile(tmp_path, "// a scene\n" + decl + SCENE, "refused.hip")
    assert not ok
    assert f"refused.hip:{line}:" in log, log


@pytest.mark.parametrize("name", ["u_resolution", "u_pos", "u_mouse", "u_time", "u_sample", "u_sample_part",
                                  "u_seed1", "u_seed2"])
def test_pass_uniform_cannot_be_declared(tmp_path, name):
    ok, log = _compile(tmp_path, f"\n\nuniform vec2 {name};\n" + SCENE, "pass.hip")
    assert not ok
    assert "pass.hip:3:" in log and "pass" in log and name in log, log


def test_compile_error_after_declarations_keeps_its_line(tmp_path):
    text = ("uniform float u_a = 2.0;\nuniform vec4 u_b =\n    vec4(1.5);\n"
            "SdResult sceneSDF(vec3 p) { return SdResult(u_a, undefined_material); }\n")
    ok, log = _compile(tmp_path, text, "broken.hip")
    assert not ok
    assert "broken.hip:4" in log, log
    assert "broken.hip:3" not in log and "broken.hip:5" not in log, log


def test_uniform_elsewhere_is_not_a_declaration(tmp_path):
    text = ("// uniform float u_in_a_comment = sin(1.0);\n"
            "/* uniform sampler2D u_in_a_block;\n   uniform float a, b; */\n"
            "const float uniformity = 0.5;\n"
            "float last_uniform(float x) { return x * uniformity; }\n"
            "const char* kNote = \"uniform float u_in_a_string = 1.0 + 2.0;\";\n"
            "uniform float u_real = 1.5;\n" + SCENE.replace("- 1.0", "- last_uniform(u_real)"))
    ok, log = _compile(tmp_path, text)
    assert ok, log
    # inside a function body the word is left to the compiler, which has no such keyword
    body = "SdResult sceneSDF(vec3 p)\n{\n    uniform float r = 1.0;\n    return SdResult(length(p) - r, " + MAT + ");\n}\n"
    ok, log = _compile(tmp_path, body, "body.hip")
    assert not ok
    assert "body.hip:3" in log and "error: " in log, log


def test_writing_to_a_uniform_does_not_compile(tmp_path):
    for stmt in ("u_r = 2.0;", "u_c.x = 2.0;", "u_rs[1] = 2.0;"):
        text = ("uniform float u_r = 1.0;\nuniform vec4 u_c;\nuniform float u_rs[2];\n"
                "SdResult sceneSDF(vec3 p)\n{\n    " + stmt + "\n    return SdResult(length(p) - u_r - u_c.x - u_rs[0], "
                + MAT + ");\n}\n")
        ok, log = _compile(tmp_path, text, "write.hip")
        assert not ok, stmt
        assert "write.hip:6" in log, log


REF = "/root/reference"  # build container only; this test skips elsewhere
needs_ref = pytest.mark.skipif(not os.path.isdir(REF), reason="reference tree absent (GPU box)")


@needs_ref
def test_reference_scene_part_with_a_uniform_compiles_as_a_plugin(tmp_path, monkeypatch):
    """The reference's workflow, with a uniform of the user's own: add
    `uniform float u_lift = 2.0;` to output_shader.frag's scene part, use it
    as the sphere's height, reload."""
    src = open(os.path.join(REF, "output_shader.frag")).read()
    k = src.index("\n", src.index("#include")) + 1
    # the sphere of sceneSDF: the second component of its vec4 is its height
    head, n = re.subn(r"(sphere\(vec4\([^,()]+,)[^,()]+,", r"\1 u_lift,", src[k:], count=1)
    assert n == 1
    src = src[:k] + "uniform float u_lift = 2.0;\n" + head
    (tmp_path / "output_shader.frag").write_text(src)
    (tmp_path / "common.frag").write_text(open(os.path.join(REF, "common.frag")).read())
    monkeypatch.chdir(tmp_path)
    ok, log = rm.compile_scene("output_shader.frag")
    assert ok, log
    assert "compiled-in" not in log
