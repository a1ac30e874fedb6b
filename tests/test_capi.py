"""The C-ABI library (no GPU compute): it loads, exports every symbol
include/rm.h declares, and its host-side logic behaves."""
import os
import re
import subprocess

import pytest

import raymarching_amd as rm
from raymarching_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header_symbols():
    txt = open(os.path.join(ROOT, "include", "rm.h")).read()
    return sorted(set(re.findall(r"^\s*(?:const\s+)?\w+\s*\*?\s*(rm_\w+)\s*\(", txt, re.M)))


def test_header_declares_the_binding():
    assert header_symbols() == sorted(_lib.EXPORTS)


def test_library_exports_every_header_symbol():
    out = subprocess.run(["nm", "-D", "--defined-only", rm.LIB_PATH], capture_output=True, text=True, check=True)
    exported = set(re.findall(r"\sT\s(rm_\w+)$", out.stdout, re.M))
    missing = set(header_symbols()) - exported
    assert not missing, missing
    L = rm.lib()
    for s in header_symbols():
        assert getattr(L, s) is not None


def test_library_has_gfx950_code_object():
    data = open(rm.LIB_PATH, "rb").read()
    assert b"amdgcn-amd-amdhsa--gfx950" in data


def test_status_strings():
    L = rm.lib()
    assert L.rm_status_string(0) == b"RM_OK"
    assert L.rm_status_string(2) == b"RM_ERR_FILE"


@pytest.mark.parametrize("H,band,n", [(4096, 16, 8), (1080, 16, 8), (1080, 27, 8), (100, 7, 3), (5, 16, 4),
                                      (8192, 16, 1), (17, 1, 17)])
def test_shard_rows_partition_the_frame(H, band, n):
    counts = [rm.shard_rows(H, band, n, s) for s in range(n)]
    assert sum(counts) == H
    # the bands are dealt round robin, so every shard owns the rows
    # {y : (y // band) % n == s}
    for s in range(n):
        assert counts[s] == sum(1 for y in range(H) if (y // band) % n == s)


def test_shard_rows_rejects_bad_arguments():
    with pytest.raises(rm.RmError):
        rm.shard_rows(0, 16, 8, 0)
    with pytest.raises(rm.RmError):
        rm.shard_rows(16, 16, 8, 8)


def test_no_gpu_means_no_context():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    with pytest.raises(rm.RmError) as e:
        rm.Renderer(0)
    assert e.value.status == 5  # RM_ERR_DEVICE: no silent CPU fallback


def test_abi_version_matches_header_and_binding():
    """include/rm.h RM_ABI_VERSION, librm.so's rm_abi_version() and the ctypes
    structs of _lib.py describe the same layout (a stale build is refused)."""
    import ctypes
    txt = open(os.path.join(ROOT, "include", "rm.h")).read()
    v = int(re.search(r"#define RM_ABI_VERSION (\d+)", txt).group(1))
    assert v == _lib.ABI_VERSION == rm.lib().rm_abi_version()
    # rm_stats: 5 x 8-byte counters/ids + kernel_ms, dispatch, lat_tiles, gather_ms, deinterleave_ms
    assert ctypes.sizeof(_lib.RmStats) == 56
    assert [f[0] for f in _lib.RmStats._fields_][-4:] == ["dispatch", "lat_tiles", "gather_ms", "deinterleave_ms"]


def test_c_struct_layout_matches_binding(tmp_path):
    """The C compiler's rm_stats / rm_params layout is the one _lib.py binds."""
    import ctypes
    src = tmp_path / "layout.c"
    src.write_text('#include "rm.h"\n#include <stddef.h>\n'
                   f'_Static_assert(sizeof(rm_stats) == {ctypes.sizeof(_lib.RmStats)}, "rm_stats");\n'
                   f'_Static_assert(offsetof(rm_stats, dispatch) == {_lib.RmStats.dispatch.offset}, "dispatch");\n'
                   f'_Static_assert(offsetof(rm_stats, deinterleave_ms) == {_lib.RmStats.deinterleave_ms.offset}, "d");\n'
                   f'_Static_assert(sizeof(rm_params) == {ctypes.sizeof(_lib.RmParams)}, "rm_params");\n')
    subprocess.run(["gcc", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)], check=True)


# --- the whole binding against include/rm.h: every prototype, struct and enum table ---------------------

def header_text(strip=True):
    txt = open(os.path.join(ROOT, "include", "rm.h")).read()
    if strip:  # comments, then preprocessor lines
        txt = re.sub(r"/\*.*?\*/", " ", txt, flags=re.S)
        txt = re.sub(r"^\s*#.*$", "", txt, flags=re.M)
    return txt


SCALAR_CLASS = {"int": "i4", "int32_t": "i4", "uint32_t": "i4", "rm_status": "i4", "int64_t": "i8", "uint64_t": "i8",
                "size_t": "i8", "float": "f4"}


def c_param(text):
    """A C parameter or return type -> (base type, number of *): 'const rm_view *views' -> ('rm_view', 1)."""
    stars = text.count("*")
    words = [w for w in text.replace("*", " ").split() if w != "const"]
    return " ".join(words), stars


def header_prototypes():
    """name -> (return (base, stars), [parameter (base, stars)]) of every function rm.h declares."""
    protos = {}
    for ret, name, params in re.findall(r"(?:^|[;}])\s*((?:const\s+)?\w+\s*\*?)\s*(rm_\w+)\s*\(([^()]*)\)\s*(?=;)",
                                        header_text(), re.M):
        plist = [] if params.strip() == "void" else [p.strip() for p in params.split(",")]
        # a parameter's last word is its name; the rest is its type
        protos[name] = (c_param(ret), [c_param(re.sub(r"\w+$", "", p)) for p in plist])
    return protos


def abi_class(c_type, what):
    """The ABI class of a header type: ptr, i4 (4-byte integer or enum), i8, f4.  Unknown: a failure."""
    base, stars = c_type
    if stars:
        return "ptr"
    assert base in SCALAR_CLASS, f"{what}: the classifier does not know the C type {base!r}"
    return SCALAR_CLASS[base]


def ctypes_class(t, what):
    import ctypes
    if t in (ctypes.c_void_p, ctypes.c_char_p) or issubclass(t, ctypes._Pointer):
        return "ptr"
    known = {ctypes.c_int: "i4", ctypes.c_int32: "i4", ctypes.c_uint32: "i4", ctypes.c_int64: "i8",
             ctypes.c_uint64: "i8", ctypes.c_size_t: "i8", ctypes.c_float: "f4"}
    assert t in known, f"{what}: the classifier does not know the ctypes type {t!r}"
    return known[t]


def test_signature_table_is_the_headers_prototypes():
    """Every entry of _lib.SIGNATURES against its prototype in rm.h: the parameter count, each parameter's and
    the return type's ABI class, and what a typed POINTER points to (a struct of _lib.STRUCTS by its C name, a
    scalar of the same class, or another pointer)."""
    import ctypes
    protos = header_prototypes()
    assert sorted(protos) == header_symbols() == sorted(_lib.SIGNATURES) and len(protos) == len(_lib.SIGNATURES)
    c_name = {cls: name for name, cls in _lib.STRUCTS.items()}
    assert len(c_name) == len(_lib.STRUCTS)
    for name, (argtypes, restype) in _lib.SIGNATURES.items():
        ret, params = protos[name]
        assert len(argtypes) == len(params), f"{name}: {len(argtypes)} argtypes for {len(params)} parameters"
        if restype is ctypes.c_char_p:
            assert ret == ("char", 1), name
        else:
            assert ctypes_class(restype, name) == abi_class(ret, name) and ret[0] in ("rm_status", "int", "int64_t"), name
        for i, (t, p) in enumerate(zip(argtypes, params)):
            what = f"{name} parameter {i} ({' '.join(p[0].split())}{'*' * p[1]})"
            assert ctypes_class(t, what) == abi_class(p, what), what
            if issubclass(t, ctypes._Pointer):
                to = t._type_
                if to in c_name:
                    assert p == (c_name[to], 1), f"{what}: bound as a pointer to {c_name[to]}"
                elif to is ctypes.c_void_p:
                    assert p[1] == 2, what
                else:
                    assert p[1] == 1 and ctypes_class(to, what) == abi_class((p[0], 0), what), what


def _compile_asserts(tmp_path, lines):
    src = tmp_path / "asserts.c"
    src.write_text('#include "rm.h"\n#include <stddef.h>\n' + "".join(
        f'_Static_assert({cond}, "{cond}");\n' for cond in lines))
    done = subprocess.run(["gcc", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)],
                          capture_output=True, text=True)
    assert done.returncode == 0, done.stderr


def test_every_bound_struct_has_the_c_layout(tmp_path):
    """sizeof of every struct of _lib.STRUCTS, and offsetof and the size of every field, by the C compiler."""
    import ctypes
    assert set(_lib.STRUCTS.values()) == {v for v in vars(_lib).values() if isinstance(v, type)
                                          and issubclass(v, ctypes.Structure) and hasattr(v, "_fields_")}
    lines = []
    for c_name, cls in _lib.STRUCTS.items():
        lines.append(f"sizeof({c_name}) == {ctypes.sizeof(cls)}")
        for field, *_ in cls._fields_:
            d = getattr(cls, field)
            lines += [f"offsetof({c_name}, {field}) == {d.offset}", f"sizeof((({c_name} *)0)->{field}) == {d.size}"]
    _compile_asserts(tmp_path, lines)


# table key -> the header constant it stands for, per table of _lib.py
ENUM_TABLES = [
    ("RM_DISPATCH_", {v: k for k, v in _lib.DISPATCH.items()},
     {"row-major": "RM_DISPATCH_ROW_MAJOR", "explicit": "RM_DISPATCH_EXPLICIT", "adaptive": "RM_DISPATCH_ADAPTIVE"}),
    ("RM_POST_SAMPLE_", _lib.POST_SAMPLES,
     {"fxaa": "RM_POST_SAMPLE_FXAA", "texel": "RM_POST_SAMPLE_TEXEL", "chromatic": "RM_POST_SAMPLE_CHROMATIC"}),
    ("RM_TONEMAP_", _lib.TONEMAPS,
     {"none": "RM_TONEMAP_NONE", "aces": "RM_TONEMAP_ACES", "reinhard": "RM_TONEMAP_REINHARD",
      "jodie": "RM_TONEMAP_REINHARD_JODIE", "uncharted2": "RM_TONEMAP_UNCHARTED2"}),
    ("RM_UNIFORM_", {v: k for k, v in _lib.UNIFORM_TYPES.items()},
     {"float": "RM_UNIFORM_FLOAT", "int": "RM_UNIFORM_INT", "bool": "RM_UNIFORM_BOOL"}),
    ("RM_RAY_", {v: k for k, v in _lib.RAY_STATUS.items()},
     {"miss": "RM_RAY_MISS", "hit": "RM_RAY_HIT", "exhausted": "RM_RAY_EXHAUSTED"}),
    ("RM_SHADE_", _lib.SHADE_OUTPUTS, {"linear": "RM_SHADE_LINEAR", "display": "RM_SHADE_DISPLAY"}),
    ("RM_FORM_", _lib.SCENE_FORMS,
     {"exact": "RM_FORM_EXACT", "probe": "RM_FORM_PROBE", "probe_nb1": "RM_FORM_PROBE_NB1"}),
    # rm_status: the table's names are the constants themselves
    ("RM_ERR_", {k: v for k, v in _lib.STATUS_CODES.items() if k != "RM_OK"},
     {k: k for k in _lib.STATUS_CODES if k != "RM_OK"}),
]


def test_every_enum_table_has_the_headers_values(tmp_path):
    """RM_... == value for every entry of every name-to-value table of _lib.py, by the C compiler; and each
    table names every constant the header has with its prefix."""
    txt = header_text()
    lines = [f"RM_OK == {_lib.RM_OK}", f"RM_OK == {_lib.STATUS_CODES['RM_OK']}",
             f"RM_ABI_VERSION == {_lib.ABI_VERSION}",
             f"RM_POST_BATCH_SCRATCH_DEFAULT == {_lib.POST_BATCH_SCRATCH_DEFAULT}",
             f"RM_SHADE_LINEAR == {_lib.RM_SHADE_LINEAR}", f"RM_SHADE_DISPLAY == {_lib.RM_SHADE_DISPLAY}"]
    for prefix, table, constant in ENUM_TABLES:
        assert set(table) == set(constant), prefix
        assert set(constant.values()) == set(re.findall(rf"\b{prefix}\w+", txt)), prefix
        lines += [f"{constant[key]} == {value}" for key, value in table.items()]
    _compile_asserts(tmp_path, lines)
    assert rm.Renderer.SCENE_FORMS is _lib.SCENE_FORMS


def test_kernel_and_schedule_names_are_the_comments_numbers():
    """rm_params.kernel and rm_params.schedule have no constants in rm.h: their numbers are literals in the
    members' comments.  Asserted by hand: each name's number, and that the comment still says that number's
    phrase."""
    params = re.search(r"typedef struct rm_params \{(.*?)\} rm_params;", header_text(strip=False), re.S).group(1)
    comment = {m.group(1): " ".join(m.group(2).split())
               for m in re.finditer(r"int32_t (\w+);\s*/\*(.*?)\*/", params, re.S)}
    for name, number, phrase in (("auto", 0, "0 auto (= 2)"), ("tile16", 1, "1 16x16 px (4 waves)"),
                                 ("tile8", 2, "2 8x8 px (1 wave)"), ("tile16x4", 3, "3 16x4 px (1 wave)"),
                                 ("persist", 4, "4 8x8 px tiles pulled by persistent waves")):
        assert _lib.KERNELS[name] == number and phrase in comment["kernel"], name
    assert len(_lib.KERNELS) == 5
    for name, number, phrase in (("adaptive", 1, "1 (default) = the costliest tiles"), ("rowmajor", 0, "0 = row-major")):
        assert _lib.SCHEDULES[name] == number and phrase in comment["schedule"], name
    assert len(_lib.SCHEDULES) == 2
