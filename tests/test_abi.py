"""The C-ABI library builds for gfx950, loads, and exports every symbol include/splat_hip.h declares.
No compute calls here (there is no GPU in the build container)."""
import ctypes
import os
import re

import pytest

from conftest import ROOT


def _declared_functions():
    txt = open(os.path.join(ROOT, "include", "splat_hip.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    names = re.findall(r"\b((?:sgr|sknn|se3)_[A-Za-z0-9_]+)\s*\(", txt)
    return sorted(set(n for n in names if n.startswith(("sgr_", "sknn_", "se3_"))))


def test_header_symbols_are_exported_and_bound():
    from splat_slam_amd.build import build_native
    from splat_slam_amd import _native as nat
    path = build_native(verbose=False)
    assert os.path.exists(path)
    declared = _declared_functions()
    assert len(declared) >= 20, declared
    h = ctypes.CDLL(path)
    for name in declared:
        assert hasattr(h, name), f"{name} declared in splat_hip.h but not exported by libsplat_hip.so"
        assert name in nat.SIGNATURES, f"{name} has no ctypes signature in splat_slam_amd/_native.py"
    assert sorted(nat.SIGNATURES) == declared
    lib = nat.lib()
    assert lib.sgr_abi_version() == 10
    assert isinstance(nat.last_error(), str)


def test_dropin_cpp_extension_builds_loads_and_links_the_c_abi():
    """diff_gaussian_rasterization/_dgr.so (host-only C++: libtorch autograd nodes + workspace state over the C ABI) builds with g++,
    loads next to libsplat_hip.so and exposes its entry points; the product sources under csrc/ never mention the oracle."""
    from splat_slam_amd.build import build_dropin_ext
    path = build_dropin_ext(verbose=False)
    assert os.path.exists(path)
    import diff_gaussian_rasterization as drg
    ext = drg.native_extension()
    assert ext is not None and ext.abi_version() == 10
    for name in ("try_rasterize", "mapping_loss", "adam_group_step", "densify_stats_views", "saved_block_of", "check_overflow", "stats",
                 "set_capacity", "profile_enable", "profile_read"):
        assert callable(getattr(ext, name)), name
    import subprocess
    needed = subprocess.run(["readelf", "-d", path], capture_output=True, text=True).stdout
    assert "libsplat_hip.so" in needed and "$ORIGIN/../splat_slam_amd/lib" in needed
    src = open(os.path.join(ROOT, "diff_gaussian_rasterization", "csrc", "dgr_native.cpp")).read()
    assert "oracle" not in src


def test_struct_layouts_match_the_header():
    from splat_slam_amd import _native as nat
    # 10 x 4-byte scalars, then 5 pointers (8-aligned) -- see SgrSettings in include/splat_hip.h
    assert ctypes.sizeof(nat.SgrSettings) == 40 + 5 * 8
    assert ctypes.sizeof(nat.SgrInputs) == 7 * 8
    assert ctypes.sizeof(nat.SgrOutputs) == 5 * 8
    assert ctypes.sizeof(nat.SgrWorkspace) == 6 * 8
    assert ctypes.sizeof(nat.SgrGradOutputs) == 2 * 8
    assert ctypes.sizeof(nat.SgrGradInputs) == 9 * 8 + 8 + 3 * 8
    assert ctypes.sizeof(nat.SgrAdamGroup) == 4 * 8 + 8 + 8


def test_workspace_sizes_cover_every_carved_array():
    """sgr_saved_bytes / sgr_scratch_bytes are pure host functions of (N, H, W, capacity): lower bounds that follow from
    the layout described in DESIGN.md section 2 (the tile-major per-pixel state needs whole 8x8 tiles, also for ragged
    image sizes), monotone in every argument."""
    from splat_slam_amd import _native as nat
    lib = nat.lib()
    for (n, h, w, cap) in [(1, 1, 1, 1), (1000, 17, 9, 500), (20000, 320, 640, 40000), (300000, 480, 640, 200000),
                           (300001, 481, 643, 200001)]:
        tiles = ((w + 7) // 8) * ((h + 7) // 8)
        saved, scratch = lib.sgr_saved_bytes(n, h, w, cap), lib.sgr_scratch_bytes(n, h, w, cap)
        # saved: 64-B record + 3 index words per Gaussian, 4 B per pair, (T, last contributor) per pixel of whole tiles
        assert saved >= 64 * n + 12 * n + 4 * cap + 8 * 64 * tiles
        # scratch: forward keys (runs + one bucket of >= 64 entries per tile: 256 since round 6) FOLLOWED by (not aliased with: the fused tile kernel
        # writes partials while other tiles still read their keys) 48-B partials + 64-B records
        assert scratch >= (8 * cap + 8 * 64 * tiles) + (48 * cap + 64 * n)
        assert lib.sgr_saved_bytes(n + 256, h, w, cap) > saved and lib.sgr_saved_bytes(n, h + 8, w, cap) > saved
        assert lib.sgr_saved_bytes(n, h, w, cap + 4096) > saved and lib.sgr_scratch_bytes(n, h, w, cap + 4096) > scratch
        assert saved % 16 == 0 and scratch % 16 == 0


def test_product_path_has_no_cpu_fallback_and_never_imports_the_oracle():
    import torch
    from diff_gaussian_rasterization import GaussianRasterizationSettings, GaussianRasterizer
    s = GaussianRasterizationSettings(8, 8, 1.0, 1.0, torch.zeros(3), 1.0, torch.eye(4), torch.eye(4), torch.eye(4), 0,
                                      torch.zeros(3), False, False)
    r = GaussianRasterizer(s)
    with pytest.raises(RuntimeError, match="GPU tensor"):
        r(means3D=torch.zeros(2, 3), means2D=torch.zeros(2, 3), opacities=torch.ones(2, 1), shs=torch.zeros(2, 1, 3),
          scales=torch.ones(2, 3), rotations=torch.tensor([[1.0, 0, 0, 0]] * 2))
    with pytest.raises(Exception, match="excatly one"):
        r(means3D=torch.zeros(2, 3), means2D=torch.zeros(2, 3), opacities=torch.ones(2, 1))
    for pkg in ("splat_slam_amd", "diff_gaussian_rasterization", "simple_knn", "lietorch"):
        for dirpath, _, files in os.walk(os.path.join(ROOT, pkg)):
            for f in files:
                if f.endswith(".py"):
                    src = open(os.path.join(dirpath, f)).read()
                    assert "import oracle" not in src and "from oracle" not in src, os.path.join(dirpath, f)


# ---- the binding is generated from the header: the reader's model against the compiler, then the reader on small inputs --------------
def _c_decl(t, name):
    """The C declaration of `name` with the model's type t."""
    return f"{'const ' if t.const else ''}{t.base}{'*' if t.pointer else ''} {name}" + ("" if t.array is None else f"[{t.array}]")


def _py_name(name):
    import keyword
    return name + "_" if keyword.iskeyword(name) else name


def test_generated_binding_matches_the_compilers_layouts_and_prototypes(tmp_path):
    """A C program written from the parsed model prints sizeof of every struct, offsetof and sizeof of every field and the value of
    every constant and enumerator; each line is held against the ctypes classes and constants of _native.  The same file declares
    every function again from the model and is compiled as C with warnings as errors: a redeclaration that differs from the header's
    in arity, in a type or in a const does not compile."""
    import subprocess
    from splat_slam_amd import _native as nat
    from splat_slam_amd.build import host_compiler
    model = nat.HEADER
    src = ["#include <stddef.h>", "#include <stdio.h>", '#include "splat_hip.h"']
    for name, (res, args) in model.functions.items():
        params = ", ".join(_c_decl(t, f"a{i}") for i, t in enumerate(args)) or "void"
        src.append(f"{_c_decl(res, name)}({params});")
    src.append("int main(void) {")
    for name in model.constants:
        src.append(f'  printf("const {name} %lld\\n", (long long)({name}));')
    for name, fields in model.structs.items():
        src.append(f'  printf("struct {name} %zu\\n", sizeof({name}));')
        for f, _ in fields:
            src.append(f'  printf("field {name} {f} %zu %zu\\n", offsetof({name}, {f}), sizeof((({name}*)0)->{f}));')
    src += ["  return 0;", "}"]
    c_file, exe = tmp_path / "layout.c", tmp_path / "layout"
    c_file.write_text("\n".join(src) + "\n")
    subprocess.run([host_compiler(), "-x", "c", "-std=c11", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), str(c_file),
                    "-o", str(exe)], check=True)
    lines = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines()

    seen = {"const": 0, "struct": 0, "field": 0}
    for line in lines:
        kind, name, *rest = line.split()
        seen[kind] += 1
        if kind == "const":
            assert getattr(nat, name) == model.constants[name] == int(rest[0]), line
        elif kind == "struct":
            assert ctypes.sizeof(getattr(nat, name)) == int(rest[0]), line
        else:
            desc = getattr(getattr(nat, name), _py_name(rest[0]))
            assert (desc.offset, desc.size) == (int(rest[1]), int(rest[2])), line
    # nothing skipped: by the model's own counts, by the classes' and by a plain count over the header's text
    assert seen == {"const": len(model.constants), "struct": len(model.structs), "field": sum(len(f) for f in model.structs.values())}
    for name, fields in model.structs.items():
        assert [f for f, _ in getattr(nat, name)._fields_] == [_py_name(f) for f, _ in fields], name
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "splat_hip.h")).read(), flags=re.S)
    assert len(model.structs) == len(re.findall(r"\btypedef\s+struct\b", txt)) >= 43
    assert sorted(model.functions) == sorted(nat.SIGNATURES) == _declared_functions()
    defines = re.findall(r"^#define\s+(\w+)[ \t]+\S", txt, flags=re.M)
    assert set(defines) <= set(model.constants) and len(defines) == len(set(defines)) >= 50
    assert nat.SGR_ABI_VERSION == 10


def test_generated_binding_types_pointers_by_their_declaration():
    """Struct pointers keep their type; pointers to scalars and to void are plain addresses unless the header marks them SGR_HOST,
    and a marked field keeps the array assigned to it alive."""
    from splat_slam_amd import _native as nat
    fields = dict(nat.SgrMapRun._fields_)
    assert fields["picks"] is ctypes.POINTER(ctypes.c_int32) and fields["lr0"] is ctypes.POINTER(ctypes.c_float)
    assert fields["pool_exp_row"] is ctypes.POINTER(ctypes.c_int32) and fields["window"] is ctypes.POINTER(nat.SgrMapView)
    assert dict(nat.SgrSettings._fields_)["bg"] is ctypes.c_void_p and dict(nat.SgrWorkspace._fields_)["saved"] is ctypes.c_void_p
    assert dict(nat.SgrVitCall._fields_)["out"] is ctypes.c_void_p * 2
    assert dict(nat.SgrMapStep._fields_)["in_"] is ctypes.POINTER(nat.SgrInputs) and "in_" in dict(nat.SgrRowTensor._fields_)
    run = nat.SgrMapRun()
    run.picks = (ctypes.c_int32 * 3)(4, 5, 6)
    assert run._objects and run.picks[2] == 6
    res, args = nat.SIGNATURES["sgr_query_header"]
    assert res is ctypes.c_int and args == [ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint32), ctypes.c_void_p]
    assert nat.SIGNATURES["sgr_encoder_pack"][1][4:6] == [ctypes.POINTER(ctypes.c_float)] * 2
    assert nat.SIGNATURES["sgr_gaussian_adam_shard"][1][1:4] == [ctypes.POINTER(nat.SgrAdamGroup)] + [ctypes.POINTER(ctypes.c_int64)] * 2
    assert nat.SIGNATURES["sgr_last_error"] == (ctypes.c_char_p, []) and nat.SIGNATURES["sgr_tsdf_bytes"][0] is ctypes.c_size_t
    # the name dicts keep their keys: the internal activations stay out of reach
    assert nat.SGR_UPDATE_ACTS == {"none": 0, "relu": 1, "sigmoid": 2, "tanh": 3} and nat.SGR_ENCODER_LAUNCHES == {0: 17, 1: 32}


def _T(base, const=False, pointer=False, array=None, host=False):
    from splat_slam_amd._cdecl import Type
    return Type(base, const, pointer, array, host)


_ACCEPTED = {
    "comments, include guard, includes, extern C": (
        '/* a block\n * comment */\n#ifndef T_H_\n#define T_H_\n#include <stdint.h>\n#include "other.h"\n#ifdef __cplusplus\nextern "C" {\n#endif\n'
        '#define A 1   /* trailing */\n// a line comment\n#ifdef __cplusplus\n}\n#endif\n#endif /* T_H_ */\n',
        ({"A": 1}, {}, {})),
    "integer defines": (
        "#define A 3\n#define B (5 * 4096)\n#define C (A + B - 1)\n#define D (1 << 4)\n#define E (256 >> A)\n#define F 0x10\n",
        ({"A": 3, "B": 20480, "C": 20482, "D": 16, "E": 32, "F": 16}, {}, {})),
    "enum with negative and implicit values": (
        "typedef enum St {\n  OK = 0,\n  BAD = -1,   /* why */\n  WORSE = -2,\n  NEXT\n} St;\n",
        ({"OK": 0, "BAD": -1, "WORSE": -2, "NEXT": -1}, {}, {})),
    "scalar fields": (
        "typedef struct S {\n  int32_t a;\n  uint8_t b;\n  int64_t c;\n  float d;\n  size_t e;\n  int f;\n  uint64_t g;\n} S;\n",
        ({}, {"S": [("a", _T("int32_t")), ("b", _T("uint8_t")), ("c", _T("int64_t")), ("d", _T("float")), ("e", _T("size_t")),
                    ("f", _T("int")), ("g", _T("uint64_t"))]}, {})),
    "pointer fields": (
        "typedef struct P { int32_t n; } P;\ntypedef struct S {\n  const float* a;\n  int32_t* b;\n  void* c;\n  const void* d;\n  const P* e;\n"
        "  P* f;\n} S;\n",
        ({}, {"P": [("n", _T("int32_t"))],
              "S": [("a", _T("float", True, True)), ("b", _T("int32_t", False, True)), ("c", _T("void", False, True)),
                    ("d", _T("void", True, True)), ("e", _T("P", True, True)), ("f", _T("P", False, True))]}, {})),
    "struct by value": (
        "typedef struct P { int32_t n; } P;\ntypedef struct S { P p; float x; } S;\n",
        ({}, {"P": [("n", _T("int32_t"))], "S": [("p", _T("P")), ("x", _T("float"))]}, {})),
    "fixed arrays": (
        "#define N 14\ntypedef struct P { int32_t n; } P;\ntypedef struct S {\n  P layer[N];\n  float w2c[16];\n  void* out[2];\n  const float* lin[5];\n} S;\n",
        ({"N": 14}, {"P": [("n", _T("int32_t"))],
                     "S": [("layer", _T("P", array=14)), ("w2c", _T("float", array=16)), ("out", _T("void", False, True, 2)),
                           ("lin", _T("float", True, True, 5))]}, {})),
    "several declarators": (
        "typedef struct S {\n  float mean[3], std_[3];\n  int32_t h, w;\n} S;\n",
        ({}, {"S": [("mean", _T("float", array=3)), ("std_", _T("float", array=3)), ("h", _T("int32_t")), ("w", _T("int32_t"))]}, {})),
    "prototypes": (
        "#define K 7\ntypedef struct P { int32_t n; } P;\nint f(void);\nconst char* g(void);\nsize_t h(int32_t a, int64_t b);\n"
        "int q(const void* saved, uint32_t words_host[16], const int64_t row0[5],\n      float ms[K], const P groups[5], const P* in, void* stream);\nvoid r(double* x);\n",
        ({"K": 7}, {"P": [("n", _T("int32_t"))]},
         {"f": (_T("int"), []), "g": (_T("char", True, True), []), "h": (_T("size_t"), [_T("int32_t"), _T("int64_t")]),
          "q": (_T("int"), [_T("void", True, True), _T("uint32_t", array=16), _T("int64_t", True, array=5), _T("float", array=7),
                            _T("P", True, array=5), _T("P", True, True), _T("void", False, True)]),
          "r": (_T("void"), [_T("double", False, True)])})),
    "host marker": (
        "#define SGR_HOST\ntypedef struct S {\n  SGR_HOST const int32_t* picks;\n  const int32_t* dev;\n} S;\n"
        "int f(SGR_HOST int64_t* n_host, SGR_HOST uint32_t words[16], const float* dev);\n",
        ({}, {"S": [("picks", _T("int32_t", True, True, host=True)), ("dev", _T("int32_t", True, True))]},
         {"f": (_T("int"), [_T("int64_t", False, True, host=True), _T("uint32_t", array=16, host=True), _T("float", True, True)])})),
}

# the construct that must be refused stands on line 3
_REJECTED = {
    "unknown type": "#define A 1\n\ntypedef struct S { long a; } S;\n",
    "bit-field": "typedef struct S {\n  int32_t a;\n  int32_t b : 3;\n} S;\n",
    "union": "\n\ntypedef union U { int32_t a; float b; } U;\n",
    "union field": "typedef struct S {\n  int32_t a;\n  union { int32_t b; float c; } u;\n} S;\n",
    "function pointer": "typedef struct S {\n  int32_t a;\n  void (*callback)(int32_t);\n} S;\n",
    "function pointer parameter": "\n\nint f(int (*cb)(void));\n",
    "non-integer define": "#define A 1\n\n#define SCALE 0.5f\n",
    "string define": "\n\n#define NAME \"x\"\n",
    "function-like define": "\n\n#define SQ(x) ((x) * (x))\n",
    "define from an unknown name": "\n\n#define B (A + 1)\n",
    "struct used before it is declared": "typedef struct S {\n  int32_t a;\n  const Later* p;\n} S;\ntypedef struct Later { int32_t n; } Later;\n",
    "struct by value before it is declared": "\n\nint f(Later x);\ntypedef struct Later { int32_t n; } Later;\n",
    "array length from an unknown name": "typedef struct S {\n  int32_t a;\n  float w[N];\n} S;\n",
    "pointer to pointer": "\n\nint f(float** p);\n",
    "host marker on a value": "#define SGR_HOST\n\nint f(SGR_HOST int32_t n);\n",
    "host marker on void": "#define SGR_HOST\n\nint f(SGR_HOST void* p);\n",
    "conditional other than ifdef": "\n\n#if A > 1\n#endif\n",
    "plain typedef": "\n\ntypedef int32_t index_t;\n",
    "stray character": "\n\nint f(int32_t a) { return a ? 1 : 0; }\n",
}


@pytest.mark.parametrize("case", sorted(_ACCEPTED))
def test_reader_accepts(case):
    from splat_slam_amd import _cdecl
    text, (constants, structs, functions) = _ACCEPTED[case]
    got = _cdecl.parse(text, "t.h")
    assert got.constants == constants and list(got.constants) == list(constants)
    assert got.structs == structs and got.functions == functions


@pytest.mark.parametrize("case", sorted(_REJECTED))
def test_reader_refuses_and_names_the_line(case):
    from splat_slam_amd import _cdecl
    with pytest.raises(_cdecl.CDeclError, match=r"^t\.h:3: "):
        _cdecl.parse(_REJECTED[case], "t.h")
