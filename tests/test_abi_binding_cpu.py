"""The ctypes binding is derived from include/mvkpconv.h by _lib.parse_header; here the host C++ compiler referees
what the parser read: every prototype and field type through static_assert on the real header, every struct layout
and integer #define through a small program, and the parser's strictness on synthetic headers. CPU only."""
import ctypes
import os
import re
import shutil
import subprocess

import pytest

import mvkpconv

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")
L = mvkpconv.sub("_lib")


def host_compiler():
    """The host clang of the ROCm install build.py compiles with, else the system's c++. None is a test failure."""
    hipcc = shutil.which(mvkpconv.sub("build")._hipcc())
    found = []
    if hipcc:
        rocm = os.path.dirname(os.path.dirname(os.path.realpath(hipcc)))
        found = [p for p in (os.path.join(rocm, "llvm", "bin", "clang++"), os.path.join(rocm, "lib", "llvm", "bin", "clang++"))
                 if os.path.exists(p)]
    cxx = (found + [shutil.which("c++")])[0]
    assert cxx, "no host C++ compiler: neither the ROCm install's clang++ nor c++"
    return cxx


def prototype_asserts(functions, structs):
    """One translation unit over the real header: the compiler's own reading of every declaration against the parser's."""
    lines = ["#include <type_traits>", '#include "mvkpconv.h"']
    for name, (ret, params) in functions.items():
        lines.append('static_assert(std::is_same<decltype(&%s), %s (*)(%s)>::value, "%s");'
                     % (name, ret, ", ".join(t for t, _ in params), name))
    for name, fields in structs.items():
        for t, f in fields:
            lines.append('static_assert(std::is_same<decltype(%s::%s), %s>::value, "%s.%s");' % (name, f, t, name, f))
    return "\n".join(lines) + "\n"


def syntax_check(tmp_path, source):
    src = tmp_path / "abi_prototypes.cpp"
    src.write_text(source)
    return subprocess.run([host_compiler(), "-std=c++17", "-fsyntax-only", "-I", INCLUDE, str(src)],
                          capture_output=True, text=True)


def test_compiler_confirms_every_prototype_and_field_type(tmp_path):
    assert len(L.FUNCTIONS) == len(L.EXPORTS) == 133 and len(L.STRUCTS) == 6
    r = syntax_check(tmp_path, prototype_asserts(L.FUNCTIONS, L.STRUCTS))
    assert r.returncode == 0, r.stderr[-4000:]


def test_compiler_rejects_a_wrong_width_a_dropped_argument_and_a_swapped_field(tmp_path):
    """The referee has teeth: the three drifts a hand-written table could carry silently each fail the compile."""
    ret, params = L.FUNCTIONS["mvk_gemm_f32"]
    assert params[3] == ("int64_t", "M")
    narrowed = dict(L.FUNCTIONS, mvk_gemm_f32=(ret, params[:3] + (("int", "M"),) + params[4:]))
    dropped = dict(L.FUNCTIONS, mvk_gemm_f32=(ret, params[:-2] + params[-1:]))
    fields = L.STRUCTS["mvk_rev_list"]
    swapped = dict(L.STRUCTS, mvk_rev_list=fields[:3] + ((fields[3][0], fields[4][1]), (fields[4][0], fields[3][1])) + fields[5:])
    for functions, structs, label in ((narrowed, L.STRUCTS, '"mvk_gemm_f32"'), (dropped, L.STRUCTS, '"mvk_gemm_f32"'),
                                      (L.FUNCTIONS, swapped, '"mvk_rev_list.width"')):
        r = syntax_check(tmp_path, prototype_asserts(functions, structs))
        assert r.returncode != 0 and label in r.stderr, (label, r.stderr[-2000:])


@pytest.fixture(scope="module")
def compiled_layout(tmp_path_factory):
    """{line label: value} printed by a program built from the real header: sizeof and offsetof of every struct with the
    field names the parser read, and the value of every MVK_* #define an independent regular expression finds."""
    header = open(os.path.join(INCLUDE, "mvkpconv.h")).read()
    defines = re.findall(r"^[ \t]*#[ \t]*define[ \t]+(MVK_\w+)[ \t]+\S", header, re.M)
    body = []
    for name, fields in L.STRUCTS.items():
        body.append('  std::printf("sizeof %s %%zu\\n", sizeof(%s));' % (name, name))
        body += ['  std::printf("offsetof %s.%s %%zu\\n", offsetof(%s, %s));' % (name, f, name, f) for _, f in fields]
    body += ['  std::printf("define %s %%lld\\n", (long long)(%s));' % (d, d) for d in defines]
    d = tmp_path_factory.mktemp("abi_layout")
    src, exe = d / "layout.cpp", d / "layout"
    src.write_text('#include <cstddef>\n#include <cstdio>\n#include "mvkpconv.h"\nint main() {\n%s\n  return 0;\n}\n' % "\n".join(body))
    subprocess.run([host_compiler(), "-std=c++17", "-I", INCLUDE, str(src), "-o", str(exe)], check=True,
                   capture_output=True, text=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout
    return {" ".join(line.split()[:-1]): int(line.split()[-1]) for line in out.splitlines()}


def test_struct_layouts_match_the_compiler(compiled_layout):
    classes = {"mvk_bn_fwd_problem": L.BnFwdProblem, "mvk_bn_bwd_problem": L.BnBwdProblem, "mvk_rev_list": L.RevList,
               "mvk_reg_layer": L.RegLayer, "mvk_bn_finish": L.BnFinish, "mvk_a_transform": L.ATransform}
    assert set(classes) == set(L.STRUCTS)
    checked = 0
    for name, cls in classes.items():
        assert issubclass(cls, ctypes.Structure)
        assert [f for f, _ in cls._fields_] == [f for _, f in L.STRUCTS[name]]
        assert ctypes.sizeof(cls) == compiled_layout["sizeof " + name], name
        for _, f in L.STRUCTS[name]:
            assert getattr(cls, f).offset == compiled_layout["offsetof %s.%s" % (name, f)], (name, f)
            checked += 1
    assert checked == sum(len(f) for f in L.STRUCTS.values()) == 64
    assert ctypes.sizeof(L.BnFwdProblem) == 144 and L.BnFwdProblem.ext_rows.offset == 136 and ctypes.sizeof(L.RegLayer) == 64


def test_constants_match_the_compiler_and_the_library(compiled_layout):
    compiled = {k.split()[1]: v for k, v in compiled_layout.items() if k.startswith("define ")}
    assert compiled == L.CONSTANTS and len(compiled) == 9
    assert L.ABI_VERSION == L.CONSTANTS["MVK_ABI_VERSION"] == L.lib().mvk_abi_version()
    ops = mvkpconv.sub("ops")
    assert (ops.REG_MANY, ops.REV_MANY, ops.REV_MAX_WIDTH) == (compiled["MVK_REG_MANY"], compiled["MVK_REV_MANY"],
                                                               compiled["MVK_REV_MAX_WIDTH"]) == (16, 12, 8192)
    assert ops.INFLUENCE == {"constant": 0, "linear": 1, "gaussian": 2} and ops.AGGREGATION == {"sum": 0, "closest": 1}


def test_type_mapping():
    used = {t for ret, params in L.FUNCTIONS.values() for t in (ret,) + tuple(p for p, _ in params)}
    used |= {t for fields in L.STRUCTS.values() for t, _ in fields}
    assert all(t in L.CTYPES or t.endswith("*") for t in used), sorted(used)
    assert {t for t in used if not t.endswith("*")} == {"int", "int32_t", "int64_t", "float", "double"}
    size = {t: ctypes.sizeof(c) for t, c in L.CTYPES.items()}
    assert (size["int64_t"], size["int"], size["int32_t"], size["float"], size["double"]) == (8, 4, 4, 4, 8)
    assert L.CTYPES["float"] is ctypes.c_float and L.CTYPES["double"] is ctypes.c_double
    assert L.CTYPES["const char*"] is ctypes.c_char_p
    protos = L._PROTOTYPES
    assert protos["mvk_last_error"] == (ctypes.c_char_p, [])
    assert protos["mvk_xent_workspace_floats"] == (ctypes.c_int64, [ctypes.c_int64])
    assert protos["mvk_reverse_finish_many"][1] == [ctypes.POINTER(L.RevList), ctypes.c_int, ctypes.c_void_p]
    assert protos["mvk_gemm_f32_bn"][1][-3:] == [ctypes.POINTER(L.BnFinish), ctypes.POINTER(L.ATransform), ctypes.c_void_p]
    assert protos["mvk_unproject_depth"][1][0] is ctypes.c_void_p          # const uint16_t*: an address like every array
    loaded = L.lib()
    for name, (res, args) in protos.items():
        assert getattr(loaded, name).restype is res and list(getattr(loaded, name).argtypes) == args, name


@pytest.mark.parametrize("function, struct, cls", [("mvk_bn_lrelu_fwd", "mvk_bn_fwd_problem", "BnFwdProblem"),
                                                   ("mvk_bn_lrelu_bwd", "mvk_bn_bwd_problem", "BnBwdProblem")])
def test_bn_argument_tuple_serves_the_call_and_the_struct(function, struct, cls):
    """ops._bn_fwd_problem / _bn_bwd_problem build ONE tuple: the positional arguments of the single-problem entry point
    and the initialiser of the paired launch's struct. Types must agree position by position (names need not)."""
    ret, params = L.FUNCTIONS[function]
    assert params[-1] == ("void*", "stream")
    plain = {"int32_t": "int"}      # the entry points spell D and ext_rows `int`, the structs `int32_t`
    assert [plain.get(t, t) for t, _ in params[:-1]] == [plain.get(t, t) for t, _ in L.STRUCTS[struct]]
    assert L._PROTOTYPES[function][1][:-1] == [t for _, t in getattr(L, cls)._fields_]


def wrap(*lines):
    return "\n".join(('extern "C" {', "int mvk_ok(const float* a, int64_t n, void* stream);") + lines + ("}", ""))


REJECTED = {      # label -> (lines 3.. of wrap(), the line the error must name)
    "long parameter": (["int mvk_f(long n);"], 3),
    "unsigned parameter": (["int mvk_f(unsigned n);"], 3),
    "unsigned int parameter": (["int mvk_f(unsigned int n);"], 3),
    "size_t parameter": (["int mvk_f(size_t n);"], 3),
    "bool parameter": (["int mvk_f(bool flag);"], 3),
    "pointer to an unknown type": (["int mvk_f(const size_t* n);"], 3),
    "unnamed parameter": (["int mvk_f(int64_t, float x);"], 3),
    "unnamed pointer parameter": (["int mvk_f(int64_t n, const float*);"], 3),
    "empty parameter list": (["int mvk_f();"], 3),
    "function-pointer parameter": (["int mvk_f(void (*done)(int), void* stream);"], 3),
    "array parameter": (["int mvk_f(float v[3]);"], 3),
    "parameter on a continuation line": (["int mvk_f(const float* a,", "          long n, void* stream);"], 4),
    "struct passed by value": (["typedef struct mvk_s { int a; } mvk_s;", "int mvk_f(mvk_s s);"], 4),
    "void return": (["void mvk_f(int a);"], 3),
    "array field": (["typedef struct mvk_s {", "  int a;", "  float v[3];", "} mvk_s;"], 5),
    "bit-field": (["typedef struct mvk_s {", "  int32_t a : 3;", "} mvk_s;"], 4),
    "nested struct": (["typedef struct mvk_s { struct { int a; } in; int b; } mvk_s;"], 3),
    "two pointer fields in one declaration": (["typedef struct mvk_s { float *a, *b; } mvk_s;"], 3),
    "field without a semicolon": (["typedef struct mvk_s { int a; int b } mvk_s;"], 3),
    "enum": (["enum mvk_mode { MVK_A, MVK_B };"], 3),
    "declaration with a body": (["int mvk_f(int a) { return a; }"], 3),
    "stray text between two declarations": (["stray", "int mvk_g(int a);"], 3),
    "stray semicolon": ([";"], 3),
    "function that is not mvk_*": (["int other(int a);"], 3),
    "second declaration": (["int mvk_ok(int a);"], 3),
    "conditional block": (["#if 0", "int mvk_f(int a);", "#endif"], 3),
    "switch that could hide declarations": (["#ifndef MVK_NO_VOTE", "int mvk_f(int a);", "#endif"], 3),
    "define that is not an integer literal": (["#define MVK_N 16u"], 3),
    "function-like macro": (["#define MVK_F(x) (x)"], 3),
    "define without a value": (["#define MVK_FLAG"], 3),
}


@pytest.mark.parametrize("label", sorted(REJECTED))
def test_parser_raises_and_names_the_line(label):
    lines, line = REJECTED[label]
    with pytest.raises(ValueError, match=r"mvkpconv\.h line %d: " % line):
        L.parse_header(wrap(*lines))


def test_parser_rejects_text_outside_the_extern_block_and_a_missing_block():
    for text in ('int mvk_f(int a);\n', wrap() + "int mvk_f(int a);\n", 'extern "C" {\nint mvk_f(int a);\n'):
        with pytest.raises(ValueError, match=r"mvkpconv\.h line \d+: "):
            L.parse_header(text)


def test_parser_accepts_the_real_headers_style():
    text = "\n".join([
        "/* a comment with int mvk_not_a_function(long n); inside */",
        "#ifndef MVKTEST_H", "#define MVKTEST_H", "#include <stdint.h>",
        "#ifdef __cplusplus", 'extern "C" {', "#endif",
        "#define MVK_N 0x10   /* 16: a comment; with, punctuation */",
        "typedef struct mvk_s {",
        "  const float* x; const int32_t* n_valid; int64_t R; int32_t D;   /* [R,D] */",
        "  float eps, momentum, slope; float* y;      // three fields in one declaration",
        "} mvk_s;",
        "int mvk_f(const float* q, int64_t Nq, const void* idx,",
        "          int32_t* min_arg /* [Nq,K] or NULL: the first entry attaining min_d2; a, b */,",
        "          const mvk_s* s, double r, const uint8_t* valid, void* stream);",
        "const char* mvk_msg(void);", "int64_t mvk_bytes(void);",
        "#ifdef __cplusplus", "}", "#endif", "#endif /* MVKTEST_H */", ""])
    functions, structs, constants = L.parse_header(text)
    assert constants == {"MVK_N": 16}
    assert structs == {"mvk_s": (("const float*", "x"), ("const int32_t*", "n_valid"), ("int64_t", "R"), ("int32_t", "D"),
                                 ("float", "eps"), ("float", "momentum"), ("float", "slope"), ("float*", "y"))}
    assert list(functions) == ["mvk_f", "mvk_msg", "mvk_bytes"]
    assert functions["mvk_f"] == ("int", (("const float*", "q"), ("int64_t", "Nq"), ("const void*", "idx"),
                                          ("int32_t*", "min_arg"), ("const mvk_s*", "s"), ("double", "r"),
                                          ("const uint8_t*", "valid"), ("void*", "stream")))
    assert functions["mvk_msg"] == ("const char*", ()) and functions["mvk_bytes"] == ("int64_t", ())
    classes, protos = L._bind(functions, structs)
    assert protos["mvk_f"] == (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p,
                                              ctypes.POINTER(classes["mvk_s"]), ctypes.c_double, ctypes.c_void_p,
                                              ctypes.c_void_p])
    assert classes["mvk_s"].__name__ == "S" and classes["mvk_s"].slope.offset == 36 and ctypes.sizeof(classes["mvk_s"]) == 48


def test_missing_header_is_a_loud_error(monkeypatch):
    monkeypatch.setattr(L, "HEADER_PATH", os.path.join(ROOT, "include", "no_such_header.h"))
    with pytest.raises(RuntimeError, match="mvkpconv.h is not there"):
        L._read_header()
