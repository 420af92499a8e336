"""CPU: the C-ABI shared library loads without a GPU and exports exactly the symbols include/fmx.h declares; the ctypes
binding (forge_amd/_lib.py) lists the same set.  No compute call is made here."""
import ctypes
import os
import re
import subprocess

import pytest

import forge_amd  # noqa: F401
from forge_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "fmx.h")


def declared_symbols():
    src = open(HEADER).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(fmx_[a-z0-9_]+)\s*\(", src)))


@pytest.fixture(scope="module")
def built():
    return _lib.build()


def test_header_declares_something():
    syms = declared_symbols()
    assert "fmx_gemm_conv_f16" in syms and "fmx_attention_f16" in syms and len(syms) >= 25


def test_library_exports_every_declared_symbol(built):
    handle = ctypes.CDLL(built)
    for s in declared_symbols():
        assert hasattr(handle, s), f"{s} declared in include/fmx.h but not exported by {built}"


def test_no_undeclared_fmx_exports(built):
    out = subprocess.run(["nm", "-D", "--defined-only", built], capture_output=True, text=True, check=True).stdout
    exported = sorted({ln.split()[-1] for ln in out.splitlines() if re.search(r" T fmx_", ln)})
    declared = set(declared_symbols())
    extra = [s for s in exported if s not in declared and s != "fmx_set_error"]
    assert not extra, f"exported but not declared in include/fmx.h: {extra}"


def test_ctypes_binding_matches_header(built):
    declared = set(declared_symbols())
    bound = set(_lib.SIGNATURES) | {"fmx_last_error", "fmx_build_info"}
    assert declared == bound, (sorted(declared - bound), sorted(bound - declared))
    L = _lib.lib()
    assert L.fmx_abi_version() == 12


STRUCTS = (("fmx_gemm_args", _lib.GemmArgs), ("fmx_attn_args", _lib.AttnArgs), ("fmx_conv_gn_args", _lib.ConvGnArgs))
HOST_CXX = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin", "clang++")   # the host compiler hipcc drives (csrc/Makefile)


def test_struct_layouts_match_header(tmp_path):
    """size of the three argument structs and offset + size of every field, as the C++ compiler lays include/fmx.h out, against the ctypes classes
    _lib derives from the same header (a mismatch would silently corrupt every launch).  The field names come from the ctypes side: one the
    header does not have fails the compilation.  Host code only: nothing is offloaded, nothing is loaded into this process."""
    lines = ['#include <cstddef>', '#include <cstdio>', '#include "fmx.h"', "int main() {"]
    want = []
    for cname, cls in STRUCTS:
        lines.append(f'  std::printf("{cname} %zu\\n", sizeof({cname}));')
        want.append(f"{cname} {ctypes.sizeof(cls)}")
        for field, ctype in cls._fields_:
            lines.append(f'  std::printf("{cname}.{field} %zu %zu\\n", offsetof({cname}, {field}), sizeof((({cname}*)0)->{field}));')
            want.append(f"{cname}.{field} {getattr(cls, field).offset} {ctypes.sizeof(ctype)}")
    lines += ["  return 0;", "}"]
    src, exe = tmp_path / "layout.cpp", tmp_path / "layout"
    src.write_text("\n".join(lines) + "\n")
    subprocess.run([HOST_CXX, "-std=c++17", "-I", os.path.dirname(HEADER), str(src), "-o", str(exe)], check=True, capture_output=True, text=True)
    got = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split("\n")
    assert [ln for ln in got if ln] == want
    assert sum(len(cls._fields_) for _, cls in STRUCTS) == 52 + 26 + 21   # fields counted in include/fmx.h by hand: none dropped on either side


def _parse(text):
    return _lib.parse_header(text)


def test_parser_maps_prototypes_structs_constants_and_accessors():
    vp, i32, i64, f32 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, ctypes.c_float
    sigs, accessors, structs, constants = _parse('''
        #ifdef __cplusplus
        extern "C" {
        #endif
        #define FMX_ABI_VERSION 12
        #define FMX_MASK 0x10 /* hex */
        #define FMX_PAD4(x) (((x) + 3) / 4 * 4)
        #define FMX_LONG(a, b) \\
          ((a) + 7 * (b))
        #define FMX_GUARD
        typedef struct fmx_t {
          int32_t a, b;      /* two scalars */
          const void *p, *q; // two pointers
          float* w;
          int64_t big; double d; uint32_t u; uint64_t v;
        } fmx_t;
        int fmx_abi_version(void);
        const char* fmx_text(void);
        int fmx_broken(const void* x, /* device */
                       int64_t n,     // elements
                       void* stream);
        int fmx_unnamed(void*, int32_t);
        int fmx_mixed(const fmx_t* args /* host */, char* buf, int len, const float* const* srcs, void** out, const uint8_t* bytes, float s,
                      double d, uint32_t u, uint64_t v);
        #ifdef __cplusplus
        }
        #endif
    ''')
    assert accessors == ["fmx_text"]
    assert constants == {"FMX_ABI_VERSION": 12, "FMX_MASK": 16}
    T = structs["fmx_t"]
    assert list(structs) == ["fmx_t"] and issubclass(T, ctypes.Structure)
    assert T._fields_ == [("a", i32), ("b", i32), ("p", vp), ("q", vp), ("w", vp), ("big", i64), ("d", ctypes.c_double), ("u", ctypes.c_uint32),
                          ("v", ctypes.c_uint64)]
    assert sigs == {"fmx_abi_version": [], "fmx_broken": [vp, i64, vp], "fmx_unnamed": [vp, i32],
                    "fmx_mixed": [ctypes.POINTER(T), ctypes.c_char_p, i32, vp, vp, vp, f32, ctypes.c_double, ctypes.c_uint32, ctypes.c_uint64]}


@pytest.mark.parametrize("text, named", [
    ("int fmx_x(const void* a, long double b, void* stream);", "long double b"),                 # a type outside the map
    ("int fmx_x(const void* a, unsigned n);", "unsigned n"),
    ("int fmx_x(size_t n);", "size_t n"),
    ("int fmx_x(int64_t strides[4]);", "strides[4]"),                                            # a declarator the map has no rule for
    ("float fmx_x(void);", "float fmx_x"),                                                       # a return type that is neither int nor const char*
    ("const char* fmx_x(int32_t which);", "fmx_x(int32_t which)"),                               # an accessor takes no arguments
    ("int fmx_x(void* a);\nint fmx_x(void* a, void* b);", "fmx_x(void* a, void* b)"),            # declared twice
    ("int fmx_ok(void* a);\nstatic inline int fmx_helper(int a) { return a; }", "fmx_helper"),   # fmx_ and ( in a form that is no prototype
    ("typedef struct fmx_t { long double a; } fmx_t;", "long double a"),
    ("typedef struct fmx_t { int32_t a[4]; } fmx_t;", "int32_t a[4]"),
    ("typedef struct fmx_t { int32_t a; } fmx_u;", "fmx_u"),
    ("int fmx_x(void* a)", None),                                                                # the missing ; swallows the next declaration
])
def test_parser_fails_loudly(text, named):
    if named is None:
        text, named = text + "\nint fmx_y(void* a);", "fmx_y"
    with pytest.raises(_lib.FmxError) as e:
        _parse(text)
    assert named in str(e.value)


def test_missing_header_fails_loudly(tmp_path, monkeypatch):
    monkeypatch.setattr(_lib, "HEADER", str(tmp_path / "nope.h"))
    with pytest.raises(_lib.FmxError, match="nope.h"):
        _lib._read_header()


def test_binding_tables_come_from_the_header():
    """the module-level tables are parse_header of include/fmx.h: all 97 int entry points, the two accessors, the constants hipops reads"""
    sigs, accessors, structs, constants = _parse(open(HEADER).read())
    names = lambda table: {k: [t.__name__ for t in v] for k, v in table.items()}  # noqa: E731  (a second parse makes struct classes of its own)
    assert names(sigs) == names(_lib.SIGNATURES) and len(sigs) == 97 and accessors == _lib.ACCESSORS == ["fmx_last_error", "fmx_build_info"]
    assert [c for c, _ in STRUCTS] == list(structs) and constants == _lib.CONSTANTS
    assert [[(f, t.__name__) for f, t in structs[c]._fields_] for c, _ in STRUCTS] == [[(f, t.__name__) for f, t in cls._fields_] for _, cls in STRUCTS]
    assert {k: constants[k] for k in ("FMX_ABI_VERSION", "FMX_OK", "FMX_E_BADARG", "FMX_E_UNSUPPORTED", "FMX_ACT_NONE", "FMX_ACT_GEGLU", "FMX_ACT_GELU_TANH",
                                      "FMX_FREEU_CHUNK_PIXELS", "FMX_DYNTHRESH_SEPARATE", "FMX_DYNTHRESH_ZERO", "FMX_DYNTHRESH_STD", "FMX_DYNTHRESH_CHUNK")} == {
        "FMX_ABI_VERSION": 12, "FMX_OK": 0, "FMX_E_BADARG": 10001, "FMX_E_UNSUPPORTED": 10002, "FMX_ACT_NONE": 0, "FMX_ACT_GEGLU": 1, "FMX_ACT_GELU_TANH": 2,
        "FMX_FREEU_CHUNK_PIXELS": 256, "FMX_DYNTHRESH_SEPARATE": 1, "FMX_DYNTHRESH_ZERO": 2, "FMX_DYNTHRESH_STD": 4, "FMX_DYNTHRESH_CHUNK": 2048}
    assert not any("(" in k for k in constants) and "FMX_FREEU_PAD4" not in constants and "FMX_H" not in constants


def test_missing_library_fails_loudly(tmp_path, monkeypatch):
    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setattr(_lib, "LIB_PATH", str(tmp_path / "nope.so"))
    with pytest.raises(_lib.FmxError):
        _lib.lib()


def test_build_info_carries_the_hash_of_the_sources_on_disk(built):
    """fmx_build_info(): the .so knows which kernel sources it was built from (csrc/Makefile bakes csrc/src_hash.py's value in); after build() it
    equals the hash of the tree -- bench.py credits a committed PMC summary to THE BINARY's hash, so a stale .so cannot borrow newer measurements."""
    import importlib.util
    info = _lib.build_info()
    spec = importlib.util.spec_from_file_location("fmx_src_hash", os.path.join(ROOT, "stable-diffusion-webui-forge_amd", "csrc", "src_hash.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert info["abi"] == "12" and info["arch"] == "gfx950"
    assert re.fullmatch(r"[0-9a-f]{16}", info["src"]) and info["src"] == mod.kernel_source_hash()


def test_python_side_knobs_need_the_allow_flag(monkeypatch):
    monkeypatch.delenv("FMX_ALLOW_KNOBS", raising=False)
    monkeypatch.setenv("FMX_LN_FOLD", "0")
    assert _lib.knob("FMX_LN_FOLD", "1") == "1" and _lib.IGNORED_KNOBS.get("FMX_LN_FOLD") == "0"
    monkeypatch.setenv("FMX_ALLOW_KNOBS", "1")
    assert _lib.knob("FMX_LN_FOLD", "1") == "0" and _lib.ACTIVE_KNOBS.get("FMX_LN_FOLD") == "0"
    _lib.ACTIVE_KNOBS.clear(); _lib.IGNORED_KNOBS.clear()
    buf = ctypes.create_string_buffer(64)
    assert _lib.lib().fmx_active_knobs(buf, 64, 0) == 0 and _lib.lib().fmx_active_knobs(None, 0, 0) != 0
