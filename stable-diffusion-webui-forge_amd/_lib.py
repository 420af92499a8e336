"""ctypes binding of libfmx_gfx950.so (C-ABI declared in include/fmx.h; include/fmx_ext.h, include/fmx_lllite.h, include/fmx_ipadapter.h and include/fmx_clipvision.h hold entry points not yet declared there).

The library is built in-tree by `build()` (hipcc --offload-arch=gfx950) so that it travels with the
repo snapshot.  There is deliberately NO fallback: if the shared object is missing or a symbol is
absent, importing `lib()` raises -- a Forge install that selected this backend must fail loudly rather
than silently run PyTorch eager ops.
"""
import ctypes as C
import os
import re
import subprocess
import threading

_HERE = os.path.dirname(os.path.abspath(__file__))


def knob(name, default=None):
    """Development A/B knob: the value of environment variable `name` ONLY in a process that also carries FMX_ALLOW_KNOBS=1 (the same rule as
    fmx_knob() inside the library) -- a stray FMX_* variable must not change what a production process runs.  Knobs that took effect are recorded
    in ACTIVE_KNOBS (bench.py prints them, together with the library's own list, into its line)."""
    v = os.environ.get(name)
    if v is None:
        return default
    if os.environ.get("FMX_ALLOW_KNOBS") != "1":
        IGNORED_KNOBS[name] = v
        if name == "FMX_LIB":   # a tool that meant to measure another binary must not silently measure the production one
            import warnings
            warnings.warn(f"FMX_LIB={v} is IGNORED (set FMX_ALLOW_KNOBS=1 to load it); using the in-tree libfmx_gfx950.so")
        return default
    ACTIVE_KNOBS[name] = v
    return v


ACTIVE_KNOBS, IGNORED_KNOBS = {}, {}
# FMX_LIB: developer hook for tools/ (timing builds of the same library, tools/build_patched*.sh); a knob like the others
LIB_PATH = knob("FMX_LIB") or os.path.join(_HERE, "libfmx_gfx950.so")
CSRC = os.path.join(_HERE, "csrc")

_lock = threading.Lock()
_lib = None


class FmxError(RuntimeError):
    pass


HEADER = os.path.join(_HERE, "..", "include", "fmx.h")
_SCALARS = {"int": C.c_int32, "int32_t": C.c_int32, "int64_t": C.c_int64, "uint32_t": C.c_uint32, "uint64_t": C.c_uint64,
            "float": C.c_float, "double": C.c_double}
_STRUCT_NAMES = {"fmx_gemm_args": "GemmArgs", "fmx_attn_args": "AttnArgs", "fmx_conv_gn_args": "ConvGnArgs"}
_HEADER_OF_PREFIX = {"fmx_": "fmx.h", "fmxe_": "fmx_ext.h", "fmxl_": "fmx_lllite.h", "fmxi_": "fmx_ipadapter.h", "fmxv_": "fmx_clipvision.h"}
_PARAM = re.compile(r"(?:const )?(\w+) ?((?:\* ?(?:const ?)?)*)(\w+)?")


def parse_header(text, prefix="fmx_", known_structs=None):
    """The text of include/fmx.h (or, with prefix "fmxe_" and fmx.h's structs, of include/fmx_ext.h) -> (signatures, accessors, structs, constants):
    {name: [ctypes of the parameters]} of every `int fmx_*(...);`
    prototype, the names of the `const char* fmx_*(void);` accessors, {C name: ctypes.Structure class} of every `typedef struct fmx_x {...} fmx_x;`
    and {name: int} of every `#define NAME <integer literal>`.  Scalars map through _SCALARS; a pointer to one of the structs is POINTER(struct),
    `char*` is c_char_p, every other pointer -- and every pointer field of a struct -- c_void_p.  Whatever is left between the declarations and
    does not parse as one of these forms raises FmxError naming the text: nothing is skipped."""
    def bad(what):
        return FmxError(f"include/{_HEADER_OF_PREFIX.get(prefix, prefix + '*.h')}: cannot bind {' '.join(what.split())!r}")

    def scalar(ctype, where):
        if ctype not in _SCALARS:
            raise bad(where)
        return _SCALARS[ctype]

    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S).replace("\\\n", " ")
    constants, code = {}, []
    for line in text.split("\n"):
        if line.lstrip().startswith("#"):   # function-like macros, guards and includes declare nothing the binding uses
            m = re.fullmatch(r"\s*#\s*define\s+(\w+)\s+(-?(?:0[xX][0-9a-fA-F]+|\d+))[uUlL]*\s*", line)
            if m:
                constants[m.group(1)] = int(m.group(2), 0)
        else:
            code.append(line)
    text = re.sub(r'extern\s+"C"\s*\{(.*)\}', r"\1", " ".join(code), flags=re.S)

    structs = dict(known_structs or {})

    def struct(m):
        if m.group(1) != m.group(3):
            raise bad(m.group(0))
        fields = []
        for decl in filter(None, (" ".join(d.split()) for d in m.group(2).split(";"))):
            head = re.fullmatch(r"(?:const )?(\w+) ?(.*)", decl)
            if not head:
                raise bad(decl)
            for item in head.group(2).split(","):
                d = re.fullmatch(r"(\*[* ]*)?(?:const )?(\w+)", item.strip())
                if not d:
                    raise bad(decl)
                fields.append((d.group(2), C.c_void_p if d.group(1) else scalar(head.group(1), decl)))
        structs[m.group(1)] = type(_STRUCT_NAMES.get(m.group(1), m.group(1)), (C.Structure,), {"_fields_": fields})
        return " "
    text = re.sub(r"typedef\s+struct\s+(\w+)\s*\{(.*?)\}\s*(\w+)\s*;", struct, text, flags=re.S)

    signatures, accessors = {}, []
    for stmt in filter(None, (" ".join(s.split()) for s in text.split(";"))):
        m = re.fullmatch(r"(int|const char ?\*) ?(" + re.escape(prefix) + r"\w+) ?\((.*)\)", stmt)
        if not m or m.group(2) in signatures or m.group(2) in accessors:
            raise bad(stmt)
        params = [] if m.group(3).strip() == "void" else [p.strip() for p in m.group(3).split(",")]
        if m.group(1) != "int":
            if params:
                raise bad(stmt)
            accessors.append(m.group(2))
            continue
        argtypes = []
        for p in params:
            pm = _PARAM.fullmatch(p)
            if not pm:
                raise bad(stmt)
            ctype, depth = pm.group(1), pm.group(2).count("*")
            if not depth:
                argtypes.append(scalar(ctype, stmt))
            elif depth == 1 and ctype in structs:
                argtypes.append(C.POINTER(structs[ctype]))
            else:
                argtypes.append(C.c_char_p if depth == 1 and ctype == "char" else C.c_void_p)
        signatures[m.group(2)] = argtypes
    return signatures, accessors, structs, constants


def _read_header(path=None):
    path = path or HEADER
    try:
        with open(path) as f:
            return f.read()
    except OSError as e:
        raise FmxError(f"{path} not found: the ctypes binding is generated from it") from e


# name -> argtypes of the entry points that return int (0 = ok); the const char* accessors; the argument structs; the integer #defines
SIGNATURES, ACCESSORS, _structs, CONSTANTS = parse_header(_read_header())
GemmArgs, AttnArgs, ConvGnArgs = (_structs[_n] for _n in ("fmx_gemm_args", "fmx_attn_args", "fmx_conv_gn_args"))
# the entry points declared in include/fmx_ext.h (prefix fmxe_; that header says why they are not in fmx.h), bound the same way
EXT_HEADER = os.path.join(_HERE, "..", "include", "fmx_ext.h")
EXT_SIGNATURES = parse_header(_read_header(EXT_HEADER), prefix="fmxe_", known_structs=_structs)[0]
# the ControlNet-LLLite entry point of include/fmx_lllite.h (prefix fmxl_; that header says why it is in neither of the other two) and its slot struct
LLLITE_HEADER = os.path.join(_HERE, "..", "include", "fmx_lllite.h")
LLLITE_SIGNATURES, _, _lllite_structs, _ = parse_header(_read_header(LLLITE_HEADER), prefix="fmxl_", known_structs=_structs)
LlliteSlot = _lllite_structs["fmxl_lllite_slot"]
# the IP-Adapter entry point of include/fmx_ipadapter.h (prefix fmxi_; that header says why it is in none of the other three) and its argument struct
IPADAPTER_HEADER = os.path.join(_HERE, "..", "include", "fmx_ipadapter.h")
IPADAPTER_SIGNATURES, _, _ipadapter_structs, IPADAPTER_CONSTANTS = parse_header(_read_header(IPADAPTER_HEADER), prefix="fmxi_", known_structs=_structs)
DualAttnArgs = _ipadapter_structs["fmxi_dual_attn_args"]
# the two CLIP-vision front-end entry points of include/fmx_clipvision.h (prefix fmxv_; that header says why they are in none of the other four)
CLIPVISION_HEADER = os.path.join(_HERE, "..", "include", "fmx_clipvision.h")
CLIPVISION_SIGNATURES, _, _, CLIPVISION_CONSTANTS = parse_header(_read_header(CLIPVISION_HEADER), prefix="fmxv_", known_structs=_structs)


def source_tree_hash():
    """hash of the kernel sources in the tree (csrc/src_hash.py: what the Makefile bakes into fmx_build_info of the binary it builds)"""
    res = subprocess.run(["python3", os.path.join(CSRC, "src_hash.py")], capture_output=True, text=True, cwd=CSRC)
    if res.returncode != 0:
        raise FmxError("csrc/src_hash.py failed: " + res.stderr[-1000:])
    return res.stdout.strip()


def binary_matches_sources(path=None):
    """True when the shared object carries the hash of the sources in the tree (read from the file: nothing is loaded)"""
    path = path or os.path.join(_HERE, "libfmx_gfx950.so")
    if not os.path.exists(path):
        return False
    with open(path, "rb") as f:
        return ("src=" + source_tree_hash()).encode() in f.read()


def build(force=False, verbose=False):
    """Compile csrc/*.hip for gfx950 into libfmx_gfx950.so.  make is incremental (a prebuilt binary that travelled with the tree is reused), but the
    result is only accepted if the hash baked into it equals the hash of the sources in the tree: file times do not survive every way a tree is
    copied, so on a mismatch the objects are thrown away and everything is compiled again.  -> path of the library;
    LAST_BUILD says what happened ("reused" / "incremental" / "full rebuild after hash mismatch" / "forced")."""
    global LAST_BUILD
    lib_path = os.path.join(_HERE, "libfmx_gfx950.so")
    existed = os.path.exists(lib_path)
    mtime = os.path.getmtime(lib_path) if existed else None

    def make(*extra):
        res = subprocess.run(["make", "-C", CSRC, "-j8", *extra], capture_output=True, text=True)
        if verbose:
            print(res.stdout[-2000:])
        if res.returncode != 0:
            raise FmxError("building libfmx_gfx950.so failed:\n" + res.stdout[-4000:] + res.stderr[-4000:])

    if force:
        make("clean")
    make()
    LAST_BUILD = "forced" if force else ("reused" if existed and os.path.getmtime(lib_path) == mtime else "incremental")
    if not binary_matches_sources(lib_path):
        make("clean")
        make()
        LAST_BUILD = "full rebuild after hash mismatch"
        if not binary_matches_sources(lib_path):
            raise FmxError("libfmx_gfx950.so does not carry the hash of the sources it was just built from")
    if not os.path.exists(lib_path):
        raise FmxError("build finished but %s is missing" % lib_path)
    return lib_path


LAST_BUILD = None


def lib():
    """Load the shared library (once) and bind every declared symbol; raises if anything is missing."""
    global _lib
    if _lib is not None:
        return _lib
    with _lock:
        if _lib is not None:
            return _lib
        if not os.path.exists(LIB_PATH):
            raise FmxError(f"{LIB_PATH} not found: run `python -c 'import __graft_entry__ as g; g.build()'` "
                           "(hipcc --offload-arch=gfx950).  There is no CPU/PyTorch fallback by design.")
        handle = C.CDLL(LIB_PATH)
        for name, argtypes, restype in [(n, a, C.c_int) for n, a in {**SIGNATURES, **EXT_SIGNATURES, **LLLITE_SIGNATURES, **IPADAPTER_SIGNATURES, **CLIPVISION_SIGNATURES}.items()] + [(n, [], C.c_char_p) for n in ACCESSORS]:
            try:
                fn = getattr(handle, name)
            except AttributeError as e:
                raise FmxError(f"symbol {name} missing from {LIB_PATH}") from e
            fn.argtypes, fn.restype = argtypes, restype
        if handle.fmx_abi_version() != CONSTANTS["FMX_ABI_VERSION"]:
            raise FmxError("libfmx ABI version mismatch")
        _lib = handle
    return _lib


def build_info():
    """{'src': hash of the kernel sources the LOADED binary was built from, 'abi': ..., 'arch': ...} (fmx_build_info)."""
    return dict(kv.split("=", 1) for kv in lib().fmx_build_info().decode().split())


def active_knobs(ignored=False):
    """Development knobs that took effect in this process (library side + Python side), or -- ignored=True -- that were set without FMX_ALLOW_KNOBS=1."""
    buf = C.create_string_buffer(2048)
    check(lib().fmx_active_knobs(buf, len(buf), 1 if ignored else 0), "fmx_active_knobs")
    out = dict(kv.split("=", 1) for kv in buf.value.decode().split(",") if "=" in kv)
    out.update(IGNORED_KNOBS if ignored else ACTIVE_KNOBS)
    return out


def check(code, what=""):
    if code != 0:
        msg = lib().fmx_last_error()
        raise FmxError(f"{what} failed with code {code}: {msg.decode() if msg else ''}")
