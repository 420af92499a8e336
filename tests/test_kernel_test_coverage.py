"""CPU: every entry point of include/fmx.h is exercised by some GPU test -- named in a tests/test_gpu_*.py file by its C name, or reached through
a forge_amd.hipops wrapper that such a file calls (wrappers that call wrappers count transitively).  Entry points without a test route are
in ALLOWED with a one-line reason; adding a kernel without a test fails this file.  Note the granularity: a wrapper dispatching fp16 and bf16
covers both twins as far as this check can see -- tests/test_gpu_kernels_bf16.py is what launches the bf16 forms."""
import ast
import glob
import os
import re

from test_capi_symbols import declared_symbols

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPOPS = os.path.join(ROOT, "stable-diffusion-webui-forge_amd", "hipops.py")

ALLOWED = {
    "fmx_abi_version": "ABI handshake, checked by tests/test_capi_symbols.py on the CPU",
    "fmx_last_error": "error-string accessor behind every failing call; tests/test_capi_contracts.py reads it",
    "fmx_build_info": "build metadata, checked by tests/test_capi_symbols.py on the CPU",
    "fmx_active_knobs": "diagnostic string of the environment knobs, no arithmetic",
    "fmx_device_info": "device query, no kernel",
    "fmx_attention_route": "host-only, no kernel: the dispatch plan by name, checked by tests/test_kernel_ref_teeth.py on the CPU",
    "fmx_graph_begin": "graph-capture helper for C callers; the Python side captures with torch.cuda.graph",
    "fmx_graph_end": "graph-capture helper for C callers; the Python side captures with torch.cuda.graph",
    "fmx_graph_launch": "graph-capture helper for C callers; the Python side captures with torch.cuda.graph",
    "fmx_graph_destroy": "graph-capture helper for C callers; the Python side captures with torch.cuda.graph",
    "fmx_event_create": "timing helper of the launch profiler, no arithmetic",
    "fmx_event_record": "timing helper of the launch profiler, no arithmetic",
    "fmx_event_elapsed_ms": "timing helper of the launch profiler, no arithmetic",
    "fmx_event_destroy": "timing helper of the launch profiler, no arithmetic",
}


def wrapper_symbols():
    """hipops top-level function -> the fmx_* entry points it reaches (string literals "fmx_x" possibly completed by a dtype suffix,
    `lib().fmx_x` attributes, and the wrappers it calls, transitively)"""
    src = open(HIPOPS).read()
    tree = ast.parse(src)
    declared = set(declared_symbols())
    funcs = {n.name: n for n in tree.body if isinstance(n, ast.FunctionDef)}
    direct, calls = {}, {}
    for name, node in funcs.items():
        syms, callees = set(), set()
        for sub in ast.walk(node):
            if isinstance(sub, ast.Constant) and isinstance(sub.value, str) and sub.value.startswith("fmx_"):
                syms |= {s for s in (sub.value, sub.value + "_f16", sub.value + "_bf16") if s in declared}
            elif isinstance(sub, ast.Attribute) and sub.attr in declared:
                syms.add(sub.attr)
            elif isinstance(sub, ast.Call) and isinstance(sub.func, ast.Name) and sub.func.id in funcs:
                callees.add(sub.func.id)
        direct[name], calls[name] = syms, callees
    out = {}
    for name in funcs:
        seen, stack, syms = set(), [name], set()
        while stack:
            f = stack.pop()
            if f in seen:
                continue
            seen.add(f)
            syms |= direct[f]
            stack.extend(calls[f])
        out[name] = syms
    return out


def symbols_reached_by_gpu_tests():
    wraps = wrapper_symbols()
    declared = set(declared_symbols())
    hit = {}
    for path in sorted(glob.glob(os.path.join(ROOT, "tests", "test_gpu_*.py"))):
        text = open(path).read()
        for s in declared:
            if re.search(r"\b%s\b" % s, text):
                hit.setdefault(s, os.path.basename(path))
        for w in set(re.findall(r"\b(?:ops|hipops)\.(\w+)\(", text)):
            for s in wraps.get(w, ()):
                hit.setdefault(s, os.path.basename(path))
    return hit


def test_wrapper_map_sees_the_dtype_dispatch():
    wraps = wrapper_symbols()
    assert {"fmx_gemm_conv_f16", "fmx_gemm_conv_bf16", "fmx_gemm_conv_stats_f16", "fmx_gemm_conv_stats_bf16"} <= wraps["conv_gemm"]
    assert {"fmx_timestep_embedding", "fmx_timestep_embedding_bf16"} <= wraps["timestep_embedding"]
    assert "fmx_groupnorm_stats_bf16" in wraps["groupnorm"]            # through groupnorm_stats
    assert "fmx_gemm_conv_f16" in wraps["linear"]                       # through conv_gemm
    assert {"fmx_layernorm_f16", "fmx_layernorm_bf16"} <= wraps["layernorm"]


def test_every_entry_point_has_a_gpu_test():
    hit = symbols_reached_by_gpu_tests()
    missing = sorted(s for s in declared_symbols() if s not in hit and s not in ALLOWED)
    assert not missing, f"entry points of include/fmx.h that no tests/test_gpu_*.py file reaches (add a test or an ALLOWED reason): {missing}"


def test_allowlist_is_current():
    declared = set(declared_symbols())
    stale = sorted(s for s in ALLOWED if s not in declared)
    assert not stale, f"ALLOWED names entry points that include/fmx.h no longer declares: {stale}"
    assert all(len(r) > 10 for r in ALLOWED.values())
