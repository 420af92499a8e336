"""float8 / bitsandbytes 4-bit expansion: rate of the kernels against a plain device copy of the same bytes and against the GGUF Q4_0 stream, and
the load time of a full-size synthetic nested-NF4 Flux transformer.

    python tools/bench_quant.py rates [--out profiles/quant_expand_rates.json]
    python tools/bench_quant.py load  [--blocks 19,38] [--out profiles/quant_flux_nf4_load.json]

rates: a 3072 x 21504 tensor (Flux's widest matrix) of seeded random bytes, bf16 and fp16 output, for fp8 e4m3fn / e5m2, bnb4 flat and nested
(blocksize 64, nested blocksize 256) and, as a yardstick, fmx_gguf_dequant Q4_0 on the same element count (the closest existing stream: 0.56 bytes
in, 2 out per weight): median of 25 launches after 5 warm-up launches, device events around each launch; in the same process, a `copy_` between two
device buffers of (bytes in + bytes out) / 2 bytes -- it reads and writes that many, so it moves the same number of bytes as the kernel.
`ratio` = copy time / kernel time (1.0: the kernel streams as fast as a copy does); `bnb4_vs_q4_0` = the bnb4 rows' ratio / Q4_0's.
load: a Flux.1-dev-shaped transformer (19 + 38 blocks) as an in-memory state dict in the bitsandbytes packed format -- every matrix nested NF4 of
random bytes, vectors bf16 -- through forge_loader (wall clock, ends in a device synchronise), twice; no file is read, so this is the wrapping,
staging, host-to-device and kernel time."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import forge_amd  # noqa: E402,F401
import bnb_write as W  # noqa: E402
from forge_amd import _lib, hipops as ops, synth  # noqa: E402
from forge_amd.backend import loader  # noqa: E402
from forge_amd.backend.quant_state import BnbQuantState  # noqa: E402

ROWS, COLS = 3072, 21504


def _timed(fn, warmup=5, reps=25):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms), min(ms), max(ms)


def rates(out_path):
    n = ROWS * COLS
    rng = np.random.default_rng(0)
    dev = lambda a: torch.from_numpy(a).cuda()  # noqa: E731
    nb = n // 64
    flat = BnbQuantState("nf4", (ROWS, COLS), 64, dev(W.TABLES["nf4"]), dev(rng.uniform(0.01, 2.0, nb).astype(np.float32)), False, None, None, 0, 0.0, None)
    nested = BnbQuantState("nf4", (ROWS, COLS), 64, dev(W.TABLES["nf4"]), dev(rng.integers(0, 256, nb, dtype=np.uint8)), True, dev(W.nested_table(0)),
                           dev(rng.uniform(0.01, 2.0, nb // 256).astype(np.float32)), 256, 0.05, None)
    cases = [("gguf_q4_0", n // 32 * 18, lambda raw, dt, out: ops.gguf_dequant(raw, 2, (ROWS, COLS), dt, out=out)),
             ("fp8_e4m3fn", n, lambda raw, dt, out: ops.fp8_expand(raw, 0, (ROWS, COLS), dt, out=out)),
             ("fp8_e5m2", n, lambda raw, dt, out: ops.fp8_expand(raw, 1, (ROWS, COLS), dt, out=out)),
             ("bnb4_flat", n // 2 + nb * 4, lambda raw, dt, out: ops.bnb4_dequant(raw[:n // 2], flat, dt, out=out)),
             ("bnb4_nested", n // 2 + nb + nb // 256 * 4, lambda raw, dt, out: ops.bnb4_dequant(raw[:n // 2], nested, dt, out=out))]
    rows = []
    for name, bytes_in, fn in cases:
        raw = dev(rng.integers(0, 256, bytes_in, dtype=np.uint8))
        if name == "gguf_q4_0":
            raw.view(-1, 18)[:, 1] &= 0x3F          # finite, small fp16 scales
        moved = bytes_in + 2 * n
        src, dst = torch.empty(moved // 2, dtype=torch.uint8, device="cuda"), torch.empty(moved // 2, dtype=torch.uint8, device="cuda")
        copy_ms = _timed(lambda: dst.copy_(src))
        for dt, tag in ((torch.bfloat16, "bf16"), (torch.float16, "f16")):
            out = torch.empty((ROWS, COLS), dtype=dt, device="cuda")
            k_ms = _timed(lambda: fn(raw, dt, out))
            rows.append(dict(kernel=name, out=tag, bytes_in=bytes_in, bytes_out=2 * n, kernel_ms_median=round(k_ms[0], 4), kernel_ms_min=round(k_ms[1], 4),
                             kernel_ms_max=round(k_ms[2], 4), kernel_TBps=round(moved / k_ms[0] * 1e-9, 3), copy_ms_median=round(copy_ms[0], 4),
                             copy_TBps=round(moved / copy_ms[0] * 1e-9, 3), ratio=round(copy_ms[0] / k_ms[0], 3)))
            print(json.dumps(rows[-1]), flush=True)
        del raw, src, dst
    q4 = {r["out"]: r["ratio"] for r in rows if r["kernel"] == "gguf_q4_0"}
    versus = {f"{r['kernel']}_{r['out']}": round(r["ratio"] / q4[r["out"]], 3) for r in rows if r["kernel"].startswith("bnb4")}
    res = dict(shape=[ROWS, COLS], launches=25, warmup=5, device=torch.cuda.get_device_name(0), library=_lib.build_info(), rows=rows, bnb4_vs_q4_0=versus,
               expectation="bnb4 copy ratio >= 0.9 x Q4_0's", expectation_met=all(v >= 0.9 for v in versus.values()))
    print(json.dumps(dict(bnb4_vs_q4_0=versus, expectation_met=res["expectation_met"])), flush=True)
    if out_path:
        json.dump(res, open(out_path, "w"), indent=1)
    return res


def synth_flux_nf4(depth, depth_single, blocksize=64, blocksize2=256):
    """-> (cfg, state dict in the packed format, bytes).  One buffer of random bytes per tensor size: the content does not matter, its size does"""
    from forge_amd.backend.nn.layout import flux_param_shapes
    cfg = dict(synth.FLUX_DEV_CONFIG, depth=depth, depth_single_blocks=depth_single)
    rng = np.random.default_rng(1)
    code, code2 = torch.from_numpy(W.TABLES["nf4"].copy()), torch.from_numpy(W.nested_table(0))
    pool, sd, total = {}, {}, 0
    for name, shape in flux_param_shapes(cfg).items():
        n = int(np.prod(shape))
        if len(shape) < 2:
            sd[name] = torch.zeros(shape, dtype=torch.bfloat16)
            continue
        if n not in pool:
            nb = (n + blocksize - 1) // blocksize
            pool[n] = (torch.from_numpy(rng.integers(0, 256, ((n + 1) // 2, 1), dtype=np.uint8)), torch.from_numpy(rng.integers(96, 160, nb, dtype=np.uint8)),
                       torch.from_numpy(rng.uniform(0.01, 0.05, (nb + blocksize2 - 1) // blocksize2).astype(np.float32)))
        packed, absmax, absmax2 = pool[n]
        meta = dict(quant_type="nf4", blocksize=blocksize, dtype="bfloat16", shape=list(shape), nested_blocksize=blocksize2, nested_dtype="float32", nested_offset=0.02)
        sd.update({name: packed, name + ".quant_map": code, name + ".absmax": absmax, name + ".nested_absmax": absmax2, name + ".nested_quant_map": code2,
                   name + ".quant_state.bitsandbytes__nf4": torch.tensor(list(json.dumps(meta).encode()), dtype=torch.uint8)})
        total += packed.numel() + absmax.numel() + absmax2.numel() * 4
    return cfg, sd, total


def load(depth, depth_single, out_path):
    t0 = time.perf_counter()
    cfg, sd, size = synth_flux_nf4(depth, depth_single)
    make_s = time.perf_counter() - t0
    walls = []
    for _ in range(2):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        eng = loader.forge_loader(sd, device="cuda")
        torch.cuda.synchronize()
        walls.append(time.perf_counter() - t0)
        assert eng.model_guess["flux_config"] == cfg and eng.model_guess["dtype"] == torch.bfloat16
        del eng
    res = dict(packed_bytes=size, depth=[depth, depth_single], tensors_nf4=sum(1 for k in sd if k.endswith("__nf4")), make_state_dict_s=round(make_s, 2),
               forge_loader_wall_s=round(walls[0], 3), forge_loader_wall_second_call_s=round(walls[1], 3), source="in-memory state dict, no file read",
               device=torch.cuda.get_device_name(0), library=_lib.build_info())
    print(json.dumps(res), flush=True)
    if out_path:
        json.dump(res, open(out_path, "w"), indent=1)
    return res


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("mode", choices=["rates", "load"])
    ap.add_argument("--out", default=None)
    ap.add_argument("--blocks", default="19,38")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_quant.py measures on the GPU: no device found")
    if a.mode == "rates":
        rates(a.out)
    else:
        d, s = (int(x) for x in a.blocks.split(","))
        load(d, s, a.out)
